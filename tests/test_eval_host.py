"""CPU checks of the device-side validation epoch's host pieces: the float64 restatement the GPU
tests lean on (tests/_eval_ref.py) against the golden written by the reference's own
eval_epoch_hetero (tests/golden/make_golden_eval.py), the order of the 9-tuple, the z thresholds
and the non-positive-target error.  No GPU work."""
import inspect

import numpy as np
import pytest

import _eval_ref as R
from conftest import load_golden


@pytest.fixture(scope="module")
def gold():
    return load_golden("eval")


def _restate(g, case):
    floor = float(g["meta/min_logvar_floor"])
    lm, ls = g["meta/target_log_means"], g["meta/target_log_stds"]
    z, p = g["meta/z_thresholds"], g["meta/prob_levels"]
    if case == "model":
        return R.eval_epoch(R.split(g["b/heads"], (3, 3)), R.split(g["b/y"], (3, 3)), int(g["b/dataset_size"]), lm, ls,
                            floor, z, p)
    sizes = g["a/batch_sizes"]
    heads = g["a/heads"].copy()
    if case == "nan":
        heads[tuple(g["a/nan_at"])] = np.nan
    if case == "notf":
        return R.eval_epoch(R.split(heads, sizes), R.split(g["a/y_notf"], sizes), int(g["a/dataset_size"]), None, None,
                            floor, z, p, compute_log_mae=False)
    return R.eval_epoch(R.split(heads, sizes), R.split(g["a/y"], sizes), int(g["a/dataset_size"]), lm, ls, floor, z, p)


@pytest.mark.parametrize("case", ["tf", "notf", "nan", "model"])
def test_restatement_matches_reference(gold, case):
    want = gold["b/out"] if case == "model" else gold[f"a/{case}/out"]
    R.check_metrics(_restate(gold, case)["out"], want, label=f"{case} ")


def test_nan_case_is_what_the_reference_does(gold):
    """One NaN mean: the four error sums become NaN, Spearman masks the pair, sigma_max, coverage,
    mean log-variance and ECE stay finite."""
    out = gold["a/nan/out"]
    assert np.isnan(out[:4]).all() and np.isfinite(out[4:]).all()
    r = _restate(gold, "nan")
    assert R.spearman(r["err"], r["sig"])[1] == r["err"].size - 1


def test_reference_ece_is_per_batch_not_pooled(gold):
    r = _restate(gold, "tf")
    want = float(gold["a/tf/out"][8])
    assert abs(r["out"][8] - want) <= 1e-6
    assert abs(r["ece_pooled"] - want) > 1e-3  # the fixture tells the two apart


def test_average_ranks_with_ties():
    assert R.average_ranks([3.0, 1.0, 3.0, 2.0, 3.0]).tolist() == [4.0, 1.0, 4.0, 2.0, 4.0]
    rho, m, _, _ = R.spearman([1.0, 2.0, np.nan, 4.0], [2.0, 1.0, 5.0, np.inf])
    assert m == 2 and abs(rho + 1.0) < 1e-12
    assert np.isnan(R.spearman([1.0, 2.0, 3.0], [7.0, 7.0, 7.0])[0])
    assert np.isnan(R.spearman([1.0], [2.0])[0])


def test_tuple_order_thresholds_and_signature(gold):
    from alignn_mi355x import evaluate
    import alignn_mi355x as A
    assert evaluate.METRIC_NAMES == R.NAMES
    assert A.eval_epoch_hetero is evaluate.eval_epoch_hetero and A.EvalMetrics is evaluate.EvalMetrics
    p, z = evaluate.calibration_levels()
    assert np.array_equal(p.numpy(), gold["meta/prob_levels"])
    assert np.array_equal(z.numpy(), gold["meta/z_thresholds"])  # bitwise the reference's float32 expression
    assert float(gold["meta/min_logvar_floor"]) == evaluate.MIN_LOGVAR_FLOOR
    params = list(inspect.signature(evaluate.eval_epoch_hetero).parameters)
    assert params == ["model", "loader", "device", "transformer", "use_amp", "compute_log_mae", "progress_desc",
                      "min_logvar_floor"]


def test_state_layout_matches_header():
    import os
    import re
    from alignn_mi355x import evaluate
    from conftest import REPO
    src = open(os.path.join(REPO, "include", "alignn_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define ALIGNN_EVAL_(\w+) (\d+)\b", src)}
    for name in ("LOSS", "GRAPHS", "LV_SUM", "LV_COUNT", "SIGMA_MAX", "COV_HITS", "ELEMS", "ECE_SUM", "ECE_TERMS", "ABS",
                 "SQ", "LOGABS", "BAD", "CURSOR", "SPEARMAN"):
        assert defs["S_" + name] == getattr(evaluate, "S_" + name), name
    assert defs["STATE_DOUBLES"] == evaluate.STATE_DOUBLES and defs["OUT_DOUBLES"] == evaluate.OUT_DOUBLES
    assert defs["LEVELS"] == evaluate.LEVELS and defs["RANK_TILE"] == evaluate.RANK_TILE


def test_non_positive_target_error(gold):
    from alignn_mi355x import evaluate
    assert evaluate.BAD_TARGET_MESSAGE == R.BAD_TARGET_MESSAGE == "Log transform encountered non-positive targets."
    y = gold["a/y"].copy()
    y[4, 0] = 0.0
    sizes = gold["a/batch_sizes"]
    with pytest.raises(ValueError, match="non-positive targets"):
        R.eval_epoch(R.split(gold["a/heads"], sizes), R.split(y, sizes), 25, gold["meta/target_log_means"],
                     gold["meta/target_log_stds"], float(gold["meta/min_logvar_floor"]), gold["meta/z_thresholds"],
                     gold["meta/prob_levels"])


def test_resident_batch_is_not_moved():
    """eval_epoch_hetero calls batch.to(device) only for a batch that is elsewhere: Data.to drops the
    batch's device-side caches even when nothing moves."""
    import torch
    import alignn_mi355x as A
    from alignn_mi355x import evaluate
    b = A.Data(x=torch.zeros(2, 3), y=torch.ones(1))
    assert evaluate._resident(b, torch.device("cpu"))
    assert not evaluate._resident(b, torch.device("cuda", 0))
    assert not evaluate._resident(A.Data(), torch.device("cpu"))
