"""The device-side validation epoch (alignn_mi355x/evaluate.py, csrc/evalmetrics.hip) against the
golden written by the reference's own eval_epoch_hetero (tests/golden/make_golden_eval.py), and,
where the golden has no case, against the float64 restatement of tests/_eval_ref.py (itself
checked against the golden on the CPU, tests/test_eval_host.py).  Sorts after the core suites."""
import numpy as np
import pytest
import torch

import _eval_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("x", "edge_index", "edge_attr", "lg_edge_index", "lg_edge_attr", "global_x", "sg_one_hot", "y", "batch",
        "ptr")


@pytest.fixture(scope="module")
def gold():
    return load_golden("eval")


def _transformer(g):
    return g["meta/target_log_means"], g["meta/target_log_stds"]


def _case(g, case):
    """(heads [25, 4], y [25, 2], transformer, compute_log_mae) of a metric case."""
    heads = g["a/heads"].copy()
    if case == "nan":
        heads[tuple(g["a/nan_at"])] = np.nan
    if case == "notf":
        return heads, g["a/y_notf"], None, False
    return heads, g["a/y"], _transformer(g), True


def _metrics(g, transformer=None, compute_log_mae=True, **kw):
    from alignn_mi355x.evaluate import EvalMetrics
    return EvalMetrics(2, transformer, float(g["meta/min_logvar_floor"]), compute_log_mae, device=DEV, **kw)


def _epoch(em, heads, y, sizes, dtype=torch.float32):
    h = torch.from_numpy(np.ascontiguousarray(heads)).to(DEV).to(dtype)
    t = torch.from_numpy(np.ascontiguousarray(y)).to(DEV)
    r = 0
    for b in sizes:
        em.update(h[r:r + b], t[r:r + b])
        r += int(b)
    return em


def _restate(g, heads, y, sizes, transformer, compute_log_mae, dataset_size):
    lm, ls = transformer if transformer is not None else (None, None)
    return R.eval_epoch(R.split(heads, sizes), R.split(y, sizes), dataset_size, lm, ls,
                        float(g["meta/min_logvar_floor"]), g["meta/z_thresholds"], g["meta/prob_levels"], compute_log_mae)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


@pytest.mark.parametrize("case", ["tf", "notf", "nan"])
def test_metric_cases_match_reference(gold, case):
    heads, y, tf, log_mae = _case(gold, case)
    em = _epoch(_metrics(gold, tf, log_mae), heads, y, gold["a/batch_sizes"])
    R.check_metrics(em.result(int(gold["a/dataset_size"])), gold[f"a/{case}/out"], label=f"{case} ")


def _model_and_loader(gold):
    """The package's model with the weights of ensemble.npz's member ``b/member`` and that file's two
    batches (on the host) as a loader with a dataset of length 6."""
    import alignn_mi355x as A
    ens = load_golden("ensemble")
    node, edge, angle, glob, hidden, layers, heads = (int(v) for v in ens["meta/dims"])
    j = int(gold["b/member"])
    model = A.HeteroAlignnRegressor(A.AlignnRegressor(node, edge, angle, glob, 2, hidden, layers, heads, 0.15), 2)
    model.load_state_dict({k[3:]: torch.from_numpy(np.array(v)) for k, v in ens.items() if k.startswith(f"m{j}/")})

    class Loader(list):
        dataset = range(int(gold["b/dataset_size"]))

    loader = Loader()
    for bi in range(2):
        b = A.Batch()
        for k in KEYS:
            setattr(b, k, torch.from_numpy(np.array(ens[f"in/b{bi}/{k}"])))
        b.num_graphs = int(b.ptr.numel() - 1)
        loader.append(b)
    return model.to(DEV), loader


def test_model_case_matches_reference(gold):
    """eval_epoch_hetero with the package's model over the batches and weights of ensemble.npz."""
    import alignn_mi355x as A
    model, loader = _model_and_loader(gold)
    out = A.eval_epoch_hetero(model, loader, torch.device(DEV), transformer=_transformer(gold))
    R.check_metrics(out, gold["b/out"], label="model ")


def test_use_amp_epoch_widens_the_autocast_heads(gold):
    """use_amp: the model runs under bf16 autocast and returns bf16 heads; the metrics are the fp32
    ones of those heads widened (the stated deviation from the reference's CUDA autocast path)."""
    import alignn_mi355x as A
    model, loader = _model_and_loader(gold)
    out = A.eval_epoch_hetero(model, loader, torch.device(DEV), transformer=_transformer(gold), use_amp=True)
    heads = []
    model.eval()
    with torch.no_grad(), torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        for b in loader:   # moved to the device in place by the epoch above
            mean, logvar = model(b)
            assert mean.dtype == torch.bfloat16
            heads.append(torch.cat([mean, logvar], 1).float().cpu().numpy())
    r = _restate(gold, np.concatenate(heads), gold["b/y"], (3, 3), _transformer(gold), True, 6)
    R.check_metrics(out, r["out"], label="amp ")


def test_bf16_heads_are_widened(gold):
    heads, y, tf, _ = _case(gold, "tf")
    sizes, n = gold["a/batch_sizes"], int(gold["a/dataset_size"])
    widened = torch.from_numpy(heads).bfloat16().float().numpy()
    em = _epoch(_metrics(gold, tf), heads, y, sizes, dtype=torch.bfloat16)
    R.check_metrics(em.result(n), _restate(gold, widened, y, sizes, tf, True, n)["out"], label="bf16 ")


def _spearman_inputs(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 6, n).astype(np.float32)   # integer-valued: heavy ties
    s = rng.integers(0, 4, n).astype(np.float32)
    if n >= 63:
        bad = rng.choice(n, size=n // 9, replace=False)
        x[bad[0::3]] = np.nan
        s[bad[1::3]] = np.inf
        x[bad[2::3]] = -np.inf
    return x, s


@pytest.mark.parametrize("n", [1, 2, 63, 65, 2 * 1024 + 37])
def test_spearman_alone(n):
    from alignn_mi355x import evaluate
    assert evaluate.RANK_TILE == 1024  # the last size is two LDS tiles plus 37
    x, s = _spearman_inputs(n, 100 + n)
    if n == 2:
        x[:], s[:] = (1.0, 2.0), (5.0, 3.0)
    rho, m, rx, rs = evaluate.spearman(torch.from_numpy(x).to(DEV), torch.from_numpy(s).to(DEV))
    want_rho, want_m, want_rx, want_rs = R.spearman(x, s)
    assert int(m.item()) == want_m
    assert np.array_equal(rx.cpu().numpy()[:want_m], want_rx)  # ranks exact
    assert np.array_equal(rs.cpu().numpy()[:want_m], want_rs)
    print(f"n={n} m={want_m} rho got {rho.item()!r} want {want_rho!r}")
    if np.isnan(want_rho):
        assert n == 1 and np.isnan(rho.item())
    else:
        assert abs(rho.item() - want_rho) <= 1e-9


def test_spearman_degenerate_cases():
    from alignn_mi355x import evaluate

    def rho(x, s):
        return evaluate.spearman(torch.tensor(x, dtype=torch.float32, device=DEV),
                                 torch.tensor(s, dtype=torch.float32, device=DEV))[0].item()

    x, s = _spearman_inputs(65, 7)
    assert np.isnan(rho(x, np.full(65, 0.25, np.float32)))            # one constant array
    assert np.isnan(rho([1.0, float("nan")], [2.0, 3.0]))             # fewer than two finite pairs
    assert np.isnan(rho([float("inf"), 1.0, 2.0], [2.0, float("nan"), 3.0]))
    assert np.isnan(rho([], []))
    assert abs(rho([1.0, 2.0, 3.0], [3.0, 2.0, 1.0]) + 1.0) <= 1e-12


def test_two_epochs_are_bitwise_equal(gold):
    heads, y, tf, _ = _case(gold, "tf")
    runs = []
    for _ in range(2):
        em = _epoch(_metrics(gold, tf), heads, y, gold["a/batch_sizes"])
        out = em.result(25)
        runs.append((_bits(em.state), np.asarray(out).view(np.int64), _bits(em.err_buf[:50]), _bits(em.sig_buf[:50])))
    for a, b in zip(*runs):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    em.reset()
    out = _epoch(em, heads, y, gold["a/batch_sizes"]).result(25)   # reset() starts the same epoch again
    assert np.array_equal(np.asarray(out).view(np.int64), runs[0][1])


def test_state_and_per_batch_ece(gold):
    """The five batches against the restatement: every entry of the state block, and the ECE of the
    reference (per batch, a ragged last batch weighing as much as a full one), which on this fixture
    differs from the ECE of hits pooled over the epoch."""
    from alignn_mi355x import evaluate as E
    heads, y, tf, _ = _case(gold, "tf")
    sizes = gold["a/batch_sizes"]
    em = _epoch(_metrics(gold, tf), heads, y, sizes)
    r = _restate(gold, heads, y, sizes, tf, True, 25)
    ece = em.result(25)[8]
    st = em.state.cpu().numpy()
    for idx, key in ((E.S_GRAPHS, "graphs"), (E.S_LV_COUNT, "lv_count"), (E.S_COV_HITS, "hits"), (E.S_ELEMS, "elems"),
                     (E.S_ECE_TERMS, "ece_terms")):
        assert st[idx] == r[key], key
    assert st[E.S_CURSOR] == 50 and st[E.S_BAD] == 0 and em.elements == 50
    for idx, key in ((E.S_LOSS, "loss"), (E.S_LV_SUM, "lv_sum"), (E.S_ABS, "abs"), (E.S_SQ, "sq"), (E.S_LOGABS, "logabs")):
        assert abs(st[idx] - r[key]) <= 1e-4 * abs(r[key]), key
    assert abs(st[E.S_SIGMA_MAX] - r["sigma_max"]) <= 1e-5 * r["sigma_max"]
    # |mean - y_z| cancels, so its bound is absolute: logf within 2 ulp, the subtraction of m, the
    # division by s and mean - y_z within half an ulp each, all at the magnitude of log y and scaled
    # by 1/s: 4 ulp(|log y| / s), doubled
    err_tol = 8 * 2.0 ** -24 * float(np.abs(np.log(y.astype(np.float64))).max()) / float(np.min(tf[1]))
    assert np.abs(em.err_buf[:50].cpu().numpy() - r["err"]).max() <= err_tol
    assert np.allclose(em.sig_buf[:50].cpu().numpy(), r["sig"], rtol=1e-5, atol=0)
    print(f"ece got {ece!r} per-batch {r['out'][8]!r} pooled {r['ece_pooled']!r}")
    assert abs(r["ece_pooled"] - r["out"][8]) > 1e-3
    assert abs(ece - r["out"][8]) <= 1e-6


def test_update_is_capturable_no_host_reads(gold):
    """One update on a batch of 7 captured with torch.cuda.graph (a synchronizing call or a host
    read would make the capture raise), replayed for the three 7-graph batches through its static
    inputs: the state is bitwise that of three eager updates."""
    heads, y, tf, _ = _case(gold, "tf")
    h = torch.from_numpy(heads).to(DEV)
    t = torch.from_numpy(np.ascontiguousarray(y)).to(DEV)
    eager = _metrics(gold, tf, capacity=64)
    for i in range(3):
        eager.update(h[7 * i:7 * i + 7], t[7 * i:7 * i + 7])
    em = _metrics(gold, tf, capacity=64)
    hs, ts = h[:7].clone(), t[:7].clone()
    em.update(hs, ts)  # the kernel's code object is loaded before the capture
    em.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        em.update(hs, ts)
    for i in range(3):
        hs.copy_(h[7 * i:7 * i + 7])
        ts.copy_(t[7 * i:7 * i + 7])
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(em.state), _bits(eager.state))
    assert torch.equal(em.err_buf[:42], eager.err_buf[:42]) and torch.equal(em.sig_buf[:42], eager.sig_buf[:42])
    assert float(em.state[13].item()) == 42.0


def test_buffer_growth(gold):
    heads, y, tf, _ = _case(gold, "tf")
    sizes = gold["a/batch_sizes"]
    small = _epoch(_metrics(gold, tf, capacity=4), heads, y, sizes)
    assert small.capacity >= 50
    big = _epoch(_metrics(gold, tf, capacity=4096), heads, y, sizes)
    assert np.array_equal(np.asarray(small.result(25)).view(np.int64), np.asarray(big.result(25)).view(np.int64))
    assert torch.equal(small.err_buf[:50], big.err_buf[:50])


def test_non_positive_target_raises_at_result(gold):
    heads, y, tf, _ = _case(gold, "tf")
    y = y.copy()
    y[9, 1] = 0.0
    y[20, 0] = -1.0
    em = _epoch(_metrics(gold, tf), heads, y, gold["a/batch_sizes"])   # update does not raise
    with pytest.raises(ValueError, match="Log transform encountered non-positive targets."):
        em.result(25)
    assert float(em.state[12].item()) == 2.0
    # without a transformer the target is used as it is: nothing to raise
    _epoch(_metrics(gold, None, False), heads, y, gold["a/batch_sizes"]).result(25)


def test_padded_batch_passes_real_rows_only(gold):
    heads, y, tf, _ = _case(gold, "tf")
    h = torch.from_numpy(heads).to(DEV)
    t = torch.from_numpy(np.ascontiguousarray(y)).to(DEV)
    padded, exact = _metrics(gold, tf), _metrics(gold, tf)
    padded.update(h[:7], t[:7], real_graphs=5)
    exact.update(h[:5], t[:5])
    assert torch.equal(_bits(padded.state), _bits(exact.state))
    before = _bits(padded.state)
    padded.update(h[:7], t[:7], real_graphs=0)   # B == 0 is a no-op
    assert torch.equal(_bits(padded.state), before)
    assert np.array_equal(np.asarray(padded.result(5)).view(np.int64), np.asarray(exact.result(5)).view(np.int64))
