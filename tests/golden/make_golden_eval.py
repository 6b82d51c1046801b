"""Golden vectors for the device-side validation epoch, written by the reference's own
``eval_epoch_hetero`` (scripts/train.py:726-846) on the CPU (build container only; PyG replaced by
``oracle/torch_geometric`` as in ``make_golden.py``; SciPy installed, so Spearman is computed).

(a) Metric cases: a stub model returns stored heads, so the metric path is pinned apart from the
    network.  Batches of 7, 7, 7, 3 and 1 graphs, T = 2, about a fifth of the logvars under the
    floor (tied sigma), ``loader.dataset`` of length 25.  Cases: ``tf`` (with transformer),
    ``notf`` (no transformer, ``compute_log_mae=False``; its own targets, drawn around the means),
    ``nan`` (``tf`` with one mean set to NaN).
(b) One model case: a ``HeteroAlignnRegressor`` member of ``ensemble.npz`` (hidden 64, 2 layers,
    4 heads; the first member whose heads keep the margins below, recorded as ``b/member``) over
    that file's two batches of 3 MP-like graphs, ``loader.dataset`` of length 6.  Weights and
    inputs are read from ``ensemble.npz`` by the tests; this generator rebuilds them and asserts
    they are the same.

Margins asserted on every finite case (the seed is advanced until they hold), so that fp32
arithmetic differences of 1e-4 cannot flip a count or a rank:
  * every |d| is at least 1e-3 relative away from sigma and from each z_l * sigma,
  * sorted |d| values differ pairwise by more than 1e-3 relative,
  * distinct max(sigma, 1e-6) values differ by more than 1e-3 relative.

Output: ``tests/golden/eval.npz`` (allow_pickle=False, arrays only).

Run:  python tests/golden/make_golden_eval.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REFERENCE = "/root/reference"
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))  # shim torch_geometric
sys.path.insert(0, os.path.join(REPO, "gnn-elasticity-predictor_amd"))
sys.path.insert(0, REFERENCE)

import scripts.train as ref  # noqa: E402  (the reference, through the shim)
from torch_geometric.data import Batch as ShimBatch, Data as ShimData  # noqa: E402

from alignn_mi355x.synthetic import TARGET_LOG_MEANS, TARGET_LOG_STDS, mp_like_graph  # noqa: E402

INPUT_KEYS = ("x", "edge_index", "edge_attr", "lg_edge_index", "lg_edge_attr", "global_x", "sg_one_hot", "y")
DIMS = dict(node=206, edge=36, angle=11, glob=289, hidden=64, layers=2, heads=4)
SEEDS = (11, 12, 13)  # make_golden_ensemble.py
BATCH_SIZES = (7, 7, 7, 3, 1)
T = 2
MARGIN = 1e-3
NAN_AT = (9, 1)  # second batch, third graph, second target


class StubModel(torch.nn.Module):
    def forward(self, batch):
        return batch.heads[:, :T], batch.heads[:, T:]


class Loader:
    def __init__(self, batches, dataset_size):
        self.batches, self.dataset = batches, list(range(dataset_size))

    def __iter__(self):
        return iter(self.batches)


def levels():
    p = torch.linspace(0.1, 0.9, steps=9, dtype=torch.float32)  # train.py:796-801
    normal = torch.distributions.Normal(torch.tensor(0.0, dtype=torch.float32), torch.tensor(1.0, dtype=torch.float32))
    return p, normal.icdf((1.0 + p) / 2.0)


def margins_ok(heads, y, transformer, floor):
    """The three margin conditions on the finite elements of one case."""
    heads, y = torch.as_tensor(heads), torch.as_tensor(y)
    yz = transformer.transform_tensor(y) if transformer is not None else y
    mean, lv = heads[:, :T], torch.clamp(heads[:, T:], min=floor)
    sigma = torch.sqrt(torch.exp(lv)).double().numpy().ravel()
    d = (mean - yz).abs().double().numpy().ravel()
    ok = np.isfinite(d) & np.isfinite(sigma)
    d, sigma = d[ok], sigma[ok]
    z = np.concatenate([[1.0], levels()[1].double().numpy()])
    thr = z[:, None] * sigma[None, :]
    if np.any(np.abs(d[None, :] - thr) < MARGIN * np.maximum(d[None, :], thr)):
        return False
    ds = np.sort(d)
    if np.any(np.diff(ds) <= MARGIN * ds[1:]):
        return False
    su = np.unique(np.maximum(sigma, 1e-6))
    return not np.any(np.diff(su) <= MARGIN * su[1:])


def draw(seed, floor, log_means, log_stds):
    rng = np.random.RandomState(seed)
    n = sum(BATCH_SIZES)
    mean = rng.standard_normal((n, T))
    logvar = rng.uniform(-3.6, 0.0, (n, T))  # 0.7 / 3.6 of them under the floor of -2.9
    sigma = np.sqrt(np.exp(np.maximum(logvar, floor)))
    yz = mean + 1.2 * sigma * rng.standard_normal((n, T))
    heads = np.concatenate([mean, logvar], 1).astype(np.float32)
    y = np.exp(yz * np.asarray(log_stds)[None] + np.asarray(log_means)[None]).astype(np.float32)
    y_notf = (mean + 1.2 * sigma * rng.standard_normal((n, T))).astype(np.float32)
    return heads, y, y_notf


def metric_batches(heads, y):
    out, r = [], 0
    for b in BATCH_SIZES:
        d = ShimData(heads=torch.from_numpy(heads[r:r + b].copy()), y=torch.from_numpy(y[r:r + b].copy()))
        d.num_graphs = b
        out.append(d)
        r += b
    return out


def main():
    torch.set_default_dtype(torch.float32)
    assert ref.spearmanr_fn is not None, "SciPy is needed: the reference skips Spearman without it"
    floor = float(ref.MIN_LOGVAR_FLOOR)
    transformer = ref.LogTransformer().load_state_dict(
        {"means": np.asarray(TARGET_LOG_MEANS), "stds": np.asarray(TARGET_LOG_STDS)})
    cpu = torch.device("cpu")
    arrays = {}

    # (a) metric cases
    seed = 0
    while True:
        heads, y, y_notf = draw(seed, floor, TARGET_LOG_MEANS, TARGET_LOG_STDS)
        if margins_ok(heads, y, transformer, floor) and margins_ok(heads, y_notf, None, floor):
            break
        seed += 1
    frac = float((heads[:, T:] < floor).mean())
    assert 0.1 < frac < 0.3, frac
    heads_nan = heads.copy()
    heads_nan[NAN_AT] = np.nan
    assert margins_ok(heads_nan, y, transformer, floor)
    n = sum(BATCH_SIZES)
    stub = StubModel()
    out_tf = ref.eval_epoch_hetero(stub, Loader(metric_batches(heads, y), n), cpu, transformer=transformer)
    out_notf = ref.eval_epoch_hetero(stub, Loader(metric_batches(heads, y_notf), n), cpu, transformer=None,
                                     compute_log_mae=False)
    out_nan = ref.eval_epoch_hetero(stub, Loader(metric_batches(heads_nan, y), n), cpu, transformer=transformer)
    # the behaviour the tests rely on: the four error sums NaN, the pair masked, the rest finite
    assert all(np.isnan(out_nan[i]) for i in (0, 1, 2, 3)) and all(np.isfinite(out_nan[i]) for i in (4, 5, 6, 7, 8))
    assert all(np.isfinite(v) for v in out_tf) and np.isnan(out_notf[2])
    arrays.update({"a/heads": heads, "a/y": y, "a/y_notf": y_notf, "a/nan_at": np.asarray(NAN_AT),
                   "a/tf/out": np.asarray(out_tf, dtype=np.float64), "a/notf/out": np.asarray(out_notf, dtype=np.float64),
                   "a/nan/out": np.asarray(out_nan, dtype=np.float64), "a/seed": np.asarray(seed),
                   "a/batch_sizes": np.asarray(BATCH_SIZES), "a/dataset_size": np.asarray(n)})

    # (b) model case: a member and the batches of ensemble.npz
    ens = np.load(os.path.join(HERE, "ensemble.npz"))
    batches = []
    for bi in range(2):
        gs = [mp_like_graph(100 + 3 * bi + g) for g in range(3)]
        bt = ShimBatch.from_data_list([ShimData(**{k: getattr(d, k) for k in INPUT_KEYS}) for d in gs])
        for k in INPUT_KEYS + ("batch", "ptr"):
            assert np.array_equal(getattr(bt, k).numpy(), ens[f"in/b{bi}/{k}"]), k
        batches.append(bt)
    yb = torch.cat([bt.y.view(bt.num_graphs, -1) for bt in batches]).numpy()
    for member, member_seed in enumerate(SEEDS):  # the first member whose heads keep the margins
        torch.manual_seed(member_seed)
        base = ref.AlignnRegressor(DIMS["node"], DIMS["edge"], DIMS["angle"], DIMS["glob"], 2, DIMS["hidden"],
                                   DIMS["layers"], DIMS["heads"], 0.15)
        model = ref.HeteroAlignnRegressor(base, 2)
        for k, v in model.state_dict().items():
            assert np.array_equal(v.detach().float().numpy(), ens[f"m{member}/{k}"]), k
        model.eval()
        with torch.no_grad():
            hb = torch.cat([torch.cat(model(bt), 1) for bt in batches]).numpy()
        if margins_ok(hb, yb, transformer, floor):
            break
    else:
        raise AssertionError("no member of ensemble.npz keeps the margins")
    out_b = ref.eval_epoch_hetero(model, Loader(batches, 6), cpu, transformer=transformer)
    assert all(np.isfinite(v) for v in out_b)
    arrays.update({"b/out": np.asarray(out_b, dtype=np.float64), "b/heads": hb, "b/y": yb,
                   "b/dataset_size": np.asarray(6), "b/member": np.asarray(member)})

    p, z = levels()
    arrays["meta/prob_levels"], arrays["meta/z_thresholds"] = p.numpy(), z.numpy()
    arrays["meta/target_log_means"] = np.asarray(TARGET_LOG_MEANS)
    arrays["meta/target_log_stds"] = np.asarray(TARGET_LOG_STDS)
    arrays["meta/min_logvar_floor"] = np.asarray(floor)
    arrays["meta/margin"] = np.asarray(MARGIN)
    path = os.path.join(HERE, "eval.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {len(arrays)} arrays; seed {seed}, {frac:.2f} of logvars under the floor")
    for name, o in (("tf", out_tf), ("notf", out_notf), ("nan", out_nan), ("model", out_b)):
        print(name, " ".join(f"{v:.6g}" for v in o))


if __name__ == "__main__":
    main()
