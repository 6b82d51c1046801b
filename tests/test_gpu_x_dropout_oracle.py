"""Dropout-on training (p = 0.15, the rate of every real run and of the benchmarked configuration)
against the fp64 oracle with the engine's own masks reproduced on the host.

The kernels draw no random numbers: a dropout element is kept iff hash_u32(site seed, element index)
>= p * 2^32 (csrc/common.h).  tests/_dropout_ref.py restates that hash, the per-site seeds and each
site's element index ("dropout sites and mask indices") and hands the masks to the oracle
through its ``dropout_fn`` hook — so the mask's place (after the ReLU), its scale 1/(1-p), its reach
(alpha AND the edge-feature aggregate S, every readout column) and the index each backward re-draws
it under are all compared with an independent fp64 statement of the reference model, at the
project's usual 1e-4 (tests/test_gpu_parity.py).

Subjects: the module API under autograd (its step seed is model._next_seed's draw from torch's CPU
generator, restated here) and FusedTrainer's eager step with an explicit seed.  The replayed plan is
not repeated here: tests/test_gpu_x_round6.py::test_replayed_step_host_reads_equal_eager already
ties it bitwise (loss, flat gradient, parameters) to the eager step at dropout 0.15, B = 4 and 32.

Tolerance: the parity suite's — forward and loss 1e-4 relative, each parameter's normwise gradient
error below max(1e-4, 1.5 x the error of the oracle run in fp32 under the same masks) with the
GRAD_FLOOR denominator floor (which is what handles lin_key.bias, zero in exact arithmetic), max-abs
below 5e-3.  Measured figures: DESIGN.md §"dropout sites and mask indices"."""
import copy

import numpy as np
import pytest
import torch

import _dropout_ref as dr
from _golden_util import grad_norm_scale, meta, norm_err, rel_err, state_from
from oracle import model_ref
from test_gpu_parity import GRAD_FLOOR, MAXABS_TOL, TOL, _ref_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
P_DROP = 0.15
LOG_MEANS, LOG_STDS = (4.3228, 3.5567), (0.9051, 0.9405)
PROD = dict(node=206, edge=36, angle=11, glob=289, hidden=256, layers=4, heads=4)

# name: (reference case, attention policy).  quirk: the PyG offset rule — bonds without line-graph
# in-edges, so the compacted line-graph CSR and the gate's outp_rows = -1 rows are exercised.
CASES = {
    "prod_quirk_b2": ("prod_quirk_b2", None),
    "prod_fixed_b3": ("prod_fixed_b3", None),
    "prod_quirk_b2_light_heavy": ("prod_quirk_b2", dict(wave_items=False)),   # tconv.hip carries the line graph too
    "d64_quirk_b2": ("d64_quirk_b2", None),
}
_REF = {}


def _drawn_seed(k):
    """model._next_seed() right after torch.manual_seed(k): the module API's step seed."""
    torch.manual_seed(k)
    return int(torch.randint(0, 2 ** 62, (1,)).item())


def _model(arch, dropout):
    import alignn_mi355x as A
    base = A.AlignnRegressor(arch["node"], arch["edge"], arch["angle"], arch["glob"], 2, arch["hidden"],
                             arch["layers"], arch["heads"], dropout)
    return A.HeteroAlignnRegressor(base, 2)


def _oracle(st, ref_b, heads, dropout_fn, grads=True):
    params = {k: v.clone().requires_grad_(grads) for k, v in st.items()}
    mean, logvar = model_ref.hetero_forward(params, ref_b, heads, dropout_fn=dropout_fn)
    if not grads:
        return mean.detach(), logvar.detach(), None, None
    tz = model_ref.log_transform(ref_b.y.view(ref_b.num_graphs, -1), LOG_MEANS, LOG_STDS)
    loss = model_ref.hetero_loss(mean, logvar, tz, 0.1)
    loss.backward()
    return mean.detach(), logvar.detach(), loss.detach(), {k: v.grad for k, v in params.items() if v.grad is not None}


def _reference(name, golden):
    """Weights, batch, step seed and the fp64 oracle's forward / loss / gradients under the engine's
    masks, computed once per reference case and left unchanged."""
    if name in _REF:
        return _REF[name]
    from alignn_mi355x.synthetic import mp_like_batch
    if name == "d64_quirk_b2":
        g = golden("mp_d64_quirk")
        m = meta(g)
        arch = dict(node=int(m["node"]), edge=int(m["edge"]), angle=int(m["angle"]), glob=int(m["global"]),
                    hidden=int(m["hidden"]), layers=int(m["layers"]), heads=int(m["heads"]))
        st = state_from(g, dtype=torch.float32)
        B, lg_offset, k = 2, "num_nodes", 13
    else:
        arch = PROD
        B, lg_offset, k = (2, "num_nodes", 11) if name == "prod_quirk_b2" else (3, "num_edges", 12)
        torch.manual_seed(5)
        st = {kk: v.detach().clone() for kk, v in _model(arch, P_DROP).state_dict().items()}
    cpu_batch = mp_like_batch(B, lg_offset=lg_offset)
    seed = _drawn_seed(k)
    H, L = arch["heads"], arch["layers"]
    b64 = _ref_batch(cpu_batch, B, torch.float64)
    fn = dr.OracleDropout(seed, P_DROP, b64, H, L)
    ref = _oracle({kk: v.double() for kk, v in st.items()}, b64, H, fn)
    # the parity suite's rule: never stricter than the reference's own fp32 path under the same masks
    b32 = _ref_batch(cpu_batch, B, torch.float32)
    g32 = _oracle({kk: v.float() for kk, v in st.items()}, b32, H, dr.OracleDropout(seed, P_DROP, b32, H, L))[3]
    nfloor = GRAD_FLOOR * grad_norm_scale(ref[3].values())
    err32 = {kk: norm_err(g32[kk], ref[3][kk], nfloor) for kk in ref[3]}
    tols = {kk: max(TOL, 1.5 * e) for kk, e in err32.items()}
    _REF[name] = dict(arch=arch, st=st, batch=cpu_batch, B=B, k=k, seed=seed, ref=ref, stats=dict(fn.stats),
                      tols=tols, err32=err32, b64=b64)
    return _REF[name]


def _loss(mean, logvar, b, B):
    y = b.y.view(B, -1)
    tz = (torch.log(y) - torch.tensor(LOG_MEANS, device=DEV)) / torch.tensor(LOG_STDS, device=DEV)
    lv = torch.clamp(logvar, min=-2.9)
    return (0.5 * (lv + (mean - tz) ** 2 / torch.exp(lv))).mean(1).mean() + 0.1 * (0.5 * lv).pow(2).mean()


def _check_grads(tag, named_grads, rgrads, tols, min_params):
    floor = GRAD_FLOOR * max(float(v.abs().max()) for v in rgrads.values())
    nfloor = GRAD_FLOOR * grad_norm_scale(rgrads.values())
    worst, worst_abs, n = (0.0, None), 0.0, 0
    fails = []
    for k, gr in named_grads:
        if k not in rgrads:
            assert gr is None or float(gr.abs().max()) == 0.0, k
            continue
        assert gr is not None, k
        e, ea = norm_err(gr, rgrads[k], nfloor), rel_err(gr.cpu(), rgrads[k], floor)
        if e > worst[0]:
            worst = (e, k)
        worst_abs = max(worst_abs, ea)
        if not (e < tols[k] and ea < MAXABS_TOL):
            fails.append((k, e, tols[k], ea))
        n += 1
    print(f"[dropout-oracle] {tag}: worst normwise grad err {worst[0]:.3e} ({worst[1]}), "
          f"worst max-abs {worst_abs:.3e}, {n} parameters")
    assert not fails, fails
    assert n >= min_params


def _device_batch(c, policy, monkeypatch):
    from alignn_mi355x import ops
    if policy is not None:
        monkeypatch.setattr(ops, "DEFAULT_SCHEDULE", ops.SchedulePolicy(**policy))
    return copy.copy(c["batch"]).to(DEV)   # (Batch.to moves in place: the cached batch stays on the host)


def _min_params(arch):
    return 25 * arch["layers"]


@pytest.mark.parametrize("case", list(CASES))
def test_mask_order_and_guards(case, golden, monkeypatch):
    """What the comparison below rests on.  (a) The edge order the attention masks are indexed in: the
    host's stable sort by target equals GraphCSR.perm_dst on both graphs — for the compacted line
    graph through rows / cmap (its targets are renumbered monotonically).  (b) The masks are not
    vacuous: every site of 500+ elements drops a fraction in [0.10, 0.20], and the masked oracle's
    mean differs from the unmasked one by more than 0.1 relative."""
    from alignn_mi355x.engine import batch_cache
    refname, policy = CASES[case]
    c = _reference(refname, golden)
    b = _device_batch(c, policy, monkeypatch)
    bc = batch_cache(b)
    if policy is not None:
        assert bc.lg.policy.wave_items is False and bc.ag.policy.wave_items is False
    for g, ei in ((bc.ag, c["batch"].edge_index), (bc.lg, c["batch"].lg_edge_index)):
        m = ei.size(1)
        perm = torch.argsort(ei[1], stable=True)
        assert torch.equal(g.perm_dst[:m].long().cpu(), perm)
        src_at, dst_at = g.src_at[:m].long().cpu(), g.dst_at[:m].long().cpu()
        if g.rows is not None:
            rows, cmap = g.rows.long().cpu(), g.cmap.long().cpu()
            assert bool((rows[1:] > rows[:-1]).all())               # monotone renumbering
            assert torch.equal(cmap[rows], torch.arange(rows.numel()))
            assert int((cmap < 0).sum()) == g.n_full - rows.numel() > 0
            src_at, dst_at = rows[src_at], rows[dst_at]
        assert torch.equal(dst_at, ei[1][perm]) and torch.equal(src_at, ei[0][perm])
    if "quirk" in case:
        assert bc.lg.rows is not None   # the compacted CSR and the gate's outp_rows = -1 rows are exercised
    L = c["arch"]["layers"]
    assert sorted(c["stats"]) == list(range(4 * L + 2))
    big = 0
    for site, (numel, frac) in c["stats"].items():
        if numel >= 500:
            assert 0.10 <= frac <= 0.20, (site, numel, frac)
            big += 1
    assert big >= 4 * L + 1
    if case == refname:
        st64 = {k: v.double() for k, v in c["st"].items()}
        m0 = _oracle(st64, c["b64"], c["arch"]["heads"], None, grads=False)[0]
        moved = rel_err(c["ref"][0], m0)
        print(f"[dropout-oracle] {case}: masks move the oracle's mean by {moved:.3f} relative")
        assert moved > 0.1


def test_wrong_convention_at_one_site_moves_the_oracle(golden):
    """The comparison can see a fault confined to one site: with one attention site's and one gate
    site's mask rows reversed, some parameter gradient of the oracle moves by more than 1e-2."""
    c = _reference("prod_quirk_b2", golden)
    arch = c["arch"]
    st64 = {k: v.double() for k, v in c["st"].items()}
    rg = c["ref"][3]
    nfloor = GRAD_FLOOR * grad_norm_scale(rg.values())
    for site in (4 * 1 + 2, 4 * 2 + 1):   # atom-graph attention of layer 1, line-graph gate of layer 2
        fn = dr.OracleDropout(c["seed"], P_DROP, c["b64"], arch["heads"], arch["layers"], flip=site)
        g = _oracle(st64, c["b64"], arch["heads"], fn)[3]
        moved = max(norm_err(g[k], rg[k], nfloor) for k in rg)
        print(f"[dropout-oracle] site {site} reversed: largest gradient move {moved:.3e}")
        assert moved > 1e-2, (site, moved)


@pytest.mark.parametrize("case", list(CASES))
def test_module_autograd_dropout_vs_oracle(case, golden, monkeypatch):
    refname, policy = CASES[case]
    c = _reference(refname, golden)
    rmean, rlogvar, rloss, rgrads = c["ref"]
    model = _model(c["arch"], P_DROP)
    model.load_state_dict(c["st"])
    model.to(DEV).train()
    b = _device_batch(c, policy, monkeypatch)
    assert _drawn_seed(c["k"]) == c["seed"]
    torch.manual_seed(c["k"])            # _next_seed draws the step seed from this generator
    mean, logvar = model(b)
    e_mean, e_lv = rel_err(mean.detach().cpu(), rmean), rel_err(logvar.detach().cpu(), rlogvar)
    loss = _loss(mean, logvar, b, c["B"])
    e_loss = abs(float(loss) - float(rloss)) / abs(float(rloss))
    print(f"[dropout-oracle] module {case}: forward err mean {e_mean:.3e} logvar {e_lv:.3e} loss {e_loss:.3e}; "
          f"fp32-oracle worst grad err {max(c['err32'].values()):.3e}")
    assert e_mean < TOL and e_lv < TOL
    assert e_loss < TOL
    loss.backward()
    _check_grads(f"module {case}", ((k, p.grad) for k, p in model.named_parameters()), rgrads, c["tols"],
                 _min_params(c["arch"]))


@pytest.mark.parametrize("case", list(CASES))
def test_fused_eager_step_dropout_vs_oracle(case, golden, monkeypatch):
    """FusedTrainer's eager step with an explicit seed: its loss, and its flat gradient — clipped in
    place by the step — against the oracle's gradient times torch's clip coefficient."""
    from alignn_mi355x import FusedTrainer
    from alignn_mi355x.layout import offsets
    refname, policy = CASES[case]
    c = _reference(refname, golden)
    rmean, rlogvar, rloss, rgrads = c["ref"]
    model = _model(c["arch"], P_DROP)
    model.load_state_dict(c["st"])
    model.to(DEV).train()
    b = _device_batch(c, policy, monkeypatch)
    tr = FusedTrainer(model, feature_jitter_std=0.0, target_log_means=LOG_MEANS, target_log_stds=LOG_STDS)
    loss = tr.step(b, seed=c["seed"])
    torch.cuda.synchronize()
    e_loss = abs(float(loss) - float(rloss)) / abs(float(rloss))
    print(f"[dropout-oracle] fused {case}: loss err {e_loss:.3e}")
    assert e_loss < TOL
    offs, _, _ = offsets(model.config, True)
    total = float(torch.sqrt(sum((v.double() ** 2).sum() for v in rgrads.values())))
    coef = min(1.0, 5.0 / (total + 1e-6))
    grads = [(k, tr.st.grad[o:o + int(np.prod(shape))].view(shape)) for k, (o, shape) in offs.items()]
    _check_grads(f"fused {case}", grads, {k: v * coef for k, v in rgrads.items()}, c["tols"],
                 _min_params(c["arch"]))
