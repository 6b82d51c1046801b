"""The row-wise kernels of csrc/rowops.hip against float64 PyTorch restatements, at dropout 0 and
0.15 with the masks reproduced on the host (tests/_dropout_ref.py):

* ``dropout`` (+ ``relu_ref``): pins the host restatement of hash_u32 / the threshold / the scale to
  the kernels — exact equality;
* ``gate_ln_fwd`` / ``gate_ln_bwd``:  beta = sigmoid(w . [o, r, o - r]),  y = beta r + (1 - beta) o,
  Xnew = X + mask * relu(LayerNorm(y)) / (1 - p)  (eps 1e-5), every output of both kernels against
  autograd on that formula;
* ``readout_feats_fwd`` / ``readout_pool_bwd``: mean pool | global_x | sg, dropout over all columns.

Tolerance: max-abs error below 2e-5 of each output's max (``_rel``, as the attention kernel tests).
The ReLU kink would make that ill-posed (an fp32 LayerNorm output on the other side of zero than
the fp64 one flips a whole gradient term), so each case's input seed is chosen — on the CPU, from the
fp64 reference alone — such that no LayerNorm output lies within 2e-6 of zero, and that is asserted."""
import numpy as np
import pytest
import torch

import _dropout_ref as dr
from test_gpu_x_pending import _rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 2e-5
KINK = 2e-6


def _ops():
    from alignn_mi355x import ops
    ops.set_step_seed(None)   # host seeds only: the masks are those of _dropout_ref
    return ops


# ------------------------------------------------------------------------------------------------
# dropout kernel == host restatement, exactly
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.15, 0.5])
@pytest.mark.parametrize("shape,strided", [((7, 5), False), ((1, 1), False), ((300, 257), False), ((37, 19), True)])
def test_dropout_kernel_equals_host_masks(shape, strided, p):
    ops = _ops()
    r, c = shape
    seed = dr.site_seed(1234567, 17)
    keep = torch.from_numpy(dr.keep_mask(seed, r * c, p).reshape(r, c))
    mul = keep.float() * float(np.float32(dr.inv_keep(p)))
    assert abs(dr.inv_keep(p) * (1.0 - p) - 1.0) < 2e-7          # the kernels' fp32 1/(1-p)
    g = torch.Generator().manual_seed(r * 1000 + c)

    def buf(fill):   # a [r, c] view: contiguous, or a column block of a wider tensor
        if not strided:
            return torch.full((r, c), fill, device=DEV)
        return torch.full((r, c + 11), fill, device=DEV)[:, 3:3 + c]

    x = buf(1.0)
    y = buf(float("nan"))
    ops.dropout(x, y, None, p, seed)
    assert torch.equal(y.cpu(), mul)                               # keep_mask / (1 - p), exactly
    if strided:
        assert bool(torch.isnan(y._base[:, :3]).all()) and bool(torch.isnan(y._base[:, 3 + c:]).all())
    # with relu_ref (the ReLU-mask backward): where(ref > 0, x * mask, 0), exactly
    xv = torch.randn(r, c, generator=g)
    ref = torch.randn(r, c, generator=g)
    ref[0, 0] = 0.0                                                # ref == 0 is not > 0
    x, rf, y = buf(0.0), buf(0.0), buf(float("nan"))
    x.copy_(xv)
    rf.copy_(ref)
    ops.dropout(x, y, rf, p, seed)
    want = torch.where(ref > 0, xv * mul, torch.zeros(()))
    assert torch.equal(y.cpu(), want)
    # p = 0 is the identity (and the ReLU mask alone)
    y0 = buf(float("nan"))
    ops.dropout(x, y0, None, 0.0, seed)
    assert torch.equal(y0.cpu(), xv)


# ------------------------------------------------------------------------------------------------
# gate + LayerNorm + ReLU + dropout + residual
# ------------------------------------------------------------------------------------------------
def _gate_inputs(D, n, seed, compact):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    t = dict(R=r(n, D), X=r(n, D), dXn=r(n, D), add=r(n, D), wbeta=r(3 * D) / (3 * D) ** 0.5,
             lnw=1 + 0.1 * r(D), lnb=0.1 * r(D), pre=[r(3 * D), r(D), r(D)])
    if compact:
        # full row -> compacted conv-output row; -1 (no output row: o = 0) at the first and the last
        # row and at every third one between; the mapped rows in shuffled order, two rows of outp
        # (and of dout) belong to no full row
        rows = torch.full((n,), -1, dtype=torch.int64)
        mapped = torch.tensor([i for i in range(1, n - 1) if i % 3 != 0], dtype=torch.int64)
        na = mapped.numel() + 2
        rows[mapped] = torch.randperm(na, generator=g)[:mapped.numel()]
        t["rows"] = rows
        t["outp"] = r(na, D)
    else:
        t["rows"] = None
        t["outp"] = r(n, D)
    return t


def _gate_ref(t, p, mask, dx_mode, dtype=torch.float64):
    """Autograd on the formula.  dx_mode: the incoming gradient — 'plain' dXn, 'add' dXn + add,
    'zero' add alone."""
    c = lambda k: t[k].to(dtype).clone()  # noqa: E731
    outp, R, X = c("outp").requires_grad_(True), c("R").requires_grad_(True), c("X")
    wb, lnw, lnb = (c(k).requires_grad_(True) for k in ("wbeta", "lnw", "lnb"))
    rows = t["rows"]
    if rows is None:
        o = outp
    else:
        o = torch.where((rows >= 0)[:, None], outp[rows.clamp(min=0)], torch.zeros((), dtype=dtype))
    beta = torch.sigmoid(torch.cat([o, R, o - R], 1) @ wb)
    y = beta[:, None] * R + (1 - beta[:, None]) * o
    mu = y.mean(1)
    rstd = 1.0 / torch.sqrt(((y - mu[:, None]) ** 2).mean(1) + 1e-5)
    ln = (y - mu[:, None]) * rstd[:, None] * lnw + lnb
    a = torch.relu(ln)
    if p > 0:
        a = a * mask.to(dtype) / (1.0 - p)
    Xn = X + a
    gin = {"plain": c("dXn"), "add": c("dXn") + c("add"), "zero": c("add")}[dx_mode]
    (Xn * gin).sum().backward()
    return dict(Xn=Xn.detach(), beta=beta.detach(), mu=mu.detach(), rstd=rstd.detach(), dout=outp.grad, dR=R.grad,
                d_wbeta=wb.grad, d_lnw=lnw.grad, d_lnb=lnb.grad, gin=gin, near_kink=int((ln.detach().abs() < KINK).sum()))


_GATE_CASES = {}
_GATE_INPUTS = {}
# Input seeds chosen on the CPU (the search below, fp64 reference only) so that no LayerNorm output
# lies within KINK of zero; other shapes start at 1000 D + n.  The search re-checks the listed seed.
_SEEDS = {(64, 4097, False): 68098, (64, 4097, True): 68099, (64, 8195, False): 72195, (64, 8195, True): 72195,
          (256, 4097, False): 260109, (256, 4097, True): 260098, (256, 8195, False): 264196,
          (256, 8195, True): 264283}


def _kink_free_inputs(D, n, compact):
    key = (D, n, compact)
    if key not in _GATE_INPUTS:
        first = _SEEDS.get(key, 1000 * D + n)
        for seed in range(first, first + 400):
            t = _gate_inputs(D, n, seed, compact)
            with torch.no_grad():
                o, R = t["outp"].double(), t["R"].double()
                if t["rows"] is not None:
                    o = torch.where((t["rows"] >= 0)[:, None], o[t["rows"].clamp(min=0)], torch.zeros((), dtype=o.dtype))
                beta = torch.sigmoid(torch.cat([o, R, o - R], 1) @ t["wbeta"].double())[:, None]
                y = beta * R + (1 - beta) * o
                ln = torch.nn.functional.layer_norm(y, (D,), t["lnw"].double(), t["lnb"].double(), 1e-5)
            if int((ln.abs() < KINK).sum()) == 0:
                break
        t["seed"] = seed
        _GATE_INPUTS[key] = t
    return _GATE_INPUTS[key]


def _gate_case(D, n, compact, p, dx_mode="plain"):
    """Inputs (kink-free seed), mask and fp64 reference; computed once per case and left unchanged."""
    key = (D, n, compact, p, dx_mode)
    if key not in _GATE_CASES:
        drop_seed = dr.site_seed(99, 4 * (D % 7) + 1)
        mask = dr.dense_mask(drop_seed, n, D, p) if p > 0 else None
        t = _kink_free_inputs(D, n, compact)
        _GATE_CASES[key] = (t, _gate_ref(t, p, mask, dx_mode), drop_seed, mask)
    return _GATE_CASES[key]


def _gate_run(t, p, drop_seed, strided, flat, dx_mode="plain", reduce_stream=None):
    ops = _ops()
    n, D = t["R"].shape
    d = lambda x: x.to(DEV)  # noqa: E731
    if strided:
        # R a column block of the [n, 4D] projection output (as the engine's uncompacted blocks), X,
        # Xnew, dXnew and dR with row strides above D
        R = torch.zeros(n, 4 * D, device=DEV)[:, 3 * D:]
        X = torch.zeros(n, D + 8, device=DEV)[:, :D]
        Xn = torch.full((n, D + 4), float("nan"), device=DEV)[:, :D]
        dXn = torch.zeros(n, D + 12, device=DEV)[:, 4:4 + D]
        dR = torch.full((n, 4 * D), float("nan"), device=DEV)[:, 3 * D:]
    else:
        R, X, dXn = (torch.empty(n, D, device=DEV) for _ in range(3))
        Xn, dR = (torch.full((n, D), float("nan"), device=DEV) for _ in range(2))
    R.copy_(t["R"])
    X.copy_(t["X"])
    if dx_mode == "zero":
        dXn.fill_(float("nan"))       # holds nothing yet: must not be read
    else:
        dXn.copy_(t["dXn"])
    outp, wbeta, lnw, lnb = d(t["outp"]), d(t["wbeta"]), d(t["lnw"]), d(t["lnb"])
    rows = None if t["rows"] is None else d(t["rows"].to(torch.int32))
    beta, mu, rstd = (torch.full((n,), float("nan"), device=DEV) for _ in range(3))
    ops.gate_ln_fwd(outp, R, wbeta, X, lnw, lnb, Xn, beta, mu, rstd, p, drop_seed, outp_rows=rows)
    dout = torch.full_like(outp, float("nan"))
    # the reductions ADD into the parameter gradients: prefilled, the sum is expected
    if flat:   # adjacent in one flat buffer (the flat gradient layout): one 5D-wide reduction
        G = torch.cat(t["pre"]).to(DEV)
        grads = [G[:3 * D], G[3 * D:4 * D], G[4 * D:]]
    else:      # separate tensors: one reduction per slice
        grads = [d(x).clone() for x in t["pre"]]
    kw = {}
    if dx_mode != "plain":
        kw = dict(dX_add=d(t["add"]), dX_zero=dx_mode == "zero")
    ops.gate_ln_bwd(dXn, outp, R, wbeta, lnw, lnb, beta, mu, rstd, dout, dR, *grads, p, drop_seed, outp_rows=rows,
                    reduce_stream=reduce_stream, **kw)
    if reduce_stream is not None:
        torch.cuda.current_stream().wait_stream(reduce_stream)
    torch.cuda.synchronize()
    return dict(Xn=Xn, beta=beta, mu=mu, rstd=rstd, dout=dout, dR=dR, d_wbeta=grads[0], d_lnw=grads[1],
                d_lnb=grads[2], dXn=dXn)


def _gate_check(t, ref, got, tag):
    assert ref["near_kink"] == 0, tag      # the seed search found a case off the ReLU kink
    errs = {}
    for k in ("Xn", "beta", "mu", "rstd", "dR"):
        errs[k] = _rel(got[k].cpu(), ref[k])
    rows = t["rows"]
    if rows is None:
        errs["dout"] = _rel(got["dout"].cpu(), ref["dout"])
    else:
        used = torch.zeros(t["outp"].size(0), dtype=torch.bool)
        used[rows[rows >= 0]] = True
        gd = got["dout"].cpu()
        assert bool(torch.isnan(gd[~used]).all()), tag      # only mapped rows are written
        assert int((~used).sum()) == 2
        errs["dout"] = _rel(gd[used], ref["dout"][used])
        assert float(ref["dout"][~used].abs().max()) == 0.0
    for k, pre in zip(("d_wbeta", "d_lnw", "d_lnb"), t["pre"]):
        errs[k] = _rel(got[k].cpu(), pre.double() + ref[k])
    errs["dXn"] = _rel(got["dXn"].cpu(), ref["gin"])       # the incoming gradient, summed where there is an addend
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, (tag, bad, errs)
    return errs


SMALL = [(D, n) for D in (32, 64, 128, 256, 512) for n in (1, 5)]
LARGE = [(D, n) for D in (64, 256) for n in (4097, 8195)]


@pytest.mark.parametrize("p", [0.0, 0.15])
@pytest.mark.parametrize("variant", ["plain", "strided_compact_flat"])
@pytest.mark.parametrize("D,n", SMALL + LARGE)
def test_gate_ln_fwd_bwd_vs_fp64(D, n, variant, p):
    """D: VPL 1 with half the lanes idle (32), then VPL 1, 2, 4, 8.  n: fewer rows than one
    workgroup; the backward's paired-row walk with a clamped second row; a third trip of its loop
    (ALIGNN_GATE_BWD_WAVES = 4096); a last workgroup that is not full.  plain: contiguous operands,
    every row with an output row, the parameter gradients in separate tensors.
    strided_compact_flat: R a column block of [n, 4D], X / Xnew / dXnew / dR with row strides above D,
    outp_rows with -1 entries (first and last row included; dout NaN-prefilled, compacted), the
    parameter gradients adjacent in one flat buffer.  Both reductions accumulate (prefilled)."""
    full = variant != "plain"
    compact = full and n >= 3
    t, ref, drop_seed, _ = _gate_case(D, n, compact, p)
    got = _gate_run(t, p, drop_seed, strided=full, flat=full)
    _gate_check(t, ref, got, (D, n, variant, p))


def test_gate_ln_first_and_last_row_without_output_row():
    """The compacted case's -1 rows really include the first and the last row, and those rows'
    new state is the o = 0 formula's (their own check, beside the max-norm one above)."""
    D, n, p = 256, 4097, 0.15
    t, ref, drop_seed, _ = _gate_case(D, n, True, p)
    assert int(t["rows"][0]) == -1 and int(t["rows"][-1]) == -1 and int((t["rows"] >= 0).sum()) > n // 2
    got = _gate_run(t, p, drop_seed, strided=True, flat=True)
    for r in (0, n - 1):
        assert _rel(got["Xn"][r].cpu(), ref["Xn"][r]) < TOL
        assert _rel(got["dR"][r].cpu(), ref["dR"][r]) < TOL


@pytest.mark.parametrize("dx_mode", ["add", "zero"])
@pytest.mark.parametrize("D,n,compact", [(256, 4097, True), (64, 5, False)])
def test_gate_ln_bwd_dx_add_vs_fp64(D, n, compact, dx_mode):
    """An fp32 addend of the incoming gradient (the atom block's edge-feature gradient): dXnew +
    dX_add, and with dX_zero dX_add alone — dXnew NaN-filled, so a read of it shows — against the
    reference with that incoming gradient (not against another variant); the sum is written back."""
    p = 0.15
    t, ref, drop_seed, _ = _gate_case(D, n, compact, p, dx_mode)
    got = _gate_run(t, p, drop_seed, strided=compact, flat=True, dx_mode=dx_mode)
    _gate_check(t, ref, got, (D, n, dx_mode))


def test_gate_ln_bwd_reduce_stream_vs_fp64():
    """The parameter-gradient reduction on another stream."""
    D, n, p = 256, 4097, 0.15
    t, ref, drop_seed, _ = _gate_case(D, n, True, p)
    got = _gate_run(t, p, drop_seed, strided=True, flat=True, reduce_stream=torch.cuda.Stream())
    _gate_check(t, ref, got, "reduce_stream")


def test_gate_ln_refuses_unsupported_hidden():
    from alignn_mi355x._lib import AlignnHipError
    ops = _ops()
    n, D = 4, 96
    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    sc = [z(n) for _ in range(3)]
    with pytest.raises(AlignnHipError, match="unsupported hidden"):
        ops.gate_ln_fwd(z(n, D), z(n, D), z(3 * D), z(n, D), z(D), z(D), z(n, D), *sc, 0.0, 1)
    with pytest.raises(AlignnHipError, match="unsupported hidden"):
        ops.gate_ln_bwd(z(n, D), z(n, D), z(n, D), z(3 * D), z(D), z(D), *sc, z(n, D), z(n, D), z(3 * D), z(D), z(D),
                        0.0, 1)


# ------------------------------------------------------------------------------------------------
# readout: mean pool | global_x | sg, dropout; pooling backward
# ------------------------------------------------------------------------------------------------
SIZES = [0, 1, 7, 8, 9, 60]   # an empty graph, the 8-row unroll boundary


def _readout_case(D, gdim, sgdim, p, seed=3):
    g = torch.Generator().manual_seed(seed + D)
    B, N = len(SIZES), sum(SIZES)
    ptr = torch.tensor([0] + list(np.cumsum(SIZES)), dtype=torch.int64)
    batch = torch.repeat_interleave(torch.arange(B), torch.tensor(SIZES))
    W = D + gdim + sgdim
    t = dict(h=torch.randn(N, D, generator=g), gx=torch.randn(B, gdim, generator=g),
             sg=torch.randn(B, sgdim, generator=g), dfeats=torch.randn(B, W, generator=g),
             dh0=torch.randn(N, D, generator=g), ptr=ptr, batch=batch, W=W)
    drop_seed = dr.site_seed(5, 16)
    mask = dr.dense_mask(drop_seed, B, W, p) if p > 0 else torch.ones(B, W, dtype=torch.bool)
    h = t["h"].double().requires_grad_(True)
    cnt = torch.tensor(SIZES, dtype=torch.float64).clamp(min=1)
    pooled = torch.zeros(B, D, dtype=torch.float64).index_add(0, batch, h) / cnt[:, None]
    feats = torch.cat([pooled, t["gx"].double(), t["sg"].double()], 1) * mask.double() / (1.0 - p)
    (feats * t["dfeats"].double()).sum().backward()
    return t, drop_seed, mask, feats.detach(), h.grad


def _sgdim():
    from alignn_mi355x.synthetic import mp_like_batch
    b = mp_like_batch(1)
    return b.global_x.numel(), b.sg_one_hot.numel()


@pytest.mark.parametrize("p", [0.0, 0.15])
@pytest.mark.parametrize("D", [64, 256])
@pytest.mark.parametrize("split", ["model", "wide"])
def test_readout_feats_and_pool_bwd_vs_fp64(split, D, p):
    """split 'model': global_x / sg widths as the model's batches carry them (they sum to the
    model's global_dim 289); 'wide': gdim = 289 beside the same sg.  The backward with the engine's
    dfeats (row stride W), written and accumulated; then with dfeats at another row stride — a
    [B, W] view of a wider buffer — where the mask must still be the forward's (index b * W + c)."""
    ops = _ops()
    g_model, sgdim = _sgdim()
    assert g_model + sgdim == 289
    gdim = g_model if split == "model" else 289
    t, drop_seed, mask, feats_ref, dh_ref = _readout_case(D, gdim, sgdim, p)
    B, W, N = len(SIZES), t["W"], sum(SIZES)
    d = lambda x: x.to(DEV).contiguous()  # noqa: E731
    ptr, batch = d(t["ptr"]), d(t["batch"])
    feats = torch.full((B, W), float("nan"), device=DEV)
    ops.readout_feats_fwd(d(t["h"]), ptr, d(t["gx"]).view(-1), gdim, d(t["sg"]).view(-1), sgdim, feats, p, drop_seed)
    assert _rel(feats.cpu(), feats_ref) < TOL
    if p > 0:
        # every column block is dropped: pooled, global_x and sg (exact zeros where the mask says so)
        # (graph 0 is empty: its pooled block is 0 whatever the mask)
        assert torch.equal((feats.cpu() == 0)[1:], ~mask[1:]) and torch.equal((feats.cpu() == 0)[0, D:], ~mask[0, D:])
        for lo, hi in ((0, D), (D, D + gdim), (D + gdim, W)):
            assert int((~mask[:, lo:hi]).sum()) > 0
    assert float(feats_ref[0, :D].abs().max()) == 0.0            # the empty graph pools to 0
    dfe = d(t["dfeats"])
    dh = torch.full((N, D), float("nan"), device=DEV)
    ops.readout_pool_bwd(dfe, ptr, batch, dh, False, p, drop_seed)
    assert _rel(dh.cpu(), dh_ref) < TOL
    dh = d(t["dh0"])
    ops.readout_pool_bwd(dfe, ptr, batch, dh, True, p, drop_seed)
    assert _rel(dh.cpu(), t["dh0"].double() + dh_ref) < TOL
    wide = torch.full((B, W + 5), float("nan"), device=DEV)
    wide[:, :W] = dfe
    dh = torch.full((N, D), float("nan"), device=DEV)
    ops.readout_pool_bwd(wide[:, :W], ptr, batch, dh, False, p, drop_seed)
    assert _rel(dh.cpu(), dh_ref) < TOL
