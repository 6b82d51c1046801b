"""NaN / +-inf through every activation, clamp and clip of the HIP library, against torch.

torch.relu(NaN) and torch.clamp(NaN, min=f) are NaN, threshold_backward passes the gradient where the
forward result is NaN, and clip_grad_norm_ with a NaN norm scales every gradient by NaN.  A bare
fmaxf(v, 0) (or a packed max, or a ``v > 0 ? g : 0`` mask) turns the NaN into 0 instead, and a diverged
row then looks like a row that skipped its block.  DESIGN.md, "Non-finite values", states the rule and
lists the sites; csrc/common.h holds the helpers.

Method, the same for every case: one poison value (NaN, +inf or -inf — never a large finite value,
which overflows fp32 but not the fp64 reference) is planted in one element (or row) of one input, and
the identical input goes to the kernel and to a plain high-precision torch restatement of the
operation (the kernel's existing one where its own test file has one).  ``_cmp`` then asserts, per
output: the finite masks are equal elementwise; every element the reference makes NaN is NaN; where
the reference is +-inf the kernel gives the same signed inf; the finite elements agree at the
tolerance that kernel's existing fp64 test uses.  Each case also asserts that its reference outputs
hold at least one finite and one non-finite element (so neither side of the mask is vacuous), except
where the reference leaves nothing finite (the optimizer with a NaN gradient, a poisoned weight end to
end) or nothing non-finite (a -inf log-variance, which the clamp absorbs): those assert exactly that.

Not compared where the reference is NaN: ``mstat``, the attention kernels' running softmax maximum.
It is a statistic of the online softmax with no counterpart in torch's softmax output, a max that
skips NaN by construction (the outputs computed from it are NaN all the same, and are compared).
csrc/knn.hip is left out: a top-k over NaN distances has ordering semantics of its own."""
import copy
import math

import pytest
import torch

import _dropout_ref as dr
from oracle import ensemble_ref, model_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN, INF = float("nan"), float("inf")
POISON = {"nan": NAN, "+inf": INF, "-inf": -INF}
LOG_MEANS, LOG_STDS = (4.3228, 3.5567), (0.9051, 0.9405)
FLOOR = -2.9
BF16_ULP = 2.0 ** -7   # one bf16 rounding step of x is at most 2^-7 |x|
# an fp32 result within 5e-6 of the reference's largest element, rounded to bf16: 8 significand bits, so
# a step of x is at most 2^-7 |x| and rounding to nearest moves x by at most half of it
C16_TOL = 2.0 ** -8 + 1e-5


def _ops():
    from alignn_mi355x import ops
    ops.set_step_seed(None)   # host seeds only: dropout masks are those of _dropout_ref
    return ops


def _cmp(got, ref, tol, tag, count=None, norm=False):
    """The mask rule (module docstring) for one output.  ``count``: a [finite, non-finite] tally of
    the reference the case checks at its end.  norm: the finite elements normwise instead of max-abs."""
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    assert g.shape == r.shape, (tag, g.shape, r.shape)
    fin = torch.isfinite(r)
    if count is not None:
        count[0] += int(fin.sum())
        count[1] += int((~fin).sum())
    gf = torch.isfinite(g)
    assert torch.equal(gf, fin), (tag, "finite masks differ", int((gf & ~fin).sum()), "finite where the reference "
                                  "is not,", int((~gf & fin).sum()), "non-finite where the reference is finite")
    nan = torch.isnan(r)
    assert bool(torch.isnan(g)[nan].all()), (tag, "NaN of the reference is not NaN")
    inf = torch.isinf(r)
    assert torch.equal(g[inf], r[inf]), (tag, "signed inf differs")
    if bool(fin.any()):
        d = g[fin] - r[fin]
        if norm:
            err = float(d.norm() / r[fin].norm().clamp(min=1e-30))
        else:
            err = float(d.abs().max() / r[fin].abs().max().clamp(min=1e-30))
        assert err < tol, (tag, err, tol)


def _mixed(count, tag):
    assert count[0] > 0 and count[1] > 0, (tag, "vacuous: reference finite / non-finite elements", count)


def _same(a, b):
    """Bitwise tie of two kernel paths on a poisoned input: NaN at the same places, equal elsewhere."""
    na, nb = torch.isnan(a), torch.isnan(b)
    z = torch.zeros((), dtype=a.dtype, device=a.device)
    return torch.equal(na, nb) and torch.equal(torch.where(na, z, a), torch.where(nb, z, b))


# ------------------------------------------------------------------------------------------------
# GEMM epilogues: bias -> ReLU (-> mask)
# ------------------------------------------------------------------------------------------------
# family: (M, N, K, flags of the path under test, flags of the path it is tied to bitwise or None,
#          bf16 arithmetic, bf16 C).  Shapes: the smallest each family's own test file routes to it.
def _gemm_families():
    from alignn_mi355x import ops
    BF = ops.GEMM_BF16
    return {
        # one-stage tiled loop, M / N / K tails (test_gpu_x_gemm_pipe.py's fallback shape)
        "tiled": (300, 257, 129, ops.GEMM_NOPIPE, None, False, False),
        # pipelined loop (full stages, vectorisable operands) tied to the one-stage loop
        "pipe": (2580, 768, 256, 0, ops.GEMM_NOPIPE, False, False),
        # bf16 LDS images tied to the fp32 images (test_gpu_x_gemm_lds16.py), ragged shape
        "lds16": (300, 257, 129, BF | ops.GEMM_LDS16, BF | ops.GEMM_NOLDS16, True, False),
        # row-streaming kernel below its 4096-row threshold on request, M tail; tied to the tiled kernel
        "rows": (33, 256, 8, BF | ops.GEMM_ROWS, BF | ops.GEMM_NOROWS, True, False),
        # bf16-storage C: tiled (M / N tails) and row-streaming
        "c16_tiled": (300, 257, 129, BF | ops.GEMM_NOROWS, None, True, True),
        "c16_rows": (33, 256, 8, BF | ops.GEMM_ROWS, BF | ops.GEMM_NOROWS, True, True),
    }


# (a bf16 C is write-only: the library takes no mask with it)
GEMM_CASES = [(f, e) for f in ("tiled", "pipe", "lds16", "rows", "c16_tiled", "c16_rows")
              for e in ("bias_relu", "bias_relu_mask") if not (f.startswith("c16") and e == "bias_relu_mask")]


@pytest.mark.parametrize("poison", ["A", "bias"])
@pytest.mark.parametrize("family,epi", GEMM_CASES)
def test_gemm_relu_epilogue_propagates(family, epi, poison):
    """NaN in one element of A: the whole output row is NaN after the ReLU.  Bias NaN / -inf / +inf:
    that column is NaN / 0 / +inf.  With ``mask`` behind the ReLU, a masked-out element is 0 whatever
    it held (a select, as torch.where).  Tolerances: fp32 5e-6 (test_gpu_x_gemm_pipe.py); bf16
    arithmetic 5e-6 against the fp64 product of the bf16-rounded operands (test_gpu_x_gemm_rows.py);
    bf16 C: that plus the rounding to bf16 (C16_TOL)."""
    ops = _ops()
    M, N, K, flags, tied, bf, c16 = _gemm_families()[family]
    g = torch.Generator(device="cpu").manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g)            # "nt": W k-contiguous
    bias = torch.randn(N, generator=g)
    mask = torch.randn(M, N, generator=g) if epi == "bias_relu_mask" else None
    r0, cn, cm, cp = M - 1, N - 1, 3, 2 * N // 3   # a tail row, the last column, two inner columns
    if poison == "A":
        A[r0, K - 1] = NAN
    else:
        bias[cn], bias[cm], bias[cp] = NAN, -INF, INF
    rnd = (lambda t: t.bfloat16().double()) if bf else (lambda t: t.double())
    ref = rnd(A) @ rnd(W).t() + bias.double()
    ref = torch.relu(ref)
    if mask is not None:
        ref = torch.where(mask > 0, ref, torch.zeros((), dtype=torch.float64))
    Ad, Wd, bd = A.to(DEV), W.to(DEV), bias.to(DEV)
    md = None if mask is None else mask.to(DEV)

    def run(fl):
        C = torch.full((M, N), 7.0, device=DEV, dtype=torch.bfloat16 if c16 else torch.float32)
        if family.endswith("rows"):     # the row-streaming kernel is the one that runs (2), its tie the tiled one (0)
            path = ops.gemm(Ad, Wd.t(), C, bias=bd, relu=True, mask=md, tile=fl, path_only=True)
            assert path == (2 if fl == flags else 0)
        ops.gemm(Ad, Wd.t(), C, bias=bd, relu=True, mask=md, tile=fl)
        torch.cuda.synchronize()
        return C

    C = run(flags)
    count = [0, 0]
    _cmp(C, ref, C16_TOL if c16 else 5e-6, (family, poison, epi), count)
    _mixed(count, (family, poison, epi))
    keep = torch.ones(M, N, dtype=torch.bool) if mask is None else mask > 0
    Cc = C.float().cpu()
    if poison == "A":
        assert bool(torch.isnan(Cc[r0][keep[r0]]).all()) and bool(torch.isfinite(Cc[:r0]).all())
    else:
        assert bool(torch.isnan(Cc[:, cn][keep[:, cn]]).all())
        assert bool((Cc[:, cm] == 0).all())
        assert bool((Cc[:, cp][keep[:, cp]] == INF).all())
    if tied is not None:
        assert _same(C, run(tied)), (family, "the bitwise tie between the two paths broke on the poisoned input")


# ------------------------------------------------------------------------------------------------
# The angle encoder's first layer: linear_smallk (fp32) and linear_smallk_bf16
# ------------------------------------------------------------------------------------------------
def _smallk_inputs(M, K, N, poison):
    g = torch.Generator(device="cpu").manual_seed(M + 7 * K + N)
    X = torch.randn(M, (K + 3) // 4 * 4, generator=g)
    W = torch.randn(N, K, generator=g)
    b = torch.randn(N, generator=g)
    if poison == "x_row":
        X[M // 2, :K] = NAN
    else:   # one element of W1 and +-inf biases
        W[N - 1, K - 1] = NAN
        b[0], b[N // 2] = -INF, INF
    return X, W, b


def _smallk_expect(out, M, N, poison):
    o = out.float().cpu()
    if poison == "x_row":
        assert bool(torch.isnan(o[M // 2]).all())
    else:
        assert bool(torch.isnan(o[:, N - 1]).all()) and bool((o[:, 0] == 0).all()) and bool((o[:, N // 2] == INF).all())


@pytest.mark.parametrize("poison", ["x_row", "w_bias"])
@pytest.mark.parametrize("M,K,N", [(63, 11, 256), (77, 5, 8)])
def test_linear_smallk_relu_propagates(M, K, N, poison):
    """fp32 Linear + ReLU over K <= 16 inputs (tolerance 1e-6: test_gpu_x_skinny.py)."""
    ops = _ops()
    X, W, b = _smallk_inputs(M, K, N, poison)
    Xd = X.to(DEV)[:, :K]
    out = torch.full((M, N), 7.0, device=DEV)
    ops.linear_smallk(Xd, W.to(DEV), b.to(DEV), out, relu=True)
    ref = torch.relu(X[:, :K].double() @ W.double().t() + b.double())
    count = [0, 0]
    _cmp(out, ref, 1e-6, (M, K, N, poison), count)
    _mixed(count, (M, K, N, poison))
    _smallk_expect(out, M, N, poison)


@pytest.mark.parametrize("poison", ["x_row", "w_bias"])
def test_linear_smallk_bf16_relu_propagates(poison):
    """The Linear + ReLU as bf16 autocast computes it, on the matrix cores: against the fp64 sum of the
    bf16-rounded operands, ReLU, rounded to bf16 once — within one bf16 rounding step
    (test_gpu_x_bf16.py::test_cast_and_skinny_bf16_outputs_bitwise)."""
    ops = _ops()
    M, K, N = 63, 11, 256
    X, W, b = _smallk_inputs(M, K, N, poison)
    Xd = X.to(DEV)[:, :K]
    out = torch.full((M, N), 7.0, device=DEV, dtype=torch.bfloat16)
    assert ops.linear_smallk_bf16_ok(Xd, W.to(DEV), out)
    ops.linear_smallk_bf16(Xd, W.to(DEV), b.to(DEV), out, relu=True)
    bf = lambda t: t.bfloat16().double()  # noqa: E731
    ref = torch.relu(bf(X[:, :K]) @ bf(W).t() + bf(b)).bfloat16()
    count = [0, 0]
    _cmp(out, ref, BF16_ULP, poison, count)
    _mixed(count, poison)
    _smallk_expect(out, M, N, poison)


# ------------------------------------------------------------------------------------------------
# gate + LayerNorm + ReLU + dropout + residual, forward and backward
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", ["outp", "R", "X", "ln_w"])
@pytest.mark.parametrize("p", [0.0, 0.15])
@pytest.mark.parametrize("D", [64, 256])
def test_gate_ln_fwd_bwd_propagate(D, p, poison):
    """n = 9 rows, one NaN element in outp / R / the residual X / ln_w, with the host dropout masks.
    Every output of both kernels against autograd of test_gpu_x_rowops.py's fp64 restatement
    (torch.relu: the LayerNorm row that is NaN stays NaN, and its gradient passes the ReLU), at that
    file's tolerance."""
    from test_gpu_x_rowops import TOL, _gate_inputs, _gate_ref, _gate_run
    _ops()
    n, r0, c0 = 9, 4, D // 3
    t = _gate_inputs(D, n, 7000 + D, False)
    key = {"outp": "outp", "R": "R", "X": "X", "ln_w": "lnw"}[poison]
    if poison == "ln_w":
        t[key][c0] = NAN
    else:
        t[key][r0, c0] = NAN
    drop_seed = dr.site_seed(99, 4 * (D % 7) + 1)
    mask = dr.dense_mask(drop_seed, n, D, p) if p > 0 else None
    ref = _gate_ref(t, p, mask, "plain")
    assert ref["near_kink"] == 0
    got = _gate_run(t, p, drop_seed, strided=False, flat=False)
    count = [0, 0]
    tag = (D, p, poison)
    for k in ("Xn", "beta", "mu", "rstd", "dout", "dR"):
        _cmp(got[k], ref[k], TOL, tag + (k,), count)
    for k, pre in zip(("d_wbeta", "d_lnw", "d_lnb"), t["pre"]):     # the reductions add into prefilled buffers
        _cmp(got[k], pre.double() + ref[k], TOL, tag + (k,), count)
    _mixed(count, tag)
    Xn = got["Xn"].cpu()
    if poison in ("outp", "R"):      # the row's LayerNorm is NaN: the whole new row, and nothing else
        assert bool(torch.isnan(Xn[r0]).all()) and bool(torch.isfinite(Xn[torch.arange(n) != r0]).all())
        assert bool(torch.isnan(got["beta"][r0])) and bool(torch.isnan(got["rstd"][r0]))
    elif poison == "ln_w":
        assert bool(torch.isnan(Xn[:, c0]).all())
    else:
        assert bool(torch.isnan(Xn[r0, c0])) and int(torch.isnan(Xn).sum()) == 1


# ------------------------------------------------------------------------------------------------
# Attention: atom graph (tconv.hip) and line graph (lgconv.hip, lgmx.hip)
# ------------------------------------------------------------------------------------------------
def _attention_ref(csr, m, t, D, H):
    """test_gpu_x_pending.py::_attention_ref at dropout 0, with the dF ReLU mask written as torch's
    threshold_backward (a select on ``F <= 0``) instead of a product with ``F > 0``."""
    n, C = csr.n, D // H
    d64 = lambda x: x.detach().double().cpu()  # noqa: E731
    src, dst = csr.src_at[:m].long().cpu(), csr.dst_at[:m].long().cpu()
    row = t["feat_row"][:m].long().cpu() if t["feat_row"] is not None else torch.arange(m)
    QKVR = d64(t["QKVR"])
    Q, K, V = (QKVR[:, i * D:(i + 1) * D].reshape(n, H, C) for i in range(3))
    U, Vd, F = d64(t["U"]), d64(t["Vd"]), d64(t["F"])[row]
    wb = d64(t["wbar"]).view(H, C) if t["wbar"] is not None else torch.zeros(H, C, dtype=torch.float64)
    dout = d64(t["dout"]).view(n, H, C)
    z64 = lambda *s: torch.zeros(*s, dtype=torch.float64)  # noqa: E731
    z = ((Q[dst] * K[src]).sum(-1) + torch.einsum("mhd,md->mh", U[dst], F) + (Q[dst] * wb).sum(-1)) / math.sqrt(C)
    mst = torch.full((n, H), -INF, dtype=torch.float64).scatter_reduce(0, dst[:, None].expand(m, H), z, "amax",
                                                                       include_self=True)
    ex = torch.exp(z - mst[dst])
    den = z64(n, H).index_add_(0, dst, ex) + 1e-16
    al = ex / den[dst]
    outp = z64(n, H, C).index_add_(0, dst, al[..., None] * V[src]).view(n, D)
    S = z64(n, H, D).index_add_(0, dst, al[..., None] * F[:, None, :])
    sumA = z64(n, H).index_add_(0, dst, al)
    g = (dout[dst] * V[src]).sum(-1) + torch.einsum("mhd,md->mh", Vd[dst], F) + (dout[dst] * wb).sum(-1)
    pdl = (dout * outp.view(n, H, C)).sum(-1)
    dz = al * (g - pdl[dst]) / math.sqrt(C)
    dq = z64(n, H, C).index_add_(0, dst, dz[..., None] * K[src]).view(n, D)
    Sz = z64(n, H, D).index_add_(0, dst, dz[..., None] * F[:, None, :])
    sigz = z64(n, H).index_add_(0, dst, dz)
    dF = d64(t["dF0"])
    upd = torch.einsum("mh,mhd->md", dz, U[dst]) + torch.einsum("mh,mhd->md", al, Vd[dst])
    dF[row] = torch.where(F <= 0, z64(()), dF[row] + upd)      # accumulate_dF = 3: add, then the ReLU mask
    # source side (alignn_tconv_bwd_src): dK_s = sum dz Q_d, dV_s = sum alpha dout_d
    dK = z64(n, H, C).index_add_(0, src, dz[..., None] * Q[dst]).view(n, D)
    dV = z64(n, H, C).index_add_(0, src, al[..., None] * dout[dst]).view(n, D)
    return dict(outp=outp, S=S, sumA=sumA, mstat=mst, den=den, dq=dq, Sz=Sz, sigz=sigz, dz=dz, al=al, dF=dF,
                dKV=torch.cat([dK, dV], 1))


def _cmp_attention(got, ref, tol, tag, count, tol_bwd=None):
    for k, r in ref.items():
        if k not in got:
            continue
        g = got[k]
        if k == "mstat":      # module docstring: compared where the reference's maximum is not NaN
            ok = ~torch.isnan(r.cpu())
            _cmp(g.cpu()[ok], r.cpu()[ok], tol, tag + (k,))
            continue
        bwd = k in ("dq", "Sz", "sigz", "dz", "dF", "dKV")
        _cmp(g, r, tol_bwd if (bwd and tol_bwd) else tol, tag + (k,), count)


def _poison_attention(t, poison, d0, t0, s0, D, frow=None):
    """d0: a target of degree >= 5; t0: the edge position of one of its in-edges; s0: that edge's source."""
    if poison == "f_row":
        t["F"][t0 if frow is None else frow] = NAN
    elif poison == "q_row":
        t["QKVR"][d0, :D] = NAN
    else:   # one K element of the source, in head 1's columns when there is more than one head
        t["QKVR"][s0, D + (D // 4 + 5 if D >= 128 else 5)] = INF


def _expect_one_target(got, poison, d0, n):
    """An edge-feature row or a query row poisons every contribution to its target, and no other target."""
    if poison in ("f_row", "q_row"):
        o = got["outp"].cpu()
        assert bool(torch.isnan(o[d0]).all()) and bool(torch.isfinite(o[torch.arange(n) != d0]).all())


@pytest.mark.parametrize("poison", ["f_row", "q_row", "k_inf"])
@pytest.mark.parametrize("D,H,feat_row", [(256, 4, False), (32, 4, True)])
def test_atom_attention_propagates(D, H, feat_row, poison):
    """tconv_fwd / tconv_bwd_dst (dF accumulated then ReLU-masked) / tconv_bwd_src on a 40-node graph
    with in-degrees 0..69 (heavy threshold 32: the 4-wave and the 1-wave kernels both run), at
    test_gpu_x_pending.py's 2e-5; the source side at test_gpu_kernels.py's 1e-5."""
    from test_gpu_x_pending import _run_tconv, _tconv_case
    ops = _ops()
    n = 40
    csr, m, t = _tconv_case(D, H, n, 70, 31 + D, True, feat_row)
    dst_at, src_at = csr.dst_at[:m].long().cpu(), csr.src_at[:m].long().cpu()
    deg = torch.bincount(dst_at, minlength=n)
    assert int((deg == 0).sum()) > 0 and int(deg.max()) > 32
    d0 = int(torch.nonzero((deg >= 5) & (deg <= 32))[0])
    t0 = int(torch.nonzero(dst_at == d0)[1])
    frow = int(t["feat_row"][t0]) if feat_row else None
    _poison_attention(t, poison, d0, t0, int(src_at[t0]), D, frow)
    ref = _attention_ref(csr, m, t, D, H)
    got = _run_tconv(csr, m, t, D, H, 0.0, 32)
    # the source side on the reference's per-edge terms (so it is checked on its own)
    dz32, al32 = ref["dz"].float().to(DEV).contiguous(), ref["al"].float().to(DEV).contiguous()
    r2 = dict(ref)
    r2.pop("dKV")
    count = [0, 0]
    tag = (D, H, feat_row, poison)
    _cmp_attention(got, r2, 2e-5, tag, count)
    _mixed(count, tag)
    _expect_one_target(got, poison, d0, n)
    if m:
        C = D // H
        Q64, do64 = t["QKVR"][:, :D].double().cpu().view(n, H, C), t["dout"].double().cpu().view(n, H, C)
        dzr, alr = dz32.double().cpu(), al32.double().cpu()
        z64 = lambda *s: torch.zeros(*s, dtype=torch.float64)  # noqa: E731
        dK = z64(n, H, C).index_add_(0, src_at, dzr[..., None] * Q64[dst_at]).view(n, D)
        dV = z64(n, H, C).index_add_(0, src_at, alr[..., None] * do64[dst_at]).view(n, D)
        for by in (False, True):
            dKV = torch.full((n, 2 * D), 7.0, device=DEV)
            ops.tconv_bwd_src(csr, D, H, t["QKVR"], t["dout"], dz32, al32, dKV, by_source=by)
            torch.cuda.synchronize()
            c2 = [0, 0]
            _cmp(dKV, torch.cat([dK, dV], 1), 1e-5, tag + ("dKV", by), c2)
            _mixed(c2, tag + ("dKV",))


def _lg_case(seed):
    """test_gpu_x_lg3.py's ragged line graph (20 targets, in-degrees 0..255) with the raw angle rows
    and the encoder layer of test_gpu_x_recompute.py; the poisoned target has 7 in-edges."""
    from test_gpu_x_lg3 import DEGREES
    from test_gpu_x_recompute import _xcase
    degs = DEGREES["ragged"]
    csr, m, t, x, W1, b1 = _xcase(degs, seed, True)
    d0 = 7
    assert degs[d0] >= 5 and 0 in degs
    t0 = sum(degs[:d0]) + 2                     # edges are drawn target-sorted: position t is edge t
    assert int(t["dst"][t0]) == d0
    return csr, m, t, x, W1, b1, d0, t0, int(t["src"][t0])


@pytest.mark.parametrize("poison", ["f_row", "q_row", "k_inf"])
@pytest.mark.parametrize("path", ["f32", "bf16"])
def test_line_attention_streamed_rows_propagates(path, poison):
    """The single-wave-item kernels on a materialised hidden layer F: fp32 rows (tconv_fwd /
    tconv_bwd_dst, kernel family 3) and bf16 K|V and F rows (lg_fwd_bf16 / lg_bwd_dst_bf16, which widen
    bf16 exactly: the reference takes the rounded K, V and F), both against test_gpu_x_lg3.py's fp64
    PyG attention at its 1e-5.  k_inf: the +inf key element stays inside its head (the kernels route a
    lane's q.k partial to its head by a select once a wave sees a non-finite value, lgconv.hip odd()),
    and a padded row's zero weight never meets another target's K or V row (group_src)."""
    from test_gpu_x_lg3 import _pyg_reference, _run
    from test_gpu_x_recompute import _outs
    ops = _ops()
    D, H = 256, 4
    csr, m, t, _, _, _, d0, t0, s0 = _lg_case(51)
    n = csr.n
    _poison_attention(t, poison, d0, t0, s0, D)
    tr = dict(t)
    if path == "f32":
        fam, got = _run(csr, m, t, D, H, 0.0, True)
        assert fam == 3
    else:
        QKV = t["QKVR"]
        KV16 = ops.cast_bf16(QKV[:, :3 * D].contiguous())[:, D:3 * D]
        F16 = t["F"].bfloat16()
        got = _outs(n, m)
        ops.lg_fwd_bf16(csr, D, H, QKV, KV16, t["U"], t["wbar"], F16, got["outp"], got["S"], got["sumA"], got["mstat"],
                        got["den"], 0.0, 77)
        ops.lg_bwd_dst_bf16(csr, D, H, QKV, KV16, t["U"], t["Vd"], t["wbar"], F16, t["dout"], got["outp"], got["mstat"],
                            got["den"], got["dq"], got["Sz"], got["sigz"], got["dz"], got["al"], 0.0, 77)
        torch.cuda.synchronize()
        got["dz"], got["al"] = got["dz"][:m], got["al"][:m]
        tr["QKVR"] = torch.cat([QKV[:, :D], KV16.float(), QKV[:, 3 * D:]], 1)
        tr["F"] = F16.float()
    ref = _pyg_reference((t["src"], t["dst"]), n, tr, H)
    count = [0, 0]
    _cmp_attention(got, ref, 1e-5, (path, poison), count)
    _mixed(count, (path, poison))
    _expect_one_target(got, poison, d0, n)


@pytest.mark.parametrize("poison", ["x_row", "q_row", "k_inf"])
def test_line_attention_recomputed_f32_propagates(poison):
    """lg_fwd_x / lg_bwd_dst_x in fp32: the hidden layer relu(W1 x + b1) recomputed per edge group, with
    a NaN raw angle row.  Against the fp64 PyG attention on the fp64 hidden layer (1e-5), and tied to
    the streamed kernels on linear_smallk's layer as test_gpu_x_recompute.py ties them: forward
    bitwise, backward 1e-6."""
    from test_gpu_x_lg3 import _pyg_reference
    from test_gpu_x_recompute import FWD, _recomputed, _streamed
    _ops()
    D, H = 256, 4
    csr, m, t, x, W1, b1, d0, t0, s0 = _lg_case(52)
    if poison == "x_row":
        x[t0] = NAN
    else:
        _poison_attention(t, poison, d0, t0, s0, D)
    tr = dict(t)
    tr["F"] = torch.relu(x[:m].double() @ W1.double().t() + b1.double())
    ref = _pyg_reference((t["src"], t["dst"]), csr.n, tr, H)
    got = _recomputed(csr, m, t, x, W1, b1, 0.0, False)
    st = _streamed(csr, m, t, x, W1, b1, 0.0, False)
    for o in (got, st):
        o["dz"], o["al"] = o["dz"][:m], o["al"][:m]
    count = [0, 0]
    _cmp_attention(got, ref, 1e-5, ("x_f32", poison), count)
    _mixed(count, ("x_f32", poison))
    _expect_one_target(got, "f_row" if poison == "x_row" else poison, d0, csr.n)
    for k in got:
        if k in FWD:
            assert _same(got[k], st[k]), k
        else:
            _cmp(got[k], st[k], 1e-6, ("x_f32 vs streamed", poison, k))


@pytest.mark.parametrize("poison", ["x_row", "q_row", "k_inf"])
def test_line_attention_matrix_core_propagates(poison):
    """The bf16 line-graph attention on the matrix cores (lgmx.hip, opt-in): its packed bf16 ReLU keeps
    a NaN of either sign.  Against test_gpu_x_lgmx.py's fp64 restatement on the matrix cores' operands
    at its tolerances (2e-4 forward, 5e-4 backward)."""
    from test_gpu_x_lgmx import _mx, _reference
    _ops()
    D = 256
    csr, m, t, x, W1, b1, d0, t0, s0 = _lg_case(53)
    if poison == "x_row":
        x[t0] = NAN
    else:
        _poison_attention(t, poison, d0, t0, s0, D)
    got, KV16 = _mx(csr, m, t, x, W1, b1, 0.0)
    ref = _reference(t, x, W1, b1, KV16, got["outp"], csr.n, m)
    got["dz"], got["al"] = got["dz"][:m], got["al"][:m]
    count = [0, 0]
    _cmp_attention(got, ref, 2e-4, ("mx", poison), count, tol_bwd=5e-4)
    _mixed(count, ("mx", poison))
    _expect_one_target(got, "f_row" if poison == "x_row" else poison, d0, csr.n)


# ------------------------------------------------------------------------------------------------
# Deferred angle-encoder backward
# ------------------------------------------------------------------------------------------------
def _enc_case(n, D, H, L, kin, poison):
    from test_gpu_x_encbwd import _case
    csr, x, W1, b1, U, Vd, dz, al = _case(n, D, H, L, kin, seed=n * 31 + D + H + L + kin)
    T = x.size(0)
    t0 = T // 2
    if poison == "row":
        x[t0] = NAN
    else:
        x[t0, kin - 1] = NAN
    d = csr.dst_at[:T].long()
    gsum = torch.zeros(T, D, dtype=torch.float64, device=DEV)
    return csr, x, W1, b1, U, Vd, dz, al, T, t0, d, gsum


def _relu_keep(pre64, fwd_positive):
    """Where the ReLU passes the gradient.  Non-finite pre-activations: torch's rule on the fp64 value
    (threshold_backward zeroes where the result is <= 0, so NaN passes).  Finite ones: the sign the
    forward kernel itself produced, as test_gpu_x_encbwd.py takes it (an fp32 pre-activation within
    rounding of 0 may sit on the other side of the kink than the fp64 one)."""
    return torch.where(torch.isfinite(pre64), fwd_positive, ~(torch.relu(pre64) <= 0))


@pytest.mark.parametrize("poison", ["row", "elem"])
def test_enc_bwd_f32_propagates(poison):
    """alignn_enc_bwd_f32 at the smallest shape of test_gpu_x_encbwd.py, one NaN angle row (or one NaN
    element of it): torch passes the gradient through the NaN ReLU output, so db1 receives that row's
    (finite) gradient and dW1 is NaN in the poisoned input columns.  1e-5 as there."""
    ops = _ops()
    n, D, H, L, kin = 17, 32, 1, 1, 7
    csr, x, W1, b1, U, Vd, dz, al, T, t0, d, gsum = _enc_case(n, D, H, L, kin, poison)
    for Ul, Vl, zl, al_l in zip(U, Vd, dz, al):
        gsum += torch.einsum("th,thd->td", zl[:T].double(), Ul[d].double())
        gsum += torch.einsum("th,thd->td", al_l[:T].double(), Vl[d].double())
    pre = x.double() @ W1.double().t() + b1.double()
    h1 = torch.empty(T, D, device=DEV)
    ops.linear_smallk(x, W1, b1, h1, relu=True)
    keep = _relu_keep(pre, h1 > 0)
    assert bool(keep[t0].all())
    dpre = torch.where(keep, gsum, torch.zeros((), dtype=torch.float64, device=DEV))
    rW, rb = dpre.t() @ x.double(), dpre.sum(0)
    dW1 = torch.full((D, kin), 7.0, device=DEV)
    db1 = torch.full((D,), 7.0, device=DEV)
    ops.enc_bwd(csr, x, W1, b1, U, Vd, dz, al, dW1, db1)
    torch.cuda.synchronize()
    count = [0, 0]
    _cmp(dW1, rW, 1e-5, ("dW1", poison), count)
    _cmp(db1, rb, 1e-5, ("db1", poison), count)
    _mixed(count, poison)
    assert bool(torch.isfinite(db1).all()) and bool(torch.isnan(dW1[:, kin - 1]).all())
    # db1 really holds the poisoned row's gradient: without it the sum is elsewhere
    assert float((rb - (dpre.sum(0) - dpre[t0])).abs().max()) > 1e-3 * float(rb.abs().max())


@pytest.mark.parametrize("poison", ["row", "elem"])
def test_enc_bwd_bf16_propagates(poison):
    """alignn_enc_bwd_bf16, mask read from the stored bf16 layer and mask recomputed on the matrix
    cores: against test_gpu_x_encbwd.py's fp64 restatement of its arithmetic (normwise 2e-3), and the
    two forms still tied bitwise (test_gpu_x_lgmx.py) with linear_smallk_bf16's layer."""
    ops = _ops()
    n, D, H, L, kin = 9, 256, 4, 2, 11
    csr, x, W1, b1, U, Vd, dz, al, T, t0, d, g = _enc_case(n, D, H, L, kin, poison)
    bf = lambda t: t.to(torch.bfloat16).double()  # noqa: E731
    f16 = torch.empty(T, D, dtype=torch.bfloat16, device=DEV)
    ops.linear_smallk_bf16(x, W1, b1, f16, relu=True)
    for Ul, Vl, zl, al_l in zip(U, Vd, dz, al):
        g += torch.einsum("th,thd->td", bf(zl[:T]), bf(Ul)[d]) + torch.einsum("th,thd->td", bf(al_l[:T]), bf(Vl)[d])
    pre = bf(x) @ bf(W1).t() + bf(b1)
    keep = _relu_keep(pre, f16.float() > 0)
    assert bool(keep[t0].all())
    dpre = bf(torch.where(keep, g.float(), torch.zeros((), device=DEV)))
    rW, rb = dpre.t() @ bf(x), dpre.sum(0)
    outs = []
    for kw in (dict(F=f16), dict(bf16=True)):
        dW1 = torch.full((D, kin), 7.0, device=DEV)
        db1 = torch.full((D,), 7.0, device=DEV)
        ops.enc_bwd(csr, x, W1, b1, U, Vd, dz, al, dW1, db1, **kw)
        torch.cuda.synchronize()
        count = [0, 0]
        _cmp(dW1, rW, 2e-3, ("dW1", poison, tuple(kw)), count, norm=True)
        _cmp(db1, rb, 2e-3, ("db1", poison, tuple(kw)), count, norm=True)
        _mixed(count, poison)
        outs.append((dW1, db1))
    assert _same(outs[0][0], outs[1][0]) and _same(outs[0][1], outs[1][1])


# ------------------------------------------------------------------------------------------------
# Heteroscedastic NLL: fp32 and the autocast form
# ------------------------------------------------------------------------------------------------
NLL_POISONS = [("mean", "nan"), ("mean", "+inf"), ("mean", "-inf"), ("logvar", "nan"), ("logvar", "+inf"),
               ("logvar", "-inf"), ("y", "zero"), ("y", "+inf")]


def _nll_inputs(where, what, weighted):
    g = torch.Generator(device="cpu").manual_seed(11)
    B, T = 3, 2
    heads = torch.randn(B, 2 * T, generator=g)
    y = torch.rand(B, T, generator=g) * 299 + 1
    w = (torch.rand(B, generator=g) + 0.5) if weighted else None
    if where == "mean":
        heads[1, 1] = POISON[what]
    elif where == "logvar":
        heads[1, T] = POISON[what]
    else:
        y[2, 0] = 0.0 if what == "zero" else INF
    return B, T, heads, y, w


def _cmp_scalar(got, ref, tol, tag):
    got, ref = float(got), float(ref)
    if math.isfinite(ref):
        assert math.isfinite(got) and abs(got - ref) <= tol * abs(ref), (tag, got, ref)
    elif math.isnan(ref):
        assert math.isnan(got), (tag, got, ref)
    else:
        assert got == ref, (tag, got, ref)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("where,what", NLL_POISONS)
def test_hetero_nll_f32_propagates(where, what, weighted):
    """Loss and dheads against fp64 autograd of oracle.model_ref.hetero_loss (weighted: the same lines
    with train.py:660-674's per-graph weight on the NLL term), at 1e-5 (test_gpu_x_pending.py).  A NaN
    log-variance stays NaN through the clamp (and clamp's backward gives it a zero gradient); a -inf
    one is absorbed by the clamp: everything stays finite, asserted as such."""
    ops = _ops()
    B, T, heads, y, w = _nll_inputs(where, what, weighted)
    h = heads.double().clone().requires_grad_(True)
    tz = model_ref.log_transform(y.double(), LOG_MEANS, LOG_STDS)
    if w is None:
        ref = model_ref.hetero_loss(h[:, :T], h[:, T:], tz, 0.1, FLOOR)
    else:
        lv = torch.clamp(h[:, T:], min=FLOOR)
        nll = 0.5 * (lv + (h[:, :T] - tz) ** 2 / torch.exp(lv)) * w.double().view(-1, 1)
        ref = nll.mean(1).mean() + 0.1 * (0.5 * lv).pow(2).mean()
    ref.backward()
    loss = torch.zeros(1, device=DEV)
    dh = torch.full((B, 2 * T), 7.0, device=DEV)
    ops.hetero_nll(heads.to(DEV), y.view(-1).to(DEV), torch.tensor(LOG_MEANS, device=DEV),
                   torch.tensor(LOG_STDS, device=DEV), FLOOR, 0.1, loss, dh, weights=None if w is None else w.to(DEV))
    torch.cuda.synchronize()
    tag = (where, what, weighted)
    _cmp_scalar(loss, ref.detach(), 1e-5, tag)
    count = [0, 0]
    _cmp(dh, h.grad, 1e-5, tag, count)
    if (where, what) == ("logvar", "-inf"):
        assert count[1] == 0 and math.isfinite(float(ref))
    else:
        _mixed(count, tag)
        assert not math.isfinite(float(ref))      # the loss: exempt from the mixed guard, non-finite throughout


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("where,what", NLL_POISONS)
def test_hetero_nll_amp_propagates(where, what, weighted):
    """The autocast form against torch's own bf16 autograd of the reference's loss lines on the same
    bf16 heads (test_gpu_x_round5.py): gradients bit for bit with NaN at the same places, the loss to
    2e-6."""
    from test_gpu_x_round5 import _ref_loss
    ops = _ops()
    B, T, heads, y, w = _nll_inputs(where, what, weighted)
    heads, y = heads.to(DEV), y.to(DEV)
    w = None if w is None else w.to(DEV)
    lm, ls = torch.tensor(LOG_MEANS, device=DEV), torch.tensor(LOG_STDS, device=DEV)
    S = 65536.0
    h16 = heads.to(torch.bfloat16).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        ref = _ref_loss(h16[:, :T], h16[:, T:], y, lm, ls, 0.1, w)
    (ref * torch.tensor(S, device=DEV)).backward()
    rg = h16.grad.float() / S
    loss = torch.zeros(1, device=DEV)
    dh = torch.full((B, 2 * T), 7.0, device=DEV)
    ops.hetero_nll(heads, y.view(-1), lm, ls, FLOOR, 0.1, loss, dh, weights=w, amp=True)
    torch.cuda.synchronize()
    tag = (where, what, weighted)
    _cmp_scalar(loss, ref.detach(), 2e-6, tag)
    count = [0, 0]
    _cmp(dh, rg, 1e-30, tag, count)
    assert _same(dh, rg), tag
    if (where, what) == ("logvar", "-inf"):
        assert count[1] == 0 and math.isfinite(float(ref))
    else:
        _mixed(count, tag)
        assert not math.isfinite(float(ref))


# ------------------------------------------------------------------------------------------------
# clip_grad_norm_ + AdamW
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["nan", "+inf"])
def test_clip_adamw_propagates(what):
    """grad_norm + adamw_step (fp32, no GradScaler) against torch's clip_grad_norm_ + single-tensor AdamW
    on the CPU, n = 5000 in two groups, max_norm 5.  One NaN gradient element: the norm is NaN, torch's
    clamp(NaN, max=1) is NaN, so every gradient, parameter and moment is NaN — asserted explicitly (the
    case is exempt from the mixed guard).  One +inf element: the norm is inf, the coefficient 0, the
    element inf * 0 = NaN and everything else finite.  Tolerances of
    test_gpu_x_pending.py::test_hip_clip_adamw_matches_torch."""
    ops = _ops()
    g0 = torch.Generator(device="cpu").manual_seed(4)
    n, split, i0 = 5000, 2500, 1234
    p0 = torch.randn(n, generator=g0)
    g = torch.randn(n, generator=g0) * 4.0
    g[i0] = POISON[what]
    pa, pb = torch.nn.Parameter(p0[:split].clone()), torch.nn.Parameter(p0[split:].clone())
    opt = torch.optim.AdamW([{"params": [pa], "lr": 3e-4}, {"params": [pb], "lr": 1e-4}], lr=3e-4, weight_decay=1e-4,
                            foreach=False, fused=False)
    pa.grad, pb.grad = g[:split].clone(), g[split:].clone()
    rnorm = torch.nn.utils.clip_grad_norm_([pa, pb], max_norm=5.0, foreach=False)
    opt.step()
    rg = torch.cat([pa.grad, pb.grad])
    rp = torch.cat([pa.detach(), pb.detach()])
    rm = torch.cat([opt.state[pa]["exp_avg"], opt.state[pb]["exp_avg"]])
    rv = torch.cat([opt.state[pa]["exp_avg_sq"], opt.state[pb]["exp_avg_sq"]])
    p, gg = p0.to(DEV), g.to(DEV)
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    step, norm = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    ops.grad_norm(gg, norm)
    ops.adamw_step(p, gg, m, v, split, 3e-4, 1e-4, 1e-4, norm=norm, max_norm=5.0, step=step)
    torch.cuda.synchronize()
    _cmp_scalar(norm, rnorm, 1e-5, what)
    assert not math.isfinite(float(rnorm))
    count = [0, 0]
    _cmp(gg, rg, 1e-6, (what, "g"), count)
    _cmp(m, rm, 1e-5, (what, "m"), count)
    _cmp(v, rv, 1e-5, (what, "v"), count)
    _cmp(p, rp, 1.0, (what, "p"), count)     # masks here; the finite values elementwise below
    fin = torch.isfinite(rp)
    tol = 1e-4 * (rp - p0)[fin].abs().max() + 2 * torch.finfo(torch.float32).eps * rp.abs() if bool(fin.any()) else None
    if tol is not None:
        assert bool(((p.cpu() - rp).abs()[fin] <= tol[fin]).all())
    if what == "nan":
        assert count[0] == 0 and count[1] == 4 * n          # nothing finite is left, in torch and here
    else:
        _mixed(count, what)
        assert int((~torch.isfinite(rp)).sum()) == 1 and bool(torch.isnan(p[i0]))
    assert float(step) == 1.0


# ------------------------------------------------------------------------------------------------
# Ensemble moments
# ------------------------------------------------------------------------------------------------
def _ensemble_ref(heads64, T):
    mean_z, var_z = ensemble_ref.mixture([h[:, :T] for h in heads64], [h[:, T:] for h in heads64], FLOOR)
    std_z = ensemble_ref.std_from_var(var_z)
    out = dict(mean_z=mean_z, std_z=std_z)
    out.update(ensemble_ref.predict_moments(mean_z, std_z, LOG_MEANS, LOG_STDS))
    return out


@pytest.mark.parametrize("poison", ["mean_nan", "logvar_nan", "logvar_+inf"])
def test_ensemble_moments_propagate(poison):
    """alignn_ensemble_moments, M = 3 members, B = 4, T = 2, all six outputs against
    oracle/ensemble_ref.py (torch.clamp at all four clamp sites), 1e-5 as test_gpu_x_ensemble.py.  A
    NaN member must not come back as a confident interval (std_z 1e-6, lo90 0)."""
    from alignn_mi355x.ensemble import ensemble_moments
    _ops()
    M, B, T = 3, 4, 2
    heads = torch.randn(M, B, 2 * T, generator=torch.Generator(device="cpu").manual_seed(3)) * 0.5
    b0, t1 = 2, 1
    if poison == "mean_nan":
        heads[1, b0, t1] = NAN
    elif poison == "logvar_nan":
        heads[1, b0, T + t1] = NAN
    else:
        heads[0, b0, T + t1] = INF
    ref = _ensemble_ref([h.double() for h in heads], T)
    lm, ls = torch.tensor(LOG_MEANS, device=DEV), torch.tensor(LOG_STDS, device=DEV)
    got = ensemble_moments(heads.to(DEV), FLOOR, lm, ls)
    torch.cuda.synchronize()
    assert set(got) == set(ref) and len(ref) == 6
    count = [0, 0]
    for k in ref:
        _cmp(got[k], ref[k], 1e-5, (poison, k), count)
    _mixed(count, poison)
    if poison != "logvar_+inf":
        for k in ("std_z", "lo90", "hi90", "std_lin"):
            assert bool(torch.isnan(got[k][b0, t1])), k
    else:
        assert float(got["std_z"][b0, t1]) == INF and float(got["lo90"][b0, t1]) == 0.0


# ------------------------------------------------------------------------------------------------
# End to end: production dims (two layers) and the D = 64 golden model, mp_like_batch(4)
# ------------------------------------------------------------------------------------------------
PROD = (206, 36, 11, 289, 2, 256, 2, 4, 0.15)
_E2E = {}


def _arch_state(which, golden):
    """(dims, fp32 state dict) of the model: 'prod' seeded as test_gpu_x_infer.py's, 'd64' the golden weights."""
    import alignn_mi355x as A
    from _golden_util import meta, state_from
    if which == "prod":
        dims = PROD
        torch.manual_seed(0)
        model = A.HeteroAlignnRegressor(A.AlignnRegressor(*dims), 2)
        st = {k: v.detach().clone() for k, v in model.state_dict().items()}
    else:
        g = golden("mp_d64_quirk")
        m = meta(g)
        dims = tuple(int(m[k]) for k in ("node", "edge", "angle", "global")) + (2, int(m["hidden"]), int(m["layers"]),
                                                                                 int(m["heads"]), 0.15)
        st = state_from(g, dtype=torch.float32)
    return dims, st


def _e2e_case(which, poison, golden):
    """Poisoned (state, batch) and the fp64 oracle's heads, computed once per case and left unchanged.
    (a): one atom, one bond and one angle feature of graph 1 (the angle row one whose target bond lies
    in graph 1).  Under the PyG offset rule of mp_like_batch's default batch the line graph joins bonds
    of graph 1 to bonds of graph 0 (every graph-1 bond it holds reaches one), so there the oracle makes
    graph 0 NaN as well; 'a_fixed' is the same poison on the batch with per-graph line graphs
    (lg_offset="num_edges"), where graph 1 alone is NaN.  (b): one element of the last layer's atom-conv query weight.
    (c): one LayerNorm weight element +inf."""
    key = (which, poison)
    if key in _E2E:
        return _E2E[key]
    from alignn_mi355x.synthetic import mp_like_batch
    from test_gpu_parity import _ref_batch
    dims, st = _arch_state(which, golden)
    st = {k: v.clone() for k, v in st.items()}
    L, H = dims[6], dims[7]
    b = mp_like_batch(4, lg_offset="num_edges") if poison == "a_fixed" else mp_like_batch(4)
    if poison in ("a", "a_fixed"):
        bond_graph = b.batch[b.edge_index[1]]
        atom = int(torch.nonzero(b.batch == 1)[3])
        bond = int(torch.nonzero(bond_graph == 1)[5])
        angle = int(torch.nonzero(bond_graph[b.lg_edge_index[1]] == 1)[7])
        b.x[atom, 17] = NAN
        b.edge_attr[bond, 5] = NAN
        b.lg_edge_attr[angle, 2] = NAN
    elif poison == "b":
        st[f"base.node_blocks.{L - 1}.conv.lin_query.weight"][3, 9] = NAN
    else:
        st["base.edge_blocks.0.norm.weight"][11] = INF
    rb = _ref_batch(b, 4, torch.float64)
    with torch.no_grad():
        rm, rl = model_ref.hetero_forward({k: v.double() for k, v in st.items()}, rb, H)
    _E2E[key] = dict(dims=dims, st=st, batch=b, ref=torch.cat([rm, rl], 1), H=H, L=L, rb=rb)
    return _E2E[key]


def _model_from(c, train=False):
    import alignn_mi355x as A
    m = A.HeteroAlignnRegressor(A.AlignnRegressor(*c["dims"]), 2)
    m.load_state_dict(c["st"])
    m.to(DEV)
    return m.train() if train else m.eval()


@pytest.mark.parametrize("poison", ["a", "a_fixed", "b", "c"])
@pytest.mark.parametrize("which", ["prod", "d64"])
def test_eval_forward_propagates(which, poison, golden):
    """The module API under no_grad three ways — eager, the recorded plan (second call), bf16 autocast —
    against oracle.model_ref.hetero_forward in fp64.  (a_fixed): graph 1's heads are NaN, graphs 0, 2
    and 3 finite and within the eval tolerance (1e-4 fp32 as tests/test_gpu_parity.py, 3e-2 under
    autocast as test_gpu_x_round5.py); (a): the same with graph 0 as the oracle has it (_e2e_case).
    (b), (c): the mask is the oracle's, which leaves nothing finite."""
    from test_gpu_x_infer import _eager, _planned
    _ops()
    c = _e2e_case(which, poison, golden)
    ref = c["ref"]
    fin = torch.isfinite(ref)
    if poison == "a_fixed":
        assert bool((~fin[1]).all()) and bool(fin[[0, 2, 3]].all())
    elif poison == "a":
        assert bool((~fin[1]).all()) and bool(fin[[2, 3]].all())
    else:
        assert not bool(fin.any())                 # exempt from the mixed guard: asserted instead
    model = _model_from(c)
    b = copy.copy(c["batch"]).to(DEV)
    outs = {"eager": _eager(model, b)}
    _planned(model, b)
    outs["plan"] = _planned(model, b)
    assert len(model.__dict__.get("_fwd_plans", {})) == 1
    outs["autocast"] = _eager(model, b, amp=True).float()
    for k, o in outs.items():
        _cmp(o, ref, 3e-2 if k == "autocast" else 1e-4, (which, poison, k))


def _oracle_step(c, seed, p_drop):
    """One reference training step (train.py:647-699) in fp64 with the engine's dropout masks: forward,
    hetero NLL, backward, clip_grad_norm_(5), single-tensor AdamW in the reference's two groups."""
    params = {k: v.double().clone().requires_grad_(True) for k, v in c["st"].items()}
    fn = dr.OracleDropout(seed, p_drop, c["rb"], c["H"], c["L"])
    mean, logvar = model_ref.hetero_forward(params, c["rb"], c["H"], dropout_fn=fn)
    tz = model_ref.log_transform(c["rb"].y.view(4, -1), LOG_MEANS, LOG_STDS)
    loss = model_ref.hetero_loss(mean, logvar, tz, 0.1)
    loss.backward()
    used = {k: v for k, v in params.items() if v.grad is not None}
    base = [v for k, v in used.items() if not k.startswith("logvar_heads.")]
    sigma = [v for k, v in used.items() if k.startswith("logvar_heads.")]
    opt = torch.optim.AdamW([{"params": base, "lr": 3e-4}, {"params": sigma, "lr": 3e-4}], lr=3e-4, weight_decay=1e-4,
                            foreach=False, fused=False)
    gnorm = torch.nn.utils.clip_grad_norm_(list(used.values()), max_norm=5.0, foreach=False)
    opt.step()
    return loss.detach(), gnorm.detach(), {k: v.detach() for k, v in used.items()}


@pytest.mark.parametrize("mode", ["eager", "replay"])
@pytest.mark.parametrize("poison", ["a", "b"])
def test_fp32_fused_step_propagates(poison, mode, golden):
    """FusedTrainer's fp32 step (no GradScaler, dropout 0.15) on a poisoned feature / weight, eager and
    on the replayed plan: the oracle's loss is non-finite, so its gradient norm and — through
    clip_grad_norm_'s NaN coefficient — every parameter it updates are non-finite; the engine's loss,
    gnorm and every parameter must be too (before the fix the step trained on with a finite loss).
    Nothing finite is left to compare, which is asserted."""
    import alignn_mi355x as A
    ops = _ops()
    c = _e2e_case("prod", poison, golden)
    seed = 1234567
    rloss, rnorm, rparams = _oracle_step(c, seed, 0.15)
    assert not math.isfinite(float(rloss)) and not math.isfinite(float(rnorm))
    assert all(not bool(torch.isfinite(v).any()) for v in rparams.values())
    model = _model_from(c, train=True)
    b = copy.copy(c["batch"]).to(DEV)
    tr = A.FusedTrainer(model, feature_jitter_std=0.0, target_log_means=LOG_MEANS, target_log_stds=LOG_STDS)
    assert tr.scaler is None
    if mode == "replay":
        tr.capture(b, mode="plan")
    loss = tr.step(b, seed=seed)
    torch.cuda.synchronize()
    if mode == "replay":
        assert tr.replays >= 1
    _cmp_scalar(loss, rloss, 1e-4, (poison, mode, "loss"))
    _cmp_scalar(tr.gnorm, rnorm, 1e-4, (poison, mode, "gnorm"))
    assert set(tr.st.names) == set(rparams)
    for k in tr.st.names:
        _cmp(tr.st.P.named[k], rparams[k], 1e-4, (poison, mode, k))
    ops.set_step_seed(None)      # a capture registers its device step seed


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def test_bf16_scaled_step_is_skipped_on_poisoned_weight(golden):
    """bf16 step with the GradScaler, one NaN weight element: the step is skipped — parameters, moments
    and step count bitwise unchanged, the scale halves, one skipped step — and the loss it returns is
    non-finite."""
    import alignn_mi355x as A
    _ops()
    c = _e2e_case("prod", "b", golden)
    model = _model_from(c, train=True)
    b = copy.copy(c["batch"]).to(DEV)
    tr = A.FusedTrainer(model, precision="bf16", feature_jitter_std=0.0)
    assert tr.scaler is not None
    f0, m0, v0 = tr.st.flat.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone()
    assert int(torch.isnan(f0).sum()) == 1
    loss = tr.step(b, seed=99)
    torch.cuda.synchronize()
    assert not math.isfinite(float(loss))
    assert torch.equal(_bits(tr.st.flat), _bits(f0))
    assert torch.equal(_bits(tr.exp_avg), _bits(m0)) and torch.equal(_bits(tr.exp_avg_sq), _bits(v0))
    assert float(tr.hip_step) == 0.0
    sc = tr.scaler.tolist()
    assert sc[0] == 32768.0 and sc[3] == 1.0


def test_ensemble_predict_batch_with_poisoned_member(golden):
    """EnsemblePredictor.predict_batch, three members of which one has a NaN weight element: the mask of
    every returned field equals that of oracle/ensemble_ref.py on the fp64 oracle's member heads."""
    from alignn_mi355x.ensemble import EnsemblePredictor
    _ops()
    # members: clean weights (case (a) poisons its batch only), the NaN query weight, clean — on the clean batch
    cases = [_e2e_case("prod", "a", golden), _e2e_case("prod", "b", golden), _e2e_case("prod", "a", golden)]
    from alignn_mi355x.synthetic import mp_like_batch
    from test_gpu_parity import _ref_batch
    cpu_b = mp_like_batch(4)
    rb = _ref_batch(cpu_b, 4, torch.float64)
    heads64 = []
    with torch.no_grad():
        for c in cases:
            rm, rl = model_ref.hetero_forward({k: v.double() for k, v in c["st"].items()}, rb, c["H"])
            heads64.append(torch.cat([rm, rl], 1))
    assert bool(torch.isfinite(heads64[0]).all()) and not bool(torch.isfinite(heads64[1]).any())
    ref = _ensemble_ref(heads64, 2)
    ep = EnsemblePredictor([_model_from(c) for c in cases], FLOOR, LOG_MEANS, LOG_STDS)
    got = ep.predict_batch(cpu_b.to(DEV))
    torch.cuda.synchronize()
    assert set(got) == set(ref)
    for k in ref:
        _cmp(got[k], ref[k], 1e-4, k)
        assert not bool(torch.isfinite(ref[k]).any()), k     # exempt from the mixed guard: asserted instead
