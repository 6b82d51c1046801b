"""Single-wave-item attention kernels (csrc/lgconv.hip, schedule flag ALIGNN_SCHED_WAVE_ITEMS): the
line-graph path of the training step (D = 256, materialised angle hidden layer F, deferred encoder
backward so no dF).  Checked against the compact-register kernels of tconv.hip (same arithmetic and
dropout masks, softmax sums in another order: 1e-5 relative) and against a float64 PyTorch
restatement of PyG's TransformerConv attention on the same operands (the oracle's formula,
oracle/pyg_ref.py, with the edge-feature algebra of DESIGN.md §3 applied by hand)."""
import pytest
import torch

from test_gpu_x_pending import _rel

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from alignn_mi355x import ops
    return ops


def _case(H, degs, seed, with_wbar, D=256):
    ops = _ops()
    g = torch.Generator().manual_seed(seed)
    degs = torch.as_tensor(degs)
    n = degs.numel()
    dst = torch.repeat_interleave(torch.arange(n), degs)
    src = torch.randint(0, n, (dst.numel(),), generator=g)
    ei = torch.stack([src, dst]).to(DEV)
    csr = ops.GraphCSR(ei, n)
    m = dst.numel()
    r = lambda *s: (torch.randn(*s, generator=g) * 0.5).to(DEV)  # noqa: E731
    t = dict(QKVR=r(n, 4 * D), U=r(n, H, D), Vd=r(n, H, D), F=r(max(m, 1), D), dout=r(n, D),
             wbar=r(D) if with_wbar else None, src=src, dst=dst)
    return csr, m, t


def _run(csr, m, t, D, H, drop, wave_items, xcd_items=None):
    ops = _ops()
    n = csr.n
    csr._sched = None
    prev = csr.policy
    csr.policy = ops.SchedulePolicy(wave_items=wave_items, xcd_items=True if xcd_items is None else xcd_items)
    try:
        fam = csr.family(D, H, t["F"])
        outp, S = torch.empty(n, D, device=DEV), torch.empty(n, H, D, device=DEV)
        sumA, mstat, den = (torch.empty(n, H, device=DEV) for _ in range(3))
        ops.tconv_fwd(csr, D, H, t["QKVR"], t["U"], t["wbar"], t["F"], None, outp, S, sumA, mstat, den, drop, 77)
        dq = torch.full((n, D), float("nan"), device=DEV)
        Sz, sigz = torch.empty(n, H, D, device=DEV), torch.empty(n, H, device=DEV)
        dz, al = torch.empty(max(m, 1), H, device=DEV), torch.empty(max(m, 1), H, device=DEV)
        ops.tconv_bwd_dst(csr, D, H, t["QKVR"], t["U"], t["Vd"], t["wbar"], t["F"], None, t["dout"], outp,
                          mstat, den, dq, Sz, sigz, dz, al, None, 0, drop, 77)
    finally:
        csr.policy = prev
        csr._sched = None
    torch.cuda.synchronize()
    return fam, dict(outp=outp, S=S, sumA=sumA, mstat=mstat, den=den, dq=dq, Sz=Sz, sigz=sigz, dz=dz[:m], al=al[:m])


DEGREES = {
    # the B = 32 line graph's in-degree mix (1,260 x 132, 11..121 step 11) at reduced count
    "mp_mix": [132] * 40 + [11 * k for k in range(1, 12) for _ in range(4)],
    # ragged: zeros, group tails of every length (1..8), one segment of 255 (below the heavy cut)
    "ragged": [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 0, 13, 255, 17, 0, 31, 64, 65, 3, 1],
    "empty_edges": [0, 0, 0],
}


@pytest.mark.parametrize("H", [1, 2, 4])
@pytest.mark.parametrize("drop", [0.0, 0.15])
@pytest.mark.parametrize("degs", list(DEGREES))
def test_wave_items_match_compact_kernels(H, drop, degs):
    for seed, with_wbar in enumerate((True, False)):
        csr, m, t = _case(H, DEGREES[degs], 40 + seed, with_wbar)
        fa, a = _run(csr, m, t, 256, H, drop, False)
        fb, b = _run(csr, m, t, 256, H, drop, True)
        assert (fa, fb) == (2, 3)  # the new kernels ran (and the reference arm did not)
        for k in a:
            if k in ("dz", "al") and m == 0:
                continue
            assert _rel(b[k], a[k]) < 1e-5, (k, H, drop, degs, seed)


@pytest.mark.parametrize("drop", [0.0, 0.15])
def test_xcd_item_order_bitwise(drop):
    """XCD-contiguous, edge-balanced work-item order (GraphCSR.XCD_ITEMS) only permutes which wave
    runs which target: every output bitwise equal to the plain longest-first order."""
    csr, m, t = _case(4, DEGREES["mp_mix"] * 3, 5, True)
    _, a = _run(csr, m, t, 256, 4, drop, True, xcd_items=False)
    _, b = _run(csr, m, t, 256, 4, drop, True, xcd_items=True)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _pyg_reference(csr_cpu_ei, n, t, H, D=256, mask=None, p=0.0):
    """Float64 PyG TransformerConv attention on the engine's operands: with
    M_h the per-head edge map, z = <Q_d, K_s + M_h f_t + w̄_h>/sqrt(C) is written as
    <Q_dh, K_sh>/sqrt(C) + (<u_dh, f_t> + <w̄_h, Q_dh>)/sqrt(C) (u = M_h^T Q_dh given as U).
    mask (bool [m, H] by edge position) and p: attention dropout, alpha' = alpha * mask / (1 - p) in
    outp, S, sumA and in the target-side backward (dq, Sz, sigz, dz, al: the contract of
    alignn_tconv_bwd_dst on Vd / dout, al = alpha'); ``alpha`` stays the softmax itself."""
    C = D // H
    src, dst = csr_cpu_ei
    QKV = t["QKVR"].double().cpu()
    Q, K, V = QKV[:, :D].view(n, H, C), QKV[:, D:2 * D].view(n, H, C), QKV[:, 2 * D:3 * D].view(n, H, C)
    U = t["U"].double().cpu()
    F = t["F"].double().cpu()
    m = dst.numel()  # _case draws the edges target-sorted: edge position t is edge t
    Fe = F[:m]
    wb = t["wbar"].double().cpu().view(H, C) if t["wbar"] is not None else torch.zeros(H, C, dtype=torch.float64)
    z = ((Q[dst] * K[src]).sum(-1) + (U[dst] * Fe[:, None, :]).sum(-1) + (Q[dst] * wb).sum(-1)) / C ** 0.5
    zmax = torch.full((n, H), float("-inf"), dtype=torch.float64).scatter_reduce(0, dst[:, None].expand(-1, H), z,
                                                                                  "amax")
    ex = torch.exp(z - zmax[dst])
    den = torch.zeros(n, H, dtype=torch.float64).index_add(0, dst, ex) + 1e-16
    alpha = ex / den[dst]
    keep = torch.ones(m, H, dtype=torch.float64) if mask is None else mask.double() / (1.0 - p)
    al = alpha * keep
    aggV = torch.zeros(n, H, C, dtype=torch.float64).index_add(0, dst, al[:, :, None] * V[src])
    S = torch.zeros(n, H, D, dtype=torch.float64).index_add(0, dst, al[:, :, None] * Fe[:, None, :])
    out = dict(outp=aggV.reshape(n, D), S=S, sumA=torch.zeros(n, H, dtype=torch.float64).index_add(0, dst, al),
               alpha=alpha)
    # target-side backward (the kernels' contract, as tests/test_gpu_x_pending.py::_attention_ref)
    Vd, dout = t["Vd"].double().cpu(), t["dout"].double().cpu().view(n, H, C)
    g = (dout[dst] * V[src]).sum(-1) + (Vd[dst] * Fe[:, None, :]).sum(-1) + (dout[dst] * wb).sum(-1)
    pdl = (dout * aggV).sum(-1)
    dz = alpha * (g * keep - pdl[dst]) / C ** 0.5
    out.update(dq=torch.zeros(n, H, C, dtype=torch.float64).index_add(0, dst, dz[:, :, None] * K[src]).reshape(n, D),
               Sz=torch.zeros(n, H, D, dtype=torch.float64).index_add(0, dst, dz[:, :, None] * Fe[:, None, :]),
               sigz=torch.zeros(n, H, dtype=torch.float64).index_add(0, dst, dz), dz=dz, al=al)
    return out


@pytest.mark.parametrize("H", [1, 4])
def test_wave_items_forward_vs_float64_pyg(H):
    """The forward outputs (dropout 0) against PyG's attention in float64."""
    degs = DEGREES["ragged"]
    csr, m, t = _case(H, degs, 7, True)
    _, b = _run(csr, m, t, 256, H, 0.0, True)
    ref = _pyg_reference((t["src"], t["dst"]), len(degs), t, H)
    assert _rel(b["outp"].cpu(), ref["outp"]) < 1e-5
    assert _rel(b["S"].cpu(), ref["S"]) < 1e-5
    assert _rel(b["sumA"].cpu(), ref["sumA"]) < 1e-5


@pytest.mark.parametrize("H", [1, 4])
def test_wave_items_dropout_vs_float64_pyg(H):
    """Forward and target-side backward at dropout 0.15 against PyG's attention in float64 with the
    kernels' keep mask reproduced on the host (tests/_dropout_ref.py: element t * H + h of the call's
    seed): the mask scales alpha in outp, S and sumA alike and the backward re-draws the same one."""
    import _dropout_ref as dr
    _ops().set_step_seed(None)
    p = 0.15
    degs = DEGREES["ragged"]
    csr, m, t = _case(H, degs, 7, True)
    fam, b = _run(csr, m, t, 256, H, p, True)
    assert fam == 3
    mask = torch.from_numpy(dr.keep_mask(77, m * H, p).reshape(m, H))   # _run's seed
    assert 0.10 < float((~mask).double().mean()) < 0.20
    ref = _pyg_reference((t["src"], t["dst"]), len(degs), t, H, mask=mask, p=p)
    assert torch.equal(b["al"].cpu() == 0, ~mask)
    for k in ("outp", "S", "sumA", "dq", "Sz", "sigz", "dz", "al"):
        assert _rel(b[k].cpu(), ref[k]) < 1e-5, (k, H)
