"""Host restatement of the dropout masks (tests/_dropout_ref.py): the properties the GPU tests that
inject these masks into the fp64 oracle rely on, and the oracle's ``dropout_fn`` hook.  No GPU."""
import numpy as np
import torch

import _dropout_ref as dr


def _hash_scalar(seed, idx):
    """common.h hash_u32 in Python integers (an independent second statement of the definition)."""
    m = (1 << 64) - 1
    x = (seed ^ (idx * 0x9E3779B97F4A7C15)) & m
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & m
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & m
    x ^= x >> 33
    return x >> 32


def test_hash_matches_integer_arithmetic():
    seeds = [0, 1, 77, 2 ** 63 - 1, 2 ** 64 - 1, dr.site_seed(12345, 7)]
    idxs = [0, 1, 2, 63, 64, 255, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 3, 2 ** 63,
            2 ** 64 - 1]
    for s in seeds:
        got = dr.hash_u32(s, np.asarray(idxs, dtype=np.uint64))
        assert got.dtype == np.uint32
        assert got.tolist() == [_hash_scalar(s, i) for i in idxs], s


def test_helper_is_deterministic():
    a = dr.keep_mask(dr.site_seed(9, 3), 10_000, 0.15)
    b = dr.keep_mask(dr.site_seed(9, 3), 10_000, 0.15)
    assert a.dtype == np.bool_ and np.array_equal(a, b)
    assert not np.array_equal(a, dr.keep_mask(dr.site_seed(9, 4), 10_000, 0.15))   # sites differ
    assert not np.array_equal(a, dr.keep_mask(dr.site_seed(10, 3), 10_000, 0.15))  # steps differ
    # a window of a longer mask is that mask's slice (the element index alone decides)
    assert np.array_equal(dr.keep_mask(5, 100, 0.15, start=40), dr.keep_mask(5, 140, 0.15)[40:])


def test_keep_fraction():
    for seed in (0, 77, dr.site_seed(42, 16)):
        k = dr.keep_mask(seed, 100_000, 0.15)
        assert 0.80 <= float(k.mean()) <= 0.90
        # much tighter in fact: 3 sigma of Binomial(1e5, 0.85) is 0.0034
        assert abs(float(k.mean()) - 0.85) < 0.005
    assert abs(float(dr.keep_mask(3, 100_000, 0.5).mean()) - 0.5) < 0.006


def test_p_zero_keeps_everything():
    assert dr.thresh(0.0) == 0
    assert bool(dr.keep_mask(123, 4096, 0.0).all())
    assert dr.inv_keep(0.0) == 1.0


def test_threshold_and_scale_are_the_kernels_fp32_values():
    # make_drop: (uint32)((double)(float)p * 2^32); inv_keep = 1.0f / (1.0f - (float)p)
    assert dr.thresh(0.5) == 2 ** 31
    assert dr.thresh(0.15) == int(float(np.float32(0.15)) * 2.0 ** 32)
    assert dr.thresh(1.0) == 2 ** 32 - 1
    assert dr.inv_keep(0.5) == 2.0
    assert abs(dr.inv_keep(0.15) - 1 / 0.85) < 2e-7


def test_indices_above_2_32_wrap_as_uint64():
    seed = 77
    base = 2 ** 32 - 2
    got = dr.hash_u32(seed, np.arange(base, base + 5, dtype=np.uint64))
    assert got.tolist() == [_hash_scalar(seed, base + i) for i in range(5)]
    # not a 32-bit index: idx and idx + 2^32 draw differently
    lo = dr.hash_u32(seed, np.arange(0, 64, dtype=np.uint64))
    hi = dr.hash_u32(seed, np.arange(2 ** 32, 2 ** 32 + 64, dtype=np.uint64))
    assert not np.array_equal(lo, hi)
    # idx * 0x9E37... overflows 64 bits for every idx >= 2: the product wraps, as in C
    assert int(dr.hash_u32(seed, 2 ** 64 + 5)) == _hash_scalar(seed, 5)
    k = dr.keep_mask(seed, 5, 0.15, start=base)
    assert k.tolist() == [_hash_scalar(seed, base + i) >= dr.thresh(0.15) for i in range(5)]


def test_site_seed_is_a_63_bit_mix():
    assert dr.site_seed(0, 0) == 0x165667B1
    assert dr.site_seed(1, 0) - dr.site_seed(0, 0) == 0x9E3779B1
    assert dr.site_seed(0, 1) - dr.site_seed(0, 0) == 0x85EBCA77
    assert 0 <= dr.site_seed(2 ** 62 - 1, 17) < 2 ** 63
    assert len({dr.site_seed(5, k) for k in range(18)}) == 18


def test_site_seed_equals_the_engines():
    from alignn_mi355x.engine import site_seed
    for seed in (0, 1, 7, 42, 2 ** 31, 2 ** 62 - 1):
        for site in (0, 1, 2, 3, 15, 16, 17, 1 << 20):
            assert dr.site_seed(seed, site) == site_seed(seed, site), (seed, site)


def test_edge_mask_follows_the_stable_target_order():
    g = torch.Generator().manual_seed(0)
    dst = torch.randint(0, 9, (40,), generator=g)
    H, p, seed = 4, 0.5, 31
    mk = dr.edge_mask(seed, dst, H, p)
    perm = torch.argsort(dst, stable=True)
    flat = dr.keep_mask(seed, 40 * H, p)
    for t, e in enumerate(perm.tolist()):
        assert mk[e].tolist() == flat[t * H:(t + 1) * H].tolist()
    # relabelling the targets monotonically (the line graph's compaction) leaves the order alone
    relabel = torch.unique(dst, return_inverse=True)[1]
    assert torch.equal(torch.argsort(relabel, stable=True), perm)


def _tiny_case():
    from oracle.pyg_ref import RefData
    g = torch.Generator().manual_seed(3)
    D, H, L, B = 8, 2, 2, 2
    N, E, T = 6, 14, 30
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64) * 0.5  # noqa: E731
    st = {}
    for enc, k in (("node", 5), ("edge", 4), ("angle", 3)):
        st[f"base.{enc}_encoder.0.weight"], st[f"base.{enc}_encoder.0.bias"] = r(D, k), r(D)
        st[f"base.{enc}_encoder.2.weight"], st[f"base.{enc}_encoder.2.bias"] = r(D, D), r(D)
    for l in range(L):
        for blk in ("edge", "node"):
            pre = f"base.{blk}_blocks.{l}."
            for lin in ("query", "key", "value", "skip"):
                st[pre + f"conv.lin_{lin}.weight"], st[pre + f"conv.lin_{lin}.bias"] = r(D, D), r(D)
            st[pre + "conv.lin_edge.weight"] = r(D, D)
            st[pre + "conv.lin_beta.weight"] = r(1, 3 * D)
            st[pre + "norm.weight"], st[pre + "norm.bias"] = 1 + 0.1 * r(D), 0.1 * r(D)
            if blk == "node":
                st[pre + "edge_proj.weight"], st[pre + "edge_proj.bias"] = r(D, D), r(D)
    st["base.feat_proj.0.weight"], st["base.feat_proj.0.bias"] = r(D, D + 3 + 2), r(D)
    for t in range(2):
        st[f"mean_heads.{t}.weight"], st[f"mean_heads.{t}.bias"] = r(1, D), r(1)
        st[f"logvar_heads.{t}.weight"], st[f"logvar_heads.{t}.bias"] = r(1, D), r(1)
    data = RefData(x=r(N, 5), edge_attr=r(E, 4), lg_edge_attr=r(T, 3),
                   edge_index=torch.randint(0, N, (2, E), generator=g),
                   lg_edge_index=torch.randint(0, E, (2, T), generator=g),
                   batch=torch.tensor([0, 0, 0, 1, 1, 1]), global_x=r(B, 3), sg_one_hot=r(B, 2))
    return st, data, H, L, (N, E, T, D, B)


def test_oracle_hook_sites_and_shapes():
    """hetero_forward calls dropout_fn once per site, in site order, with the documented shapes; a
    hook that applies no mask reproduces the eval forward exactly, and the masked forward differs."""
    from oracle import model_ref
    st, data, H, L, (N, E, T, D, B) = _tiny_case()
    calls = []

    def ident(site, x):
        calls.append((site, tuple(x.shape)))
        return x

    m0, v0 = model_ref.hetero_forward(st, data, H)
    m1, v1 = model_ref.hetero_forward(st, data, H, dropout_fn=ident)
    assert torch.equal(m0, m1) and torch.equal(v0, v1)
    want = []
    for l in range(L):
        want += [(4 * l, (T, H)), (4 * l + 1, (E, D)), (4 * l + 2, (E, H)), (4 * l + 3, (N, D))]
    want += [(4 * L, (B, D + 5)), (4 * L + 1, (B, D))]
    assert calls == want
    fn = dr.OracleDropout(11, 0.5, data, H, L)
    m2, _ = model_ref.hetero_forward(st, data, H, dropout_fn=fn)
    assert sorted(fn.stats) == [s for s, _ in want]
    assert not torch.allclose(m2, m0)
    m3, _ = model_ref.hetero_forward(st, data, H, dropout_fn=dr.OracleDropout(11, 0.5, data, H, L))
    assert torch.equal(m2, m3)


def test_oracle_hook_equals_f_dropout_semantics():
    """dropout_fn given the mask F.dropout drew reproduces F.dropout's training forward: the hook
    sits exactly where the F.dropout calls are."""
    import torch.nn.functional as F
    from oracle import model_ref
    st, data, H, L, _ = _tiny_case()
    p = 0.3
    torch.manual_seed(5)
    want = model_ref.hetero_forward(st, data, H, dropout=p, training=True)[0]
    torch.manual_seed(5)

    def fn(site, x):
        return F.dropout(x, p=p, training=True)

    got = model_ref.hetero_forward(st, data, H, dropout_fn=fn)[0]
    assert torch.equal(got, want)
