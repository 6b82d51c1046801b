"""Host restatement of the engine's dropout masks (test helper, numpy only).

The kernels draw no random numbers: element ``idx`` of a dropout site is kept iff
``hash_u32(seed, idx) >= uint32(p * 2^32)`` (csrc/common.h: hash_u32, dropout_mul, make_drop) and a
kept element is scaled by ``1/(1-p)``.  ``seed`` is the site's seed, ``engine.site_seed(step seed,
site)``; a trainer that registered a device step seed mixes it in first (common.h: mix_seed).  The
element index of each site is listed in DESIGN.md ("dropout sites and mask indices"); the builders
below turn those into masks laid out like the tensors the fp64 oracle drops (original edge order).
"""
from __future__ import annotations

import numpy as np
import torch

_M64 = (1 << 64) - 1


def hash_u32(seed: int, idx) -> np.ndarray:
    """common.h hash_u32: a 64-bit finaliser of seed ^ idx * golden ratio, upper 32 bits.  ``idx``:
    integer array (or scalar), taken modulo 2^64 like the kernels' uint64_t."""
    a = np.asarray(idx)
    if a.dtype == object:   # Python ints past 2^64 - 1
        i = np.asarray([int(v) & _M64 for v in a.reshape(-1)], dtype=np.uint64).reshape(a.shape)
    else:
        i = a.astype(np.uint64)
    with np.errstate(over="ignore"):
        x = np.uint64(int(seed) & _M64) ^ (i * np.uint64(0x9E3779B97F4A7C15))
        x = x ^ (x >> np.uint64(33))
        x = x * np.uint64(0xFF51AFD7ED558CCD)
        x = x ^ (x >> np.uint64(33))
        x = x * np.uint64(0xC4CEB9FE1A85EC53)
        x = x ^ (x >> np.uint64(33))
    return (x >> np.uint64(32)).astype(np.uint32)


def thresh(p: float) -> int:
    """common.h make_drop: (uint32)(p * 2^32), p as the float the C ABI receives, capped at 2^32-1."""
    p = float(np.float32(p))
    if p <= 0.0:
        return 0
    return int(min(p * 4294967296.0, 4294967295.0))


def keep_mask(seed: int, numel: int, p: float, start: int = 0) -> np.ndarray:
    """bool[numel]: element start + i survives dropout p under ``seed``."""
    idx = np.arange(int(numel), dtype=np.uint64) + np.uint64(int(start) & _M64)
    return hash_u32(seed, idx) >= np.uint32(thresh(p))


def inv_keep(p: float) -> float:
    """The kept elements' multiplier as the kernels hold it: fp32 1/(1-p) of the fp32 p."""
    p32 = np.float32(p)
    return float(np.float32(1.0) / (np.float32(1.0) - p32)) if p32 < 1.0 else 0.0


def site_seed(seed: int, site: int) -> int:
    """engine.site_seed: the per-site seed of step seed ``seed``."""
    return (int(seed) * 0x9E3779B1 + int(site) * 0x85EBCA77 + 0x165667B1) & (2 ** 63 - 1)


def mix_seed(site: int, step: int) -> int:
    """common.h mix_seed: the seed a kernel uses when a device step seed ``step`` is registered."""
    x = ((int(step) + 0x632BE59BD9B4E019) * 0x9E3779B97F4A7C15) & _M64
    x ^= x >> 31
    return (int(site) ^ x) & _M64


# ------------------------------------------------------------------------------------------------
# Masks in the layout of the tensors the oracle drops
# ------------------------------------------------------------------------------------------------
def dense_mask(seed: int, rows: int, cols: int, p: float) -> torch.Tensor:
    """Row-major sites (gate/LayerNorm blocks, readout feats, shared layer): element r * cols + c."""
    return torch.from_numpy(keep_mask(seed, rows * cols, p).reshape(rows, cols))


def edge_mask(seed: int, dst: torch.Tensor, heads: int, p: float) -> torch.Tensor:
    """Attention sites: bool [m, H] in ORIGINAL edge order.  The kernels index element t * H + h with
    t the edge's position in the stable target-sorted order (GraphCSR.perm_dst; the line graph's
    compaction renumbers targets monotonically, so the order is that of the original targets)."""
    m = int(dst.numel())
    perm = torch.argsort(dst, stable=True)
    sorted_mask = torch.from_numpy(keep_mask(seed, m * heads, p).reshape(m, heads))
    out = torch.empty(m, heads, dtype=torch.bool)
    out[perm] = sorted_mask
    return out


class OracleDropout:
    """``dropout_fn`` for oracle.model_ref.hetero_forward: site k of a step with seed ``seed`` and
    rate p gets the engine's mask for that site.  Records each site's dropped fraction and size.
    ``flip``: a site whose mask rows are reversed (a deliberately wrong convention, for the guards)."""

    def __init__(self, seed: int, p: float, data, heads: int, layers: int, flip=None):
        self.seed, self.p, self.H, self.L, self.flip = seed, p, heads, layers, flip
        self.lg_dst = data.lg_edge_index[1]
        self.ag_dst = data.edge_index[1]
        self.stats = {}
        self._cache = {}

    def mask(self, site: int, shape) -> torch.Tensor:
        key = (site, tuple(shape))
        if key not in self._cache:
            s = site_seed(self.seed, site)
            if site < 4 * self.L and site % 2 == 0:
                dst = self.lg_dst if site % 4 == 0 else self.ag_dst
                assert tuple(shape) == (dst.numel(), self.H), (site, shape)
                mk = edge_mask(s, dst, self.H, self.p)
            else:
                assert len(shape) == 2, (site, shape)
                mk = dense_mask(s, shape[0], shape[1], self.p)
            if self.flip == site:
                mk = mk.flip(0)
            self._cache[key] = mk
        return self._cache[key]

    def __call__(self, site: int, x: torch.Tensor) -> torch.Tensor:
        mk = self.mask(site, x.shape)
        self.stats[site] = (int(mk.numel()), float((~mk).double().mean()) if mk.numel() else 0.0)
        return x * mk.to(x.dtype) / (1.0 - self.p)
