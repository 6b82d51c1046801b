"""The validation epoch on the device: ``eval_epoch_hetero`` (scripts/train.py:726-846).

The reference reads nine or more device values per batch on the host (``.item()`` / ``.cpu()``,
train.py:777-821) and ranks the collected ``|error|`` / ``sigma`` with SciPy at the end; each read
drains the stream, so the replayed forwards (:mod:`infer`) cannot run back to back.  Here
:meth:`EvalMetrics.update` is one kernel launch per batch into a device state block
(``alignn_eval_accumulate``), and :meth:`EvalMetrics.result` launches the counting-rank Spearman
(``alignn_eval_spearman``) and the finalizer (``alignn_eval_finalize``) and makes the epoch's single
device-to-host copy.

Differences from the reference, both stated in DESIGN.md ("Validation epoch"):

* bf16 heads are widened to fp32 and every metric is computed in fp32 (the reference's CPU/fp32
  path); under CUDA autocast the reference does part of the arithmetic in bf16.
* Spearman is always computed; the reference returns NaN for it when SciPy is not installed.
* A non-positive target under a transformer raises at :meth:`EvalMetrics.result`, not inside the
  batch loop.
"""
from __future__ import annotations

import contextlib
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from .engine import MIN_LOGVAR_FLOOR
from .ops import stream_ptr

STATE_DOUBLES = 16       # ALIGNN_EVAL_STATE_DOUBLES
OUT_DOUBLES = 10         # ALIGNN_EVAL_OUT_DOUBLES
LEVELS = 9               # ALIGNN_EVAL_LEVELS
RANK_TILE = 1024         # ALIGNN_EVAL_RANK_TILE
# indices into the state block (include/alignn_hip.h, ALIGNN_EVAL_S_*)
S_LOSS, S_GRAPHS, S_LV_SUM, S_LV_COUNT, S_SIGMA_MAX, S_COV_HITS, S_ELEMS, S_ECE_SUM, S_ECE_TERMS = range(9)
S_ABS, S_SQ, S_LOGABS, S_BAD, S_CURSOR, S_SPEARMAN = range(9, 15)

METRIC_NAMES = ("avg_loss", "mae_linear", "mae_log", "rmse_linear", "spearman_err_sigma", "mean_log_variance",
                "sigma_max", "coverage", "ece")
BAD_TARGET_MESSAGE = "Log transform encountered non-positive targets."  # train.py:273


def calibration_levels() -> Tuple[torch.Tensor, torch.Tensor]:
    """(prob_levels, z_thresholds), float32 [9] on the host, by the reference's own expression
    (train.py:796-801)."""
    prob_levels = torch.linspace(0.1, 0.9, steps=LEVELS, dtype=torch.float32)
    standard_normal = torch.distributions.Normal(torch.tensor(0.0, dtype=torch.float32),
                                                 torch.tensor(1.0, dtype=torch.float32))
    return prob_levels, standard_normal.icdf((1.0 + prob_levels) / 2.0)


def _transformer_stats(transformer):
    if transformer is None:
        return None
    if hasattr(transformer, "means") and hasattr(transformer, "stds"):
        means, stds = transformer.means, transformer.stds
    else:
        means, stds = transformer
    if means is None or stds is None:
        raise RuntimeError("LogTransformer must be fitted before use.")
    # as_tensor(float64 stats, dtype=float32): the rounding transform_tensor applies (train.py:275-276)
    return (torch.as_tensor(np.asarray(means, dtype=np.float64), dtype=torch.float32),
            torch.as_tensor(np.asarray(stds, dtype=np.float64), dtype=torch.float32))


class EvalMetrics:
    """Device-resident accumulator of the nine validation metrics.

    ``update`` makes no host read of device data; the host counts elements from shapes alone, to
    size the two epoch buffers (growth is an allocation and a device copy).  ``result`` is the one
    synchronizing call."""

    def __init__(self, target_dim: int = 2, transformer=None, min_logvar_floor: float = MIN_LOGVAR_FLOOR,
                 compute_log_mae: bool = True, capacity: int = 0, device="cuda"):
        self.T = int(target_dim)
        self.floor = float(min_logvar_floor)
        self.compute_log_mae = bool(compute_log_mae)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("EvalMetrics needs a HIP device; the engine has no CPU path")
        stats = _transformer_stats(transformer)
        if stats is not None and (stats[0].numel() != self.T or stats[1].numel() != self.T):
            raise ValueError(f"transformer statistics must have {self.T} entries")
        self._lm = stats[0].to(self.device) if stats is not None else None
        self._ls = stats[1].to(self.device) if stats is not None else None
        plev, zth = calibration_levels()
        self._plev, self._zth = plev.to(self.device), zth.to(self.device)
        init = torch.zeros(STATE_DOUBLES, dtype=torch.float64)
        init[S_SIGMA_MAX] = float("-inf")
        init[S_SPEARMAN] = float("nan")
        self._init = init.to(self.device)
        self.state = self._init.clone()
        self.capacity = max(int(capacity), 0)
        self.err_buf = torch.empty(self.capacity, dtype=torch.float32, device=self.device)
        self.sig_buf = torch.empty(self.capacity, dtype=torch.float32, device=self.device)
        self.elements = 0  # host-side count (from shapes) of the elements appended so far

    def reset(self) -> None:
        self.state.copy_(self._init)
        self.elements = 0

    def _reserve(self, n: int) -> None:
        if n <= self.capacity:
            return
        cap = max(n, 2 * self.capacity, 1024)
        for name in ("err_buf", "sig_buf"):
            old = getattr(self, name)
            new = torch.empty(cap, dtype=torch.float32, device=self.device)
            new[:self.elements].copy_(old[:self.elements])
            setattr(self, name, new)
        self.capacity = cap

    def update(self, heads, y: torch.Tensor, real_graphs: Optional[int] = None) -> None:
        """One batch: ``heads`` [B, 2T] (mean | logvar; fp32 or bf16) or the model's
        ``(mean, logvar)`` pair, ``y`` the raw targets [B, T] (or flat).  ``real_graphs``: the leading
        rows that hold real graphs of a batch padded to a capacity."""
        heads = _as_heads(heads, self.T)
        if heads.dim() != 2 or heads.size(1) != 2 * self.T:
            raise ValueError(f"heads must be [B, {2 * self.T}], got {tuple(heads.shape)}")
        if not heads.is_cuda:
            raise ValueError("heads must be a device (HIP) tensor; the engine has no CPU path")
        if heads.dtype not in (torch.float32, torch.bfloat16):
            heads = heads.float()
        if heads.stride(1) != 1:
            heads = heads.contiguous()
        B = heads.size(0) if real_graphs is None else int(real_graphs)
        if B < 0 or B > heads.size(0):
            raise ValueError(f"real_graphs = {real_graphs} outside [0, {heads.size(0)}]")
        y = y.reshape(heads.size(0), -1)
        if y.size(1) != self.T:
            raise ValueError(f"y must be [B, {self.T}], got {tuple(y.shape)}")
        y = y.to(device=heads.device, dtype=torch.float32).contiguous()
        if B == 0:
            return
        self._reserve(self.elements + B * self.T)
        _lib.check(_lib.lib().alignn_eval_accumulate(
            B, self.T, heads.data_ptr(), int(heads.dtype == torch.bfloat16), heads.stride(0), y.data_ptr(),
            self._lm.data_ptr() if self._lm is not None else None,
            self._ls.data_ptr() if self._ls is not None else None, self.floor, self._zth.data_ptr(),
            self._plev.data_ptr(), int(self.compute_log_mae), self.state.data_ptr(), self.err_buf.data_ptr(),
            self.sig_buf.data_ptr(), self.capacity, stream_ptr()), "alignn_eval_accumulate")
        self.elements += B * self.T

    def result(self, dataset_size: int = 0) -> Tuple[float, ...]:
        """The reference's 9-tuple (avg_loss, mae_linear, mae_log, rmse_linear, spearman,
        mean_log_variance, sigma_max, coverage, ece); one device-to-host copy."""
        n = self.elements
        workspace = torch.empty(2 + 3 * n, dtype=torch.float64, device=self.device)
        out = torch.empty(OUT_DOUBLES, dtype=torch.float64, device=self.device)
        spearman_ptr = self.state.data_ptr() + 8 * S_SPEARMAN
        lib = _lib.lib()
        _lib.check(lib.alignn_eval_spearman(n, self.err_buf.data_ptr(), self.sig_buf.data_ptr(), spearman_ptr,
                                            workspace.data_ptr(), stream_ptr()), "alignn_eval_spearman")
        _lib.check(lib.alignn_eval_finalize(self.state.data_ptr(), int(dataset_size), spearman_ptr,
                                            int(self.compute_log_mae), out.data_ptr(), stream_ptr()),
                   "alignn_eval_finalize")
        host = out.cpu().tolist()
        if host[OUT_DOUBLES - 1] != 0.0:
            raise ValueError(BAD_TARGET_MESSAGE)
        return tuple(host[:9])


def _as_heads(heads, T: int) -> torch.Tensor:
    """[B, 2T] from a tensor or from the (mean, logvar) pair a hetero model returns; the package's
    model returns two column views of one [B, 2T] buffer, which is used as it is."""
    if isinstance(heads, torch.Tensor):
        return heads
    mean, logvar = heads
    base = mean._base
    if (base is not None and base is logvar._base and base.dim() == 2 and base.size(1) == 2 * T
            and mean.shape == (base.size(0), T) and logvar.shape == mean.shape and base.stride(1) == 1
            and mean.stride() == base.stride() and logvar.stride() == base.stride()
            and mean.storage_offset() == base.storage_offset()
            and logvar.storage_offset() == base.storage_offset() + T):
        return base
    return torch.cat([mean, logvar.to(mean.dtype)], dim=1)


def spearman(err: torch.Tensor, sig: torch.Tensor):
    """``alignn_eval_spearman`` on two float32 device vectors: (rho, m, ranks_err, ranks_sig) as
    device tensors (rho a 0-dim double, m the number of pairs with both values finite as a 0-dim
    double, the rank vectors [n] doubles of which the first m are set, in the compacted order)."""
    err = err.contiguous().view(-1)
    sig = sig.contiguous().view(-1)
    if err.dtype != torch.float32 or sig.dtype != torch.float32 or not err.is_cuda or err.numel() != sig.numel():
        raise ValueError("spearman needs two float32 device vectors of one length")
    n = err.numel()
    workspace = torch.zeros(2 + 3 * n, dtype=torch.float64, device=err.device)
    out = torch.empty((), dtype=torch.float64, device=err.device)
    _lib.check(_lib.lib().alignn_eval_spearman(n, err.data_ptr(), sig.data_ptr(), out.data_ptr(),
                                                workspace.data_ptr(), stream_ptr()), "alignn_eval_spearman")
    return out, workspace[0], workspace[2:2 + n], workspace[2 + n:2 + 2 * n]


def _resident(batch, device: torch.device) -> bool:
    """True when every tensor of the batch already lives on ``device`` (``batch.to`` would move nothing)."""
    index = device.index if device.index is not None else (torch.cuda.current_device() if device.type == "cuda" else None)
    tensors = [v for v in vars(batch).values() if isinstance(v, torch.Tensor)]
    return bool(tensors) and all(t.device.type == device.type and t.device.index == index for t in tensors)


def eval_epoch_hetero(model, loader, device, transformer=None, use_amp: bool = False, compute_log_mae: bool = True,
                      progress_desc: Optional[str] = None,
                      min_logvar_floor: float = MIN_LOGVAR_FLOOR) -> Tuple[float, ...]:
    """Drop-in for the reference's ``eval_epoch_hetero`` (same arguments, same 9-tuple); the metrics
    accumulate on the device and the host reads them once, after the last batch.
    ``progress_desc`` is accepted for the signature; the reference does not use it either."""
    device = torch.device(device)
    model.eval()
    amp_enabled = use_amp and device.type == "cuda"
    metrics = None
    with torch.no_grad():
        for batch in loader:
            if not _resident(batch, device):  # Data.to drops the batch's device-side caches even when nothing moves
                batch = batch.to(device)
            ctx = torch.autocast(device_type="cuda", dtype=torch.bfloat16) if amp_enabled else contextlib.nullcontext()
            with ctx:
                mean, logvar = model(batch)
            if metrics is None:
                metrics = EvalMetrics(mean.size(1), transformer, min_logvar_floor, compute_log_mae, device=mean.device)
            metrics.update((mean, logvar), batch.y)
    dataset_size = len(loader.dataset) if hasattr(loader, "dataset") else 0
    if metrics is None:  # no batches: the reference's empty-epoch values, still formed by the finalizer
        T = getattr(getattr(model, "config", None), "target_dim", 2)
        metrics = EvalMetrics(T, transformer, min_logvar_floor, compute_log_mae, device=device)
    return metrics.result(dataset_size)
