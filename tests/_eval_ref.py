"""float64 NumPy restatement of the reference's validation epoch (``eval_epoch_hetero``,
scripts/train.py:726-846), average-rank Spearman included (no SciPy).  Checked against the golden
written by the reference itself in tests/test_eval_host.py; the GPU tests use it where the golden
has no case (bf16 heads, other batchings, the state block, the ranks).

Inputs are the fp32 values the kernel sees, widened to float64; the transformer statistics and the
z thresholds are rounded to fp32 first, as the reference rounds them."""
import math

import numpy as np

BAD_TARGET_MESSAGE = "Log transform encountered non-positive targets."  # train.py:273
NAMES = ("avg_loss", "mae_linear", "mae_log", "rmse_linear", "spearman_err_sigma", "mean_log_variance", "sigma_max",
         "coverage", "ece")


def average_ranks(x):
    """rank_i = #(x_j < x_i) + (#(x_j == x_i) + 1) / 2 (scipy.stats.rankdata, method='average')."""
    x = np.asarray(x, dtype=np.float64)
    less = (x[None, :] < x[:, None]).sum(1)
    equal = (x[None, :] == x[:, None]).sum(1)
    return less + 0.5 * (equal + 1)


def spearman(err, sig):
    """(rho, m, ranks_err, ranks_sig) over the pairs with both values finite (train.py:834-837)."""
    err, sig = np.asarray(err, dtype=np.float64).ravel(), np.asarray(sig, dtype=np.float64).ravel()
    ok = np.isfinite(err) & np.isfinite(sig)
    m = int(ok.sum())
    rx, rs = average_ranks(err[ok]), average_ranks(sig[ok])
    if m < 2:
        return float("nan"), m, rx, rs
    a, b = rx - rx.mean(), rs - rs.mean()
    sxx, syy = float((a * a).sum()), float((b * b).sum())
    if sxx == 0.0 or syy == 0.0:
        return float("nan"), m, rx, rs
    return float((a * b).sum() / math.sqrt(sxx * syy)), m, rx, rs


def eval_epoch(head_batches, y_batches, dataset_size, log_means, log_stds, floor, z_thresholds, prob_levels,
               compute_log_mae=True):
    """The epoch over lists of [B, 2T] heads and [B, T] raw targets.  Returns a dict: ``out`` (the
    9-tuple), ``err`` / ``sig`` (the collected Spearman inputs), ``ece_pooled`` (what pooling the hits
    over the epoch would give: not what the reference computes), and the epoch sums by name."""
    z = np.asarray(z_thresholds, dtype=np.float32).astype(np.float64)
    p = np.asarray(prob_levels, dtype=np.float32).astype(np.float64)
    has_tf = log_means is not None
    if has_tf:
        m = np.asarray(log_means, dtype=np.float64).astype(np.float32).astype(np.float64)[None]
        s = np.asarray(log_stds, dtype=np.float64).astype(np.float32).astype(np.float64)[None]
    st = dict(loss=0.0, graphs=0, lv_sum=0.0, lv_count=0, sigma_max=float("-inf"), hits=0, elems=0, ece_sum=0.0,
              ece_terms=0, abs=0.0, sq=0.0, logabs=0.0)
    errs, sigs, level_hits = [], [], np.zeros(len(z))
    with np.errstate(all="ignore"):
        for h, y in zip(head_batches, y_batches):
            h, y = np.asarray(h, dtype=np.float64), np.asarray(y, dtype=np.float64)
            B, T = y.shape
            if B == 0:
                continue
            mean, lv = h[:, :T], h[:, T:]
            lv = np.maximum(lv, floor)  # np.maximum keeps a NaN, as torch.clamp does
            var = np.exp(lv)
            sigma = np.sqrt(var)
            if has_tf:
                if np.any(y <= 0):
                    raise ValueError(BAD_TARGET_MESSAGE)
                yz, pred = (np.log(y) - m) / s, np.exp(mean * s + m)
            else:
                yz, pred = y, mean
            d = mean - yz
            st["loss"] += float((0.5 * (lv + d * d / var)).mean(1).sum())
            st["graphs"] += B
            st["lv_sum"] += float(lv.sum())
            st["lv_count"] += lv.size
            bmax = float("nan") if np.isnan(sigma).any() else float(sigma.max())
            st["sigma_max"] = max(st["sigma_max"], bmax)  # Python's max: a NaN second argument is dropped
            ad = np.abs(d)
            st["hits"] += int((ad <= sigma).sum())
            st["elems"] += ad.size
            hits_l = (ad[None] <= z[:, None, None] * sigma[None]).sum((1, 2))
            level_hits += hits_l
            st["ece_sum"] += float(np.abs(hits_l / ad.size - p).sum())
            st["ece_terms"] += len(p)
            st["abs"] += float(np.abs(pred - y).sum())
            st["sq"] += float(((pred - y) ** 2).sum())
            if compute_log_mae:
                st["logabs"] += float(np.abs(np.log(np.maximum(pred, 1e-6)) - np.log(np.maximum(y, 1e-6))).sum())
            errs.append(ad.ravel())
            sigs.append(np.maximum(sigma, 1e-6).ravel())
    err = np.concatenate(errs) if errs else np.zeros(0)
    sig = np.concatenate(sigs) if sigs else np.zeros(0)
    rho = spearman(err, sig)[0]
    nan = float("nan")
    out = (st["loss"] / st["graphs"] if st["graphs"] > 0 else 0.0,
           st["abs"] / dataset_size if dataset_size > 0 else 0.0,
           st["logabs"] / dataset_size if (dataset_size > 0 and compute_log_mae) else nan,
           math.sqrt(st["sq"] / st["elems"]) if st["elems"] > 0 else nan,
           rho,
           st["lv_sum"] / st["lv_count"] if st["lv_count"] > 0 else nan,
           st["sigma_max"] if st["sigma_max"] > float("-inf") else nan,
           st["hits"] / st["elems"] if st["elems"] > 0 else nan,
           st["ece_sum"] / st["ece_terms"] if st["ece_terms"] > 0 else nan)
    ece_pooled = float(np.abs(level_hits / st["elems"] - p).mean()) if st["elems"] > 0 else nan
    return dict(st, out=out, err=err, sig=sig, ece_pooled=ece_pooled)


def split(a, sizes):
    return np.split(np.asarray(a), np.cumsum(sizes)[:-1])


# Bounds of the checks against the reference (and against this restatement): the four error metrics,
# loss and mean log-variance at the project's fp32 bar (BASELINE.json), sigma_max at 1e-5 relative,
# coverage equal, ECE at 1e-6 absolute (the reference rounds nine per-batch means and levels to
# fp32, each <= 1.2e-7), Spearman at 1e-9 absolute (equal ranks, both sides correlate in double).
REL_BOUND = {"avg_loss": 1e-4, "mae_linear": 1e-4, "mae_log": 1e-4, "rmse_linear": 1e-4, "mean_log_variance": 1e-4,
             "sigma_max": 1e-5}
ABS_BOUND = {"ece": 1e-6, "spearman_err_sigma": 1e-9}


def check_metrics(got, want, label=""):
    """Assert the 9-tuple ``got`` against ``want`` under the bounds above; NaN exactly where ``want``
    has NaN.  Prints every figure first."""
    assert len(got) == len(want) == len(NAMES)
    for name, g, w in zip(NAMES, got, want):
        g, w = float(g), float(w)
        print(f"{label}{name}: got {g!r} want {w!r}")
    for name, g, w in zip(NAMES, got, want):
        g, w = float(g), float(w)
        if math.isnan(w) or math.isnan(g):
            assert math.isnan(w) and math.isnan(g), (name, g, w)
        elif name == "coverage":
            assert g == w, (name, g, w)
        elif name in ABS_BOUND:
            assert abs(g - w) <= ABS_BOUND[name], (name, g, w)
        else:
            assert abs(g - w) <= REL_BOUND[name] * abs(w), (name, g, w)
