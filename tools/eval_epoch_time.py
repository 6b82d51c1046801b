"""Wall time of one validation epoch, three ways, over resident synthetic batches (fp32, eval mode):

  host_loop   the reference's per-batch metric code (train.py:760-821: nine or more .item()/.cpu()
              reads per batch, SciPy's spearmanr at the end) restated here around the package's
              model(batch),
  device      alignn_mi355x.eval_epoch_hetero (one launch per batch, one device-to-host copy per epoch),
  forwards    model(batch) alone, the floor both are measured against.

Each figure is the median of --reps epochs after one warm-up epoch, host clock with a device
synchronize before and after.  The last line printed is one JSON object; it also carries the
host-read count of each loop and the largest relative difference between the two 9-tuples.

usage: python tools/eval_epoch_time.py [--batch 32] [--batches 32] [--reps 7] [--hidden 256] [--layers 4]
"""
import argparse
import json
import math
import os
import sys
import time

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(REPO, "gnn-elasticity-predictor_amd"))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

try:
    from scipy.stats import spearmanr
except ImportError:  # the reference then leaves Spearman at NaN
    spearmanr = None


class Reads:
    """Counts the host reads of device data the loop makes."""
    n = 0

    @classmethod
    def item(cls, t):
        cls.n += 1
        return t.item()

    @classmethod
    def cpu(cls, t):
        cls.n += 1
        return t.cpu()


def host_loop_epoch(model, loader, means, stds, floor):
    """The reference's loop body around the package's forward; returns its 9-tuple."""
    tot = dict(loss=0.0, w=0.0, abs=0.0, log=0.0, sq=0.0, n=0, lv=0.0, lvn=0, cov=0.0, ece=0.0, ecen=0)
    smax, errs, sigs, plev, zth = float("-inf"), [], [], None, None
    with torch.no_grad():
        for batch in loader:
            y = batch.y.view(batch.num_graphs, -1)
            yz = (torch.log(y) - means) / stds
            mean, logvar = model(batch)
            logvar = torch.clamp(logvar, min=floor)
            var = torch.exp(logvar)
            sigma = torch.sqrt(var)
            nll = 0.5 * (logvar + (mean - yz).pow(2) / var)
            tot["loss"] += Reads.item(nll.mean(dim=1).sum())
            tot["w"] += batch.num_graphs
            tot["lv"] += Reads.item(logvar.sum())
            tot["lvn"] += logvar.numel()
            smax = max(smax, float(Reads.item(sigma.max())))
            pred = torch.exp(mean * stds + means)
            ad = torch.abs(mean - yz)
            tot["cov"] += Reads.item((ad <= sigma).float().sum())
            if plev is None:
                plev = torch.linspace(0.1, 0.9, steps=9, device=mean.device, dtype=torch.float32)
                normal = torch.distributions.Normal(torch.tensor(0.0, device=mean.device), torch.tensor(1.0, device=mean.device))
                zth = normal.icdf((1.0 + plev) / 2.0).view(-1, 1, 1)
            cov_l = (ad.unsqueeze(0) <= zth * sigma.unsqueeze(0)).float().mean(dim=[1, 2])
            tot["ece"] += Reads.item(torch.abs(cov_l - plev).sum())
            tot["ecen"] += 9
            tot["abs"] += Reads.item(F.l1_loss(pred, y, reduction="sum"))
            tot["sq"] += Reads.item((pred - y).pow(2).sum())
            tot["n"] += y.numel()
            if spearmanr is not None:
                errs.append(Reads.cpu((yz - mean).abs()))
                sigs.append(torch.clamp(Reads.cpu(sigma), min=1e-6))
            tot["log"] += Reads.item(F.l1_loss(torch.log(torch.clamp(pred, min=1e-6)),
                                               torch.log(torch.clamp(y, min=1e-6)), reduction="sum"))
    ds = len(loader.dataset)
    rho = float("nan")
    if errs:
        e, s = torch.cat(errs).view(-1).numpy(), torch.cat(sigs).view(-1).numpy()
        ok = np.isfinite(e) & np.isfinite(s)
        if ok.sum() > 1:
            rho = float(spearmanr(e[ok], s[ok])[0])
    return (tot["loss"] / tot["w"], tot["abs"] / ds, tot["log"] / ds, math.sqrt(tot["sq"] / tot["n"]), rho,
            tot["lv"] / tot["lvn"], smax, tot["cov"] / tot["n"], tot["ece"] / tot["ecen"])


def forwards_epoch(model, loader):
    with torch.no_grad():
        for batch in loader:
            model(batch)


def timed(fn, reps):
    fn()  # warm-up epoch
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1]}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--batches", type=int, default=32)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--hidden", type=int, default=256)
    p.add_argument("--layers", type=int, default=4)
    p.add_argument("--heads", type=int, default=4)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_epoch_time: needs a HIP device (a CPU timing says nothing about the GPU)")

    import alignn_mi355x as A
    from alignn_mi355x.engine import MIN_LOGVAR_FLOOR
    from alignn_mi355x.synthetic import TARGET_LOG_MEANS, TARGET_LOG_STDS, mp_like_batch
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = A.HeteroAlignnRegressor(A.AlignnRegressor(206, 36, 11, 289, 2, args.hidden, args.layers, args.heads, 0.15),
                                    2).to(dev).eval()

    class Loader(list):
        dataset = range(args.batch * args.batches)

    loader = Loader(mp_like_batch(args.batch, first=args.batch * i).to(dev) for i in range(args.batches))
    means = torch.tensor(TARGET_LOG_MEANS, dtype=torch.float32, device=dev)
    stds = torch.tensor(TARGET_LOG_STDS, dtype=torch.float32, device=dev)
    transformer = (TARGET_LOG_MEANS, TARGET_LOG_STDS)

    Reads.n = 0
    ref_out = host_loop_epoch(model, loader, means, stds, MIN_LOGVAR_FLOOR)
    reads_host = Reads.n
    new_out = A.eval_epoch_hetero(model, loader, dev, transformer=transformer)
    diff = max(abs(a - b) / max(abs(a), 1e-30) for a, b in zip(ref_out, new_out))

    res = {
        "tool": "eval_epoch_time", "device_name": torch.cuda.get_device_name(0), "batch": args.batch,
        "batches": args.batches, "hidden": args.hidden, "layers": args.layers, "reps": args.reps,
        "forwards_epoch": timed(lambda: forwards_epoch(model, loader), args.reps),
        "host_loop_epoch": timed(lambda: host_loop_epoch(model, loader, means, stds, MIN_LOGVAR_FLOOR), args.reps),
        "device_epoch": timed(lambda: A.eval_epoch_hetero(model, loader, dev, transformer=transformer), args.reps),
        "host_reads_per_epoch": {"host_loop": reads_host, "device": 1},
        "host_loop_metrics": ref_out, "device_metrics": new_out, "max_rel_diff": diff,
        "scipy": spearmanr is not None,
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
