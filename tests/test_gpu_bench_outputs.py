"""bench.py --dump-outputs: the arrays written are what the timed path (FusedTrainer.step, replayed
plan) left after its last timed step — nothing runs between that step and the copy — ``--steps``
sets the number of timed steps, and a second run with the same arguments gives the same arrays bit
for bit (seeded weights, graphs and step seeds), so two builds can be compared output for output."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _args(monkeypatch, *argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_dump_outputs_are_the_last_timed_steps_and_repeat(monkeypatch, tmp_path):
    import bench
    out_dir = str(tmp_path / "out")
    args = _args(monkeypatch, "--gpus", "1", "--batch", "4", "--steps", "3", "--warmup", "2", "--dump-outputs", out_dir)
    assert args.e2e == 0 and args.no_roofline and args.no_cpu_baseline and args.no_secondary   # a plain run
    dev = torch.device("cuda", 0)
    runs = []
    for _ in range(2):
        r = bench.measure(args, dev, 0, 1, args.batch, args.lg_offset, args.precision, args.steps, args.warmup,
                          roofline=not args.no_roofline, keep_outputs=True)
        tr, outs = r["trainer"], r.pop("outputs")
        assert tr.replays == args.steps + args.warmup          # --steps timed steps after --warmup, all replayed
        assert r["ms_per_step"] == pytest.approx(r["dt"] / args.steps * 1e3)
        assert set(outs) == {"loss", "params", "grad", "grad_norm"}
        # the copies are the state the last timed step left
        assert torch.equal(outs["loss"], tr.loss) and torch.equal(outs["params"], tr.st.flat)
        assert torch.equal(outs["grad"], tr.st.grad) and torch.equal(outs["grad_norm"], tr.gnorm)
        assert all(bool(torch.isfinite(v).all()) for v in outs.values())
        runs.append({k: v.cpu() for k, v in outs.items()})
        bench._release(r)
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
    bench.dump_outputs(out_dir, runs[0])
    total = 0
    for k, v in runs[0].items():
        a = np.load(os.path.join(out_dir, k + ".npy"))
        assert a.dtype == np.float32 and np.array_equal(a, v.numpy().reshape(-1)), k
        total += a.nbytes
    assert total <= 64 * 2**20


def test_large_outputs_are_written_as_a_fixed_sample(monkeypatch, tmp_path):
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 1000)
    t = torch.arange(5000, dtype=torch.float32, device="cuda")
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"x": t, "small": t[:10]})
    a, b = (np.load(str(tmp_path / d / "x.npy")) for d in ("a", "b"))
    assert a.shape == (1000,) and np.array_equal(a, b) and np.all(np.diff(a) > 0)
    assert np.array_equal(np.load(str(tmp_path / "a" / "small.npy")), np.arange(10, dtype=np.float32))
