"""fp32 against bf16-mixed (engine precision="bf16-mixed") on bench.py's train loop, as alternating A/B pairs on one box: the
workload bench.make_batch builds (600x1000 panel, synthetic boxes), shipped launch-shape tables, the pipelined step with
`upcoming`, warm-up and drain as bench.py does them.  Prints ms per step and images/s of every run, then the per-layer table
of the training-shape forward convs (fp32 launch as the engine chooses it, bf16 with ksplit = 1, bf16 with the split rule).
usage: python tools/train_timing_bf16.py [pairs=5] [per_gpu_batch=1] [steps=60]
With --profile-mixed: only runs 40 bf16-mixed steps (the window for rocprofv3 --kernel-trace --stats)."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rock-art-radnet_amd")]
import torch  # noqa: E402

import bench  # noqa: E402
from faster_rcnn.config import Config  # noqa: E402
from radnet_hip import lib as L, synth  # noqa: E402
from radnet_hip.engine import FasterRCNNEngine  # noqa: E402
from radnet_hip.trainer import TrainStep  # noqa: E402


def make(precision):
    eng = FasterRCNNEngine(Config(), **({} if precision == "fp32" else dict(precision=precision)))
    eng.set_weights(synth.synthetic_weights(seed=3))
    return eng, TrainStep(eng)


def run(ts, batch, n):
    look = getattr(ts, "LOOKAHEAD", 3)
    for k in range(n):
        ts.step(batch, upcoming=[batch] * min(look, n - 1 - k))
    ts.flush()
    torch.cuda.synchronize()


def timed(ts, batch, steps):
    run(ts, batch, 10)
    t0 = time.perf_counter()
    run(ts, batch, steps)
    return (time.perf_counter() - t0) / steps * 1e3


def layer_table(eng, eng32, nb):
    """ms per launch of every distinct training-shape forward conv (base, RPN, classifier) in the three forms."""
    bp = eng._plan_base(nb, 600, 1000)
    rp = eng._plan_rpn(bp["fh"], bp["fw"], bp["F"], nb=nb)
    hp = eng._plan_head(eng.C.n_rois * nb, bp["fh"], bp["fw"], bp["F"], training=True, groups=nb)
    seen = set()
    rows = []
    for kind, d in bp["ops"] + rp["fwd"] + hp["fwd"]:
        if kind != "conv_bf16":
            continue
        M, N, K = d.nb * d.oh * d.ow, d.n, d.kh * d.kw * d.c
        if (M, N, K, d.kh, d.stride) in seen:
            continue
        seen.add((M, N, K, d.kh, d.stride))
        wt, ldk, c, _ = eng._bf16_w[d.w]
        s = int(eng.lib.radnet_conv_bf16_pick_split(M, N, K))
        d32 = L.ConvDesc.from_buffer_copy(d)
        d32.w = eng32.convs[c.name].weight.data_ptr()

        def t(fn, n=20):
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n * 1e3
        f32 = t(lambda: eng32.ctx.check(eng32.lib.radnet_conv_fwd(eng32.ctx.h, C.byref(d32)), "conv_fwd"))
        b1 = t(lambda: eng.ctx.check(eng.lib.radnet_conv_fwd_bf16_split(eng.ctx.h, C.byref(d), wt.data_ptr(), ldk, 1), "bf16"))
        bs = t(lambda: eng.ctx.check(eng.lib.radnet_conv_fwd_bf16_split(eng.ctx.h, C.byref(d), wt.data_ptr(), ldk, s), "bf16"))
        rows.append((c.name, M, N, K, f32, b1, s, bs))
    print("%-18s %6s %5s %6s %9s %9s %3s %9s" % ("layer", "M", "N", "K", "fp32 ms", "bf16 s=1", "s", "bf16 s"))
    for r in rows:
        print("%-18s %6d %5d %6d %9.4f %9.4f %3d %9.4f" % r)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    pairs = int(args[0]) if args else 5
    per_gpu = int(args[1]) if len(args) > 1 else 1
    steps = int(args[2]) if len(args) > 2 else 60
    batch = bench.make_batch(0, per_gpu, 600, 1000)
    np.random.seed(64)
    if "--profile-mixed" in sys.argv:
        _, ts = make("bf16-mixed")
        run(ts, batch, 40)
        return
    (e32, t32), (e16, t16) = make("fp32"), make("bf16-mixed")
    run(t32, batch, 20)
    run(t16, batch, 20)
    res = {"fp32": [], "bf16-mixed": []}
    for p in range(pairs):
        for name, ts in (("fp32", t32), ("bf16-mixed", t16)) if p % 2 == 0 else (("bf16-mixed", t16), ("fp32", t32)):
            ms = timed(ts, batch, steps)
            res[name].append(ms)
            print("pair %d %-10s %.4f ms/step  %.1f images/s" % (p, name, ms, per_gpu * 1e3 / ms), flush=True)
    for name, v in res.items():
        print("%-10s median %.4f ms/step  %.1f images/s  (batch %d, %d pairs)" % (name, np.median(v), per_gpu * 1e3 / np.median(v), per_gpu, pairs))
    print("speed-up %.3fx" % (np.median(res["fp32"]) / np.median(res["bf16-mixed"])))
    layer_table(e16, e32, per_gpu)


if __name__ == "__main__":
    main()
