"""fp32 against bf16-mixed against bf16-train (engine precision=...) on bench.py's train loop, as alternating rounds on one box: the
workload bench.make_batch builds (600x1000 panel, synthetic boxes), shipped launch-shape tables, the pipelined step with
`upcoming`, warm-up and drain as bench.py does them.  Prints ms per step and images/s of every run, then the per-layer table
of the training-shape forward convs (fp32 launch as the engine chooses it, bf16 with ksplit = 1, bf16 with the split rule) and the
per-layer BACKWARD table (each training-shape data gradient and weight gradient alone: the fp32 launch as the engine chooses it
against the bf16 kernel with the split rule).
usage: python tools/train_timing_bf16.py [rounds=5] [per_gpu_batch=1] [steps=60]
With --profile-mixed / --profile-train: only runs 40 steps of that mode (the window for rocprofv3 --kernel-trace --stats)."""
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
        im = eng.bf16.fwd[d.w]
        wt, ldk, c = im.wt, im.ldk, im.conv
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


def backward_table(eng, eng32, nb):
    """ms per launch of every distinct training-shape conv gradient, fp32 (radnet_conv_dgrad / radnet_conv_wgrad as the fp32 engine
    launches them, each alone) against the bf16 kernel with the engine's split."""
    bp = eng._plan_base(nb, 600, 1000)
    rp = eng._plan_rpn(bp["fh"], bp["fw"], bp["F"], nb=nb)
    hp = eng._plan_head(eng.C.n_rois * nb, bp["fh"], bp["fw"], bp["F"], training=True, groups=nb)
    by_ptr = {c.weight.data_ptr(): c for c in eng.convs.values() if c.weight is not None}
    seen, rows = set(), []

    def t(fn, n=20):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3
    for kind, d in rp["bwd"] + hp["bwd"]:
        if kind not in ("dgrad_bf16", "wgrad_bf16"):
            continue
        M, N, K = d.nb * d.oh * d.ow, d.n, d.kh * d.kw * d.c
        if (kind, M, N, K, d.kh, d.stride) in seen:
            continue
        seen.add((kind, M, N, K, d.kh, d.stride))
        c = by_ptr[d.w]
        d32 = L.ConvDesc.from_buffer_copy(d)
        d32.w = eng32.convs[c.name].weight.data_ptr()
        d32.dw = eng32.convs[c.name].dweight.data_ptr()
        d32.db = None
        if kind == "dgrad_bf16":
            wd, ldkd = eng.bf16.dgrad[d.w].wd, eng.bf16.dgrad[d.w].ldkd
            s = int(eng.lib.radnet_dgrad_bf16_pick_split(d.nb * d.h * d.w_, d.c, d.kh * d.kw * ((d.n + 7) // 8 * 8)))
            f32 = t(lambda: eng32.ctx.check(eng32.lib.radnet_conv_dgrad(eng32.ctx.h, C.byref(d32)), "dgrad"))
            b16 = t(lambda: eng.ctx.check(eng.lib.radnet_conv_dgrad_bf16_split(eng.ctx.h, C.byref(d), wd.data_ptr(), ldkd, s), "dgrad_bf16"))
        else:
            s = int(eng.lib.radnet_wgrad_bf16_pick_split(M, N, K))
            f32 = t(lambda: eng32.ctx.check(eng32.lib.radnet_conv_wgrad(eng32.ctx.h, C.byref(d32)), "wgrad"))
            b16 = t(lambda: eng.ctx.check(eng.lib.radnet_conv_wgrad_bf16(eng.ctx.h, C.byref(d), s), "wgrad_bf16"))
        rows.append((c.name, kind[:5], M, N, K, f32, s, b16, f32 / b16))
    print("%-18s %-5s %6s %5s %6s %9s %3s %9s %7s" % ("layer", "grad", "M", "N", "K", "fp32 ms", "s", "bf16 ms", "ratio"))
    for r in rows:
        print("%-18s %-5s %6d %5d %6d %9.4f %3d %9.4f %7.2f" % r)
    eng.zero_grads(eng.rpn_arena), eng.zero_grads(eng.head_arena), eng32.zero_grads(eng32.rpn_arena), eng32.zero_grads(eng32.head_arena)
    torch.cuda.synchronize()


ARMS = ("fp32", "bf16-mixed", "bf16-train")


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    pairs = int(args[0]) if args else 5
    per_gpu = int(args[1]) if len(args) > 1 else 1
    steps = int(args[2]) if len(args) > 2 else 60
    batch = bench.make_batch(0, per_gpu, 600, 1000)
    np.random.seed(64)
    for flag, mode in (("--profile-mixed", "bf16-mixed"), ("--profile-train", "bf16-train")):
        if flag in sys.argv:
            _, ts = make(mode)
            run(ts, batch, 40)
            return
    made = {name: make(name) for name in ARMS}
    for name in ARMS:
        run(made[name][1], batch, 20)
    res = {name: [] for name in ARMS}
    for p in range(pairs):
        for name in ARMS[p % 3:] + ARMS[:p % 3]:            # the order rotates from round to round
            ms = timed(made[name][1], batch, steps)
            res[name].append(ms)
            print("round %d %-10s %.4f ms/step  %.1f images/s" % (p, name, ms, per_gpu * 1e3 / ms), flush=True)
    for name, v in res.items():
        print("%-10s median %.4f ms/step  %.1f images/s  (batch %d, %d rounds)" % (name, np.median(v), per_gpu * 1e3 / np.median(v), per_gpu, pairs))
    print("bf16-mixed / fp32 speed-up %.3fx" % (np.median(res["fp32"]) / np.median(res["bf16-mixed"])))
    print("bf16-train / fp32 speed-up %.3fx" % (np.median(res["fp32"]) / np.median(res["bf16-train"])))
    print("bf16-train / bf16-mixed speed-up %.3fx" % (np.median(res["bf16-mixed"]) / np.median(res["bf16-train"])))
    layer_table(made["bf16-mixed"][0], made["fp32"][0], per_gpu)
    backward_table(made["bf16-train"][0], made["fp32"][0], per_gpu)


if __name__ == "__main__":
    main()
