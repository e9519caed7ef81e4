"""CPU emulation of the bf16-mixed training mode (engine precision="bf16-mixed"), to calibrate the bounds of
tests/test_gpu_bf16_mixed.py.  Runs the NumPy oracle's training step (oracle/step.py, OracleTrainer.step with override_R) on one
synthetic sample twice, from the same weights:
  fp32  as it is;
  bf16  both operands of every FORWARD conv with a multiple of 8 input channels rounded to bf16 (round to nearest even) before an
        fp32 accumulation -- tools/bf16_emulate.py's dense.conv2d swap.  The oracle's backward (dense.conv2d_bwd) does not call
        dense.conv2d, so it stays fp32 on the fp32 weights and on the activations the rounded forward produced: the arithmetic of
        the engine's bf16-mixed step.
  bf16-train  the bf16 run plus dense.conv2d_bwd swapped for conv2d_bwd_bf16 below: x, w and dz rounded to bf16 before the fp32
        accumulation of both gradients, the bias gradient from the unrounded dz -- the arithmetic of the engine's bf16-train step
        (csrc/conv_bf16_bwd.hip).  The swap lives here, as the forward swap lives in tools/bf16_emulate.py; oracle/ is not edited.
The proposals of the fp32 pass are fed to all three (override_R), so they label the same RoIs.  Reports the five losses, the relative
Frobenius difference of every trainable layer's gradient (before Adam) and of the weights after k = 1 and k = 4 steps.
Without arguments both the 240x400 and the 600x1000 panel are run.
usage: python tools/bf16_train_emulate.py [height width [seed=3]]"""
import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rock-art-radnet_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402

import bf16_emulate as E  # noqa: E402
from faster_rcnn.config import Config  # noqa: E402
from oracle import dense, step as ostep  # noqa: E402
from radnet_hip import synth  # noqa: E402

LOSSES = ("rpn_cls", "rpn_regr", "det_cls", "det_regr", "det_acc")


def sample_for(height, width, seed=2):
    """The smoke test's sample family: a synthetic panel and boxes of a source frame twice its size."""
    img = synth.synthetic_panel(1, height, width)
    meta = synth.synthetic_gt(seed, n=5, src_w=2 * width, src_h=2 * height, smin=50, smax=min(height, width))
    return dict(img=img, bboxes=meta["bboxes"], width=2 * width, height=2 * height)


CONV2D_BWD_FP32 = dense.conv2d_bwd


def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def conv2d_bwd_bf16(x, w, dy, stride=1, pad=(0, 0, 0, 0), need_dx=True):
    """dense.conv2d_bwd with x, w and dy rounded to bf16 (round to nearest even) before the fp32 accumulation of dx and dw; db is the
    column sum of the UNROUNDED dy.  Layers whose channel counts the bf16 kernels do not take (none among the trainable ones) stay fp32."""
    if w.shape[2] % 8 or w.shape[3] % 4:
        return CONV2D_BWD_FP32(x, w, dy, stride, pad, need_dx)
    dx, dw, _ = CONV2D_BWD_FP32(_bf16(x), _bf16(w), _bf16(dy), stride, pad, need_dx)
    return dx, dw, dy.reshape(-1, w.shape[3]).sum(0)


def run(C, W, sample, mode, steps, R_list=None):
    """`steps` oracle steps in `mode`; returns (losses of step 1, gradients of step 1, weights after 1 and after `steps` steps, R)."""
    E.MODE[0] = "bf16" if mode == "bf16-train" else mode
    dense.conv2d_bwd = conv2d_bwd_bf16 if mode == "bf16-train" else CONV2D_BWD_FP32
    try:
        np.random.seed(64)
        ot = ostep.OracleTrainer(C, copy.deepcopy(W))
        out = dict(R=[])
        for k in range(steps):
            det = {}
            L = ot.step(sample, detail=det, override_R=None if R_list is None else R_list[k])
            out["R"].append(det["R"])
            if k == 0:
                out["losses"], out["g_rpn"], out["g_head"] = L, det["g_rpn"], det.get("g_head")
                out["w1"] = copy.deepcopy(ot.P)
        out["wk"] = ot.P
    finally:
        E.MODE[0] = "fp32"
        dense.conv2d_bwd = CONV2D_BWD_FP32
    return out


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(a), 1e-30))


def trainable(C):
    nc = len(C.class_mapping)
    return list(dense.RPN_TRAINABLE) + dense.head_trainable(nc)


def report(H, Wd, seed):
    C = Config()
    C.img_size = min(H, Wd)
    W = synth.synthetic_weights(seed=seed)
    s = sample_for(H, Wd)
    a = run(C, W, s, "fp32", 4)
    print("panel %dx%d, weights seed %d" % (H, Wd, seed))
    print("losses fp32 %s" % ["%.6g" % v if v is not None else None for v in a["losses"]])
    for mode in ("bf16", "bf16-train"):
        b = run(C, W, s, mode, 4, R_list=a["R"])
        print("losses %s %s" % (mode, ["%.6g" % v if v is not None else None for v in b["losses"]]))
        print("loss rel diff %s" % ["%.3e" % (abs(x - y) / max(abs(x), 1e-12)) for x, y in zip(a["losses"], b["losses"]) if x is not None])
        print("%-28s %12s %12s %12s   (%s against fp32)" % ("layer", "grad rel", "w rel k=1", "w rel k=4", mode))
        worst = dict(g=0.0, w1=0.0, w4=0.0)
        for name in trainable(C):
            g_a = a["g_rpn"].get(name) if name in a["g_rpn"] else (a["g_head"] or {}).get(name)
            g_b = b["g_rpn"].get(name) if name in b["g_rpn"] else (b["g_head"] or {}).get(name)
            if g_a is None:
                continue
            gr = rel(g_a["kernel"], g_b["kernel"])
            w1 = rel(a["w1"][name]["kernel"], b["w1"][name]["kernel"])
            w4 = rel(a["wk"][name]["kernel"], b["wk"][name]["kernel"])
            worst["g"], worst["w1"], worst["w4"] = max(worst["g"], gr), max(worst["w1"], w1), max(worst["w4"], w4)
            print("%-28s %12.3e %12.3e %12.3e" % (name, gr, w1, w4))
        print("worst (%s): grad %.3e, weights k=1 %.3e, k=4 %.3e" % (mode, worst["g"], worst["w1"], worst["w4"]))


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    dense.conv2d = E.conv2d_torch
    seed = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    panels = [(int(sys.argv[1]), int(sys.argv[2]))] if len(sys.argv) > 2 else [(240, 400), (600, 1000)]
    for H, Wd in panels:
        report(H, Wd, seed)


if __name__ == "__main__":
    main()
