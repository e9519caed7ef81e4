"""The Adam launches alone on the chip, one `label<TAB>microseconds` line per row (two runs compare by script):
  fp32 engine, classifier arena: radnet_adam_step_fused (+ shifts + the three Winograd filter transforms in the same pass) against
    radnet_adam_step_affine against affine + three radnet_winograd4_filter launches;
  fp32 engine, RPN arena: plain radnet_adam_step;
  bf16-mixed engine, both arenas: radnet_adam_step_bf16.
usage: python tools/adam_timing.py"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rock-art-radnet_amd")]
from faster_rcnn.config import Config  # noqa: E402
from radnet_hip import make_engine, synth  # noqa: E402


def timed(label, fn, n=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    print("%s\t%.1f" % (label, e0.elapsed_time(e1) * 1e3 / n), flush=True)


def main():
    eng = make_engine(Config())
    eng.set_weights(synth.synthetic_weights(seed=3))
    eng.head_arena.g.normal_(0, 1e-3)
    eng.rpn_arena.g.normal_(0, 1e-3)
    names = list(eng.INFERENCE_WINOGRAD_LAYERS)
    timed("fp32 head: fused Adam + shifts + 3 filter transforms, one launch", lambda: eng.adam(eng.head_arena, zero_grad=False))
    eng.head_train_wino = False
    timed("fp32 head: Adam + shifts (radnet_adam_step_affine)", lambda: eng.adam(eng.head_arena, zero_grad=False))
    timed("fp32 head: Adam + shifts, then 3 x radnet_winograd4_filter", lambda: (eng.adam(eng.head_arena, zero_grad=False), eng._refresh_winograd(names)))
    timed("fp32 head: 3 x radnet_winograd4_filter", lambda: eng._refresh_winograd(names))
    ar = eng.rpn_arena
    timed("fp32 rpn: Adam (radnet_adam_step)", lambda: eng._adam_launch(ar, ar.m, ar.v, 1, 1.0, False))
    del eng, ar

    eng = make_engine(Config(), precision="bf16-mixed")
    eng.set_weights(synth.synthetic_weights(seed=3))
    for label, ar in (("head", eng.head_arena), ("rpn", eng.rpn_arena)):
        ar.g.normal_(0, 1e-3)
        timed("bf16-mixed %s: Adam + bf16 images (radnet_adam_step_bf16)" % label, lambda: eng.adam(ar, zero_grad=False))


if __name__ == "__main__":
    main()
