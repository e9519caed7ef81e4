"""The tile loop with the detection tail on the host (RADNet.device_tail = False: today's decode + per-class NMS in Python)
against the tail on the device (True, csrc/detect_tail.hip), as alternating A/B pairs in ONE process on one box -- same plans,
same launch shapes, same tiles: ms per tile of RADNet._detect and of the _detect_all sequence (8 tiles, two in flight),
2048x2048 synthetic tiles resized to img_size (BASELINE config 3).
usage: python tools/detect_tail_timing.py [--pairs 5] [--precision fp32|bf16] [--img-size 600] [--threshold 0.7]
With --profile: only runs _detect with the device tail on one tile 20 times (the window for rocprofv3 --kernel-trace --stats)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rock-art-radnet_amd")]
import torch  # noqa: E402

from faster_rcnn import models as M  # noqa: E402
from faster_rcnn.RADNet import RADNet  # noqa: E402
from faster_rcnn.base_models import resnet50  # noqa: E402
from faster_rcnn.config import Config  # noqa: E402
from radnet_hip import synth  # noqa: E402


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--img-size", type=int, default=600)
    ap.add_argument("--threshold", type=float, default=0.7, help="RADNet.bbox_threshold (0.0: every non-background RoI is decoded)")
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    C = Config()
    C.img_size = args.img_size
    kw = {} if args.precision == "fp32" else dict(precision=args.precision)
    _, _, _, m_rpn3, m_det = M.build_models(C, weights=synth.synthetic_weights(seed=3), workload="predict", **kw)
    net = RADNet(C, m_rpn3, m_det, resnet50.preprocess)
    net.bbox_threshold = args.threshold
    tiles = [np.random.RandomState(40 + i).randint(0, 256, (2048, 2048, 3)).astype(np.uint8) for i in range(8)]
    if args.profile:
        net.device_tail = True
        for _ in range(20):
            net._detect(tiles[0])
        torch.cuda.synchronize()
        return
    for flag in (False, True):                       # plans, launch shapes, graphs
        net.device_tail = flag
        for _ in range(3):
            net._detect(tiles[0])
        net._detect_all(tiles[:4])
    n_det = sum(len(v[0]) for v in net._detect(tiles[0]).values())
    res = {"detect": {0: [], 1: []}, "detect_all": {0: [], 1: []}}
    for p in range(args.pairs):
        for flag in (False, True):
            net.device_tail = flag
            res["detect"][int(flag)].append(timed(lambda: net._detect(tiles[0]), 20))
            res["detect_all"][int(flag)].append(timed(lambda: net._detect_all(tiles), 3) / len(tiles))
        print("pair %d  _detect host %.3f device %.3f   _detect_all host %.3f device %.3f  ms/tile" % (
            p, res["detect"][0][-1], res["detect"][1][-1], res["detect_all"][0][-1], res["detect_all"][1][-1]), flush=True)
    out = {"precision": args.precision, "img_size": args.img_size, "bbox_threshold": args.threshold, "pairs": args.pairs,
           "detections_on_tile_0": n_det}
    for what in res:
        a, b = res[what][0], res[what][1]
        out[what] = {"host_tail_ms": a, "device_tail_ms": b, "host_median": float(np.median(a)), "host_spread": max(a) - min(a),
                     "device_median": float(np.median(b)), "device_spread": max(b) - min(b)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
