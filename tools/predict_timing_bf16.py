"""fp32 against bf16 (engine precision="bf16") on the predict path, as alternating A/B pairs on one box: ms per tile of
RADNet._detect (device-resident) and of the _detect_all sequence (8 tiles, two in flight), 2048x2048 synthetic tiles resized to
img_size (BASELINE config 3).  usage: python tools/predict_timing_bf16.py [pairs=5] [img_size=600]
With --profile-bf16: only runs bf16 _detect on one tile 20 times (the window for rocprofv3 --kernel-trace --stats)."""
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


def make(precision, img_size):
    C = Config()
    C.img_size = img_size
    _, _, _, m_rpn3, m_det = M.build_models(C, weights=synth.synthetic_weights(seed=3), workload="predict", precision=precision)
    return RADNet(C, m_rpn3, m_det, resnet50.preprocess)


def time_detect(net, tile, n=20):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        net._detect(tile)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def time_detect_all(net, tiles):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    net._detect_all(tiles)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / len(tiles) * 1e3


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    pairs = int(args[0]) if args else 5
    img_size = int(args[1]) if len(args) > 1 else 600
    tile = np.random.RandomState(4).randint(0, 256, (2048, 2048, 3)).astype(np.uint8)
    if "--profile-bf16" in sys.argv:
        net = make("bf16", img_size)
        for _ in range(3):
            net._detect(tile)
        print("bf16 _detect: %.2f ms per tile" % time_detect(net, tile))
        return
    tiles = [np.random.RandomState(40 + i).randint(0, 256, (2048, 2048, 3)).astype(np.uint8) for i in range(8)]
    nets = {p: make(p, img_size) for p in ("fp32", "bf16")}
    for net in nets.values():                    # warm-up: launch-shape measurement, plans, hipGraph capture
        for _ in range(3):
            net._detect(tile)
        net._detect_all(tiles[:3])
    res = {p: dict(detect=[], detect_all=[]) for p in nets}
    for k in range(pairs):
        for p in (("fp32", "bf16") if k % 2 == 0 else ("bf16", "fp32")):
            res[p]["detect"].append(time_detect(nets[p], tile))
            res[p]["detect_all"].append(time_detect_all(nets[p], tiles))
    for p in nets:
        print("%s: _detect %s ms/tile (median %.2f); _detect_all %s ms/tile (median %.2f)" % (
            p, " ".join("%.2f" % v for v in res[p]["detect"]), np.median(res[p]["detect"]),
            " ".join("%.2f" % v for v in res[p]["detect_all"]), np.median(res[p]["detect_all"])))
    for key in ("detect", "detect_all"):
        r = [a / b for a, b in zip(res["fp32"][key], res["bf16"][key])]
        print("speed-up %s: %s (median %.2fx)" % (key, " ".join("%.2f" % v for v in r), np.median(r)))
    print(json.dumps(dict(img_size=img_size, pairs=pairs, ms_per_tile=res)))


if __name__ == "__main__":
    main()
