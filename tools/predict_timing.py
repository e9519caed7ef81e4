"""Time the predict path (RADNet._detect: resize -> RPN -> proposals -> classifier on all RoIs -> per-class NMS) on a
2048x2048 synthetic tile (BASELINE config 3), stage by stage.
usage: python tools/predict_timing.py [img_size] [--device-tail 0|1] [--precision fp32|bf16]
--device-tail: RADNet.device_tail for the _detect / _detect_all lines (decode + per-class NMS on the device or on the host)."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rock-art-radnet_amd")]
import torch
from faster_rcnn import models as M, rpn
from faster_rcnn.RADNet import RADNet
from faster_rcnn.base_models import resnet50
from faster_rcnn.config import Config
from radnet_hip import synth

import argparse
ap = argparse.ArgumentParser()
ap.add_argument("img_size", nargs="?", type=int, default=600)
ap.add_argument("--device-tail", type=int, choices=(0, 1), default=int(RADNet.device_tail))
ap.add_argument("--precision", default="fp32")
args = ap.parse_args()
C = Config(); C.img_size = args.img_size
m_rpn, m_cls, m_all, m_rpn3, m_det = M.build_models(C, weights=synth.synthetic_weights(seed=3), **({} if args.precision == "fp32" else dict(workload="predict", precision=args.precision)))
net = RADNet(C, m_rpn3, m_det, resnet50.preprocess)
net.device_tail = bool(args.device_tail)
print("device_tail = %d, precision %s" % (args.device_tail, args.precision))
tile = np.random.RandomState(4).randint(0, 256, (2048, 2048, 3)).astype(np.uint8)
for _ in range(3):
    net._detect(tile)
torch.cuda.synchronize()
acc = {}
def T(label, t0):
    torch.cuda.synchronize(); t = time.perf_counter(); acc[label] = acc.get(label, 0.0) + t - t0; return t
n = 10
t_all = time.perf_counter()
for _ in range(n):
    t = time.perf_counter()
    X, ratio = net.format_img(tile); t = T("format_img (device bicubic resize + preprocess)", t)
    Y1, Y2, F = m_rpn3.predict(X); t = T("model_rpn.predict (base + RPN, outputs to host)", t)
    R = rpn.rpn_to_roi(Y1, Y2, C, overlap_thresh=0.7); t = T("rpn_to_roi", t)
    R[:, 2] -= R[:, 0]; R[:, 3] -= R[:, 1]
    bb, pp = net.apply_spatial_pyramid_pooling(R, F); t = T("apply_spatial_pyramid_pooling (detector on all RoIs + decode)", t)
    for key in bb:
        rpn.non_max_suppression_fast(np.array(bb[key]), np.array(pp[key]), overlap_thresh=0.2)
    t = T("per-class NMS", t)
tot = (time.perf_counter() - t_all) / n
print("img_size %d: %.2f ms per tile (%.1f tiles/s), %d RoIs" % (C.img_size, tot * 1e3, 1 / tot, len(R)))
for k, v in acc.items():
    print("  %7.2f ms  %s" % (v / n * 1e3, k))
for mode in (False, True):
    net.device_resident = mode
    for _ in range(3):
        net._detect(tile)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        net._detect(tile)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 20
    print("RADNet._detect, %s: %.2f ms per tile (%.1f tiles/s, %.1f TFLOP/s algorithmic at %.0f GF)" % (
        "device-resident" if mode else "NumPy-facing calls", dt * 1e3, 1 / dt, (58.95 + 15 * 29.29) / dt / 1e3 if C.img_size == 600 else float("nan"), 58.95 + 15 * 29.29))

tiles = [np.random.RandomState(40 + i).randint(0, 256, (2048, 2048, 3)).astype(np.uint8) for i in range(8)]
net.device_resident = True
net._detect_all(tiles[:3])
torch.cuda.synchronize()
t0 = time.perf_counter()
net._detect_all(tiles)
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / len(tiles)
print("RADNet._detect_all, 8 tiles, two in flight: %.2f ms per tile (%.1f tiles/s)" % (dt * 1e3, 1 / dt))
