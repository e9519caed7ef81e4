"""Samples per second of faster_rcnn.data_feed.TileFeed on the host path (the default) against the same feed with
device_augment=True, over ONE synthetic 4000x4000 image with the default Config (tile_size 2000, every augmentation switch on) and a
fixed seed; with and without BackgroundFeed; one GPU, no train step running.  Median of --runs runs of --samples samples each, the
two paths alternating inside one process (the host path is the baseline, measured in the same run).  A device sample is complete
when it leaves the feed (the producing stream has drained), so the host clock around next() measures finished work.
usage: python tools/feed_timing.py [--samples 50] [--runs 3] [--size 4000] [--out FILE.json]
With --profile: only pulls --samples samples from the device path (the window for rocprofv3 --kernel-trace --stats)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rock-art-radnet_amd")]
import torch  # noqa: E402

from faster_rcnn import data_feed as F  # noqa: E402
from faster_rcnn.config import Config  # noqa: E402

CLASSES = ["boat", "human", "other", "animal", "circle", "wheel"]


def dataset(size, seed=7):
    """One size x size image: smooth relief plus noise in every channel, a black margin on two sides (scans of rock panels have
    one), and a few hundred boxes so that every tile holds some of every class."""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:size, 0:size].astype(np.float32)
    base = 128.0 + 70.0 * np.sin(x / 211.0) * np.cos(y / 173.0)
    img = np.clip(base[:, :, None] + rs.normal(0.0, 12.0, (size, size, 3)), 1, 255).astype(np.uint8)
    img[:, :size // 50] = 0
    img[-size // 80:] = 0
    boxes = []
    for j in range(360):
        bw, bh = int(rs.randint(40, 300)), int(rs.randint(40, 300))
        x1, y1 = int(rs.randint(0, size - bw)), int(rs.randint(0, size - bh))
        boxes.append({"class": CLASSES[j % len(CLASSES)], "x1": x1, "x2": x1 + bw, "y1": y1, "y2": y1 + bh})
    data = [{"filepath": "panel.png", "width": size, "height": size, "bboxes": boxes}]
    return data, img, {c: sum(1 for b in boxes if b["class"] == c) for c in CLASSES}


def make_feed(data, img, class_count, device, background, seed):
    feed = F.TileFeed([dict(d) for d in data], Config(), class_count, lambda d, t: img, rng=np.random.RandomState(seed),
                      noise_rng=np.random.default_rng(seed), device_augment=device, noise_seed=seed if device else None)
    return F.BackgroundFeed(feed, depth=8) if background else feed


def pull(feed, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = 0
    for s in feed:
        got += 1
        if got == n:
            break
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if hasattr(feed, "close"):
        feed.close()
    return n / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--size", type=int, default=4000)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("feed_timing needs a GPU: both paths run kernels (the host path warps and resizes on the device)")
    data, img, class_count = dataset(args.size)
    if args.profile:
        pull(make_feed(data, img, class_count, True, False, args.seed), 3)
        print("profile window: %.2f samples/s" % pull(make_feed(data, img, class_count, True, False, args.seed), args.samples))
        return
    for device in (False, True):                                        # warm-up: code objects, contexts, scipy's import
        pull(make_feed(data, img, class_count, device, False, args.seed), 3)
    result = {"size": args.size, "samples": args.samples, "runs": args.runs, "seed": args.seed, "device": torch.cuda.get_device_name(0)}
    for background in (False, True):
        rates = {False: [], True: []}
        for r in range(args.runs):
            for device in ((False, True) if r % 2 == 0 else (True, False)):
                rates[device].append(pull(make_feed(data, img, class_count, device, background, args.seed), args.samples))
                print("%s %s run %d: %.2f samples/s" % ("background" if background else "direct", "device" if device else "host", r, rates[device][-1]), flush=True)
        key = "background_feed" if background else "direct"
        result[key] = {"host_samples_per_s": statistics.median(rates[False]), "device_samples_per_s": statistics.median(rates[True]),
                       "host_runs": rates[False], "device_runs": rates[True]}
        result[key]["ratio"] = result[key]["device_samples_per_s"] / result[key]["host_samples_per_s"]
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
