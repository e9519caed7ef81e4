"""What the host copy and the upload of every tile cost inside RADNet.predict on a full scan, and what keeping the image on the
device saves.  One synthetic 4000x4000x3 noise image, the default Config (tile_size 2000, tile_overlap 400: 36 tiles, img_size 600),
synthetic weights (bench.py's), one GPU.  After warm-up and plan building, alternating pairs inside one process:
  predict([host_array])  against  predict([cuda_tensor])        ms per image and tiles/s;
  predict_from_path on a PNG of that image (tools/png_timing.py's encoder), this checkout against --parent DIR, another checkout of
  the project (built) that serves the same file from a child process, the two taking turns; the decode is inside both.
Medians and the spread of the runs are reported.  The detections of the variants are compared (they must be equal), once with every
decoded box kept (threshold 0: synthetic weights give none above the default 0.7, as in bench.py's predict workload) and in every
timed run at --bbox-threshold.
usage: python tools/predict_image_timing.py [--size 4000] [--runs 5] [--bbox-threshold 0.7] [--parent DIR] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np


def _arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


SCRIPT = os.path.abspath(__file__)
HERE = os.path.dirname(os.path.dirname(SCRIPT))
ROOT = os.path.abspath(_arg("--root", HERE))            # the checkout whose package is measured (a worker: the parent's)
sys.path[:0] = [ROOT, os.path.join(ROOT, "rock-art-radnet_amd"), os.path.join(HERE, "tests"), os.path.join(HERE, "tools")]
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")         # as bench.py: the lanes need more than 4 hardware queues
import torch  # noqa: E402


def build_net():
    from faster_rcnn import models as M
    from faster_rcnn.RADNet import RADNet
    from faster_rcnn.base_models import resnet50
    from faster_rcnn.config import Config
    from radnet_hip import synth
    C = Config()
    ms = M.build_models(C, weights=synth.synthetic_weights(seed=3), workload="predict")
    net = RADNet(C, ms[3], ms[4], resnet50.preprocess)
    net.bbox_threshold = float(_arg("--bbox-threshold", 0.7))
    return C, net


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def plain(dets):
    return [[d["class"], float(d["prob"]), int(d["x1"]), int(d["y1"]), int(d["x2"]), int(d["y2"])] for d in dets]


def worker(path):
    """Child process of --parent: builds the net of the checkout at --root, then answers every line on stdin with one timed
    predict_from_path (a JSON line: ms and the detections)."""
    C, net = build_net()
    for _ in range(2):
        net.predict_from_path(path)
    print(json.dumps({"ready": True}), flush=True)
    for line in sys.stdin:
        if line.strip() != "go":
            break
        ms, dets = timed(lambda: net.predict_from_path(path))
        print(json.dumps({"ms": ms, "dets": plain(dets)}), flush=True)


def answer(child):
    """The worker's next JSON line (anything else it prints is passed through)."""
    while True:
        line = child.stdout.readline()
        if not line:
            raise SystemExit("the --parent worker ended early (exit status %s)" % child.poll())
        if line.startswith("{"):
            return json.loads(line)
        print("[parent] " + line.rstrip(), flush=True)


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--bbox-threshold", type=float, default=0.7)
    ap.add_argument("--parent", default=None, help="another built checkout: its predict_from_path runs interleaved from a child process")
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("predict_image_timing needs a GPU")
    if args.worker:
        return worker(args.worker)
    if args.out:
        args.out = os.path.abspath(args.out)
    if args.parent:
        args.parent = os.path.abspath(args.parent)
    import png_timing as PT
    from faster_rcnn import utils_io
    C, net = build_net()
    img = np.random.RandomState(4).randint(0, 256, (args.size, args.size, 3)).astype(np.uint8)
    from faster_rcnn.RADNet import _spans
    spans = [(y0, y1, x0, x1) for (y0, y1) in _spans(args.size, C.tile_size, C.tile_overlap) for (x0, x1) in _spans(args.size, C.tile_size, C.tile_overlap)]
    n_tiles = len(spans) + (1 if C.include_full_img else 0)
    result = {"size": args.size, "tiles": n_tiles, "img_size": C.img_size, "runs": args.runs, "device": torch.cuda.get_device_name(0)}
    dev = torch.from_numpy(img).cuda()
    variants = {"host_array": lambda: net.predict([img]), "cuda_tensor": lambda: net.predict([dev])}
    outs = {}
    net.bbox_threshold = 0.0
    for k, fn in variants.items():                        # plans, launch shapes, graphs; every decoded box kept
        outs[k] = plain(fn())
    assert outs["host_array"] == outs["cuda_tensor"] and len(outs["host_array"]) > 0, "the two paths disagree"
    result["detections_at_threshold_0"] = len(outs["host_array"])
    net.bbox_threshold = args.bbox_threshold
    for k, fn in variants.items():
        outs[k] = plain(fn())
    assert outs["host_array"] == outs["cuda_tensor"], "the two paths disagree"
    result["bbox_threshold"] = args.bbox_threshold
    result["detections"] = len(outs["host_array"])
    ms = {k: [] for k in variants}
    for r in range(args.runs):
        for k in (list(variants) if r % 2 == 0 else list(variants)[::-1]):
            ms[k].append(timed(variants[k])[0])
            print("%s run %d: %.1f ms" % (k, r, ms[k][-1]), flush=True)
    result["predict_ms"] = {k: spread(v) for k, v in ms.items()}
    result["predict_tiles_per_s"] = {k: 1e3 * n_tiles / statistics.median(v) for k, v in ms.items()}
    # the host copy and the upload of the tiles alone, nothing else running: what they cost the enqueuing thread per image
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for (y0, y1, x0, x1) in spans:
        t = torch.from_numpy(np.copy(img[y0:y1, x0:x1, :])).cuda()
    torch.cuda.synchronize()
    result["tile_copy_and_upload_alone_ms"] = (time.perf_counter() - t0) * 1e3
    del t

    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        rel = "maps/scan.png"
        path = utils_io.image_path(rel, C.img_types[0])
        os.makedirs(os.path.dirname(path))
        with open(path, "wb") as f:
            f.write(PT.encode_rgb8(img))
        result["file_bytes"] = os.path.getsize(path)
        for _ in range(2):
            here = plain(net.predict_from_path(rel))
        assert here == outs["host_array"], "predict_from_path disagrees with predict on the decoded image"
        child = None
        if args.parent:
            child = subprocess.Popen([sys.executable, SCRIPT, "--root", args.parent, "--worker", rel, "--bbox-threshold", str(args.bbox_threshold)],
                                     stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=tmp)
            assert answer(child).get("ready")
        ms = {"this_checkout": [], "parent_checkout": []}
        try:
            for r in range(args.runs):
                order = ["this_checkout", "parent_checkout"] if r % 2 == 0 else ["parent_checkout", "this_checkout"]
                for k in order:
                    if k == "this_checkout":
                        ms[k].append(timed(lambda: net.predict_from_path(rel))[0])
                    elif child is not None:
                        child.stdin.write("go\n")
                        child.stdin.flush()
                        ans = answer(child)
                        assert ans["dets"] == here, "the parent checkout's detections differ"
                        ms[k].append(ans["ms"])
                    else:
                        continue
                    print("predict_from_path %s run %d: %.1f ms" % (k, r, ms[k][-1]), flush=True)
        finally:
            if child is not None:
                child.stdin.close()
                child.wait(timeout=60)
        result["predict_from_path_ms"] = {k: spread(v) for k, v in ms.items() if v}
        os.chdir(ROOT)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
