"""Where the time of writing an annotated map goes.  ONE synthetic 4000x4000 RGB 8-bit image on the device (tools/feed_timing.py's
panel and its 360 boxes) and, per stage of utils_io.imwrite / png.encode_device:
  the rectangle launch (radnet_draw_rects_u8, the panel's boxes at thickness 8) and the filter launch (radnet_png_filter_rows_u8,
  adaptive and Sub), by device events; the download of the filtered stream into a pinned buffer; png.assemble on that stream at 1 and
  at 8 host threads (level 1, Z_RLE); the whole imwrite to a file, wall time with the device drained;
against a host baseline inside this tool, the way a user without the writer has to go: download the image, the Sub filter in NumPy,
zlib.compress(level 1) on one thread, the container, the file.  imwrite and the baseline alternate in pairs inside one process; the
medians and the median of the per-pair ratios are reported.  Both files are read back by png.decode_device and compared with the
image.  One GPU, nothing else running.
usage: python tools/png_write_timing.py [--size 4000] [--pairs 5] [--runs 5] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rock-art-radnet_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402

import feed_timing as FT  # noqa: E402
import png_cases as K  # noqa: E402
from faster_rcnn import RADNet as R  # noqa: E402
from faster_rcnn import png, utils_io  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def event_ms(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


def host_baseline(dev, path):
    """The writer a user has without this package's: one download, Sub in NumPy, zlib level 1 on one thread, one IDAT."""
    img = dev.cpu().numpy()
    h, w = img.shape[:2]
    raw = np.ascontiguousarray(img[:, :, ::-1]).reshape(h, w * 3)
    lines = np.empty((h, 1 + w * 3), np.uint8)
    lines[:, 0] = 1
    lines[:, 1:4] = raw[:, :3]
    np.subtract(raw[:, 3:], raw[:, :-3], out=lines[:, 4:])
    data = K.SIGNATURE + K.ihdr(w, h, 8, 2) + K.chunk(b"IDAT", zlib.compress(lines, 1)) + K.chunk(b"IEND")
    with open(path, "wb") as f:
        f.write(data)
    return len(data)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4000)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out:
        args.out = os.path.abspath(args.out)
    if not torch.cuda.is_available():
        raise SystemExit("png_write_timing needs a GPU: the writer's filter and the rectangles are device kernels")
    from radnet_hip import runtime as rt
    ctx = rt.default_context()
    data, img, _ = FT.dataset(args.size)
    h, w = img.shape[:2]
    dev = torch.from_numpy(img).cuda()
    n = h * (1 + 3 * w)
    result = {"size": args.size, "stream_bytes": n, "pairs": args.pairs, "runs": args.runs, "device": torch.cuda.get_device_name(0)}
    med = statistics.median

    rects = [(b["x1"], b["y1"], b["x2"], b["y2"], 8, 255, 255, 255) for b in data[0]["bboxes"]]
    table = np.array(rects, R.RECT)
    table_dev = torch.from_numpy(table.view(np.uint8)).cuda()
    canvas = dev.clone()
    draw = lambda: ctx.call("radnet_draw_rects_u8", canvas, h, w, 3 * w, table.ctypes.data, table_dev, len(table))      # noqa: E731
    stream = torch.empty(n, dtype=torch.uint8, device="cuda")
    staged = torch.empty(n, dtype=torch.uint8, pin_memory=True)
    filt = lambda mode: ctx.call("radnet_png_filter_rows_u8", dev, h, w, 3, 3 * w, mode, stream)      # noqa: E731
    for fn in (draw, lambda: filt(5), lambda: filt(1), lambda: staged.copy_(stream, non_blocking=True)):      # warm-up: code objects
        timed(fn)
    stages = {"rectangles": len(rects),
              "draw_rects_ms": med(event_ms(draw) for _ in range(args.runs)),
              "filter_sub_ms": med(event_ms(lambda: filt(1)) for _ in range(args.runs)),
              "filter_adaptive_ms": med(event_ms(lambda: filt(5)) for _ in range(args.runs)),
              "download_stream_ms": med(timed(lambda: staged.copy_(stream, non_blocking=True))[0] for _ in range(args.runs))}
    # the bytes the two launches move at least: the image in and the stream out (the row above comes from the caches)
    stages["filter_adaptive_GBps_of_image_plus_stream"] = (h * w * 3 + n) / stages["filter_adaptive_ms"] / 1e6
    host_stream = staged.numpy()
    for workers in (1, 8):
        runs = []
        for _ in range(max(2, args.runs // 2)):
            t0 = time.perf_counter()
            blob = png.assemble(host_stream, w, h, 2, 1, "rle", workers, 1 << 20)
            runs.append((time.perf_counter() - t0) * 1e3)
        stages["assemble_%d_workers_ms" % workers] = med(runs)
    stages["file_bytes"] = len(blob)
    result["stages"] = stages
    print("stages:", json.dumps(stages), flush=True)

    with tempfile.TemporaryDirectory() as tmp:
        ours, base = os.path.join(tmp, "ours.png"), os.path.join(tmp, "baseline.png")
        timed(lambda: utils_io.imwrite(ours, dev))                        # warm-up and check, both ways
        timed(lambda: host_baseline(dev, base))
        for path in (ours, base):
            assert torch.equal(png.decode_device(np.fromfile(path, np.uint8)), dev), "%s does not decode to the image" % path
        a, b = [], []
        for k in range(args.pairs):
            for which in ((0, 1) if k % 2 == 0 else (1, 0)):
                if which == 0:
                    a.append(timed(lambda: host_baseline(dev, base))[0])
                else:
                    b.append(timed(lambda: utils_io.imwrite(ours, dev))[0])
        one = [timed(lambda: utils_io.imwrite(ours, dev, workers=1))[0] for _ in range(max(2, args.pairs // 2))]
        result["imwrite"] = {"host_baseline_ms": med(a), "imwrite_ms": med(b), "speedup_median_of_pairs": med(x / y for x, y in zip(a, b)),
                             "imwrite_1_worker_ms": med(one), "host_baseline_runs_ms": a, "imwrite_runs_ms": b,
                             "baseline_file_bytes": os.path.getsize(base), "imwrite_file_bytes": os.path.getsize(ours)}
    print("imwrite:", json.dumps(result["imwrite"]), flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
