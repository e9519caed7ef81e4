"""What unfilter="tiles" (radnet_png_unfilter_tiles_u8, csrc/png_tiles.hip) reaches against the one-workgroup reconstruction
(radnet_png_unfilter_u8), on the synthetic size x size RGB panel of tools/feed_timing.py with Paeth on every row and with adaptive rows.
  (a) the reconstruction stage alone: both entries on fresh copies of the same filtered stream, by events, as alternating pairs in one
      process (tools/png_timing.py's scheme: medians and the median of the per-pair ratios); both results are checked against the panel;
  (b) the whole png.decode_device with unfilter="band" against "tiles" under each inflate mode, wall time with the device drained, as
      alternating pairs: "host" and "device-lz" on the level-6 file, "device" on the run-length file (level 1, Z_RLE);
  (c) the stage of (a) at block widths T of 64, 128 and 256 pixels through radnet_png_unfilter_tiles_width_u8, each against the
      one-workgroup entry in pairs of its own.
usage: python tools/png_unfilter_timing.py [--size 4000] [--pairs 5] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rock-art-radnet_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402

import feed_timing as FT  # noqa: E402
import png_cases as K  # noqa: E402
from faster_rcnn import png  # noqa: E402
from radnet_hip import runtime as rt  # noqa: E402

WIDTHS = (64, 128, 256)


def filtered_stream(img_bgr, types, block=256):
    """The scanline stream [h][1 + 3 w] of the panel as 8-bit RGB with the given filter types (4, or "adaptive"), a block of rows at a
    time (each block sees the row above it), as tools/png_timing.py's encode_rgb8 does."""
    h, w = img_bgr.shape[:2]
    raw = np.ascontiguousarray(img_bgr[:, :, ::-1]).reshape(h, w * 3)
    out = np.empty((h, 1 + 3 * w), np.uint8)
    for r0 in range(0, h, block):
        lines, _ = K.filter_rows(raw[max(r0 - 1, 0):r0 + block], 3, types)
        out[r0:r0 + block] = lines[1 if r0 else 0:]
    return out, raw


def file_of(lines, w, h, run_length):
    if run_length:
        c = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
        z = c.compress(lines.tobytes()) + c.flush()
    else:
        z = zlib.compress(lines.tobytes(), 6)
    return K.SIGNATURE + K.ihdr(w, h, 8, 2) + K.chunk(b"IDAT", z) + K.chunk(b"IEND")


def by_events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stage_pairs(ctx, lines, raw, pairs, width=None):
    """radnet_png_unfilter_u8 against the tiles entry (width: through the width-given entry) on fresh device copies of `lines`:
    alternating pairs by events.  Every run's bytes are compared with the raw rows on the device."""
    rows, rowbytes = raw.shape
    host = torch.from_numpy(lines.reshape(-1))
    want = torch.from_numpy(raw).cuda()
    table = np.array([(0, rows, rowbytes)], png.SEGMENT)
    table_dev = torch.from_numpy(table.view(np.uint8)).cuda()
    times = {"band": [], "tiles": []}

    def one(kind):
        dev = host.cuda()
        if kind == "band":
            call = lambda: ctx.call("radnet_png_unfilter_u8", dev, rows, rowbytes, 3)      # noqa: E731
        elif width is None:
            call = lambda: ctx.call("radnet_png_unfilter_tiles_u8", dev, dev.numel(), table.ctypes.data, table_dev, 1, 3)      # noqa: E731
        else:
            call = lambda: ctx.call("radnet_png_unfilter_tiles_width_u8", dev, dev.numel(), table.ctypes.data, table_dev, 1, 3, width)      # noqa: E731
        times[kind].append(by_events(call))
        assert torch.equal(dev.view(rows, 1 + rowbytes)[:, 1:], want), kind

    one("band")
    one("tiles")                                                           # warm-up, not booked
    times = {"band": [], "tiles": []}
    for k in range(pairs):
        for kind in (("band", "tiles") if k % 2 == 0 else ("tiles", "band")):
            one(kind)
    ratios = [a / b for a, b in zip(times["band"], times["tiles"])]
    return {"band_ms": statistics.median(times["band"]), "tiles_ms": statistics.median(times["tiles"]), "band_over_tiles_median_of_pairs": statistics.median(ratios),
            "band_runs_ms": times["band"], "tiles_runs_ms": times["tiles"]}


def timed(fn):
    import time
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def decode_pairs(blob, img, inflate, pairs):
    data = np.frombuffer(blob, np.uint8)
    reports = {"band": {}, "tiles": {}}
    for kind in reports:                                                   # warm-up and check
        got = png.decode_device(data, inflate=inflate, unfilter=kind, report=reports[kind])
        assert np.array_equal(got.cpu().numpy(), img), (inflate, kind)
        del got
    times = {"band": [], "tiles": []}
    for k in range(pairs):
        for kind in (("band", "tiles") if k % 2 == 0 else ("tiles", "band")):
            times[kind].append(timed(lambda: png.decode_device(data, inflate=inflate, unfilter=kind)))
    ratios = [a / b for a, b in zip(times["band"], times["tiles"])]
    return {"file_bytes": len(blob), "path": reports["tiles"]["path"], "reconstruction_band": reports["band"]["reconstruction"],
            "reconstruction_tiles": reports["tiles"]["reconstruction"], "sweeps": reports["tiles"]["sweeps"], "band_ms": statistics.median(times["band"]),
            "tiles_ms": statistics.median(times["tiles"]), "band_over_tiles_median_of_pairs": statistics.median(ratios), "band_runs_ms": times["band"],
            "tiles_runs_ms": times["tiles"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4000)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _, img, _ = FT.dataset(args.size)
    h, w = img.shape[:2]
    ctx = rt.default_context()
    result = {"size": args.size, "pairs": args.pairs, "device": torch.cuda.get_device_name(0), "tile_pixels": png.TILE_PIXELS,
              "plan": png.plan_tiles(h, 3 * w, 3)._asdict()}
    for rows_kind, types in (("paeth", 4), ("adaptive", "adaptive")):
        lines, raw = filtered_stream(img, types)
        out = {"filter_types": np.bincount(lines[:, 0], minlength=5).tolist()}
        out["stage"] = stage_pairs(ctx, lines, raw, args.pairs)
        print(rows_kind, "stage", json.dumps(out["stage"]), flush=True)
        out["stage_by_width"] = {str(t): stage_pairs(ctx, lines, raw, args.pairs, width=t) for t in WIDTHS}
        print(rows_kind, "stage_by_width", json.dumps(out["stage_by_width"]), flush=True)
        level6, run_length = file_of(lines, w, h, False), file_of(lines, w, h, True)
        del lines, raw
        out["decode"] = {}
        for inflate, blob in (("host", level6), ("device", run_length), ("device-lz", level6)):
            out["decode"][inflate] = decode_pairs(blob, img, inflate, args.pairs)
            print(rows_kind, "decode", inflate, json.dumps(out["decode"][inflate]), flush=True)
        result[rows_kind] = out
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
