"""Where the time of png.decode_device(inflate="device") and of inflate="device-lz" goes, against the host path of the same file.
Files of the synthetic size x size RGB panel of tools/feed_timing.py:
  cv2      what cv2.imwrite's defaults are taken to be: level 1, Z_RLE, memLevel 8, Sub on every row, 8 KiB IDAT chunks
           (the Sub filter and the chunk size are from memory of OpenCV's writer and unverified; no test depends on them);
  imwrite  the package's own writer (png.encode_device: adaptive rows, level 1, Z_RLE, pieces of 1 MiB);
  level6   tools/png_timing.py's file (adaptive rows, level 6, one IDAT chunk): "device" falls back, and its figure is the cost of
           the wasted search; "device-lz" takes it;
  level6_idat8k  the same stream in IDAT chunks of 8 KiB, as other tools cut it.
Per file and mode: the whole decode_device on the host path and in that mode as alternating pairs in one process (tools/png_timing.py's
scheme: wall time with the device drained, medians and the median of the per-pair ratios), then ONE staged decode in that mode --
container and CRC, upload, every launch by events (emit, resolve and gather apart), the downloads, which reconstruction ran -- and the
counts of candidates, false candidates, units and, for "device-lz", rounds and units with far matches.
Last: one unit of RADNET_INFLATE_UNIT_MAX_SYMBOLS symbols (fixed-code literals) through radnet_inflate_rle_measure, by events.
usage: python tools/png_inflate_timing.py [--size 4000] [--pairs 5] [--out FILE.json]"""
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
import inflate_cases as I  # noqa: E402
import png_cases as K  # noqa: E402
import png_timing as PT  # noqa: E402
from faster_rcnn import png  # noqa: E402
from radnet_hip import lib as L  # noqa: E402
from radnet_hip import runtime as rt  # noqa: E402


def cv2_like(img_bgr, idat=8192):
    """Sub on every row, zlib level 1 with Z_RLE at memLevel 8, IDAT chunks of 8 KiB."""
    h, w = img_bgr.shape[:2]
    raw = np.ascontiguousarray(img_bgr[:, :, ::-1]).reshape(h, w * 3)
    lines = np.empty((h, 1 + 3 * w), np.uint8)
    lines[:, 0] = 1
    lines[:, 1:4] = raw[:, :3]
    lines[:, 4:] = raw[:, 3:] - raw[:, :-3]
    c = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    z = c.compress(lines.tobytes()) + c.flush()
    return b"".join([K.SIGNATURE, K.ihdr(w, h, 8, 2)] + [K.chunk(b"IDAT", z[s:s + idat]) for s in range(0, len(z), idat)] + [K.chunk(b"IEND")])


def rechunked(blob, idat=8192):
    """The file `blob` (one IDAT chunk) with the same stream in IDAT chunks of 8 KiB, as libpng's writers cut it."""
    at = blob.index(b"IDAT") - 4
    n = int.from_bytes(blob[at:at + 4], "big")
    z = blob[at + 8:at + 8 + n]
    return b"".join([blob[:at]] + [K.chunk(b"IDAT", z[s:s + idat]) for s in range(0, len(z), idat)] + [K.chunk(b"IEND")])


def one_file(name, blob, img, pairs):
    data = np.frombuffer(blob, np.uint8)
    report = {}
    got = png.decode_device(data, inflate="device", report=report)        # warm-up and check
    assert np.array_equal(got.cpu().numpy(), img) and torch.equal(got, png.decode_device(data)), name
    del got
    legs = PT.alternating_pairs(lambda: png.decode_device(data), lambda: png.decode_device(data, inflate="device"), pairs)
    out = {"file_bytes": len(blob), "path": report["path"], "reason": report["reason"],
           "host_ms": legs["sequential_ms"], "device_ms": legs["many_ms"], "host_over_device_median_of_pairs": legs["speedup_median_of_pairs"],
           "host_runs_ms": legs["sequential_runs_ms"], "device_runs_ms": legs["many_runs_ms"]}
    staged = {"stages": {}}
    png.decode_device(data, inflate="device", report=staged)
    out["stages_ms"] = {k: round(v, 3) for k, v in staged["stages"].items() if not k.startswith("_")}
    out.update({k: staged[k] for k in ("candidates", "false_candidates", "units", "blocks", "reconstruction")})
    # the same against inflate="device-lz": pairs of its own against the host path, in the same process, then one staged decode
    report = {}
    got = png.decode_device(data, inflate="device-lz", report=report)
    assert np.array_equal(got.cpu().numpy(), img), name
    del got
    legs = PT.alternating_pairs(lambda: png.decode_device(data), lambda: png.decode_device(data, inflate="device-lz"), pairs)
    staged = {"stages": {}}
    png.decode_device(data, inflate="device-lz", report=staged)
    out["device_lz"] = {"path": report["path"], "reason": report["reason"], "host_ms": legs["sequential_ms"], "device_lz_ms": legs["many_ms"],
                        "host_over_device_lz_median_of_pairs": legs["speedup_median_of_pairs"], "host_runs_ms": legs["sequential_runs_ms"],
                        "device_lz_runs_ms": legs["many_runs_ms"], "stages_ms": {k: round(v, 3) for k, v in staged["stages"].items() if not k.startswith("_")}}
    out["device_lz"].update({k: staged[k] for k in ("candidates", "false_candidates", "units", "blocks", "reconstruction", "rounds", "far_units")})
    out["host_parse_ms"] = statistics.median(PT.timed(lambda: png.parse(data))[0] for _ in range(3))
    out["parse_compressed_ms"] = statistics.median(PT.timed(lambda: png.parse_compressed(data))[0] for _ in range(3))
    return out


def unit_at_the_cap(ctx):
    """radnet_inflate_rle_measure on ONE unit of exactly RADNET_INFLATE_UNIT_MAX_SYMBOLS symbols, by events: milliseconds."""
    cap = L.header_constant("RADNET_INFLATE_UNIT_MAX_SYMBOLS")
    z, _ = I.fixed_literals(cap - 1)                                      # and the end-of-block
    dev = torch.from_numpy(np.frombuffer(z, np.uint8).copy()).cuda()
    times = []
    for _ in range(4):
        units = np.zeros(1, png.INFLATE_UNIT)
        units["start_bit"] = 16
        units_dev = torch.from_numpy(units.view(np.uint8)).cuda()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ctx.call("radnet_inflate_rle_measure", dev, len(z), units_dev, 1)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
        rec = units_dev.cpu().numpy().view(png.INFLATE_UNIT)[0]
        assert int(rec["status"]) == 0 and int(rec["symbols"]) == cap, rec
    return {"symbols": cap, "measure_ms_runs": times, "measure_ms": statistics.median(times[1:])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4000)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _, img, _ = FT.dataset(args.size)
    ctx = rt.default_context()
    result = {"size": args.size, "pairs": args.pairs, "device": torch.cuda.get_device_name(0)}
    result_blobs = {}
    files = (("cv2", lambda: cv2_like(img)), ("imwrite", lambda: png.encode_device(torch.from_numpy(img).cuda())), ("level6", lambda: PT.encode_rgb8(img)),
             ("level6_idat8k", lambda: rechunked(result_blobs["level6"])))
    for name, make in files:
        result_blobs[name] = make()
        result[name] = one_file(name, result_blobs[name], img, args.pairs)
        print(name, json.dumps(result[name]), flush=True)
    result["unit_at_the_cap"] = unit_at_the_cap(ctx)
    print("unit_at_the_cap", json.dumps(result["unit_at_the_cap"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
