"""Where the time of reading a PNG map onto the device goes, and what it does to the feed.  Writes ONE synthetic 4000x4000 RGB 8-bit
file (tools/feed_timing.py's panel, encoded by the tests' encoder tests/png_cases.py with adaptive per-row filters) and reports
  per decode: file read + container + inflate (host), staging + upload, the reconstruction launch, the expansion launch;
  samples/s of TileFeed(device_augment=True) over that file through utils_io.DeviceImageLoader with the cache off and on, next to
  the in-memory figure (the decoded array handed over by a lambda, what tools/feed_timing.py measures) from the same run.
  batched: png.decode_device_many over --batch distinct files of that size (the panel shifted, so the filter columns differ) against
  the same files through png.decode_device one after the other, and ONE file through decode_device_many (the segmented path alone)
  against decode_device; wall time per call with the device drained, in alternating pairs, the median of the per-pair ratios.
Medians of --runs runs, the variants alternating inside one process; default Config, fixed seed, one GPU, no train step running.
usage: python tools/png_timing.py [--size 4000] [--samples 20] [--runs 3] [--batch 8] [--pairs 5] [--out FILE.json]"""
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
from faster_rcnn import data_feed as F  # noqa: E402
from faster_rcnn import png, utils_io  # noqa: E402
from faster_rcnn.config import Config  # noqa: E402


def encode_rgb8(img_bgr, level=6, block=256):
    """png_cases.encode for a large RGB 8-bit image: the same forward filters and the same adaptive choice, a block of rows at a
    time (each block sees the row above it), so the candidate residuals of the whole image never exist at once."""
    h, w = img_bgr.shape[:2]
    raw = np.ascontiguousarray(img_bgr[:, :, ::-1]).reshape(h, w * 3)
    deflate = zlib.compressobj(level)
    z = []
    for r0 in range(0, h, block):
        lines, _ = K.filter_rows(raw[max(r0 - 1, 0):r0 + block], 3, "adaptive")
        z.append(deflate.compress(lines[1 if r0 else 0:].tobytes()))
    z.append(deflate.flush())
    return K.SIGNATURE + K.ihdr(w, h, 8, 2) + K.chunk(b"IDAT", b"".join(z)) + K.chunk(b"IEND")


def decode_stages(path, ctx):
    """One decode, stage by stage (png.decode_device's steps with a wait after each): milliseconds."""
    t0 = time.perf_counter()
    img = png.parse(np.fromfile(path, np.uint8))
    t1 = time.perf_counter()
    n = len(img.stream)
    staged = torch.empty(n + 768, dtype=torch.uint8, pin_memory=True)
    host = staged.numpy()
    host[:n] = np.frombuffer(img.stream, np.uint8)
    host[n:] = img.palette.reshape(-1)
    dev = staged.cuda(non_blocking=True)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    out = torch.empty((img.header.height, img.header.width, 3), dtype=torch.uint8, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    (p,) = img.passes
    ev[0].record()
    ctx.call("radnet_png_unfilter_u8", dev.data_ptr(), p.pass_h, p.rowbytes, img.bpp)
    ev[1].record()
    ctx.call("radnet_png_expand_bgr_u8", dev.data_ptr(), p.pass_h, p.pass_w, p.rowbytes, img.header.color_type, img.header.bit_depth,
             dev.data_ptr() + n, out, img.header.height, img.header.width, 0, 0, 1, 1)
    ev[2].record()
    torch.cuda.synchronize()
    return {"host_read_inflate_ms": (t1 - t0) * 1e3, "upload_ms": (t2 - t1) * 1e3, "unfilter_ms": ev[0].elapsed_time(ev[1]),
            "expand_ms": ev[1].elapsed_time(ev[2])}, out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def alternating_pairs(old, new, pairs):
    """old() and new() back to back `pairs` times, the order swapping from pair to pair: medians (ms) and the median of the
    per-pair ratios old / new."""
    a, b = [], []
    for k in range(pairs):
        for which in ((0, 1) if k % 2 == 0 else (1, 0)):
            (a if which == 0 else b).append(timed(old if which == 0 else new)[0])
    return {"sequential_ms": statistics.median(a), "many_ms": statistics.median(b),
            "speedup_median_of_pairs": statistics.median(x / y for x, y in zip(a, b)), "sequential_runs_ms": a, "many_runs_ms": b}


def batched_legs(img, blob, batch, pairs):
    """The two legs of the batched decoder on `batch` distinct files (the panel rolled by 37 rows and columns per file)."""
    shifted = [img] + [np.roll(img, (37 * k, 37 * k), axis=(0, 1)) for k in range(1, batch)]
    blobs = [blob] + [encode_rgb8(s) for s in shifted[1:]]
    files = [np.frombuffer(b, np.uint8) for b in blobs]
    many = png.decode_device_many(files)                                  # warm-up and check
    for s, t, f in zip(shifted, many, files):
        assert np.array_equal(t.cpu().numpy(), s) and torch.equal(t, png.decode_device(f)), "decode_device_many differs"
    table = png.plan_segments(png.parse(files[0]))
    del many
    out = {"batch": batch, "pairs": pairs, "segments_of_file_0": int(len(table)), "longest_segment_rows": int(table["rows"].max())}
    out["batch_leg"] = alternating_pairs(lambda: [png.decode_device(f) for f in files], lambda: png.decode_device_many(files), pairs)
    out["single_leg"] = alternating_pairs(lambda: png.decode_device(files[0]), lambda: png.decode_device_many(files[:1]), pairs)
    # where the batched call's time goes: the host threads alone (parse of every file), and the reconstruction launch alone
    out["parse_all_threads_ms"] = statistics.median(timed(lambda: _parse_all(files))[0] for _ in range(3))
    out["parse_all_one_thread_ms"] = statistics.median(timed(lambda: [png.parse(f) for f in files])[0] for _ in range(3))
    return out


def _parse_all(files):
    import concurrent.futures
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(len(files), png.MANY_DEFAULT_WORKERS)) as pool:
        return list(pool.map(png.parse, files))


def segments_kernel_ms(path, ctx):
    """The reconstruction of ONE file as segments, timed by events beside the one-workgroup launch on the same bytes."""
    img = png.parse(np.fromfile(path, np.uint8))
    n = len(img.stream)
    table = png.plan_segments(img)
    table = table[np.argsort(table["rows"] > 64, kind="stable")]
    host = np.concatenate([np.frombuffer(img.stream, np.uint8), np.zeros(-n % 8, np.uint8), table.view(np.uint8)])
    at = n + (-n % 8)
    (p,) = img.passes
    times = {"segments": [], "one_workgroup": []}
    for _ in range(3):
        for kind in times:
            dev = torch.from_numpy(host).cuda()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            if kind == "segments":
                ctx.call("radnet_png_unfilter_segments_u8", dev.data_ptr(), n, table.ctypes.data, dev.data_ptr() + at, len(table), img.bpp)
            else:
                ctx.call("radnet_png_unfilter_u8", dev.data_ptr(), p.pass_h, p.rowbytes, img.bpp)
            ev[1].record()
            torch.cuda.synchronize()
            times[kind].append(ev[0].elapsed_time(ev[1]))
    return {"unfilter_segments_ms": statistics.median(times["segments"]), "unfilter_one_workgroup_ms": statistics.median(times["one_workgroup"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4000)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--batch", type=int, default=8, help="files of the batched leg (0: skip the batched legs)")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out:
        args.out = os.path.abspath(args.out)
    if not torch.cuda.is_available():
        raise SystemExit("png_timing needs a GPU: the decoder's per-byte steps are device kernels")
    from radnet_hip import runtime as rt
    data, img, class_count = FT.dataset(args.size)
    C = Config()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        path = utils_io.image_path(data[0]["filepath"], C.img_types[0])
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        t0 = time.perf_counter()
        blob = encode_rgb8(img)
        with open(path, "wb") as f:
            f.write(blob)
        result = {"size": args.size, "file_bytes": len(blob), "encode_s": time.perf_counter() - t0, "samples": args.samples, "runs": args.runs,
                  "device": torch.cuda.get_device_name(0)}
        ctx = rt.default_context()
        stages, out = decode_stages(path, ctx)                           # warm-up: code objects, pinned pool
        assert np.array_equal(out.cpu().numpy(), img), "the decoded file is not the encoded image"
        runs = [decode_stages(path, ctx)[0] for _ in range(max(3, args.runs))]
        result["decode"] = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
        result["decode"]["total_ms"] = sum(result["decode"].values())
        print("decode (ms):", json.dumps(result["decode"]), flush=True)

        if args.batch > 0:
            result["many"] = batched_legs(img, blob, args.batch, args.pairs)
            result["many"].update(segments_kernel_ms(path, ctx))
            print("many:", json.dumps(result["many"]), flush=True)

        loaders = {"in_memory": lambda d, t: img, "file_cache_off": utils_io.DeviceImageLoader(cache_bytes=0),
                   "file_cache_on": utils_io.DeviceImageLoader(cache_bytes=1 << 30)}      # kept across runs: the steady state of a job

        def feed(kind):
            load = loaders[kind]
            return F.TileFeed([dict(d) for d in data], C, class_count, load, rng=np.random.RandomState(args.seed), device_augment=True,
                              noise_seed=args.seed)

        kinds = ["in_memory", "file_cache_off", "file_cache_on"]
        for k in kinds:
            FT.pull(feed(k), 3)
        rates = {k: [] for k in kinds}
        for r in range(args.runs):
            for k in (kinds if r % 2 == 0 else kinds[::-1]):
                rates[k].append(FT.pull(feed(k), args.samples))
                print("%s run %d: %.2f samples/s" % (k, r, rates[k][-1]), flush=True)
        result["feed_samples_per_s"] = {k: statistics.median(v) for k, v in rates.items()}
        result["feed_runs"] = rates
        result["cache"] = {k: {"hits": loaders[k].hits, "misses": loaders[k].misses} for k in kinds[1:]}
        os.chdir(ROOT)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
