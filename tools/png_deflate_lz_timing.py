"""Device deflate with far matches against the run-length device deflate when writing a map.  ONE synthetic 4000x4000 RGB 8-bit image
on the device (the panel of tools/feed_timing.py, as in tools/png_deflate_timing.py) and, in one process:
  utils_io.imwrite with deflate="device" and with deflate="device-lz", alternating in pairs, wall time with the device drained;
  medians of 7 with their spreads (min..max) and the median of the per-pair ratios; RADNet.write_predictions (four maps) the same way;
  the launches of the device-lz path by device events: filter, run-length scan, LZ scan, LZ emit, pack; its downloads;
  the file sizes of both modes, what the report says (rule, bits, matches), and the host zlib stream sizes of the same filtered
  stream at level 1 Z_RLE, level 1 and level 6.
Every file is read back by png.decode_device and compared with the image.
--parent ROOT: the defaults -- imwrite with the host deflate and with deflate="device" -- of this tree against the tree at ROOT (a
built checkout of the parent commit), each timed in a child process of its own (this file with --defaults-of), the two trees
alternating; medians with spreads.  One GPU, nothing else running.
usage: python tools/png_deflate_lz_timing.py [--size 4000] [--pairs 7] [--runs 7] [--parent ROOT] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tree(argv):
    """The tree whose package is imported: --defaults-of ROOT in a child process, else this file's own."""
    return os.path.abspath(argv[argv.index("--defaults-of") + 1]) if "--defaults-of" in argv else HERE


ROOT = _tree(sys.argv)
sys.path[:0] = [ROOT, os.path.join(ROOT, "rock-art-radnet_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402

import feed_timing as FT  # noqa: E402
from faster_rcnn import RADNet as R  # noqa: E402
from faster_rcnn import png, utils_io  # noqa: E402
from png_write_timing import event_ms, timed  # noqa: E402

med = statistics.median


class _Config:
    class_mapping = {"boat": 0, "human": 1, "animal": 2, "bg": 3}


def spread(runs):
    return {"median_ms": med(runs), "min_ms": min(runs), "max_ms": max(runs), "runs_ms": runs}


def paired(fns, pairs):
    """{name: [ms]} of two callables run in alternating order, `pairs` times each."""
    names = list(fns)
    runs = {k: [] for k in names}
    for k in range(pairs):
        for which in (names if k % 2 == 0 else names[::-1]):
            runs[which].append(timed(fns[which])[0])
    return runs


def defaults_of_this_tree(size, pairs):
    """The child's work: imwrite with the host deflate and with deflate="device" of the tree this process imported."""
    _, img, _ = FT.dataset(size)
    dev = torch.from_numpy(img).cuda()
    with tempfile.TemporaryDirectory() as tmp:
        fns = {"host": lambda: utils_io.imwrite(os.path.join(tmp, "h.png"), dev), "device": lambda: utils_io.imwrite(os.path.join(tmp, "d.png"), dev, deflate="device")}
        for fn in fns.values():
            timed(fn)
        runs = paired(fns, pairs)
        sizes = {"host": os.path.getsize(os.path.join(tmp, "h.png")), "device": os.path.getsize(os.path.join(tmp, "d.png"))}
        sums = {"host": zlib.crc32(open(os.path.join(tmp, "h.png"), "rb").read()), "device": zlib.crc32(open(os.path.join(tmp, "d.png"), "rb").read())}
    print("DEFAULTS " + json.dumps({"root": ROOT, "host_ms": runs["host"], "device_ms": runs["device"], "file_bytes": sizes, "file_crc32": sums}), flush=True)


def defaults_against(parent, size, pairs, rounds=3):
    """This tree and `parent`, `rounds` child processes each, alternating; the files of both must be the same bytes."""
    got = {"this": {"host": [], "device": []}, "parent": {"host": [], "device": []}}
    files = {}
    for k in range(rounds):
        for which in (("this", "parent") if k % 2 == 0 else ("parent", "this")):
            root = HERE if which == "this" else os.path.abspath(parent)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--defaults-of", root, "--size", str(size), "--pairs", str(pairs)], check=True,
                                 capture_output=True, text=True, timeout=900).stdout
            rec = json.loads([ln for ln in out.splitlines() if ln.startswith("DEFAULTS ")][-1][len("DEFAULTS "):])
            assert os.path.samefile(rec["root"], root), rec["root"]
            got[which]["host"] += rec["host_ms"]
            got[which]["device"] += rec["device_ms"]
            files.setdefault(which, (rec["file_bytes"], rec["file_crc32"]))
    assert files["this"] == files["parent"], "the defaults' files differ from the parent's: %r" % (files,)
    return {"rounds": rounds, "pairs_per_round": pairs, "files_equal": True, "file_bytes": files["this"][0],
            "this": {k: spread(v) for k, v in got["this"].items()}, "parent": {k: spread(v) for k, v in got["parent"].items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4000)
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--defaults-of", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out:
        args.out = os.path.abspath(args.out)
    if not torch.cuda.is_available():
        raise SystemExit("png_deflate_lz_timing needs a GPU: the filter and the deflate are device kernels")
    if args.defaults_of:
        return defaults_of_this_tree(args.size, args.pairs)
    from radnet_hip import lib as L
    from radnet_hip import runtime as rt
    ctx = rt.default_context()
    data, img, _ = FT.dataset(args.size)
    h, w = img.shape[:2]
    dev = torch.from_numpy(img).cuda()
    n = h * (1 + 3 * w)
    result = {"size": args.size, "stream_bytes": n, "pairs": args.pairs, "runs": args.runs, "device": torch.cuda.get_device_name(0)}

    # ---- the launches of the device-lz path, one by one (what png.deflate_device_lz issues) ----
    chunk = L.header_constant("RADNET_DEFLATE_CHUNK")
    chunks = -(-n // chunk)
    stream = torch.empty(n, dtype=torch.uint8, device="cuda")
    filt = lambda: ctx.call("radnet_png_filter_rows_u8", dev, h, w, 3, 3 * w, 5, stream)      # noqa: E731
    rle_buf = torch.zeros(286 * 4 + chunks * 16, dtype=torch.uint8, device="cuda")
    lz_buf = torch.zeros(320 * 4 + chunks * 16, dtype=torch.uint8, device="cuda")
    tokens = torch.empty(n, dtype=torch.int32, device="cuda")
    rle_scan = lambda: ctx.call("radnet_deflate_rle_scan_u8", stream, n, rle_buf, rle_buf.data_ptr() + 286 * 4)      # noqa: E731
    lz_scan = lambda: ctx.call("radnet_deflate_lz_scan_u8", stream, n, 3, tokens, lz_buf, lz_buf.data_ptr() + 288 * 4, lz_buf.data_ptr() + 320 * 4)      # noqa: E731
    timed(filt)
    timed(rle_scan)
    timed(lz_scan)
    host_counts = lz_buf.cpu().numpy()
    hist_ll, hist_d = host_counts[:286 * 4].view(np.uint32).copy(), host_counts[288 * 4:318 * 4].view(np.uint32).copy()
    code_ll, code_d, header_bytes, nbits = png.huffman_codes_lz(hist_ll, hist_d)
    cap = int(ctx.lib.radnet_deflate_lz_piece_cap(code_ll.ctypes.data, code_d.ctypes.data, nbits))
    pieces = torch.empty(chunks * cap, dtype=torch.uint8, device="cuda")
    sizes = torch.empty(chunks, dtype=torch.int32, device="cuda")
    header = np.frombuffer(header_bytes, np.uint8)
    emit = lambda: ctx.call("radnet_deflate_lz_emit_u8", stream, n, tokens, code_ll.ctypes.data, code_d.ctypes.data, header.ctypes.data, nbits, pieces, cap, sizes)      # noqa: E731
    timed(emit)
    out_cap = int(sizes.cpu().numpy().astype(np.int64).sum())
    out = torch.empty(out_cap, dtype=torch.uint8, device="cuda")
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    pack = lambda: ctx.call("radnet_deflate_pack", pieces, cap, sizes, chunks, out, out_cap, total)      # noqa: E731
    timed(pack)
    assert int(total.cpu()[0]) == out_cap
    staged = torch.empty(out_cap, dtype=torch.uint8, pin_memory=True)
    small = torch.empty(lz_buf.numel(), dtype=torch.uint8, pin_memory=True)
    ev = lambda fn: spread([event_ms(fn) for _ in range(args.runs)])      # noqa: E731
    stages = {"chunks": chunks, "piece_cap": cap, "packed_bytes_lz": out_cap, "filter_adaptive": ev(filt), "rle_scan": ev(rle_scan), "lz_scan": ev(lz_scan),
              "lz_emit": ev(emit), "pack": ev(pack), "download_counts": spread([timed(lambda: small.copy_(lz_buf, non_blocking=True))[0] for _ in range(args.runs)]),
              "download_packed": spread([timed(lambda: staged.copy_(out, non_blocking=True))[0] for _ in range(args.runs)])}
    result["stages"] = stages
    print("stages:", json.dumps(stages), flush=True)
    raw = stream.cpu().numpy().tobytes()
    def zsize(level, strategy):
        c = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
        return len(c.compress(raw)) + len(c.flush())

    result["host_zlib_stream_bytes"] = {"level1_rle": zsize(1, zlib.Z_RLE), "level1": zsize(1, zlib.Z_DEFAULT_STRATEGY), "level6": zsize(6, zlib.Z_DEFAULT_STRATEGY)}
    del raw, pieces, out
    print("host zlib:", json.dumps(result["host_zlib_stream_bytes"]), flush=True)

    # ---- imwrite and write_predictions, deflate="device" and "device-lz" in alternating pairs ----
    with tempfile.TemporaryDirectory() as tmp:
        paths = {k: os.path.join(tmp, k + ".png") for k in ("device", "device-lz")}
        report = {}
        write = {"device": lambda: utils_io.imwrite(paths["device"], dev, deflate="device"),
                 "device-lz": lambda: utils_io.imwrite(paths["device-lz"], dev, deflate="device-lz", report=report)}
        for k in write:                                                   # warm-up and check
            timed(write[k])
            assert torch.equal(png.decode_device(np.fromfile(paths[k], np.uint8)), dev), "%s does not decode to the image" % k
        runs = paired(write, args.pairs)
        result["imwrite"] = {"device": spread(runs["device"]), "device-lz": spread(runs["device-lz"]),
                             "lz_over_device_median_of_pairs": med(b / a for a, b in zip(runs["device"], runs["device-lz"])),
                             "file_bytes": {k: os.path.getsize(p) for k, p in paths.items()}, "report": dict(report)}
        print("imwrite:", json.dumps(result["imwrite"]), flush=True)

        net = R.RADNet(_Config(), None, None, None)
        dets = [{'class': ("boat", "human", "animal")[i % 3], 'prob': 0.9, 'x1': b["x1"], 'y1': b["y1"], 'x2': b["x2"], 'y2': b["y2"]}
                for i, b in enumerate(data[0]["bboxes"])]
        both = {"device": lambda: net.write_predictions(dets, dev, os.path.join(tmp, "wp_device"), deflate="device"),
                "device-lz": lambda: net.write_predictions(dets, dev, os.path.join(tmp, "wp_lz"), deflate="device-lz")}
        for k in both:
            timed(both[k])
        files = {}
        for a, b in zip(both["device"]()[:4], both["device-lz"]()[:4]):
            assert torch.equal(png.decode_device(np.fromfile(a, np.uint8)), png.decode_device(np.fromfile(b, np.uint8))), "%s and %s differ" % (a, b)
            files[os.path.basename(a)] = {"device": os.path.getsize(a), "device-lz": os.path.getsize(b)}
        runs = paired(both, args.pairs)
        result["write_predictions"] = {"detections": len(dets), "device": spread(runs["device"]), "device-lz": spread(runs["device-lz"]),
                                       "lz_over_device_median_of_pairs": med(b / a for a, b in zip(runs["device"], runs["device-lz"])), "file_bytes": files}
        print("write_predictions:", json.dumps(result["write_predictions"]), flush=True)
    if args.parent:
        del dev, stream, tokens
        torch.cuda.empty_cache()
        result["defaults_against_parent"] = defaults_against(args.parent, args.size, args.pairs)
        print("defaults against the parent:", json.dumps(result["defaults_against_parent"]), flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
