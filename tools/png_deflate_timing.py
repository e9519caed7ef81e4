"""Host deflate against device deflate when writing a map.  ONE synthetic 4000x4000 RGB 8-bit image on the device (the panel of
tools/feed_timing.py, as in tools/png_write_timing.py) and, on the same commit and in one process:
  utils_io.imwrite with deflate="host" (the default: zlib level 1 / Z_RLE on 8 host threads) and with deflate="device"
  (huffman="dynamic"), alternating in pairs, wall time with the device drained; medians and the median of the per-pair ratios;
  the launches of the device path by device events: filter, scan, emit, pack; its two downloads (counts + Adler parts, packed bytes);
  the host's share of it (the code builder, the container with its CRC-32, the file);
  the file sizes of the host path, the dynamic code and the fixed code;
  RADNet.write_predictions (four maps of the panel's 360 boxes) both ways, alternating.
Every file is read back by png.decode_device and compared with the image.  One GPU, nothing else running.
usage: python tools/png_deflate_timing.py [--size 4000] [--pairs 5] [--runs 5] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rock-art-radnet_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402

import feed_timing as FT  # noqa: E402
from faster_rcnn import RADNet as R  # noqa: E402
from faster_rcnn import png, utils_io  # noqa: E402
from png_write_timing import event_ms, timed  # noqa: E402


class _Config:
    class_mapping = {"boat": 0, "human": 1, "animal": 2, "bg": 3}


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
        raise SystemExit("png_deflate_timing needs a GPU: the filter and the deflate are device kernels")
    from radnet_hip import lib as L
    from radnet_hip import runtime as rt
    ctx = rt.default_context()
    data, img, _ = FT.dataset(args.size)
    h, w = img.shape[:2]
    dev = torch.from_numpy(img).cuda()
    n = h * (1 + 3 * w)
    med = statistics.median
    result = {"size": args.size, "stream_bytes": n, "pairs": args.pairs, "runs": args.runs, "device": torch.cuda.get_device_name(0)}

    # ---- the launches of the device path, one by one (what png.deflate_device issues) ----
    chunk = L.header_constant("RADNET_DEFLATE_CHUNK")
    chunks = -(-n // chunk)
    stream = torch.empty(n, dtype=torch.uint8, device="cuda")
    filt = lambda: ctx.call("radnet_png_filter_rows_u8", dev, h, w, 3, 3 * w, 5, stream)      # noqa: E731
    scan_buf = torch.zeros(286 * 4 + chunks * 16, dtype=torch.uint8, device="cuda")
    scan = lambda: ctx.call("radnet_deflate_rle_scan_u8", stream, n, scan_buf, scan_buf.data_ptr() + 286 * 4)      # noqa: E731
    timed(filt)
    scan_buf.zero_()
    timed(scan)
    hist = scan_buf.cpu().numpy()[:286 * 4].view(np.uint32).copy()
    stages = {"chunks": chunks}
    for mode, hc in (("dynamic", png.huffman_code(hist)), ("fixed", png.fixed_code())):
        cap = int(ctx.lib.radnet_deflate_piece_cap(hc.code.ctypes.data, hc.header_nbits, hc.dist_nbits))
        pieces = torch.empty(chunks * cap, dtype=torch.uint8, device="cuda")
        sizes = torch.empty(chunks, dtype=torch.int32, device="cuda")
        header = np.frombuffer(hc.header, np.uint8)
        emit = lambda: ctx.call("radnet_deflate_rle_emit_u8", stream, n, hc.code.ctypes.data, header.ctypes.data, hc.header_nbits, hc.dist_nbits,      # noqa: E731
                                pieces, cap, sizes)
        timed(emit)
        out_cap = int(sizes.cpu().numpy().astype(np.int64).sum())
        out = torch.empty(out_cap, dtype=torch.uint8, device="cuda")
        total = torch.zeros(1, dtype=torch.int64, device="cuda")
        pack = lambda: ctx.call("radnet_deflate_pack", pieces, cap, sizes, chunks, out, out_cap, total)      # noqa: E731
        timed(pack)
        assert int(total.cpu()[0]) == out_cap
        staged = torch.empty(out_cap, dtype=torch.uint8, pin_memory=True)
        stages[mode] = {"piece_cap": cap, "packed_bytes": out_cap,
                        "emit_ms": med(event_ms(emit) for _ in range(args.runs)), "pack_ms": med(event_ms(pack) for _ in range(args.runs)),
                        "download_packed_ms": med(timed(lambda: staged.copy_(out, non_blocking=True))[0] for _ in range(args.runs))}
        del pieces, out
    small = torch.empty(scan_buf.numel(), dtype=torch.uint8, pin_memory=True)
    stages.update({"filter_adaptive_ms": med(event_ms(filt) for _ in range(args.runs)), "scan_ms": med(event_ms(scan) for _ in range(args.runs)),
                   "download_counts_ms": med(timed(lambda: small.copy_(scan_buf, non_blocking=True))[0] for _ in range(args.runs))})
    t0 = time.perf_counter()
    for _ in range(20):
        png.huffman_code(hist)
    stages["huffman_code_ms"] = (time.perf_counter() - t0) * 1e3 / 20
    runs = []
    for _ in range(max(3, args.runs)):                                    # the container round the packed bytes of the fixed code (the larger)
        t0 = time.perf_counter()
        blob = png.assemble_pieces(staged.numpy(), 1, w, h, 2)
        runs.append((time.perf_counter() - t0) * 1e3)
        del blob
    stages["assemble_pieces_ms"] = med(runs)
    result["stages"] = stages
    print("stages:", json.dumps(stages), flush=True)

    # ---- imwrite and write_predictions, host deflate and device deflate in alternating pairs ----
    with tempfile.TemporaryDirectory() as tmp:
        paths = {k: os.path.join(tmp, k + ".png") for k in ("host", "device", "fixed")}
        write = {"host": lambda: utils_io.imwrite(paths["host"], dev), "device": lambda: utils_io.imwrite(paths["device"], dev, deflate="device"),
                 "fixed": lambda: utils_io.imwrite(paths["fixed"], dev, deflate="device", huffman="fixed")}
        for k in write:                                                   # warm-up and check
            timed(write[k])
            assert torch.equal(png.decode_device(np.fromfile(paths[k], np.uint8)), dev), "%s does not decode to the image" % k
        runs = {"host": [], "device": []}
        for k in range(args.pairs):
            for which in (("host", "device") if k % 2 == 0 else ("device", "host")):
                runs[which].append(timed(write[which])[0])
        fixed_runs = [timed(write["fixed"])[0] for _ in range(max(2, args.pairs // 2))]
        result["imwrite"] = {"host_ms": med(runs["host"]), "device_ms": med(runs["device"]),
                             "speedup_median_of_pairs": med(a / b for a, b in zip(runs["host"], runs["device"])), "device_fixed_ms": med(fixed_runs),
                             "host_runs_ms": runs["host"], "device_runs_ms": runs["device"],
                             "file_bytes": {k: os.path.getsize(p) for k, p in paths.items()}}
        print("imwrite:", json.dumps(result["imwrite"]), flush=True)

        net = R.RADNet(_Config(), None, None, None)
        dets = [{'class': ("boat", "human", "animal")[i % 3], 'prob': 0.9, 'x1': b["x1"], 'y1': b["y1"], 'x2': b["x2"], 'y2': b["y2"]}
                for i, b in enumerate(data[0]["bboxes"])]
        both = {"host": lambda: net.write_predictions(dets, dev, os.path.join(tmp, "wp_host")),
                "device": lambda: net.write_predictions(dets, dev, os.path.join(tmp, "wp_device"), deflate="device")}
        for k in both:
            timed(both[k])
        for a, b in zip(both["host"]()[:4], both["device"]()[:4]):
            assert torch.equal(png.decode_device(np.fromfile(a, np.uint8)), png.decode_device(np.fromfile(b, np.uint8))), "%s and %s differ" % (a, b)
        runs = {"host": [], "device": []}
        for k in range(max(3, args.pairs // 2 + 1)):
            for which in (("host", "device") if k % 2 == 0 else ("device", "host")):
                runs[which].append(timed(both[which])[0])
        result["write_predictions"] = {"detections": len(dets), "host_ms": med(runs["host"]), "device_ms": med(runs["device"]),
                                       "speedup_median_of_pairs": med(a / b for a, b in zip(runs["host"], runs["device"])),
                                       "host_runs_ms": runs["host"], "device_runs_ms": runs["device"]}
        print("write_predictions:", json.dumps(result["write_predictions"]), flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
