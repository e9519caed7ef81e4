"""What join="device" (radnet_png_join_u8, csrc/png_join.hip) changes against join="host", on the synthetic size x size RGB panel of
tools/feed_timing.py and the files of tools/png_crc_timing.py.  The yardstick of every leg is the host option in the same run:
  (a) whole png.decode_device calls as alternating pairs in one process (tools/png_timing.py's scheme: wall time with the device
      drained), join="host" against join="device", each leg with crc="host" and with crc="device":
        cv2            inflate="device", unfilter="tiles" on the cv2-parameter file (level 1, Z_RLE, IDAT chunks of 8 KiB)
        level6_idat8k  inflate="device-lz", unfilter="tiles" on a level-6 stream in IDAT chunks of 8 KiB
        level6         the same stream in ONE IDAT chunk: one large copy is replaced by one large copy
      medians, the per-run lists and the spread (max - min) of each side; "gain" is stated only where the medians differ by more than
      the spread of either side, else "no gain claimed";
  (b) the stages, each alone, median of `pairs` runs: the entry by device events, and beside it a device-to-device copy of the same n
      bytes between the same buffers (the yardstick of the kernel); the host join it replaces; the whole-file copy into the pinned
      buffer; the upload of the F bytes of the file against the n bytes of the stream; parse_compressed whole in both modes;
  (c) the defaults against another tree (--parent DIR: a built checkout of the parent commit), tools/png_crc_timing.py's
      defaults_against: alternating child processes, each on the same saved panel and file.
usage: python tools/png_join_timing.py [--size 4000] [--pairs 5] [--parent DIR] [--rounds 3] [--out FILE.json]"""
import argparse
import concurrent.futures
import json
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4000)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path[:0] = [ROOT, os.path.join(ROOT, "rock-art-radnet_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
    import torch
    import feed_timing as FT
    import png_crc_timing as PCT
    import png_inflate_timing as PIT
    import png_timing as PT
    from faster_rcnn import png
    from radnet_hip import runtime as rt

    def spread(runs):
        return max(runs) - min(runs)

    def pair_leg(host_fn, device_fn):
        legs = PT.alternating_pairs(host_fn, device_fn, args.pairs)
        host, device = legs["sequential_runs_ms"], legs["many_runs_ms"]
        out = {"host_ms": legs["sequential_ms"], "device_ms": legs["many_ms"], "host_over_device_median_of_pairs": legs["speedup_median_of_pairs"],
               "host_spread_ms": spread(host), "device_spread_ms": spread(device), "host_runs_ms": host, "device_runs_ms": device}
        gain = out["host_ms"] - out["device_ms"]
        out["verdict"] = "gain %.2f ms" % gain if gain > max(out["host_spread_ms"], out["device_spread_ms"]) else "no gain claimed"
        return out

    def median_of(fn, runs=None):
        return statistics.median(PT.timed(fn)[0] for _ in range(runs or args.pairs))

    def by_events(fn):
        """The median of `pairs` runs of fn after a warm-up, by device events round it."""
        times = []
        for _ in range(args.pairs + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        return statistics.median(times[1:])

    def host_join(source, idat, host):
        """The join of parse_compressed(join="host") alone: one slice assignment per chunk from 8 threads (above 1 MiB)."""
        starts = np.concatenate([[0], np.cumsum([e - s for s, e in idat])]).astype(np.int64).tolist()

        def piece(k):
            s, e = idat[k]
            host[starts[k]:starts[k] + e - s] = source[s:e]
        with concurrent.futures.ThreadPoolExecutor(max_workers=png.MANY_DEFAULT_WORKERS) as pool:
            list(pool.map(lambda g: [piece(k) for k in range(g, len(idat), png.MANY_DEFAULT_WORKERS)], range(min(len(idat), png.MANY_DEFAULT_WORKERS))))

    _, img, _ = FT.dataset(args.size)
    ctx = rt.default_context()
    result = {"size": args.size, "pairs": args.pairs, "device": torch.cuda.get_device_name(0)}
    blobs = {"cv2": PIT.cv2_like(img), "level6": PT.encode_rgb8(img)}
    blobs["level6_idat8k"] = PIT.rechunked(blobs["level6"])
    for name, inflate in (("cv2", "device"), ("level6_idat8k", "device-lz"), ("level6", "device-lz")):
        data = np.frombuffer(blobs[name], np.uint8)
        how = dict(inflate=inflate, unfilter="tiles")
        leg = {"file_bytes": len(data)}
        # ---- (a) whole calls ----
        for crc in png.CRC_MODES:
            report = {}
            got = png.decode_device(data, crc=crc, join="device", report=report, **how)
            assert np.array_equal(got.cpu().numpy(), img), (name, crc)
            del got
            assert report["path"] == "device" and report["join"] == "device", report
            leg["crc_" + crc] = pair_leg(lambda: png.decode_device(data, crc=crc, **how), lambda: png.decode_device(data, crc=crc, join="device", **how))
        # ---- (b) the stages ----
        comp = png.parse_compressed(data, join="device")
        ref = png.parse_compressed(data)
        idat = [(int(s), int(s + l)) for s, _, l in comp.pieces.tolist()]
        at = png.join_layout(comp)
        dev = comp.staged.cuda()
        out = torch.empty(comp.n, dtype=torch.uint8, device="cuda")
        entry = lambda: ctx.call("radnet_png_join_u8", dev.data_ptr(), comp.file_len, comp.staged.data_ptr() + at.pieces, dev.data_ptr() + at.pieces,      # noqa: E731
                                 len(comp.pieces), out.data_ptr(), comp.n)
        stages = {"stream_bytes": comp.n, "idat_chunks": len(idat), "join_entry_by_events": by_events(entry)}
        assert torch.equal(out, ref.staged[:ref.n].cuda())
        stages["device_copy_of_n_bytes_by_events"] = by_events(lambda: out.copy_(dev[:comp.n]))
        scratch = torch.empty(max(comp.file_len, comp.n), dtype=torch.uint8, pin_memory=True)
        pinned = scratch.numpy()
        stages["host_join_alone"] = median_of(lambda: host_join(data, idat, pinned))
        stages["whole_file_copy_alone"] = median_of(lambda: pinned[:len(data)].__setitem__(slice(None), data))
        stages["upload_file_bytes"] = median_of(lambda: scratch[:comp.file_len].cuda(non_blocking=True))
        stages["upload_stream_bytes"] = median_of(lambda: scratch[:comp.n].cuda(non_blocking=True))
        for crc in png.CRC_MODES:
            stages["parse_compressed_join_host_crc_" + crc] = median_of(lambda: png.parse_compressed(data, crc=crc))
            stages["parse_compressed_join_device_crc_" + crc] = median_of(lambda: png.parse_compressed(data, crc=crc, join="device"))
        leg["stages_ms"] = stages
        result[name] = leg
        print(name, json.dumps(leg), flush=True)
        del dev, out, scratch, comp, ref

    # ---- (c) the defaults against the parent tree ----
    if args.parent:
        with tempfile.TemporaryDirectory() as work:
            np.save(os.path.join(work, "panel.npy"), img)
            with open(os.path.join(work, "level6.png"), "wb") as f:
                f.write(blobs["level6"])
            torch.cuda.empty_cache()
            result["defaults_against_parent"] = PCT.defaults_against(args.parent, work, args.rounds, args.pairs)
        print("defaults_against_parent", json.dumps(result["defaults_against_parent"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
