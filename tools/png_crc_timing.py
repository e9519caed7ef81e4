"""What crc="device" (radnet_crc32_segments, csrc/crc32.hip) changes against crc="host", on the synthetic size x size RGB panel of
tools/feed_timing.py, and how the host stage it replaces splits up.  The yardstick of every leg is the host option in the same run:
  (a) whole calls as alternating pairs in one process (tools/png_timing.py's scheme: wall time with the device drained, medians and
      the median of the per-pair ratios), crc="host" against crc="device":
        write          png.encode_device(deflate="device"), what utils_io.imwrite(deflate="device") runs; the files are compared
        cv2            png.decode_device(inflate="device", unfilter="tiles") on tools/png_inflate_timing.py's cv2-parameter file
                       (level 1, Z_RLE, IDAT chunks of 8 KiB)
        level6         png.decode_device(inflate="device-lz", unfilter="tiles") on tools/png_timing.py's file (one IDAT chunk)
        level6_idat8k  the same stream in IDAT chunks of 8 KiB
  (b) the stages, each alone, median of `pairs` runs: the kernel entry by device events on the bytes where they stand; the host
      CRC-32 alone (the calls parse_compressed / assemble_pieces make, on the same chunks); the join copy alone; the chunk walk alone;
      and parse_compressed whole in both modes;
  (c) the defaults against another tree (--parent DIR: a built checkout of the parent commit): default png.encode_device and default
      png.decode_device(level6) timed in child processes, one per tree, alternating, each on the same saved panel and file.
usage: python tools/png_crc_timing.py [--size 4000] [--pairs 5] [--parent DIR] [--rounds 3] [--out FILE.json]"""
import argparse
import concurrent.futures
import json
import os
import statistics
import struct
import subprocess
import sys
import tempfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tree_paths(root):
    return [root, os.path.join(root, "rock-art-radnet_amd"), os.path.join(root, "tests"), os.path.join(root, "tools")]


def defaults_child(root, work, runs):
    """Child process: the default writer and the default reader of the tree at `root`, `runs` times each after a warm-up; one JSON line."""
    sys.path[:0] = tree_paths(root)
    import torch
    import png_timing as PT
    from faster_rcnn import png
    assert os.path.realpath(png.__file__).startswith(os.path.realpath(root)), png.__file__
    img = torch.from_numpy(np.load(os.path.join(work, "panel.npy"))).cuda()
    data = np.fromfile(os.path.join(work, "level6.png"), np.uint8)
    png.encode_device(img)
    png.decode_device(data)
    out = {"root": root, "encode_default_runs_ms": [PT.timed(lambda: png.encode_device(img))[0] for _ in range(runs)],
           "decode_default_runs_ms": [PT.timed(lambda: png.decode_device(data))[0] for _ in range(runs)]}
    print("DEFAULTS " + json.dumps(out), flush=True)


def defaults_against(parent, work, rounds, runs):
    """This tree and `parent` in alternating child processes: per tree the runs of all rounds, their medians, and the ratio."""
    got = {"this": {"encode": [], "decode": []}, "parent": {"encode": [], "decode": []}}
    for k in range(rounds):
        for which in (("this", "parent") if k % 2 == 0 else ("parent", "this")):
            root = ROOT if which == "this" else os.path.abspath(parent)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--defaults-child", root, "--work", work, "--pairs", str(runs)],
                               capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError("the defaults child of %s failed:\n%s\n%s" % (root, r.stdout[-2000:], r.stderr[-2000:]))
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("DEFAULTS ")][-1]
            rec = json.loads(line[len("DEFAULTS "):])
            got[which]["encode"] += rec["encode_default_runs_ms"]
            got[which]["decode"] += rec["decode_default_runs_ms"]
    out = {"rounds": rounds, "runs_per_round": runs}
    for leg in ("encode", "decode"):
        a, b = got["parent"][leg], got["this"][leg]
        out[leg] = {"parent_ms": statistics.median(a), "this_ms": statistics.median(b), "parent_over_this": statistics.median(a) / statistics.median(b),
                    "parent_runs_ms": a, "this_runs_ms": b}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4000)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--defaults-child", default=None)
    ap.add_argument("--work", default=None)
    args = ap.parse_args()
    if args.defaults_child:
        return defaults_child(args.defaults_child, args.work, args.pairs)
    sys.path[:0] = tree_paths(ROOT)
    import torch
    import feed_timing as FT
    import png_inflate_timing as PIT
    import png_timing as PT
    from faster_rcnn import png
    from radnet_hip import lib as L
    from radnet_hip import runtime as rt

    def spread(runs):
        return max(runs) - min(runs)

    def pair_leg(host_fn, device_fn):
        legs = PT.alternating_pairs(host_fn, device_fn, args.pairs)
        return {"host_ms": legs["sequential_ms"], "device_ms": legs["many_ms"], "host_over_device_median_of_pairs": legs["speedup_median_of_pairs"],
                "host_spread_ms": spread(legs["sequential_runs_ms"]), "device_spread_ms": spread(legs["many_runs_ms"]),
                "host_runs_ms": legs["sequential_runs_ms"], "device_runs_ms": legs["many_runs_ms"]}

    def median_of(fn, runs=None):
        return statistics.median(PT.timed(fn)[0] for _ in range(runs or args.pairs))

    def kernel_ms(ctx, dev, n, table):
        """radnet_crc32_segments on dev[:n] with `table`, by events: the median of `pairs` calls after a warm-up, and the verdict."""
        table_dev = torch.from_numpy(table.view(np.uint8)).cuda()
        out = torch.zeros(4 * len(table) + 8, dtype=torch.uint8, device="cuda")
        times = []
        for _ in range(args.pairs + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            ctx.call("radnet_crc32_segments", dev, n, table.ctypes.data, table_dev, len(table), out, out.data_ptr() + 4 * len(table))
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        verdict = out.cpu().numpy()[4 * len(table):].view(np.int32).tolist()
        assert verdict == [len(table), 0], verdict
        return statistics.median(times[1:])

    _, img, _ = FT.dataset(args.size)
    ctx = rt.default_context()
    dev_img = torch.from_numpy(img).cuda()
    result = {"size": args.size, "pairs": args.pairs, "device": torch.cuda.get_device_name(0)}

    # ---- the writer ----
    want = png.encode_device(dev_img, deflate="device")
    assert png.encode_device(dev_img, deflate="device", crc="device") == want
    leg = pair_leg(lambda: png.encode_device(dev_img, deflate="device"), lambda: png.encode_device(dev_img, deflate="device", crc="device"))
    at = want.index(b"IDAT") - 4
    packed = np.frombuffer(want, np.uint8)[at + 10:at + 8 + int.from_bytes(want[at:at + 4], "big") - 4].copy()
    view = memoryview(packed)
    head = zlib.crc32(b"IDAT" + png._zlib_header(1))
    one = np.array([(0, len(packed), head, png._crc32_threads(view, head))], png.CRC_SEGMENT)
    leg["stages_ms"] = {"packed_bytes": len(packed), "kernel_by_events": kernel_ms(ctx, torch.from_numpy(packed).cuda(), len(packed), one),
                        "host_crc_alone": median_of(lambda: png._crc32_threads(view, head)),
                        "join_copy_alone": median_of(lambda: b"".join([want[:at + 10], view, want[-20:]])),
                        "assemble_pieces_host_crc": median_of(lambda: png.assemble_pieces(packed, 1, img.shape[1], img.shape[0], 2)),
                        "assemble_pieces_given_crc": median_of(lambda: png.assemble_pieces(packed, 1, img.shape[1], img.shape[0], 2, idat_crc=int(one["expect"][0])))}
    result["write"] = leg
    print("write", json.dumps(leg), flush=True)

    # ---- the reader ----
    def walk(view):
        """parse_compressed's chunk walk alone: the headers, no sums, no copies."""
        pos, idat = 33, []
        while pos < len(view):
            length, kind = struct.unpack(">I4s", view[pos:pos + 8])
            end = pos + 8 + length
            if kind == b"IDAT":
                idat.append((pos + 8, end))
            pos = end + 4
            if kind == b"IEND":
                break
        return idat

    def host_crc(view, source, idat):
        """The IDAT sums as parse_compressed(crc="host") takes them on a file of 1 MiB or more: chunks of 4 MiB and more cut into ranges on
        host threads, the others in one radnet_png_check_crcs call."""
        large = [(s, e) for s, e in idat if e - s + 8 >= 4 << 20]
        small = [(s, e) for s, e in idat if e - s + 8 < 4 << 20]
        ok = all(png._crc32_threads(view[s:e], zlib.crc32(b"IDAT")) == int.from_bytes(view[e:e + 4], "big") for s, e in large)
        if small:
            at, end = np.array([s - 8 for s, _ in small], np.int64), np.array([e for _, e in small], np.int64)
            ok = ok and L.load_library().radnet_png_check_crcs(source.ctypes.data, len(source), at.ctypes.data, end.ctypes.data, len(small),
                                                               png.MANY_DEFAULT_WORKERS) == len(small)
        assert ok

    def join(source, idat, host):
        starts = np.concatenate([[0], np.cumsum([e - s for s, e in idat])]).astype(np.int64).tolist()

        def piece(k):
            s, e = idat[k]
            host[starts[k]:starts[k] + e - s] = source[s:e]
        with concurrent.futures.ThreadPoolExecutor(max_workers=png.MANY_DEFAULT_WORKERS) as pool:
            list(pool.map(lambda g: [piece(k) for k in range(g, len(idat), png.MANY_DEFAULT_WORKERS)], range(min(len(idat), png.MANY_DEFAULT_WORKERS))))

    blobs = {"cv2": PIT.cv2_like(img), "level6": PT.encode_rgb8(img)}
    blobs["level6_idat8k"] = PIT.rechunked(blobs["level6"])
    for name, inflate in (("cv2", "device"), ("level6", "device-lz"), ("level6_idat8k", "device-lz")):
        data = np.frombuffer(blobs[name], np.uint8)
        how = dict(inflate=inflate, unfilter="tiles")
        reports = {"host": {}, "device": {}}
        for mode in reports:
            got = png.decode_device(data, crc=mode, report=reports[mode], **how)
            assert np.array_equal(got.cpu().numpy(), img), (name, mode)
            del got
        assert reports["device"]["path"] == "device" and reports["device"]["crc"] == "device", reports["device"]
        leg = pair_leg(lambda: png.decode_device(data, **how), lambda: png.decode_device(data, crc="device", **how))
        comp = png.parse_compressed(data, crc="device")
        view = memoryview(data)
        idat = walk(view)
        assert len(idat) == len(comp.crc_segments)
        scratch = np.empty(comp.n, np.uint8)
        leg.update(file_bytes=len(data), idat_chunks=len(idat), path=reports["device"]["path"])
        leg["stages_ms"] = {"kernel_by_events": kernel_ms(ctx, comp.staged.cuda(), comp.n, comp.crc_segments),
                            "host_crc_alone": median_of(lambda: host_crc(view, data, idat)),
                            "join_copy_alone": median_of(lambda: join(data, idat, scratch)),
                            "chunk_walk_alone": median_of(lambda: walk(view)),
                            "parse_compressed_crc_host": median_of(lambda: png.parse_compressed(data)),
                            "parse_compressed_crc_device": median_of(lambda: png.parse_compressed(data, crc="device"))}
        result[name] = leg
        print(name, json.dumps(leg), flush=True)

    # ---- the defaults against the parent tree ----
    if args.parent:
        with tempfile.TemporaryDirectory() as work:
            np.save(os.path.join(work, "panel.npy"), img)
            with open(os.path.join(work, "level6.png"), "wb") as f:
                f.write(blobs["level6"])
            del dev_img
            torch.cuda.empty_cache()
            result["defaults_against_parent"] = defaults_against(args.parent, work, args.rounds, args.pairs)
        print("defaults_against_parent", json.dumps(result["defaults_against_parent"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
