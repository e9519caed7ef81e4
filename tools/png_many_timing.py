"""What png.decode_device_many(inflate="device" / "device-lz") changes against its host inflate, on one MI355X.  The yardstick of
every leg is decode_device_many with inflate="host" in the same run: the two alternate as pairs in one process, the order swapping
from pair to pair, wall time with the device drained (tools/png_timing.py's scheme); medians of `pairs` runs, the runs themselves
and the spread (max - min) of each side; a "gain" or a "loss" is stated only where the medians differ by more than the spread of
either side, else "no difference claimed" (the rules of tools/png_join_timing.py; every leg is decoded once first, as warm-up, and
checked against the source images).
  panels   eight distinct size x size panels (the panel of tools/feed_timing.py rolled by 37 rows and columns per file) as the files
           of tools/png_timing.py and tools/png_inflate_timing.py write them: cv2 (level 1, Z_RLE, IDAT chunks of 8 KiB; "device"),
           imwrite (png.encode_device; "device") and level6 (adaptive filters, one IDAT; "device-lz").  The host leg at workers=8
           and at workers=16.
  tiles    64 files of 600 x 600 cut out of the panel, cv2 ("device") and level 6 ("device-lz").
  scan     the six maps of one synthetic scan, 1500 x 1500, cv2 ("device") and level 6 ("device-lz").
Every leg also measures the same files through per-file png.decode_device calls with the same device modes, again in pairs
with the batched call.  The device side runs with everything on: unfilter="tiles", crc="device", join="device" (--plain: the inflate alone).  Per leg the
staged breakdown (report["stages"]) of one decode is recorded as well.
  defaults (--parent DIR, a built checkout of the parent commit): decode_device_many with NO keywords on the level-6 tiles and
           panels, this tree and the parent in alternating child processes.
usage: python tools/png_many_timing.py [--size 4000] [--pairs 7] [--legs panels,tiles,scan] [--kinds cv2,imwrite,level6] [--plain]
                                       [--parent DIR] [--rounds 3] [--out FILE.json]"""
import argparse
import concurrent.futures
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spread(runs):
    return max(runs) - min(runs)


def verdict(yard, new, yard_runs, new_runs):
    diff = yard - new
    if abs(diff) <= max(spread(yard_runs), spread(new_runs)):
        return "no difference claimed"
    return "%s %.2f ms" % ("gain" if diff > 0 else "loss", abs(diff))


def defaults_child(root, work, pairs):
    """decode_device_many with no keywords, in the tree `root`, on the files saved under `work`: one warm-up, then `pairs` runs."""
    sys.path[:0] = [root, os.path.join(root, "rock-art-radnet_amd"), os.path.join(root, "tests"), os.path.join(root, "tools")]
    import png_timing as PT
    from faster_rcnn import png
    out = {}
    for leg in ("tiles", "panels"):
        names = sorted(n for n in os.listdir(work) if n.startswith(leg))
        files = [np.fromfile(os.path.join(work, n), np.uint8) for n in names]
        png.decode_device_many(files)
        out[leg] = [PT.timed(lambda: png.decode_device_many(files))[0] for _ in range(pairs)]
    print("DEFAULTS " + json.dumps(out), flush=True)


def defaults_against(parent, work, rounds, pairs):
    got = {"this": {}, "parent": {}}
    for k in range(rounds):
        for which in (("this", "parent") if k % 2 == 0 else ("parent", "this")):
            root = ROOT if which == "this" else os.path.abspath(parent)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--defaults-child", root, "--work", work, "--pairs", str(pairs)],
                               capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise RuntimeError("the defaults child of %s failed:\n%s\n%s" % (root, r.stdout[-2000:], r.stderr[-2000:]))
            rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("DEFAULTS ")][-1][len("DEFAULTS "):])
            for leg, runs in rec.items():
                got[which].setdefault(leg, []).extend(runs)
    out = {"rounds": rounds, "runs_per_round": pairs}
    for leg in got["this"]:
        a, b = got["parent"][leg], got["this"][leg]
        out[leg] = {"parent_ms": statistics.median(a), "this_ms": statistics.median(b), "parent_spread_ms": spread(a), "this_spread_ms": spread(b),
                    "verdict": verdict(statistics.median(a), statistics.median(b), a, b), "parent_runs_ms": a, "this_runs_ms": b}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4000)
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--legs", default="panels,tiles,scan")
    ap.add_argument("--kinds", default="cv2,imwrite,level6")
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--defaults-child", default=None)
    ap.add_argument("--work", default=None)
    args = ap.parse_args()
    if args.defaults_child:
        return defaults_child(args.defaults_child, args.work, args.pairs)
    sys.path[:0] = [ROOT, os.path.join(ROOT, "rock-art-radnet_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
    import torch
    import feed_timing as FT
    import png_inflate_timing as PIT
    import png_timing as PT
    from faster_rcnn import png

    writers = {"cv2": ("device", PIT.cv2_like), "imwrite": ("device", lambda im: png.encode_device(torch.from_numpy(np.ascontiguousarray(im)).cuda())),
               "level6": ("device-lz", PT.encode_rgb8)}
    kinds = [k for k in args.kinds.split(",") if k]
    legs = [l for l in args.legs.split(",") if l]
    extra = {} if args.plain else dict(unfilter="tiles", crc="device", join="device")
    _, panel, _ = FT.dataset(args.size)
    result = {"size": args.size, "pairs": args.pairs, "device": torch.cuda.get_device_name(0), "device_modes": extra}

    def encode_all(kind, images):
        write = writers[kind][1]
        if kind == "imwrite":                       # the device writer: one after the other
            return [np.frombuffer(write(im), np.uint8) for im in images]
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(len(images), 16)) as pool:
            return [np.frombuffer(b, np.uint8) for b in pool.map(write, images)]

    def pair(yard_fn, new_fn):
        got = PT.alternating_pairs(yard_fn, new_fn, args.pairs)
        a, b = got["sequential_runs_ms"], got["many_runs_ms"]
        return {"yardstick_ms": got["sequential_ms"], "device_many_ms": got["many_ms"], "yardstick_over_device_median_of_pairs": got["speedup_median_of_pairs"],
                "yardstick_spread_ms": spread(a), "device_many_spread_ms": spread(b), "verdict": verdict(got["sequential_ms"], got["many_ms"], a, b),
                "yardstick_runs_ms": a, "device_many_runs_ms": b}

    def leg(name, kind, images, with_workers=False):
        inflate = writers[kind][0]
        files = encode_all(kind, images)
        how = dict(inflate=inflate, **extra)
        report = {}
        got = png.decode_device_many(files, report=report, **how)      # warm-up and check
        for g, im in zip(got, images):
            assert np.array_equal(g.cpu().numpy(), im), (name, kind)
        host = png.decode_device_many(files)
        assert all(torch.equal(g, h) for g, h in zip(got, host)), (name, kind)
        del got, host
        out = {"files": len(files), "file_bytes": int(sum(len(f) for f in files)), "inflate": inflate,
               "paths": sorted({r["path"] for r in report["files"]}), "reasons": sorted({str(r["reason"]) for r in report["files"]}),
               "batches": report["batches"], "overflow": report["overflow"]}
        many = lambda: png.decode_device_many(files, **how)      # noqa: E731
        out["host_many"] = pair(lambda: png.decode_device_many(files), many)
        out["per_file_decode_device"] = pair(lambda: [png.decode_device(f, **how) for f in files], many)
        if with_workers:
            out["host_many_workers_16"] = pair(lambda: png.decode_device_many(files, workers=16), many)
        staged = {"stages": {}}
        png.decode_device_many(files, report=staged, **how)
        out["stages_ms"] = {k: round(v, 3) for k, v in staged["stages"].items() if not k.startswith("_")}
        result.setdefault(name, {})[kind] = out
        print(name, kind, json.dumps(out), flush=True)
        torch.cuda.empty_cache()
        return files

    saved = {}
    if "panels" in legs:
        images = [panel] + [np.roll(panel, (37 * k, 37 * k), axis=(0, 1)) for k in range(1, 8)]
        for kind in kinds:
            files = leg("panels", kind, images, with_workers=True)
            if kind == "level6":
                saved["panels"] = files
        del images
    if "tiles" in legs:
        rs = np.random.RandomState(3)
        images = [np.ascontiguousarray(panel[y:y + 600, x:x + 600]) for y, x in rs.randint(0, args.size - 600, (64, 2))]
        for kind in [k for k in kinds if k != "imwrite"]:
            files = leg("tiles", kind, images)
            if kind == "level6":
                saved["tiles"] = files
    if "scan" in legs:
        images = [np.ascontiguousarray(np.roll(panel, (211 * k, 97 * k), axis=(0, 1))[:1500, :1500]) for k in range(6)]
        for kind in [k for k in kinds if k != "imwrite"]:
            leg("scan", kind, images)
    if args.parent and saved:
        with tempfile.TemporaryDirectory() as work:
            for name, files in saved.items():
                for k, f in enumerate(files):
                    f.tofile(os.path.join(work, "%s_%02d.png" % (name, k)))
            torch.cuda.empty_cache()
            result["defaults_against_parent"] = defaults_against(args.parent, work, args.rounds, args.pairs)
        print("defaults_against_parent", json.dumps(result["defaults_against_parent"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
