"""What the text labels cost on an annotated map.  ONE synthetic 4000x4000 RGB 8-bit image on the device (tools/feed_timing.py's
panel, as in tools/png_write_timing.py) and its 360 boxes as detections (class names of the panel, a spread of probabilities):
  the launches alone, by device events, several per window: radnet_draw_list_u8 with the labelled list of RADNet.draw_detections
  (per box: outline at thickness 8, the label box as a black outline and FILLED white, the text at scale 3: 1440 entries) against
  radnet_draw_rects_u8 with the 360 outlines, and the draw list with the 360 outlines only (the list kernel's price for rectangles);
  the tables are uploaded once, outside the windows, and the windows alternate;
  RADNet.write_predictions(labels=True) against labels=False, wall time with the device drained, in alternating pairs inside one
  process: four maps and the JSON each, of which the labelled call labels two.
The labelled `all` map is read back and compared with the NumPy painter of tests/draw_list_cases.py.  One GPU, nothing else running.
usage: python tools/label_timing.py [--size 4000] [--pairs 5] [--runs 7] [--launches 20] [--out FILE.json]"""
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

import draw_list_cases as D  # noqa: E402
import feed_timing as FT  # noqa: E402
from faster_rcnn import RADNet as R  # noqa: E402
from faster_rcnn import png  # noqa: E402
from radnet_hip import lib as L  # noqa: E402


class _Config:
    class_mapping = {c: k for k, c in enumerate(FT.CLASSES)}


def paint_windowed(img, prims, font):
    """tests/draw_list_cases.paint_list entry by entry on the window of the image each entry can reach (the painter makes image-sized
    masks, which 1440 entries on 16 M pixels do not need): the same pixels, since clipping to a window inside the image that holds
    everything the entry paints there is clipping to the image."""
    h, w = img.shape[:2]
    for p in prims:
        if p[0] == "rect":
            hw = max(p[5], 0) // 2
            x0, x1, y0, y1 = min(p[1], p[3]) - hw, max(p[1], p[3]) + hw, min(p[2], p[4]) - hw, max(p[2], p[4]) + hw
        else:
            x0, x1, y0, y1 = p[1], p[1] + D.ADVANCE * len(p[3]) * p[4], p[2] - D.CAP_ROWS * p[4], p[2] + p[4]
        x0, x1, y0, y1 = max(x0, 0), min(x1, w - 1), max(y0, 0), min(y1, h - 1)
        if x0 > x1 or y0 > y1:
            continue
        moved = ("rect", p[1] - x0, p[2] - y0, p[3] - x0, p[4] - y0) + tuple(p[5:]) if p[0] == "rect" else ("text", p[1] - x0, p[2] - y0) + tuple(p[3:])
        D.paint_list(img[y0:y1 + 1, x0:x1 + 1], [moved], font)
    return img


def with_bytes(prims):
    """The text entries' strings as the bytes draw_list_device sends."""
    return [p[:3] + (R.label_bytes(p[3]),) + p[4:] if p[0] == "text" else p for p in prims]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def event_ms(fn, launches):
    """Milliseconds per launch over a window of `launches` back-to-back launches."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(launches):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4000)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out:
        args.out = os.path.abspath(args.out)
    if not torch.cuda.is_available():
        raise SystemExit("label_timing needs a GPU: the painters are device kernels")
    from radnet_hip import runtime as rt
    ctx = rt.default_context()
    data, img, _ = FT.dataset(args.size)
    h, w = img.shape[:2]
    dev = torch.from_numpy(img).cuda()
    dets = [dict(b, prob=0.2 + 0.8 * ((37 * k) % 101) / 100.0) for k, b in enumerate(data[0]["bboxes"])]
    net = R.RADNet(_Config(), None, None, None)
    med = statistics.median
    result = {"size": args.size, "detections": len(dets), "pairs": args.pairs, "runs": args.runs, "launches_per_window": args.launches,
              "device": torch.cuda.get_device_name(0)}

    # ---- the launches alone ------------------------------------------------------------------------------------------------------------
    captured = []
    real = R.draw_list_device
    R.draw_list_device = lambda image, prims, inplace=False, ctx=None: captured.append(list(prims)) or image
    try:
        net.draw_detections(dev, dets, labels=True)                          # the list write_predictions sends for the `all` map
    finally:
        R.draw_list_device = real
    labelled = captured[0]
    outlines = [p for p in labelled if p[0] == "rect" and p[5] == 8]
    canvas = dev.clone()

    def list_launch(prims):
        rows, pool = D.pack(with_bytes(prims))
        table, chars = np.array(rows, R.PRIM), np.frombuffer(pool, np.uint8).copy()
        table_dev = torch.from_numpy(table.view(np.uint8)).cuda()
        chars_dev = torch.from_numpy(chars).cuda() if len(chars) else None
        return lambda: ctx.call("radnet_draw_list_u8", canvas, h, w, 3 * w, table.ctypes.data, table_dev, len(table),
                                chars.ctypes.data if len(chars) else None, chars_dev, len(chars))

    rect_table = np.array([p[1:] for p in outlines], R.RECT)
    rect_dev = torch.from_numpy(rect_table.view(np.uint8)).cuda()
    launches = {"draw_rects_outlines_ms": lambda: ctx.call("radnet_draw_rects_u8", canvas, h, w, 3 * w, rect_table.ctypes.data, rect_dev, len(rect_table)),
                "draw_list_outlines_ms": list_launch(outlines),
                "draw_list_labelled_ms": list_launch(labelled)}
    for fn in launches.values():                                             # warm-up: code objects
        timed(fn)
    runs = {name: [] for name in launches}
    for k in range(args.runs):                                               # the windows alternate
        for name in (list(launches) if k % 2 == 0 else list(launches)[::-1]):
            runs[name].append(event_ms(launches[name], args.launches))
    stages = {"outlines": len(outlines), "labelled_entries": len(labelled), "label_characters": sum(len(p[3]) for p in labelled if p[0] == "text")}
    for name in launches:
        stages[name] = med(runs[name])
        stages[name.replace("_ms", "_runs_ms")] = runs[name]
    result["launches"] = stages
    print("launches:", json.dumps(stages), flush=True)

    # ---- write_predictions, labels on and off, in alternating pairs ---------------------------------------------------------------------
    with tempfile.TemporaryDirectory() as tmp:
        on_dir, off_dir = os.path.join(tmp, "labelled"), os.path.join(tmp, "plain")
        _, on_paths = timed(lambda: net.write_predictions(dets, dev, on_dir, labels=True))      # warm-up and check
        timed(lambda: net.write_predictions(dets, dev, off_dir))
        font = {code: L.glyph_rows(code) for code in range(D.FIRST, D.LAST + 1)}
        want = paint_windowed(img.copy(), with_bytes(labelled), font)
        got = png.decode_device(np.fromfile(on_paths[0], np.uint8)).cpu().numpy()
        assert np.array_equal(got, want), "the labelled map does not decode to the painter's image"
        a, b = [], []
        for k in range(args.pairs):
            for which in ((0, 1) if k % 2 == 0 else (1, 0)):
                if which == 0:
                    a.append(timed(lambda: net.write_predictions(dets, dev, off_dir))[0])
                else:
                    b.append(timed(lambda: net.write_predictions(dets, dev, on_dir, labels=True))[0])
        result["write_predictions"] = {"plain_ms": med(a), "labelled_ms": med(b), "labelled_over_plain_median_of_pairs": med(y / x for x, y in zip(a, b)),
                                       "plain_runs_ms": a, "labelled_runs_ms": b,
                                       "plain_all_map_bytes": os.path.getsize(os.path.join(off_dir, "all_predictions.png")),
                                       "labelled_all_map_bytes": os.path.getsize(on_paths[0])}
    print("write_predictions:", json.dumps(result["write_predictions"]), flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
