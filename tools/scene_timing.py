"""What the scene painter costs.  Launches alone, by device events, several per window, the tables uploaded once outside the windows:
  the precision/recall figure: radnet_draw_scene_u8 with figures.precision_recall_scene's list (about 3000 entries: synthetic
    curves of --classes classes with --detections detections each) on a white 1200x1200 canvas;
  a labelled map: ONE synthetic 4000x4000 image (tools/feed_timing.py's panel) with the labelled list of RADNet.draw_detections for
    its 360 boxes (1440 opaque rectangles and text runs) through radnet_draw_scene_u8 AND through radnet_draw_list_u8 -- the price of
    the blending kernel on a list that does not blend -- and the same list with every entry translucent (tau = 102) through the scene;
    the windows alternate; the two opaque results are compared byte for byte on the device;
  radnet_grey3_u8 on the 4000x4000 image, out of place.
One GPU, nothing else running.
usage: python tools/scene_timing.py [--size 4000] [--figure 1200] [--classes 2] [--detections 1000] [--runs 7] [--launches 20] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rock-art-radnet_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402

import feed_timing as FT  # noqa: E402
from faster_rcnn import RADNet as R  # noqa: E402
from faster_rcnn import evaluate, figures  # noqa: E402
from label_timing import _Config, event_ms, timed  # noqa: E402


def synthetic_curves(classes, detections, seed=0):
    """calc_class_ap's curves of `classes` classes: `detections` scored detections each, six in ten of them hits."""
    rs = np.random.RandomState(seed)
    return {"class %02d" % k: evaluate.calc_class_ap(list((rs.random_sample(detections) < 0.6).astype(int)), list(rs.random_sample(detections)))
            for k in range(classes)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4000)
    ap.add_argument("--figure", type=int, default=1200)
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--detections", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out:
        args.out = os.path.abspath(args.out)
    if not torch.cuda.is_available():
        raise SystemExit("scene_timing needs a GPU: the painters are device kernels")
    from radnet_hip import runtime as rt
    ctx = rt.default_context()
    med = statistics.median
    result = {"size": args.size, "figure": args.figure, "runs": args.runs, "launches_per_window": args.launches, "device": torch.cuda.get_device_name(0)}

    def launch(entry, canvas, prims):
        table, chars = R.scene_table(prims)
        table_dev = torch.from_numpy(table.view(np.uint8)).cuda()
        chars_dev = torch.from_numpy(chars.copy()).cuda() if len(chars) else None
        h, w = canvas.shape[:2]
        return lambda: ctx.call(entry, canvas, h, w, 3 * w, table.ctypes.data, table_dev, len(table), chars.ctypes.data if len(chars) else None, chars_dev,
                                len(chars))

    # ---- the lists ---------------------------------------------------------------------------------------------------------------------
    curves = synthetic_curves(args.classes, args.detections)
    figure = figures.precision_recall_scene(curves, float(np.mean([c[0] for c in curves.values()])), args.figure)
    data, img, _ = FT.dataset(args.size)
    h, w = img.shape[:2]
    dev = torch.from_numpy(img).cuda()
    dets = [dict(b, prob=0.2 + 0.8 * ((37 * k) % 101) / 100.0) for k, b in enumerate(data[0]["bboxes"])]
    captured = []
    real = R.draw_list_device
    R.draw_list_device = lambda image, prims, inplace=False, ctx=None: captured.append(list(prims)) or image
    try:
        R.RADNet(_Config(), None, None, None).draw_detections(dev, dets, labels=True)
    finally:
        R.draw_list_device = real
    labelled = captured[0]
    translucent = [tuple(p) + ({"transparency": 102},) for p in labelled]
    kinds = {k: sum(p[0] == k for p in figure) for k in ("rect", "text", "line")}
    result["lists"] = {"figure_entries": len(figure), "figure_kinds": kinds, "figure_dashed": sum(isinstance(p[-1], dict) and "dash" in p[-1] for p in figure),
                       "detections": len(dets), "labelled_entries": len(labelled)}
    print("lists:", json.dumps(result["lists"]), flush=True)

    # ---- the launches ------------------------------------------------------------------------------------------------------------------
    white = torch.full((args.figure, args.figure, 3), 255, dtype=torch.uint8, device="cuda")
    by_scene, by_list, mixed, grey = dev.clone(), dev.clone(), dev.clone(), torch.empty_like(dev)
    launches = {"scene_figure_ms": launch("radnet_draw_scene_u8", white, figure),
                "scene_labelled_ms": launch("radnet_draw_scene_u8", by_scene, labelled),
                "list_labelled_ms": launch("radnet_draw_list_u8", by_list, labelled),
                "scene_labelled_translucent_ms": launch("radnet_draw_scene_u8", mixed, translucent),
                "grey3_ms": lambda: ctx.call("radnet_grey3_u8", dev, grey, h, w, 3 * w, 3 * w)}
    for fn in launches.values():                                             # warm-up: code objects
        timed(fn)
    assert torch.equal(by_scene, by_list), "the scene kernel and the list kernel disagree on an opaque list"
    assert not torch.equal(by_scene, dev) and not torch.equal(mixed, by_scene) and bool((white != 255).any())
    runs = {name: [] for name in launches}
    for k in range(args.runs):                                               # the windows alternate
        for name in (list(launches) if k % 2 == 0 else list(launches)[::-1]):
            runs[name].append(event_ms(launches[name], args.launches))
    stages = {}
    for name in launches:
        stages[name] = med(runs[name])
        stages[name.replace("_ms", "_runs_ms")] = runs[name]
    stages["scene_over_list_labelled"] = stages["scene_labelled_ms"] / stages["list_labelled_ms"]
    result["launches"] = stages
    print("launches:", json.dumps(stages), flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
