"""What the score-map pictures cost.  ONE synthetic 4000x4000 image (tools/feed_timing.py's panel), the default Config (tile_size 2000,
tile_overlap 400: 36 tiles, img_size 600), synthetic weights (bench.py's), one GPU, nothing else running:
  the paint launch: radnet_heat_paint_u8 with the 36 placements of RADNet.objectness_maps over a grey copy of the image, by device
    events, several launches per window, the table uploaded once outside the windows; translucent (tau = 102, every pixel loaded
    and stored) and opaque (tau = 0, stored only);
  the levels launches: radnet_score_levels_u8 on one tile's scores (38 x 38 cells, all anchors), by device events;
  RADNet.objectness_maps as a whole beside RADNet.predict on the same device image, wall clock, the two taking turns.
Medians and the runs are reported.  No time is promised anywhere; these are the first measurements of these kernels.
usage: python tools/heat_timing.py [--size 4000] [--runs 7] [--launches 20] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rock-art-radnet_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")         # as bench.py: the lanes need more than 4 hardware queues
import torch  # noqa: E402

import feed_timing as FT  # noqa: E402
from faster_rcnn import RADNet as R  # noqa: E402
from faster_rcnn import figures  # noqa: E402
from label_timing import event_ms, timed  # noqa: E402


def build_net():
    from faster_rcnn import models as M
    from faster_rcnn.base_models import resnet50
    from faster_rcnn.config import Config
    from radnet_hip import synth
    C = Config()
    ms = M.build_models(C, weights=synth.synthetic_weights(seed=3), workload="predict")
    return C, R.RADNet(C, ms[3], ms[4], resnet50.preprocess)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out:
        args.out = os.path.abspath(args.out)
    if not torch.cuda.is_available():
        raise SystemExit("heat_timing needs a GPU: the painters are device kernels")
    from radnet_hip import runtime as rt
    from radnet_hip.engine import RPN_LD
    ctx = rt.default_context()
    med = statistics.median
    C, net = build_net()
    _, img, _ = FT.dataset(args.size)
    h, w = img.shape[:2]
    dev = torch.from_numpy(img).cuda()
    result = {"size": args.size, "img_size": C.img_size, "runs": args.runs, "launches_per_window": args.launches, "device": torch.cuda.get_device_name(0)}

    # ---- the whole passes: plans, launch shapes and graphs first --------------------------------------------------------------------------
    for _ in range(2):
        maps = net.objectness_maps(dev)
        net.predict([dev])
    result["windows"] = len(maps.places)
    result["cells"] = int(maps.pool.numel())
    passes = {"objectness_maps_ms": lambda: net.objectness_maps(dev), "predict_ms": lambda: net.predict([dev])}
    runs = {name: [] for name in passes}
    for k in range(args.runs):                                               # the two take turns
        for name in (list(passes) if k % 2 == 0 else list(passes)[::-1]):
            runs[name].append(timed(passes[name])[0])
    whole = {}
    for name in passes:
        whole[name] = med(runs[name])
        whole[name.replace("_ms", "_runs_ms")] = runs[name]
    whole["objectness_maps_over_predict"] = whole["objectness_maps_ms"] / whole["predict_ms"]
    result["passes"] = whole
    print("passes:", json.dumps(whole), flush=True)

    # ---- the launches ------------------------------------------------------------------------------------------------------------------
    table = R.heat_table(maps.places)
    table_dev = torch.from_numpy(table.view(np.uint8)).cuda()
    lut_dev = torch.from_numpy(figures.heat_lut().reshape(-1).copy()).cuda()
    grey = R.grey3_device(dev)
    mixed, opaque = grey.clone(), grey.clone()

    def paint(canvas, tau):
        return lambda: ctx.call("radnet_heat_paint_u8", canvas, h, w, 3 * w, maps.pool, maps.pool.numel(), table.ctypes.data, table_dev, len(table), lut_dev, tau, 0)

    fw, fh, A = maps.places[0][4], maps.places[0][5], net._engine().A
    scores = torch.rand(fh * fw, RPN_LD, device="cuda")
    levels = torch.empty(fh * fw, dtype=torch.uint8, device="cuda")
    launches = {"paint_translucent_ms": paint(mixed, 102), "paint_opaque_ms": paint(opaque, 0),
                "levels_one_tile_ms": lambda: ctx.call("radnet_score_levels_u8", scores, RPN_LD, fh * fw, 0, A, levels)}
    for fn in launches.values():                                             # warm-up: code objects
        timed(fn)
    assert torch.equal(figures.objectness_view(dev, maps, transparency=0), opaque) and not torch.equal(opaque, grey)
    assert np.array_equal(levels.cpu().numpy(), figures.to_levels(scores[:, :A].max(dim=1).values.cpu().numpy()))
    runs = {name: [] for name in launches}
    for k in range(args.runs):                                               # the windows alternate
        for name in (list(launches) if k % 2 == 0 else list(launches)[::-1]):
            runs[name].append(event_ms(launches[name], args.launches))
    stages = {"map_cells_per_tile": [fh, fw]}
    for name in launches:
        stages[name] = med(runs[name])
        stages[name.replace("_ms", "_runs_ms")] = runs[name]
    stages["levels_all_windows_ms"] = stages["levels_one_tile_ms"] * len(maps.places)
    result["launches"] = stages
    print("launches:", json.dumps(stages), flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
