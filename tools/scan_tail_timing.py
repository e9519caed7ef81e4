"""What merging a scan's tile detections on the device (RADNet.scan_tail, csrc/scan_tail.hip) changes inside RADNet.predict.  One
synthetic 4000x4000x3 noise image on the device, the default Config (tile_size 2000, tile_overlap 400: 36 tiles,
img_size 600), synthetic weights (bench.py's), one GPU.  After warm-up and plan building, alternating pairs inside one process, per
--bbox-threshold (0.0 keeps every decoded box, so the merge has work; at the default 0.7 the synthetic weights give no box and only
the per-tile record downloads differ):
  predict([cuda_tensor]) with scan_tail off (the parent commit's path) against on           ms per image;
  the merge alone on the recorded pool of that run: the host merge (one download of the pool, the records unpacked, final_nms per
  class, NMS 0.4 per class) against radnet_scan_merge with its one download and the list built.
Medians and the spread of the runs are reported; the detections of the variants are compared in every run (they must be equal).
Stops starting new runs once --budget seconds have passed.
usage: python tools/scan_tail_timing.py [--size 4000] [--runs 7] [--budget 400] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [HERE, os.path.join(HERE, "rock-art-radnet_amd")]
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")         # as bench.py: the lanes need more than 4 hardware queues
import torch  # noqa: E402


def build_net():
    from faster_rcnn import models as M
    from faster_rcnn.RADNet import RADNet
    from faster_rcnn.base_models import resnet50
    from faster_rcnn.config import Config
    from radnet_hip import synth
    C = Config()
    ms = M.build_models(C, weights=synth.synthetic_weights(seed=3), workload="predict")
    return C, RADNet(C, ms[3], ms[4], resnet50.preprocess)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def plain(dets):
    return [[d["class"], float(d["prob"]), int(d["x1"]), int(d["y1"]), int(d["x2"]), int(d["y2"])] for d in dets]


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--budget", type=float, default=400.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scan_tail_timing needs a GPU")
    start = time.perf_counter()
    from radnet_hip.engine import read_detections
    C, net = build_net()
    eng = net._engine()
    dev = torch.from_numpy(np.random.RandomState(4).randint(0, 256, (args.size, args.size, 3)).astype(np.uint8)).cuda()
    result = {"size": args.size, "img_size": C.img_size, "device": torch.cuda.get_device_name(0), "thresholds": {}}

    def predict(scan):
        net.scan_tail = scan
        try:
            return net.predict([dev])
        finally:
            net.scan_tail = False

    for thr in (0.0, 0.7):
        net.bbox_threshold = thr
        for _ in range(2):                                 # plans, launch shapes, graphs, the pool and the workspace
            off, on = plain(predict(False)), plain(predict(True))
        assert off == on, "the two merges disagree"
        dd = net.predict_device([dev])                      # the recorded pool of this run, for the merge alone
        assert plain(dd.to_host()) == off
        pool, sw, offs = dd._pool, dd._slot_words, dd._offsets
        n_tiles = sum(len(o) for o in offs)
        pool_host = pool.cpu().numpy()
        n_records = int(sum(max(0, int(pool_host[j * sw])) for j in range(n_tiles)))
        table = eng.scan_table([(j * sw, ox, oy, 0) for j, (ox, oy) in enumerate(offs[0])])
        rows = (sw - 8) // 6

        def host_merge():
            words = pool.cpu().numpy()                      # one download, then today's host merge
            dets = [net._det_from_records(*read_detections(words[j * sw:(j + 1) * sw])) for j in range(n_tiles)]
            all_boxes, all_probs = {}, {}
            net._merge_image(dets, offs[0], all_boxes, all_probs)
            return net._merge_final(all_boxes, all_probs)

        def device_merge():
            from faster_rcnn.RADNet import DeviceDetections
            with torch.cuda.stream(eng.main_stream):
                out = eng.scan_merge(pool, rows, table)
                return DeviceDetections(out, eng.mark(), net, pool, sw, offs).to_host()

        assert plain(host_merge()) == plain(device_merge()) == off
        ms = {"predict_scan_tail_off": [], "predict_scan_tail_on": [], "merge_host": [], "merge_device": []}
        pairs = (("predict_scan_tail_off", lambda: predict(False)), ("predict_scan_tail_on", lambda: predict(True)),
                 ("merge_host", host_merge), ("merge_device", device_merge))
        for r in range(args.runs):
            if time.perf_counter() - start > args.budget * (0.55 if thr == 0.0 else 1.0):
                print("budget reached after %d runs at threshold %.1f" % (r, thr), flush=True)
                break
            for a, b in ((0, 1), (2, 3)):
                for k in ((a, b) if r % 2 == 0 else (b, a)):
                    t, out = timed(pairs[k][1])
                    assert plain(out) == off, pairs[k][0]
                    ms[pairs[k][0]].append(t)
                    print("threshold %.1f %s run %d: %.2f ms" % (thr, pairs[k][0], r, t), flush=True)
        result["thresholds"]["%.1f" % thr] = {"tiles": n_tiles, "tile_records": n_records, "detections": len(off),
                                               "ms": {k: spread(v) for k, v in ms.items() if v}}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(os.path.abspath(args.out), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
