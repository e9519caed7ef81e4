"""The launches of the NMS family alone on one GPU, each a series of --runs windows of --launches back-to-back calls timed by device
events (the windows of the series alternate; the median and the windows are reported, microseconds per call):
  rpn.rpn_to_roi at the 1000x600 step's size (38x63x12 = 28 728 candidates, scores from the synthetic-weight network, 0.7, 300 boxes):
    the default path (rocPRIM radix sort + fp64 NMS) and RADNET_PROPOSALS_SELECT=1 (one workgroup: radix select / LDS sort / integer NMS);
  radnet_nms on 4 096 random boxes (0.7, 300 boxes);
  radnet_detect_tail on 300 rows of 7 classes with bbox_threshold 0 (every row that is not background reaches the NMS 0.2);
  radnet_final_nms on one group of 2 049 boxes (sorted in the workspace) and one of 1 025 (sorted in LDS), a few hundred clusters each.
usage: python tools/proposals_timing.py [--runs 7] [--launches 20] [--out FILE.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rock-art-radnet_amd")]

from faster_rcnn.config import Config  # noqa: E402
from radnet_hip import engine as E  # noqa: E402
from radnet_hip import lib as L  # noqa: E402
from radnet_hip import make_engine, synth  # noqa: E402


def event_us(fn, launches):
    """Microseconds per call over a window of `launches` back-to-back calls."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(launches):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3 / launches


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rpn_series(eng):
    bp = eng.upload_image(synth.synthetic_panel(1, 600, 1000))
    eng.base_forward(bp)
    rp = eng.rpn_forward(bp)
    assert (rp["fh"], rp["fw"], eng.A) == (38, 63, 12)

    def call(select):
        if select:
            os.environ["RADNET_PROPOSALS_SELECT"] = "1"     # read per call
        else:
            os.environ.pop("RADNET_PROPOSALS_SELECT", None)
        eng.proposals(rp, 0.7, 300)

    return {"rpn_to_roi_38x63x12_full_sort": lambda: call(False), "rpn_to_roi_38x63x12_select": lambda: call(True)}, lambda: int(rp["Rn"].cpu()[0])


def nms_series(ctx, n=4096):
    rs = np.random.RandomState(1)
    xy, wh = rs.uniform(0.0, 600.0, (n, 2)), rs.uniform(16.0, 128.0, (n, 2))
    boxes, probs = dev(np.concatenate([xy, xy + wh], 1)), dev(rs.permutation(n).astype(np.float32) / np.float32(n))
    idx, cnt = torch.zeros(300, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(ctx.lib.radnet_proposals_ws_bytes(n)), dtype=torch.uint8, device="cuda")
    return {"nms_%d_boxes" % n: lambda: ctx.call("radnet_nms", boxes, probs, n, C.c_double(0.7), 300, idx, cnt, ws)}, lambda: int(cnt.cpu()[0])


def detect_tail_series(ctx, C_, rows=300, nc=7):
    rs = np.random.RandomState(2)
    z = rs.standard_normal((rows, nc)) * 3.0
    e = np.exp(z - z.max(axis=1, keepdims=True))
    std = [float(s) for s in C_.classifier_regr_std]
    t = [dev((e / e.sum(axis=1, keepdims=True)).astype(np.float32)), dev((rs.standard_normal((rows, 4 * (nc - 1))) * 0.15 * np.tile(std, nc - 1)).astype(np.float32)),
         dev(np.stack([rs.randint(0, 30, rows), rs.randint(0, 30, rows), rs.randint(2, 13, rows), rs.randint(2, 13, rows)], 1).astype(np.float32)),
         torch.tensor([rows], dtype=torch.int32, device="cuda")]
    out = torch.zeros(int(ctx.lib.radnet_detect_tail_out_bytes(rows)) // 4, dtype=torch.int32, device="cuda")
    d = L.DetectTailDesc()
    d.p_cls, d.p_regr, d.rois, d.n = [a.data_ptr() for a in t]
    d.rows, d.nc, d.k, d.bg = rows, nc, C_.n_rois, nc - 1
    d.bbox_threshold = E.threshold_f32(0.0)
    d.regr_std[:] = std
    d.rpn_stride, d.nms_thresh, d.ratio, d.max_boxes, d.out = float(C_.rpn_stride), 0.2, 300 / 2048, 300, out.data_ptr()
    d.tensors = t                                               # the descriptor holds addresses only: the tensors live as long as it does
    return {"detect_tail_%d_rows" % rows: lambda: ctx.check(ctx.lib.radnet_detect_tail(ctx.h, C.byref(d)), "radnet_detect_tail")}, lambda: int(out.cpu()[0])


def final_nms_series(ctx, n, centres, seed):
    rs = np.random.RandomState(seed)
    xy = rs.randint(50, 4000, (centres, 2))[rs.randint(0, centres, n)] + rs.randint(-6, 7, (n, 2))
    boxes, probs = dev(np.concatenate([xy, xy + rs.randint(30, 50, (n, 2))], 1).astype(np.int64)), dev(rs.uniform(0.7, 1.0, n).astype(np.float32))
    keep = [boxes, probs, dev(np.array([0, n], np.int32)), torch.zeros(n, 4, dtype=torch.int64, device="cuda"), torch.zeros(n, device="cuda"),
            torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"),
            torch.empty(int(ctx.lib.radnet_final_nms_ws_bytes(n, 1)), dtype=torch.uint8, device="cuda")]
    d = L.FinalNmsDesc()
    d.boxes, d.probs, d.offsets, d.out_boxes, d.out_probs, d.out_count, d.out_status, d.ws = [a.data_ptr() for a in keep]
    d.n_groups, d.capacity, d.obj_avg_threshold, d.obj_confidence_threshold, d.n_obj_avg = 1, n, 0.2, E.confidence_f32(0.8), 5
    d.tensors = keep
    return {"final_nms_group_%d" % n: lambda: ctx.check(ctx.lib.radnet_final_nms(ctx.h, C.byref(d)), "radnet_final_nms")}, lambda: int(keep[5].cpu()[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("proposals_timing needs a GPU")
    C_ = Config()
    eng = make_engine(C_)
    eng.set_weights(synth.synthetic_weights(seed=3))
    ctx = eng.ctx
    series, counts = {}, {}
    for fns, count in (rpn_series(eng), nms_series(ctx), detect_tail_series(ctx, C_), final_nms_series(ctx, 2049, 420, 6), final_nms_series(ctx, 1025, 260, 5)):
        for name, fn in fns.items():
            for _ in range(3):                                 # warm-up: code objects, rocPRIM's first call
                fn()
            counts[name] = count()                             # picks / records / clusters of the call just made: the work is there
            assert counts[name] > 0, (name, counts[name])
            series[name] = fn
    runs = {name: [] for name in series}
    for k in range(args.runs):                                 # the windows alternate
        for name in (list(series) if k % 2 == 0 else list(series)[::-1]):
            runs[name].append(event_us(series[name], args.launches))
    os.environ.pop("RADNET_PROPOSALS_SELECT", None)
    result = {"runs": args.runs, "launches_per_window": args.launches, "device": torch.cuda.get_device_name(0), "library": os.path.basename(L.LIB_PATH),
              "series": {name: {"median_us": statistics.median(v), "results": counts[name], "runs_us": v} for name, v in runs.items()}}
    for name, v in result["series"].items():
        print("%-34s %9.1f us  (%d results; windows %.1f .. %.1f)" % (name, v["median_us"], v["results"], min(v["runs_us"]), max(v["runs_us"])), flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(os.path.abspath(args.out), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
