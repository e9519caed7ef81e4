"""Edge cases of the fp64 glue kernels: radnet_nms and radnet_rpn_to_roi (both of its paths) of csrc/proposals.hip, radnet_anchor_targets,
radnet_anchor_targets_pack, radnet_roi_targets and radnet_roi_batch_pack of csrc/targets.hip, against the expected buffers that
tests/proposal_edge_cases.py builds from oracle/glue.py (checked, and shown to have teeth, by tests/test_proposal_edge_cases_reference.py).

Every case runs inside the contract of its entry point.  Every output buffer is allocated with 64 elements behind it and prefilled with
the sentinel byte; after EVERY launch the whole buffer is judged: an element the contract writes holds the reference's bits (the `log`
components of the regression targets: 4.5e-16 relative in fp64 with the fp32 casts bit-equal, the tolerance tests/test_gpu_kernels.py
states), every other element -- rows at or past the returned count, rows at or past n_dev, the tail -- still holds the sentinel.  The
rejection tests call an entry with arguments its host checks refuse: a negative code, a message that names the entry, no output element
touched; nothing is launched."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import proposal_edge_cases as E  # noqa: E402

ERR_HIP = -2
F64P = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def ctx():
    """The module's one context, on torch's current stream."""
    from radnet_hip import lib as L
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    cx = L.Context(0)
    yield cx
    torch.cuda.synchronize()
    cx.close()


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()      # a copy: the cached inputs are read-only


def _ptr(t):
    return None if t is None else t.data_ptr()


def _host(a):
    return np.ascontiguousarray(a, np.float64).ctypes.data_as(F64P)


def _fresh(exp):
    """One device buffer per output, every byte the sentinel."""
    return {k: torch.full((o.buf.nbytes,), E.SBYTE, dtype=torch.uint8, device="cuda") for k, o in exp.items()}


def _launch(what, call):
    try:
        rc = call()
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "HIP error" in str(e):                                                 # a device fault: nothing else runs on this device
            pytest.exit("%s: %s" % (what, e), returncode=3)
        raise
    return rc


def _judge(what, bufs, exp):
    bad = []
    for k, o in exp.items():
        bad += E.judge(k, bufs[k].cpu().numpy().view(o.buf.dtype), o)
    assert not bad, (what, bad)


def _run(ctx, what, exp, call):
    """Fresh buffers, one launch that must succeed, every buffer judged in full."""
    bufs = _fresh(exp)
    rc = _launch(what, lambda: call(bufs))
    if rc == ERR_HIP:
        pytest.exit("%s: %s" % (what, ctx.lib.radnet_last_error(ctx.h)), returncode=3)
    ctx.check(rc, str(what))
    _judge(what, bufs, exp)
    return bufs


# ---------------------------------------------------------------------------------------------------------------- radnet_nms
NMS = E.nms_cases()


@pytest.mark.parametrize("i", range(len(NMS)), ids=[c["name"] for c in NMS])
def test_nms(ctx, i):
    cs = NMS[i]
    n = len(cs["boxes"])
    boxes, probs = (_dev(cs["boxes"]), _dev(cs["probs"])) if n else (None, None)
    ws = torch.empty(int(ctx.lib.radnet_proposals_ws_bytes(max(n, 1))), dtype=torch.uint8, device="cuda")
    _run(ctx, ("nms", cs["name"]), E.nms_expected(cs),
         lambda b: ctx.lib.radnet_nms(ctx.h, _ptr(boxes), _ptr(probs), n, cs["thr"], cs["mb"], _ptr(b["out_idx"]), _ptr(b["out_count"]), _ptr(ws)))


# ---------------------------------------------------------------------------------------------------------------- radnet_rpn_to_roi
RPN = E.rpn_cases()


def _with_path(path, call):
    """The call on the default path or with RADNET_PROPOSALS_SELECT=1; the variable is restored in the finally."""
    before = os.environ.get("RADNET_PROPOSALS_SELECT")
    if path == "select":
        os.environ["RADNET_PROPOSALS_SELECT"] = "1"
    else:
        os.environ.pop("RADNET_PROPOSALS_SELECT", None)
    try:
        return call()
    finally:
        if before is None:
            os.environ.pop("RADNET_PROPOSALS_SELECT", None)
        else:
            os.environ["RADNET_PROPOSALS_SELECT"] = before


@pytest.mark.parametrize("path", ["full_sort", "select"])
@pytest.mark.parametrize("i", range(len(RPN)), ids=[c["name"] for c in RPN])
def test_rpn_to_roi(ctx, i, path):
    cs = RPN[i]
    pred = _dev(E.rpn_inputs(i)["pred"])
    awh = np.ascontiguousarray(E.anchor_wh(cs["C"]))
    assert awh.shape == (cs["A"], 2)
    ws = torch.empty(int(ctx.lib.radnet_proposals_ws_bytes(cs["rows"] * cs["cols"] * cs["A"])), dtype=torch.uint8, device="cuda")
    call = lambda b: _with_path(path, lambda: ctx.lib.radnet_rpn_to_roi(
        ctx.h, _ptr(pred), cs["ld"], cs["rows"], cs["cols"], cs["A"], _host(awh), E.STD_SCALING, cs["use_regr"], cs["thr"], cs["mb"],
        _ptr(b["out_boxes"]), _ptr(b["out_probs"]), _ptr(b["out_count"]), _ptr(ws)))
    _run(ctx, ("rpn_to_roi", cs["name"], path), E.rpn_expected(i), call)


# ---------------------------------------------------------------------------------------------------------------- anchor targets
ANCHOR = E.anchor_cases()


@pytest.mark.parametrize("i", range(len(ANCHOR)), ids=[c["name"] for c in ANCHOR])
def test_anchor_targets_and_pack(ctx, i):
    cs = ANCHOR[i]
    m = cs["map"]
    g = len(cs["gt"])
    gt, bg = (_dev(cs["gt"]), _dev(cs["bg"])) if g else (None, None)
    scratch = torch.zeros(max(g, 1), dtype=torch.int64, device="cuda")
    sizes, ratios = np.array(m.scales, np.float64), np.array(m.ratios, np.float64)
    _run(ctx, ("anchor_targets", cs["name"]), E.anchor_expected(i),
         lambda b: ctx.lib.radnet_anchor_targets(ctx.h, _ptr(gt), _ptr(bg), g, cs["width"], cs["height"], m.rw, m.rh, m.fw, m.fh, _host(sizes), len(m.scales),
                                                 _host(ratios), len(m.ratios), 16.0, 0.7, _ptr(b["valid"]), _ptr(b["overlap"]), _ptr(b["regr"]),
                                                 _ptr(b["best_anchor"]), _ptr(b["n_for_gt"]), _ptr(scratch)))
    ins, exp = E.anchor_pack_expected(i)
    valid, overlap, regr = _dev(ins["valid"]), _dev(ins["overlap"]), _dev(ins["regr"])
    _run(ctx, ("anchor_targets_pack", cs["name"]), exp,
         lambda b: ctx.lib.radnet_anchor_targets_pack(ctx.h, _ptr(valid), _ptr(overlap), _ptr(regr), m.fw, m.fh, len(m.scales) * len(m.ratios), E.STD_SCALING,
                                                      _ptr(b["y_cls"]), _ptr(b["y_regr"])))


# ---------------------------------------------------------------------------------------------------------------- RoI targets
ROI = E.roi_cases()


def _roi_call(ctx, cs, d, b, n_dev, max_overlap=0.5):
    Cc = E._roi_config()
    std = np.array(Cc.classifier_regr_std, np.float64)
    g = cs["g"]
    rw, rh = E.glue.new_img_size(E.ROI_W, E.ROI_H, Cc.img_size)
    return ctx.lib.radnet_roi_targets(ctx.h, _ptr(d["rois"]), cs["n"], _ptr(d["gt"]) if g else None, _ptr(d["gt_cls"]) if g else None, g, E.ROI_W, E.ROI_H, rw, rh,
                                      16.0, Cc.classifier_min_overlap, max_overlap, _host(std), Cc.class_mapping["bg"], _ptr(b["keep"]), _ptr(b["cls"]),
                                      _ptr(b["box"]), _ptr(b["t"]), _ptr(b["iou"]), _ptr(n_dev))


@pytest.mark.parametrize("i", range(len(ROI)), ids=[c["name"] for c in ROI])
def test_roi_targets(ctx, i):
    cs = ROI[i]
    d = {k: _dev(v) for k, v in E.roi_inputs(i).items()}
    n_dev = None if cs["n_dev"] is None else _dev(np.array([cs["n_dev"]], np.int32))
    bufs = _run(ctx, ("roi_targets", cs["name"]), E.roi_expected(i), lambda b: _roi_call(ctx, cs, d, b, n_dev))
    rows = E.roi_rows(i)
    if cs["n_dev"] is None and len(rows["kept"]):
        # the chain the trainer runs: every kept row packed from the device's own cls / box / t.  Labels bit for bit, the coordinates
        # (fp32 casts of targets that passed through the device's log) within the rtol tests/test_gpu_kernels.py states
        r, nreg = len(rows["kept"]), 24
        sel = _dev(rows["kept"].astype(np.int32))
        exp = dict(rois_out=E._out(E.F, (r, 4), rows["X"][0]), y1=E._out(E.F, (r, 7), rows["Y1"][0]),
                   y2=E._out(E.F, (r, 2 * nreg), rows["Y2"][0], loose=np.tile(np.arange(2 * nreg) >= nreg, (r, 1))))
        out = _fresh(exp)
        rc = _launch(("roi_batch_pack", cs["name"]), lambda: ctx.lib.radnet_roi_batch_pack(ctx.h, _ptr(sel), r, _ptr(bufs["cls"]), _ptr(bufs["box"]), _ptr(bufs["t"]), 7, 6,
                                                                                         _ptr(out["rois_out"]), _ptr(out["y1"]), _ptr(out["y2"])))
        ctx.check(rc, "roi_batch_pack")
        got = {k: out[k].cpu().numpy().view(E.F) for k in out}
        for k in ("rois_out", "y1"):
            assert not E.judge(k, got[k], exp[k]), (cs["name"], k)
        y2, ref = got["y2"], exp["y2"]
        coords = ref.loose & (ref.buf.view(np.uint32) != E.sentinel(E.F, 1).view(np.uint32)[0])
        assert np.array_equal(y2[~coords].view(np.uint32), ref.buf[~coords].view(np.uint32)), (cs["name"], "y2 labels, untouched rows or tail")
        assert np.allclose(y2[coords], ref.buf[coords], rtol=E.PACK_Y2_RTOL, atol=0), (cs["name"], "y2 coordinates")


@pytest.mark.parametrize("k", range(len(E.PACK_CASES)), ids=["r%d_nc%d" % c for c in E.PACK_CASES])
def test_roi_batch_pack(ctx, k):
    d = E.pack_inputs(k)
    sel, cls, box, t = _dev(d["sel"]), _dev(d["cls"]), _dev(d["box"]), _dev(d["t"])
    _run(ctx, ("roi_batch_pack", E.PACK_CASES[k]), E.pack_expected(k),
         lambda b: ctx.lib.radnet_roi_batch_pack(ctx.h, _ptr(sel), d["r"], _ptr(cls), _ptr(box), _ptr(t), d["nc"], d["bg"], _ptr(b["rois_out"]), _ptr(b["y1"]),
                                                 _ptr(b["y2"])))


def test_roi_batch_pack_of_an_empty_batch_writes_nothing(ctx):
    d = E.pack_inputs(1)
    sel, cls, box, t = _dev(d["sel"]), _dev(d["cls"]), _dev(d["box"]), _dev(d["t"])
    exp = E.pack_empty_expected(d["nc"])
    bufs = _fresh(exp)
    rc = _launch("roi_batch_pack r = 0", lambda: ctx.lib.radnet_roi_batch_pack(ctx.h, _ptr(sel), 0, _ptr(cls), _ptr(box), _ptr(t), d["nc"], d["bg"],
                                                                               _ptr(bufs["rois_out"]), _ptr(bufs["y1"]), _ptr(bufs["y2"])))
    assert rc == 0, (rc, ctx.lib.radnet_last_error(ctx.h))
    _judge("roi_batch_pack r = 0", bufs, exp)


# ---------------------------------------------------------------------------------------------------------------- refusals
def _refused(ctx, prefix, calls, outs):
    for what, call in calls:
        rc = call()
        msg = ctx.lib.radnet_last_error(ctx.h)
        assert rc < 0 and rc != ERR_HIP, (prefix, what, rc, msg)
        assert msg and msg.decode().startswith(prefix), (prefix, what, msg)
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == E.SBYTE).all()), (prefix, "a refused call wrote to an output")


def test_rpn_to_roi_refuses_and_writes_nothing(ctx):
    z = torch.zeros(1 << 16, device="cuda")
    outs = [torch.full((1 << 16,), E.SBYTE, dtype=torch.uint8, device="cuda") for _ in range(3)]
    ws = torch.full((int(ctx.lib.radnet_proposals_ws_bytes(3 * 5 * 33)),), E.SBYTE, dtype=torch.uint8, device="cuda")
    awh = np.ones((33, 2))
    for path in ("full_sort", "select"):
        calls = [(what, lambda rows=rows, cols=cols, a=a, ld=ld, mb=mb: _with_path(path, lambda: ctx.lib.radnet_rpn_to_roi(
            ctx.h, _ptr(z), ld, rows, cols, a, _host(awh), 4.0, 1, 0.7, mb, _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), _ptr(ws))))
            for what, rows, cols, a, ld, mb in E.RPN_REFUSED]
        _refused(ctx, "rpn_to_roi:", calls, outs + [ws])


def test_anchor_targets_refuses_and_writes_nothing(ctx):
    z = torch.zeros(1 << 14, dtype=torch.float64, device="cuda")
    zi = torch.zeros(1 << 14, dtype=torch.int32, device="cuda")
    outs = [torch.full((1 << 16,), E.SBYTE, dtype=torch.uint8, device="cuda") for _ in range(6)]
    sizes, ratios = np.full(17, 16.0), np.ones((17, 2))
    calls = [(what, lambda g=g, ns=ns, nr=nr: ctx.lib.radnet_anchor_targets(ctx.h, _ptr(z), _ptr(zi), g, 32, 32, 16, 16, 1, 1, _host(sizes), ns, _host(ratios), nr, 16.0,
                                                                            0.7, *[_ptr(o) for o in outs])) for what, g, ns, nr in E.ANCHOR_REFUSED]
    _refused(ctx, "anchor_targets:", calls, outs)


def test_roi_targets_refuses_a_max_overlap_that_is_not_positive(ctx):
    i = next(j for j, c in enumerate(ROI) if c["name"] == "n257_g40_ndev_null")
    cs = ROI[i]
    d = {k: _dev(v) for k, v in E.roi_inputs(i).items()}
    bufs = _fresh(E.roi_expected(i))
    calls = [("max_overlap = %r" % v, lambda v=v: _roi_call(ctx, cs, d, bufs, None, max_overlap=v)) for v in (0.0, -0.5)]
    _refused(ctx, "roi_targets:", calls, list(bufs.values()))
    test_roi_targets(ctx, i)                                                      # the context still works
