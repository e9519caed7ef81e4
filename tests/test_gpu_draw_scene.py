"""The scene painter on the device: radnet_draw_scene_u8 against the NumPy painter of tests/draw_scene_cases.py on the whole buffer
(pitch padding filled with sentinels that must stay), its opaque rectangles and text against radnet_draw_list_u8's bytes, its
refusals, radnet_grey3_u8 against the integer formula, RADNet.draw_scene_device, the figures of faster_rcnn/figures.py and
evaluate.evaluate_scans(pr_plot=True) end to end.  Every comparison is byte equality; every image is small."""
import os

import numpy as np
import pytest

import draw_list_cases as D
import draw_scene_cases as S
import png_write_cases as W

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import draw_gpu_helpers as G  # noqa: E402  (needs torch)
from draw_gpu_helpers import ERR_ARG, canvas  # noqa: E402


@pytest.fixture(scope="module")
def R():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    from faster_rcnn import RADNet
    return RADNet


@pytest.fixture(scope="module")
def ctx(R):
    from radnet_hip import runtime as rt
    return rt.default_context()


@pytest.fixture(scope="module")
def font(R):
    from radnet_hip import lib as L
    return {code: L.glyph_rows(code) for code in range(D.FIRST, D.LAST + 1)}


# ---- lines, discs, transparency, the lists that paint nothing ------------------------------------------------------------------------------
@pytest.mark.parametrize("size", S.SIZES, ids=["%dx%d" % s for s in S.SIZES])
def test_the_case_tables_against_the_painter(ctx, R, font, size):
    h, w = size
    nothing = S.nothing_lists(h, w)
    for pad in (0, 7):
        buf = canvas(h, w, pad, seed=h + pad)
        for name, prims in S.all_lists(h, w).items():
            got = G.check(ctx, R, G.SCENE, font, buf, h, w, pad, prims, name)
            if name in nothing:
                assert np.array_equal(got, buf), name
            elif size == S.SIZES[-1] and name != "tau 255":
                assert not np.array_equal(got, buf), name


def test_the_order_of_translucent_entries_shows(ctx, R, font):
    h, w = S.SIZES[-1]
    buf = canvas(h, w, 0)
    lists = S.translucent_lists(h, w)
    for name in ("three kinds overlapping", "opaque under translucent", "translucent under opaque", "tau 102"):
        forward = G.check(ctx, R, G.SCENE, font, buf, h, w, 0, lists[name], name)
        backward = G.check(ctx, R, G.SCENE, font, buf, h, w, 0, lists[name][::-1], name + ", reversed")
        assert not np.array_equal(forward, backward), name


@pytest.mark.parametrize("count", [255, 256, 257])
def test_lists_around_the_batch_boundaries(ctx, R, font, count):
    from radnet_hip import lib as L
    assert L.header_constant("RADNET_DRAW_RECT_BATCH") == 256
    h, w = 20, 45
    prims = S.batch_list(count, h, w)
    assert len(prims) == count and {p[0] for p in prims} == {"rect", "text", "line", "disc"}
    buf = canvas(h, w, 3, seed=count)
    G.check(ctx, R, G.SCENE, font, buf, h, w, 3, prims, "%d entries" % count)


# ---- opaque rectangles and text: the bytes of radnet_draw_list_u8 -----------------------------------------------------------------------------
def test_opaque_lists_give_the_bytes_of_draw_list(ctx, R, font):
    h, w = D.SIZES[-1]
    buf = canvas(h, w, 5, seed=4)
    lists = dict(D.text_lists(h, w))
    lists.update({"rects: " + k: [("rect",) + tuple(r) for r in v] for k, v in W.rect_lists(h, w).items()})
    lists["257 entries"] = D.batch_list(257, h, w)
    for name, prims in lists.items():
        rows, pool = D.pack(prims)
        rc, msg, want = G.prims_call(ctx, R, G.LIST.entry, buf, h, w, 3 * w + 5, rows, pool)
        assert rc == 0, (name, msg)
        rc, msg, got = G.prims_call(ctx, R, G.SCENE.entry, buf, h, w, 3 * w + 5, rows, pool)
        assert rc == 0, (name, msg)
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:4].tolist())
        assert np.array_equal(got, G.expected(S.paint_scene, buf, h, w, prims, font)), name


def test_the_three_fronts_agree_across_a_batch_boundary(ctx, R, font):
    """257 rectangles, one more than a batch, through radnet_draw_rects_u8, radnet_draw_list_u8 and radnet_draw_scene_u8: the same
    bytes, the painter's; then the 257-entry list with its text through the list and the scene.  The pairwise tests above use lists
    shorter than a batch or compare two fronts only; this pins the second staging of LDS in all three instantiations of the body."""
    h, w, pad = 20, 45, 3
    buf = canvas(h, w, pad, seed=257)
    full = D.batch_list(257, h, w)
    rects = [p for p in full if p[0] == "rect"]
    if len(rects) < 257:                                                                       # it has: half of that list is text
        rects = [p for p in D.batch_list(4 * 257, h, w) if p[0] == "rect"][:257]
    rects[255], rects[256] = ("rect", 4, 2, 36, 14, D.FILLED) + D.RED, ("rect", 20, 0, 24, 15, 1) + D.BLACK      # the boundary shows
    assert len(rects) == 257 and len(full) == 257 and any(p[0] == "text" for p in full)
    want = G.expected(D.paint_list, buf, h, w, rects, font)
    rc, msg, got = G.rects_call(ctx, R, buf, h, w, 3 * w + pad, [p[1:] for p in rects])
    assert rc == 0 and np.array_equal(got, want), (msg, np.argwhere(got != want)[:4].tolist())
    assert tuple(got[0, 3 * 20:3 * 20 + 3]) == D.BLACK and tuple(got[3, 3 * 5:3 * 5 + 3]) == D.RED      # entry 256 on entry 255
    for prims in (rects, full):
        want = G.expected(D.paint_list, buf, h, w, prims, font)
        for front in (G.LIST, G.SCENE):
            assert np.array_equal(G.check(ctx, R, front, font, buf, h, w, pad, prims, front.entry), want), front.entry


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_count_zero_and_refusals(ctx, R, font):
    h, w = 20, 30
    buf = canvas(h, w, 4)
    pitch = 3 * w + 4
    rows, pool, cases = S.refusals()
    rc, msg, got = G.prims_call(ctx, R, G.SCENE.entry, buf, h, w, pitch, rows, pool)
    assert rc == 0 and np.array_equal(got, G.expected(S.paint_scene, buf, h, w, S.GOOD, font)) and not np.array_equal(got, buf), msg
    rc, msg, got = G.prims_call(ctx, R, G.SCENE.entry, buf, h, w, pitch, [])
    assert rc == 0 and np.array_equal(got, buf)
    rc, msg, got = G.prims_call(ctx, R, G.SCENE.entry, buf, h, w, pitch, rows, pool, count=0, host=False, dev=False, chars_host=False, chars_dev=False)
    assert rc == 0 and np.array_equal(got, buf)
    for what, table, chars, entry in cases:
        rc, msg, got = G.prims_call(ctx, R, G.SCENE.entry, buf, h, w, pitch, table, chars)
        assert rc == ERR_ARG and ("entry %d " % entry) in msg, (what, msg)
        assert np.array_equal(got, buf), what                                                 # not even the entries in front of the bad one
    for what, prims in S.accepted():
        G.check(ctx, R, G.SCENE, font, buf, h, w, 4, prims, what)
    # what radnet_draw_list_u8 refuses and this entry means: bits 24..31 of the colour
    t = [list(r) for r in rows[:2]]
    t[0][7] |= 1 << 24
    assert G.prims_call(ctx, R, G.LIST.entry, buf, h, w, pitch, t, pool)[0] == ERR_ARG and G.prims_call(ctx, R, G.SCENE.entry, buf, h, w, pitch, t, pool)[0] == 0
    # and kind 2 stays unknown to the list
    assert G.prims_call(ctx, R, G.LIST.entry, buf, h, w, pitch, rows[:3], pool)[0] == ERR_ARG
    for what, kw in (("short pitch", dict(pitch=3 * w - 1)), ("negative count", dict(count=-1)), ("null host table", dict(host=False)),
                     ("null device table", dict(dev=False)), ("no context", dict(handle=False)), ("null host pool", dict(chars_host=False)),
                     ("null device pool", dict(chars_dev=False)), ("a negative pool length", dict(n_chars=-1))):
        p = kw.pop("pitch", pitch)
        rc, msg, got = G.prims_call(ctx, R, G.SCENE.entry, buf, h, w, p, rows, pool, **kw)
        assert rc == ERR_ARG and np.array_equal(got, buf), what
    for hh, ww in ((0, w), (h, 0), (-1, w)):
        rc, msg, got = G.prims_call(ctx, R, G.SCENE.entry, buf, hh, ww, pitch, rows, pool)
        assert rc == ERR_ARG and np.array_equal(got, buf)


# ---- radnet_grey3_u8 -------------------------------------------------------------------------------------------------------------------------
def grey_of(img):
    b, g, r = (img[:, :, k].astype(np.int64) for k in range(3))
    return np.repeat(((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)[:, :, None], 3, axis=2)


@pytest.mark.parametrize("size", [(1, 1), (9, 33), (67, 342), (3, 300)], ids=lambda s: "%dx%d" % s)
def test_grey3_against_the_integer_formula(ctx, R, size):
    h, w = size
    for src_pad, dst_pad in ((0, 0), (5, 2), (0, 9)):
        src, dst = canvas(h, w, src_pad, seed=w), canvas(h, w, dst_pad, seed=w + 1)
        src_dev, dst_dev = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
        ctx.call("radnet_grey3_u8", src_dev, dst_dev, h, w, 3 * w + src_pad, 3 * w + dst_pad)
        ctx.sync()
        want = dst.copy()
        want[:, :3 * w] = grey_of(src[:, :3 * w].reshape(h, w, 3)).reshape(h, 3 * w)
        assert np.array_equal(dst_dev.cpu().numpy(), want) and np.array_equal(src_dev.cpu().numpy(), src), (src_pad, dst_pad)
        ctx.call("radnet_grey3_u8", src_dev, src_dev, h, w, 3 * w + src_pad, 3 * w + src_pad)      # in place
        ctx.sync()
        want = src.copy()
        want[:, :3 * w] = grey_of(src[:, :3 * w].reshape(h, w, 3)).reshape(h, 3 * w)
        assert np.array_equal(src_dev.cpu().numpy(), want), (src_pad, "in place")


def test_grey3_extremes_and_refusals(ctx, R):
    img = np.array([[[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255], [1, 1, 1], [254, 255, 254]]], np.uint8)
    got = R.grey3_device(torch.from_numpy(img).cuda()).cpu().numpy()
    assert np.array_equal(got, grey_of(img)) and got[0, :, 0].tolist() == [255, 0, 29, 150, 76, 1, 255]
    dev = torch.from_numpy(canvas(4, 6, 2)).cuda()
    before = dev.cpu().numpy()
    for args in ((None, dev, 4, 6, 20, 20), (dev, None, 4, 6, 20, 20), (dev, dev, 0, 6, 20, 20), (dev, dev, 4, 0, 20, 20), (dev, dev, 4, 6, 17, 20),
                 (dev, dev, 4, 6, 20, 17)):
        assert ctx.lib.radnet_grey3_u8(ctx.h, args[0].data_ptr() if args[0] is not None else None, args[1].data_ptr() if args[1] is not None else None,
                                       *args[2:]) == ERR_ARG, args[2:]
    assert ctx.lib.radnet_grey3_u8(None, dev.data_ptr(), dev.data_ptr(), 4, 6, 20, 20) == ERR_ARG
    ctx.sync()
    assert np.array_equal(dev.cpu().numpy(), before)


# ---- draw_scene_device and the figures -----------------------------------------------------------------------------------------------------
def test_draw_scene_device(R, font):
    img = np.random.RandomState(6).randint(0, 256, (40, 70, 3)).astype(np.uint8)
    dev = torch.from_numpy(img).cuda()
    prims = [("rect", 3, 3, 60, 30, 2, 1, 2, 3), ("text", 5, 20, "Hello, g", 2, 250, 251, 252, {"transparency": 77}), ("line", 0, 39, 69, 0, 3, 7, 8, 9, {"dash": (3, 2)}),
             ("disc", 30, 20, 9, -1, 0, 200, 0, {"transparency": 128}), ("disc", 30, 20, 12, 2, 0, 0, 0), ("line", 2, 2, 2, 30, 1, 255, 255, 255)]
    want = S.paint_scene(img.copy(), prims, font)
    out = R.draw_scene_device(dev, prims)
    assert out.is_cuda and out.data_ptr() != dev.data_ptr() and torch.equal(dev.cpu(), torch.from_numpy(img))      # inplace=False: the input stays
    assert np.array_equal(out.cpu().numpy(), want)
    assert torch.equal(R.draw_scene_device(dev, []), dev)
    from_host = R.draw_scene_device(img, prims)                                                # a NumPy image is uploaded, the array stays
    assert from_host.is_cuda and np.array_equal(from_host.cpu().numpy(), want) and not np.array_equal(img, want)
    same = R.draw_scene_device(dev, prims, inplace=True)
    assert same.data_ptr() == dev.data_ptr() and np.array_equal(dev.cpu().numpy(), want)
    from radnet_hip import lib as L
    with pytest.raises(L.RadnetError, match="entry 1 "):
        R.draw_scene_device(dev, [prims[0], ("line", 0, 0, 1, 1, 0, 0, 0, 0)])
    assert np.array_equal(dev.cpu().numpy(), want)


def golden_curves():
    import json
    from faster_rcnn import evaluate
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "voc_ap.json")) as f:
        o = json.load(f)["objects"][0]
    return {key: evaluate.calc_class_ap(o["T"][key], o["P"][key]) for key in o["T"]}


def test_precision_recall_figure(R, font):
    from faster_rcnn import figures
    curves = golden_curves()
    got = figures.precision_recall_figure(curves, 0.4321, size=300)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (300, 300, 3)
    prims = figures.precision_recall_scene(curves, 0.4321, 300)
    want = S.paint_scene(np.full((300, 300, 3), 255, np.uint8), prims, font)
    assert np.array_equal(got.cpu().numpy(), want), np.argwhere(got.cpu().numpy() != want)[:4].tolist()
    assert (want != 255).any() and len({tuple(c) for c in want.reshape(-1, 3)[::7]}) > 6      # ink in several colours


def test_the_label_views(R, font):
    from faster_rcnn import figures

    class C:
        anchor_box_scales, anchor_box_ratios, rpn_stride = [8, 16], [[1, 1], [1, 2], [2, 1]], 16
    img = np.random.RandomState(9).randint(0, 256, (60, 90, 3)).astype(np.uint8)
    dev = torch.from_numpy(img).cuda()
    regr = np.zeros((1, 4, 6, 48))
    regr[0, 1, 2, 16:20] = 1
    regr[0, 3, 5, 0:4] = 1
    regr[0, 0, 0, 20:24] = 1
    Y = [None, regr]
    view = figures.positive_anchor_view(dev, Y, C, 3)
    want = S.paint_scene(grey_of(img), figures.positive_anchor_scene(Y, C, 3), font)
    assert view.data_ptr() != dev.data_ptr() and torch.equal(dev.cpu(), torch.from_numpy(img)) and np.array_equal(view.cpu().numpy(), want)
    assert not np.array_equal(want, grey_of(img)) and np.array_equal(figures.positive_anchor_view(img, Y, C, 3).cpu().numpy(), want)
    boxes = [{'x1': 5, 'y1': 6, 'x2': 50, 'y2': 40}, {'x1': 30, 'y1': 20, 'x2': 95, 'y2': 55}]
    view = figures.ground_truth_view(dev, boxes)
    want = S.paint_scene(img.copy(), figures.ground_truth_scene(boxes), font)
    assert torch.equal(dev.cpu(), torch.from_numpy(img)) and np.array_equal(view.cpu().numpy(), want) and not np.array_equal(want, img)
    # the reference's own arithmetic in float64 -- 0.6 * colour + 0.4 * pixel, applied once per box -- differs by at most one level
    ref = img.astype(np.float64)
    for b in boxes:
        mask = S.rect_mask(60, 90, b['x1'], b['y1'], b['x2'], b['y2'], 3)
        ref[mask] = np.rint(0.6 * np.array([28, 26, 227]) + 0.4 * ref[mask])
    assert np.abs(ref - want).max() <= 1


# ---- evaluate_scans(pr_plot=True) -----------------------------------------------------------------------------------------------------------
class _Config:
    class_mapping = {"boat": 0, "human": 1, "animal": 2, "bg": 3}


def test_evaluate_scans_writes_the_figure(R, font, tmp_path, monkeypatch):
    from faster_rcnn import evaluate, figures, png, utils_io
    monkeypatch.chdir(tmp_path)
    os.makedirs("scans/blended_grey")
    maps = {"scans/panel_a.png": np.random.RandomState(3).randint(0, 256, (96, 128, 3)).astype(np.uint8),
            "scans/panel_b.png": np.random.RandomState(4).randint(0, 256, (100, 140, 3)).astype(np.uint8)}
    for path, img in maps.items():
        utils_io.imwrite(path.replace("scans/", "scans/blended_grey/"), img)
    dets = {"scans/panel_a.png": D.DETS[:2], "scans/panel_b.png": D.DETS[2:]}
    gt = {"scans/panel_a.png": [{'class': 'boat', 'x1': 10, 'y1': 20, 'x2': 70, 'y2': 61}], "scans/panel_b.png": [{'class': 'wheel', 'x1': 0, 'y1': 70, 'x2': 30, 'y2': 99}]}
    data_test = [{'filepath': path, 'bboxes': [dict(g) for g in gt[path]]} for path in maps]
    net = R.RADNet(_Config(), None, None, None)
    monkeypatch.setattr(net, "predict_from_path", lambda path: [dict(d) for d in dets[path]])
    accuracy, elapsed, paths = evaluate.evaluate_scans(net, data_test, "model", pr_plot=True)
    plain_accuracy, _, plain_paths = evaluate.evaluate_scans(net, [dict(r, bboxes=[dict(g) for g in gt[r['filepath']]]) for r in data_test], "plain")
    assert paths == [os.path.join("model", "test", "panel_a.png"), os.path.join("model", "test", "panel_b.png"), os.path.join("model", "viz", "precision_recall.png")]
    assert accuracy == plain_accuracy and not os.path.exists(os.path.join("plain", "viz"))
    for a, b in zip(paths, plain_paths):                                                          # the maps: the same bytes with and without the plot
        assert open(a, "rb").read() == open(b, "rb").read()
    assert open(os.path.join("model", "test_accuracy.json")).read() == open(os.path.join("plain", "test_accuracy.json")).read()
    curves, again = evaluate.class_curves([dict(d) for p in maps for d in dets[p]], [dict(g) for p in maps for g in gt[p]])
    assert {k: float(v) for k, v in again.items()} == accuracy and list(curves) == ["animal", "boat", "human", "wheel"]
    want = S.paint_scene(np.full((1200, 1200, 3), 255, np.uint8), figures.precision_recall_scene(curves, again["mAP"]), font)
    data = open(paths[-1], "rb").read()
    assert np.array_equal(png.decode_device(data).cpu().numpy(), want)
    assert (want != 255).any()
