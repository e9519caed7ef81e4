"""Score maps as pictures on the device: radnet_score_levels_u8 and radnet_heat_paint_u8 against the NumPy model of
tests/heat_cases.py, byte for byte over the whole buffer (the pitch padding and the bytes behind the last level hold sentinels that
must stay); their refusals; and end to end with the models of tests/test_gpu_predict_device_image.py: RADNet.objectness_maps,
figures.objectness_view, RADNet.predict_region_proposals, and predict before and after them.  Every image is small."""
import copy

import numpy as np
import pytest

import heat_cases as H

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import draw_gpu_helpers as G  # noqa: E402  (needs torch)
from draw_gpu_helpers import ERR_ARG  # noqa: E402

SENTINEL = H.SENTINEL


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


# ---- radnet_score_levels_u8 ------------------------------------------------------------------------------------------------------------------
def levels_call(ctx, pred, ld, M, first, count, rows=None, handle=True, src=True, dst=True):
    """(rc, message, the level buffer afterwards: max(M, 1) levels and 16 sentinel bytes behind them, the scores afterwards)."""
    pred_dev = torch.from_numpy(np.ascontiguousarray(pred, np.float32)).cuda()
    out_dev = torch.full((max(rows if rows is not None else M, 1) + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    rc = ctx.lib.radnet_score_levels_u8(ctx.h if handle else None, pred_dev.data_ptr() if src else None, ld, M, first, count, out_dev.data_ptr() if dst else None)
    msg = ctx.lib.radnet_last_error(ctx.h)
    ctx.sync()
    return rc, (msg.decode() if msg else ""), out_dev.cpu().numpy(), pred_dev.cpu().numpy()


@pytest.mark.parametrize("M", H.LEVEL_MS)
def test_levels_against_the_model(ctx, M):
    for m, first, count, outside in H.level_cases():
        if m != M:
            continue
        pred = H.level_case(M, first, count, np.inf if outside == "inf" else np.nan)
        rc, msg, got, after = levels_call(ctx, pred, H.LEVEL_LD, M, first, count)
        assert rc == 0, msg
        want = np.concatenate([H.levels(pred, H.LEVEL_LD, M, first, count), np.full(16, SENTINEL, np.uint8)])
        assert np.array_equal(got, want), (M, first, count, outside, np.argwhere(got != want)[:4].tolist())
        assert np.array_equal(after.view(np.uint32), pred.view(np.uint32))                 # the scores are only read


def test_levels_of_a_short_last_row(ctx):
    """ld = first + count and a buffer that ends with the last row's last column: nothing behind it is there to be read."""
    pred = H.level_case(65, 6, 3, np.inf)[:, :9].copy()
    rc, msg, got, _ = levels_call(ctx, pred, 9, 65, 6, 3)
    assert rc == 0 and np.array_equal(got[:65], H.levels(pred, 9, 65, 6, 3)) and (got[65:] == SENTINEL).all()


def test_levels_refusals(ctx):
    pred = H.level_case(64, 0, 12, np.inf)
    for what, kw in (("ld below first + count", dict(ld=11)), ("count 0", dict(count=0)), ("a negative count", dict(count=-1)), ("a negative first", dict(first=-1)),
                     ("M 0", dict(M=0)), ("a negative M", dict(M=-5)), ("first + count past int32", dict(first=2 ** 31 - 1, count=2)),
                     ("null scores", dict(src=False)), ("null levels", dict(dst=False))):
        a = dict(ld=64, M=64, first=0, count=12)
        flags = {k: kw.pop(k) for k in ("src", "dst") if k in kw}
        a.update(kw)
        rc, msg, got, _ = levels_call(ctx, pred, a["ld"], a["M"], a["first"], a["count"], rows=64, **flags)
        assert rc == ERR_ARG and "score_levels" in msg, (what, msg)
        assert (got == SENTINEL).all(), what
    assert levels_call(ctx, pred, 64, 64, 0, 12, handle=False)[0] == ERR_ARG


# ---- radnet_heat_paint_u8 -------------------------------------------------------------------------------------------------------------------
def paint_call(ctx, R, buf, h, w, pitch, pool, places, lut, tau, min_level, count=None, pool_len=None, handle=True, img=True, pool_ptr=True, host=True, dev=True,
               lut_ptr=True):
    """radnet_heat_paint_u8 on a copy of the host buffer `buf` (h rows of `pitch` bytes): (rc, message, the buffer afterwards)."""
    pool_dev = torch.from_numpy(np.ascontiguousarray(pool, np.uint8)).cuda()
    lut_dev = torch.from_numpy(np.ascontiguousarray(lut, np.uint8).reshape(-1)).cuda()
    return G.raw_call(ctx, "radnet_heat_paint_u8", buf, h, w, pitch, R.heat_table(places),
                      before=(pool_dev.data_ptr() if pool_ptr else None, len(pool) if pool_len is None else pool_len),
                      after=(lut_dev.data_ptr() if lut_ptr else None, tau, min_level), count=count, handle=handle, img=img, host=host, dev=dev)


@pytest.fixture(scope="module")
def tables():
    t, pool = H.paint_tables()
    return t, pool, H.luts()


@pytest.mark.parametrize("size", H.SIZES, ids=["%dx%d" % s for s in H.SIZES])
def test_the_paint_cases_against_the_model(ctx, R, tables, size):
    from radnet_hip import lib as L
    assert L.header_constant("RADNET_DRAW_RECT_BATCH") == 256 and len(tables[0]["257: two batches"]) == 257
    t, pool, luts = tables
    h, w = size
    buf = H.canvas(h, w, seed=h)
    ran = 0
    for sz, name, tau, min_level, lut in H.paint_cases():
        if sz != size:
            continue
        rc, msg, got = paint_call(ctx, R, buf, h, w, H.PITCH, pool, t[name], luts[lut], tau, min_level)
        assert rc == 0, (name, msg)
        want = H.expected(buf, h, w, pool, t[name], luts[lut], tau, min_level)
        assert np.array_equal(got, want), (name, tau, min_level, lut, np.argwhere(got != want)[:4].tolist())
        ran += 1
    assert ran == len(t) * (24 if size == H.SIZES[0] else 3)


def test_paint_refusals_leave_the_image_untouched(ctx, R, tables):
    t, pool, luts = tables
    h, w = H.SIZES[0]
    buf = H.canvas(h, w, seed=3)
    lut = luts["random"]
    good, _, cases = H.refused_tables()
    places = t["two: 5x4 and 1x1"]
    rc, msg, got = paint_call(ctx, R, buf, h, w, H.PITCH, pool, places, lut, 0, 0)
    assert rc == 0 and not np.array_equal(got, buf), msg
    # count 0 is a no-op whatever the pointers
    rc, msg, got = paint_call(ctx, R, buf, h, w, H.PITCH, pool, places, lut, 0, 0, count=0, img=False, pool_ptr=False, host=False, dev=False, lut_ptr=False)
    assert rc == 0 and np.array_equal(got, buf)
    # the tables the host check refuses (tests/test_heat_host.py): refused through the launch wrapper too, before anything is launched
    for what, bad_places, pool_len, hh, ww, entry, field in cases:
        rc, msg, got = paint_call(ctx, R, buf, h, w, H.PITCH, pool, bad_places, lut, 0, 0, pool_len=pool_len)
        assert rc == ERR_ARG and ("entry %d " % entry) in msg and (" %s = " % field) in msg, (what, msg)
        assert np.array_equal(got, buf), what                                               # not even the entries in front of the bad one
    for what, kw in (("a short pitch", dict(pitch=3 * w - 1)), ("a negative count", dict(count=-1)), ("a null image", dict(img=False)),
                     ("a null pool", dict(pool_ptr=False)), ("a null host table", dict(host=False)), ("a null device table", dict(dev=False)),
                     ("a null colour table", dict(lut_ptr=False)), ("no context", dict(handle=False)), ("a negative pool length", dict(pool_len=-1)),
                     ("a pool shorter than its maps", dict(pool_len=24)), ("tau -1", dict(tau=-1)), ("tau 256", dict(tau=256)),
                     ("min_level -1", dict(min_level=-1)), ("min_level 256", dict(min_level=256))):
        pitch, tau, min_level = kw.pop("pitch", H.PITCH), kw.pop("tau", 0), kw.pop("min_level", 0)
        rc, msg, got = paint_call(ctx, R, buf, h, w, pitch, pool, places, lut, tau, min_level, **kw)
        assert rc == ERR_ARG and np.array_equal(got, buf), (what, msg)
    for hh, ww in ((0, w), (h, 0), (-1, w)):
        rc, msg, got = paint_call(ctx, R, buf, hh, ww, H.PITCH, pool, places, lut, 0, 0)
        assert rc == ERR_ARG and np.array_equal(got, buf)


def test_heat_paint_device(R, tables):
    t, pool, luts = tables
    h, w = 21, 37
    img = np.random.RandomState(6).randint(0, 256, (h, w, 3)).astype(np.uint8)
    dev = torch.from_numpy(img).cuda()
    places = t["two overlapping, shifted"]
    want = H.paint(img.copy(), pool, places, luts["random"], 77, 2)
    out = R.heat_paint_device(dev, pool, places, lut=luts["random"], transparency=77, min_level=2)
    assert out.is_cuda and out.data_ptr() != dev.data_ptr() and torch.equal(dev.cpu(), torch.from_numpy(img))      # inplace=False: the input stays
    assert np.array_equal(out.cpu().numpy(), want) and not np.array_equal(want, img)
    assert torch.equal(R.heat_paint_device(dev, pool, []), dev)
    pool_dev = torch.from_numpy(pool).cuda()
    from_host = R.heat_paint_device(img, pool_dev, places, lut=luts["random"], transparency=77, min_level=2)      # a NumPy image is uploaded
    assert from_host.is_cuda and np.array_equal(from_host.cpu().numpy(), want) and not np.array_equal(img, want)
    from faster_rcnn import figures
    default = R.heat_paint_device(dev, bytes(pool), places)                                  # the default table, opaque, every level
    assert np.array_equal(default.cpu().numpy(), H.paint(img.copy(), pool, places, figures.heat_lut(), 0, 0))
    same = R.heat_paint_device(dev, pool_dev, places, lut=luts["random"], transparency=77, min_level=2, inplace=True)
    assert same.data_ptr() == dev.data_ptr() and np.array_equal(dev.cpu().numpy(), want)
    from radnet_hip import lib as L
    with pytest.raises(L.RadnetError, match="entry 1 .* mw = "):
        R.heat_paint_device(dev, pool_dev, [places[0], (0, 0, 4, 4, 0, 1, 0)])
    for kw in (dict(transparency=256), dict(min_level=-1), dict(lut=luts["random"][:255])):
        with pytest.raises(ValueError):
            R.heat_paint_device(dev, pool_dev, places, **kw)
    assert np.array_equal(dev.cpu().numpy(), want)


def test_score_map_figure(R):
    import draw_list_cases as D
    import draw_scene_cases as S
    from faster_rcnn import figures
    from radnet_hip import lib as L
    font = {code: L.glyph_rows(code) for code in range(D.FIRST, D.LAST + 1)}
    values = np.random.RandomState(8).random_sample((19, 25)).astype(np.float32)
    values[3, 4], values[0, 0] = np.nan, 2.0
    got = figures.score_map_figure(values, "7", size=300)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (300, 300, 3)
    scene = figures.score_map_scene((19, 25), "7", 300)
    pool = np.concatenate([figures.to_levels(values).reshape(-1), np.arange(255, -1, -1).astype(np.uint8)])
    want = np.full((300, 300, 3), 255, np.uint8)
    H.paint(want, pool, [scene["map"] + (25, 19, 0), scene["bar"] + (1, 256, 19 * 25)], figures.heat_lut(), 0, 0)
    x0, y0, w, h = scene["map"]
    assert tuple(want[y0, x0]) == tuple(figures.heat_lut()[255]) and tuple(want[y0, scene["bar"][0]]) == tuple(figures.heat_lut()[255])      # 2.0, and the bar's top
    S.paint_scene(want, scene["prims"], font)
    assert np.array_equal(got.cpu().numpy(), want), np.argwhere(got.cpu().numpy() != want)[:4].tolist()
    assert np.array_equal(figures.score_map_figure(torch.from_numpy(values).cuda(), "7", size=300).cpu().numpy(), want)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def _models():
    """As tests/test_gpu_predict_device_image.py:_models."""
    from faster_rcnn import models as M
    from faster_rcnn.base_models import resnet50 as base
    from faster_rcnn.config import Config
    from faster_rcnn.RADNet import RADNet
    from oracle import dense
    Cc = Config()
    Cc.img_size = 300
    ms = M.build_models(Cc, weights=copy.deepcopy(dense.init_params(seed=3)), workload="predict")
    return Cc, ms, RADNet(Cc, ms[3], ms[4], base.preprocess)


@pytest.fixture(scope="module")
def setup(R):
    Cc, ms, rnet = _models()
    Cc.tile_size, Cc.tile_overlap = 400, 250           # 700 x 900: 3 x 3 tiles, last row and column clipped to the far edge
    assert Cc.max_n_tiles_train > 0
    Cc.include_full_img = True
    rnet.bbox_threshold = 0.0
    img = np.random.RandomState(41).randint(0, 256, (700, 900, 3)).astype(np.uint8)
    before = rnet.predict([img])                        # computed first; compared with predict after everything else (the last test)
    assert len(before) > 0
    windows = [(x0, y0, 400, 400) for y0 in (0, 250, 300) for x0 in (0, 250, 500)] + [(0, 0, 900, 700)]
    scores = []                                         # the reference: the NumPy-facing RPN on every window, computed once
    for (x0, y0, ww, wh) in windows:
        X, ratio = rnet.format_img(np.copy(img[y0:y0 + wh, x0:x0 + ww, :]))
        scores.append(ms[3].predict(X)[0][0].copy())    # [fh][fw][A]
    return Cc, ms, rnet, img, before, windows, scores


@pytest.mark.parametrize("full", [True, False])
def test_objectness_maps_are_the_levels_of_the_rpn_scores(setup, R, full):
    from faster_rcnn import figures
    Cc, ms, rnet, img, before, windows, scores = setup
    Cc.include_full_img = full
    n = 10 if full else 9
    maps = rnet.objectness_maps(img)
    assert isinstance(maps, R.ScoreMaps) and maps.shape == (700, 900) and maps.pool.is_cuda and maps.pool.dtype == torch.uint8
    assert [p[:4] for p in maps.places] == windows[:n]
    host = maps.to_host()
    assert len(host) == n
    offset = 0
    for place, got, Y in zip(maps.places, host, scores):
        fh, fw, A = Y.shape
        assert place[4:] == (fw, fh, offset) and got.shape == (fh, fw) and got.dtype == np.uint8
        assert np.array_equal(got, figures.to_levels(Y.max(axis=2))), np.argwhere(got != figures.to_levels(Y.max(axis=2)))[:4].tolist()
        offset += fh * fw
    assert maps.pool.numel() == offset and len({int(v) for m in host for v in np.unique(m)}) > 4      # not one flat level
    # the same bytes as a device image: the same pool
    again = rnet.objectness_maps(torch.from_numpy(img).cuda())
    assert again.places == maps.places and torch.equal(again.pool, maps.pool)
    # a range of anchors
    some = rnet.objectness_maps(img, anchors=(6, 3)).to_host()
    for got, Y in zip(some, scores):
        assert np.array_equal(got, figures.to_levels(Y[:, :, 6:9].max(axis=2)))
    Cc.include_full_img = True


def test_objectness_maps_refusals(setup, R):
    Cc, ms, rnet, img, before, windows, scores = setup

    class Fake:
        def predict(self, X):
            raise AssertionError("a duck-typed model was run")
    duck = R.RADNet(Cc, Fake(), Fake(), None)
    for call in (duck.objectness_maps, duck.predict_region_proposals):
        with pytest.raises(TypeError, match="engine-backed"):
            call(img)
    for anchors in ((-1, 2), (0, 0), (10, 3), (0, 13)):
        with pytest.raises(ValueError, match="anchors"):
            rnet.objectness_maps(img, anchors=anchors)
    with pytest.raises((TypeError, ValueError)):
        rnet.objectness_maps(torch.from_numpy(img).cuda().float())
    with pytest.raises(ValueError):
        rnet.objectness_maps(img[:, :, 0])


def test_objectness_view(setup, R, tmp_path):
    from faster_rcnn import figures, png, utils_io
    Cc, ms, rnet, img, before, windows, scores = setup
    Cc.include_full_img = True
    dev = torch.from_numpy(img).cuda()
    maps = rnet.objectness_maps(dev)
    grey = R.grey3_device(dev).cpu().numpy()
    pool = maps.pool.cpu().numpy()
    top = int(pool.max())                               # a min_level that leaves the best cells only
    assert top > 0
    for kw, args in ((dict(), (figures.heat_lut(), 102, 0)), (dict(transparency=0, min_level=top, lut=H.luts()["random"]), (H.luts()["random"], 0, top))):
        view = figures.objectness_view(dev, maps, **kw)
        want = H.paint(grey.copy(), pool, maps.places, *args)
        assert view.is_cuda and view.data_ptr() != dev.data_ptr() and torch.equal(dev.cpu(), torch.from_numpy(img))
        assert np.array_equal(view.cpu().numpy(), want) and not np.array_equal(want, grey)
    colour = figures.objectness_view(dev, maps, grey=False)
    assert np.array_equal(colour.cpu().numpy(), H.paint(img.copy(), pool, maps.places, figures.heat_lut(), 102, 0)) and torch.equal(dev.cpu(), torch.from_numpy(img))
    path = str(tmp_path / "objectness.png")
    utils_io.imwrite(path, view)                        # the last view of the loop
    with open(path, "rb") as f:
        assert np.array_equal(png.decode_device(f.read()).cpu().numpy(), want)
    with pytest.raises(ValueError, match="scan"):
        figures.objectness_view(dev[:100], maps)


@pytest.mark.parametrize("full", [True, False])
def test_predict_region_proposals(setup, R, full):
    Cc, ms, rnet, img, before, windows, scores = setup
    Cc.include_full_img = full
    got = rnet.predict_region_proposals(img, gt_bboxes=[{'class': 'boat', 'x1': 1, 'y1': 2, 'x2': 30, 'y2': 40}])
    want = []
    for (x0, y0, ww, wh) in windows[:10 if full else 9]:
        tile = np.copy(img[y0:y0 + wh, x0:x0 + ww, :])
        img_dev, ratio = rnet.format_img_size(tile, keep_on_device=True)
        boxes, _ = ms[3].propose_device(img_dev, overlap_thresh=0.7)
        assert boxes.dtype == np.int64 and 0 < len(boxes) <= 300
        for (x1, y1, x2, y2) in boxes * Cc.rpn_stride:
            rx1, ry1, rx2, ry2 = rnet.get_real_coordinates(ratio, x1, y1, x2, y2)
            want.append((x0 + rx1, y0 + ry1, x0 + rx2, y0 + ry2))
    assert len(got) == len(want) > 0
    for d, box in zip(got, want):
        assert list(d) == ['class', 'prob', 'x1', 'y1', 'x2', 'y2'] and d['class'] == 'object'
        assert type(d['prob']) is np.float32 and 0.0 <= d['prob'] <= 1.0
        assert all(type(d[k]) is np.int64 for k in ('x1', 'y1', 'x2', 'y2'))
        assert (d['x1'], d['y1'], d['x2'], d['y2']) == box
    assert got == rnet.predict_region_proposals(torch.from_numpy(img).cuda())               # a device image, and no gt_bboxes
    Cc.include_full_img = True


def test_predict_is_what_it_was_before_these_calls(setup, R):
    """Runs last in this module: objectness_maps, objectness_view and predict_region_proposals have all run on the shared engine."""
    Cc, ms, rnet, img, before, windows, scores = setup
    Cc.include_full_img = True
    rnet.objectness_maps(img)
    rnet.predict_region_proposals(img)
    after = rnet.predict([img])
    assert len(after) == len(before)
    for x, y in zip(after, before):
        assert list(x) == list(y)
        for key in x:
            assert type(x[key]) is type(y[key]) and np.array_equal(x[key], y[key]), (key, x[key], y[key])
