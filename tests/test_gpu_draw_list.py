"""The ordered draw list on the device: radnet_draw_list_u8 against the NumPy painter of tests/draw_list_cases.py on the whole
buffer (pitch padding filled with sentinels that must stay), its rectangles against radnet_draw_rects_u8's bytes, its refusals,
RADNet.draw_detections / write_predictions with labels=True and evaluate.evaluate_scans end to end.  Every comparison is byte
equality; every image is small."""
import json
import os

import numpy as np
import pytest

import draw_list_cases as D
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


# ---- text --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", D.SIZES, ids=["%dx%d" % s for s in D.SIZES])
def test_text_against_the_painter(ctx, R, font, size):
    h, w = size
    for pad in (0, 7):
        buf = canvas(h, w, pad, seed=h + pad)
        for name, prims in D.text_lists(h, w).items():
            got = G.check(ctx, R, G.LIST, font, buf, h, w, pad, prims, name)
            if name in D.NOTHING:
                assert np.array_equal(got, buf), name
            elif size == D.SIZES[-1]:
                assert not np.array_equal(got, buf), name


def test_every_code_once(ctx, R, font):
    h, w = 16, 600
    buf = canvas(h, w, 5, seed=3)
    got = G.check(ctx, R, G.LIST, font, buf, h, w, 5, [("text", 7, 11, D.ALL_CODES, 1) + D.WHITE], "all 95 codes")
    img = got[:, :3 * w].reshape(h, w, 3)
    for k, code in enumerate(D.ALL_CODES):                                                     # glyph by glyph, straight from the table
        cell = (img[4:12, 7 + 6 * k:7 + 6 * k + 6] == 255).all(axis=2)
        want = np.array([[(font[code][r] >> (4 - c)) & 1 if c < 5 else 0 for c in range(6)] for r in range(8)], bool)
        noise = (buf[:, :3 * w].reshape(h, w, 3)[4:12, 7 + 6 * k:7 + 6 * k + 6] == 255).all(axis=2)
        assert np.array_equal(cell, want | noise), chr(code)


def test_a_pool_longer_than_one_batch(ctx, R, font):
    """Runs anywhere in a pool of 700 bytes: at offset 0, at the pool's last byte, across byte 256, and the whole pool as one run."""
    h, w = 30, 90
    pool = D.printable(700, 11)
    runs = [(0, 9, 2, 9, 1, D.WHITE), (699, 1, 80, 9, 1, D.RED), (250, 12, 3, 19, 1, D.BLUE), (0, 700, -4000, 29, 1, D.RED), (690, 10, 10, 27, 1, D.WHITE)]
    rows = [(D.PRIM_TEXT, x, y, s, 0, a, n, c[0] | c[1] << 8 | c[2] << 16) for a, n, x, y, s, c in runs]
    prims = [("text", x, y, pool[a:a + n], s) + c for a, n, x, y, s, c in runs]
    buf = canvas(h, w, 2, seed=8)
    rc, msg, got = G.prims_call(ctx, R, G.LIST.entry, buf, h, w, 3 * w + 2, rows, pool)
    assert rc == 0, msg
    want = G.expected(D.paint_list, buf, h, w, prims, font)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()
    assert not np.array_equal(got, buf)


# ---- order -------------------------------------------------------------------------------------------------------------------------------
def test_the_later_entry_wins(ctx, R, font):
    h, w = D.SIZES[-1]
    lists = D.text_lists(h, w)
    buf = canvas(h, w, 0)
    for name in ("text over a filled rectangle", "a filled rectangle over text", "overlapping runs", "outline over text over fill"):
        forward = G.check(ctx, R, G.LIST, font, buf, h, w, 0, lists[name], name)
        backward = G.check(ctx, R, G.LIST, font, buf, h, w, 0, lists[name][::-1], name + ", reversed")
        assert not np.array_equal(forward, backward), name


@pytest.mark.parametrize("count", [255, 256, 257, 513])
def test_lists_around_the_batch_boundaries(ctx, R, font, count):
    from radnet_hip import lib as L
    assert L.header_constant("RADNET_DRAW_RECT_BATCH") == 256
    h, w = 20, 45
    prims = D.batch_list(count, h, w)
    assert len(prims) == count
    buf = canvas(h, w, 3, seed=count)
    G.check(ctx, R, G.LIST, font, buf, h, w, 3, prims, "%d entries" % count)


# ---- rectangles ----------------------------------------------------------------------------------------------------------------------------
def test_rectangles_give_the_bytes_of_draw_rects(ctx, R, font):
    h, w = 70, 130
    buf = canvas(h, w, 7, seed=4)
    for name, rects in W.rect_lists(h, w).items():
        table = np.array([tuple(r) for r in rects], R.RECT).reshape(-1)
        img_dev, table_dev = torch.from_numpy(buf.copy()).cuda(), torch.from_numpy(table.view(np.uint8).copy()).cuda()
        ctx.call("radnet_draw_rects_u8", img_dev, h, w, 3 * w + 7, table.ctypes.data, table_dev, len(table))
        ctx.sync()
        got = G.check(ctx, R, G.LIST, font, buf, h, w, 7, [("rect",) + tuple(r) for r in rects], name)
        assert np.array_equal(got, img_dev.cpu().numpy()), name


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_count_zero_and_refusals(ctx, R, font):
    h, w = 20, 30
    buf = canvas(h, w, 4)
    pitch = 3 * w + 4
    good = [("rect", 2, 2, 9, 9, 8, 1, 2, 3), ("text", 3, 12, "ok: 1", 1, 255, 0, 255), ("rect", 1, 1, 5, 5, D.FILLED, 0, 0, 0), ("text", 1, 18, "gy", 1, 9, 9, 9)]
    rows, pool = D.pack(good)
    rc, msg, got = G.prims_call(ctx, R, G.LIST.entry, buf, h, w, pitch, rows, pool)
    assert rc == 0 and np.array_equal(got, G.expected(D.paint_list, buf, h, w, good, font)) and not np.array_equal(got, buf)
    rc, msg, got = G.prims_call(ctx, R, G.LIST.entry, buf, h, w, pitch, [])
    assert rc == 0 and np.array_equal(got, buf)
    rc, msg, got = G.prims_call(ctx, R, G.LIST.entry, buf, h, w, pitch, rows, pool, count=0, host=False, dev=False, chars_host=False, chars_dev=False)
    assert rc == 0 and np.array_equal(got, buf)

    names = list(R.PRIM.names)

    def with_entry(i, **fields):
        t = [list(r) for r in rows]
        for k, v in fields.items():
            t[i][names.index(k)] = v
        return t

    def with_byte(k, v):
        p = bytearray(pool)
        p[k] = v
        return bytes(p)

    assert rows[1][5:7] == (0, 5) and rows[3][5:7] == (5, 2) and len(pool) == 7
    for what, table, chars, entry in (("an unknown kind", with_entry(2, kind=2), pool, 2), ("a negative kind", with_entry(0, kind=-1), pool, 0),
                                      ("thickness 0", with_entry(2, a=0), pool, 2), ("scale 0", with_entry(1, x2=0), pool, 1),
                                      ("scale 65", with_entry(3, x2=65), pool, 3), ("scale -1", with_entry(1, x2=-1), pool, 1),
                                      ("y2 on a text entry", with_entry(3, y2=1), pool, 3), ("a negative offset", with_entry(1, a=-1), pool, 1),
                                      ("a negative length", with_entry(3, b=-1), pool, 3), ("a run past the pool", with_entry(3, b=3), pool, 3),
                                      ("an offset past the pool", with_entry(1, a=8, b=0), pool, 1),
                                      ("offset + length past int32", with_entry(1, a=2 ** 31 - 1, b=2 ** 31 - 1), pool, 1),
                                      ("a control code", rows, with_byte(2, 0x1F), 1), ("DEL", rows, with_byte(6, 0x7F), 3),
                                      ("a byte above ASCII", rows, with_byte(0, 0xE5), 1),
                                      ("colour bit 24", with_entry(0, bgr=1 << 24), pool, 0), ("a negative colour", with_entry(3, bgr=-1), pool, 3)):
        rc, msg, got = G.prims_call(ctx, R, G.LIST.entry, buf, h, w, pitch, table, chars)
        assert rc == ERR_ARG and ("entry %d " % entry) in msg, (what, msg)
        assert np.array_equal(got, buf), what                                                 # not even the entries in front of the bad one
    # a byte outside the font that no run refers to is nobody's business
    rows2, pool2 = D.pack(good, pool=b"\x00\xff")
    rc, msg, got = G.prims_call(ctx, R, G.LIST.entry, buf, h, w, pitch, rows2, pool2)
    assert rc == 0 and np.array_equal(got, G.expected(D.paint_list, buf, h, w, good, font)), msg
    for what, kw in (("short pitch", dict(pitch=3 * w - 1)), ("negative count", dict(count=-1)), ("null host table", dict(host=False)),
                     ("null device table", dict(dev=False)), ("no context", dict(handle=False)), ("null host pool", dict(chars_host=False)),
                     ("null device pool", dict(chars_dev=False)), ("a negative pool length", dict(n_chars=-1))):
        p = kw.pop("pitch", pitch)
        rc, msg, got = G.prims_call(ctx, R, G.LIST.entry, buf, h, w, p, rows, pool, **kw)
        assert rc == ERR_ARG and np.array_equal(got, buf), what
    rc, msg, got = G.prims_call(ctx, R, G.LIST.entry, buf, 0, w, pitch, rows, pool)
    assert rc == ERR_ARG and np.array_equal(got, buf)


# ---- draw_list_device, draw_detections and write_predictions ----------------------------------------------------------------------------
class _Config:
    class_mapping = {"boat": 0, "human": 1, "animal": 2, "bg": 3}


def test_draw_list_device(R, font):
    img = np.random.RandomState(6).randint(0, 256, (40, 70, 3)).astype(np.uint8)
    dev = torch.from_numpy(img).cuda()
    prims = [("rect", 3, 3, 60, 30, 2, 1, 2, 3), ("text", 5, 20, "Héllo, g", 2, 250, 251, 252), ("rect", 20, 10, 30, 25, -1, 7, 8, 9), ("text", 22, 24, "~", 1, 0, 0, 0)]
    want = D.paint_list(img.copy(), [prims[0], ("text", 5, 20, "H?llo, g", 2, 250, 251, 252)] + prims[2:], font)
    out = R.draw_list_device(dev, prims)
    assert out.is_cuda and out.data_ptr() != dev.data_ptr() and torch.equal(dev.cpu(), torch.from_numpy(img))      # inplace=False: the input stays
    assert np.array_equal(out.cpu().numpy(), want)
    assert torch.equal(R.draw_list_device(dev, []), dev)
    assert np.array_equal(R.draw_list_device(dev, prims[:1]).cpu().numpy(), D.paint_list(img.copy(), prims[:1], font))      # no pool at all
    from_host = R.draw_list_device(img, prims)                                                 # a NumPy image is uploaded, the array stays
    assert from_host.is_cuda and np.array_equal(from_host.cpu().numpy(), want) and not np.array_equal(img, want)
    same = R.draw_list_device(dev, prims, inplace=True)
    assert same.data_ptr() == dev.data_ptr() and np.array_equal(dev.cpu().numpy(), want)
    with pytest.raises(ValueError, match="entry 1"):
        R.draw_list_device(dev, [prims[0], ("circle", 1, 2, 3)])
    from radnet_hip import lib as L
    with pytest.raises(L.RadnetError, match="entry 0 "):
        R.draw_list_device(dev, [("text", 1, 9, "x", 65, 0, 0, 0)])


def test_draw_detections_with_labels(R, font):
    net = R.RADNet(_Config(), None, None, None)
    img = np.random.RandomState(1).randint(0, 256, (96, 128, 3)).astype(np.uint8)
    dev = torch.from_numpy(img).cuda()
    out = net.draw_detections(dev, D.DETS, labels=True)
    assert out.is_cuda and out.data_ptr() != dev.data_ptr() and torch.equal(dev.cpu(), torch.from_numpy(img))
    want = D.paint_list(img.copy(), D.labelled(D.DETS, D.LABELS, D.WHITE), font)
    assert np.array_equal(out.cpu().numpy(), want)
    assert not np.array_equal(want, W.paint(img.copy(), [p[1:] for p in D.outlines(D.DETS, D.WHITE)]))      # the labels do show
    out = net.draw_detections(dev, D.DETS, color=(1, 2, 3), thickness=1, classes=("human", "wheel"), labels=True, label_scale=1)
    assert np.array_equal(out.cpu().numpy(), D.paint_list(img.copy(), D.labelled(D.DETS[1::2], D.LABELS[1::2], (1, 2, 3), 1, 1), font))
    assert torch.equal(net.draw_detections(dev, D.DETS, classes=(), labels=True), dev)
    assert torch.equal(net.draw_detections(img, D.DETS, labels=True).cpu(), torch.from_numpy(want))      # a NumPy image
    same = net.draw_detections(dev, D.DETS, labels=True, inplace=True)
    assert same.data_ptr() == dev.data_ptr() and np.array_equal(dev.cpu().numpy(), want)


def test_write_predictions_with_labels(R, font, tmp_path):
    from faster_rcnn import png
    net = R.RADNet(_Config(), None, None, None)
    img = np.random.RandomState(2).randint(0, 256, (96, 128, 3)).astype(np.uint8)
    dev = torch.from_numpy(img).cuda()
    paths = net.write_predictions(D.DETS, dev, str(tmp_path / "out"), labels=True)
    plain = net.write_predictions(D.DETS, dev, str(tmp_path / "plain"))
    assert [os.path.basename(p) for p in paths] == ["all_predictions.png", "boat_predictions.png", "human_predictions.png", "other_predictions.png",
                                                    "predictions.json"]
    assert torch.equal(dev.cpu(), torch.from_numpy(img))
    wants = [D.labelled(D.DETS, D.LABELS, D.WHITE), D.outlines(D.DETS[:1], (28, 26, 228)), D.outlines(D.DETS[1:2], (184, 126, 55)),
             D.labelled(D.DETS[2:], D.LABELS[2:], (0, 127, 255))]
    for path, prims in zip(paths, wants):
        want = D.paint_list(img.copy(), prims, font)
        data = open(path, "rb").read()
        assert np.array_equal(W.decode_bgr(data), want), path
        assert np.array_equal(png.decode_device(data).cpu().numpy(), want), path
    for k in (1, 2, 4):                                                                         # boats, humans and the JSON: today's bytes
        assert open(paths[k], "rb").read() == open(plain[k], "rb").read()
    for k in (0, 3):
        assert open(paths[k], "rb").read() != open(plain[k], "rb").read()
        assert np.array_equal(W.decode_bgr(open(plain[k], "rb").read()), W.paint(img.copy(), [p[1:] for p in wants[k] if p[0] == "rect" and p[5] == 8]))
    again = net.write_predictions(D.DETS, img, str(tmp_path / "again"), labels=True)            # a NumPy map: the same files
    for a, b in zip(paths, again):
        assert open(a, "rb").read() == open(b, "rb").read()
    scaled = net.write_predictions(D.DETS, dev, str(tmp_path / "scaled"), labels=True, label_scale=1)
    assert np.array_equal(W.decode_bgr(open(scaled[3], "rb").read()), D.paint_list(img.copy(), D.labelled(D.DETS[2:], D.LABELS[2:], (0, 127, 255), 1), font))


# ---- evaluate_scans ----------------------------------------------------------------------------------------------------------------------
def test_evaluate_scans_end_to_end(R, font, tmp_path, monkeypatch):
    from faster_rcnn import evaluate, utils_io
    monkeypatch.chdir(tmp_path)
    os.makedirs("scans/blended_grey")
    maps = {"scans/panel_a.png": np.random.RandomState(3).randint(0, 256, (96, 128, 3)).astype(np.uint8),
            "scans/panel_b": np.random.RandomState(4).randint(0, 256, (100, 140, 3)).astype(np.uint8)}
    utils_io.imwrite("scans/blended_grey/panel_a.png", maps["scans/panel_a.png"])
    utils_io.imwrite("scans/blended_grey/panel_b.png", maps["scans/panel_b"])
    os.rename("scans/blended_grey/panel_b.png", "scans/blended_grey/panel_b")                   # the reference's scans carry no extension
    dets = {"scans/panel_a.png": D.DETS[:2], "scans/panel_b": D.DETS[2:]}
    labels = {"scans/panel_a.png": D.LABELS[:2], "scans/panel_b": D.LABELS[2:]}
    gt = {"scans/panel_a.png": [{'class': 'boat', 'x1': 10, 'y1': 20, 'x2': 70, 'y2': 61}], "scans/panel_b": [{'class': 'wheel', 'x1': 0, 'y1': 70, 'x2': 30, 'y2': 99}]}
    data_test = [{'filepath': path, 'bboxes': [dict(g) for g in gt[path]]} for path in maps]
    net = R.RADNet(_Config(), None, None, None)
    monkeypatch.setattr(net, "predict_from_path", lambda path: [dict(d) for d in dets[path]])
    accuracy, elapsed, paths = evaluate.evaluate_scans(net, data_test, "model")
    assert paths == [os.path.join("model", "test", "panel_a.png"), os.path.join("model", "test", "panel_b.png")]
    assert len(elapsed) == 2 and all(t >= 0 for t in elapsed)
    for path, written in zip(maps, paths):
        want = D.paint_list(maps[path].copy(), D.labelled(dets[path], labels[path], D.WHITE), font)
        assert np.array_equal(W.decode_bgr(open(written, "rb").read()), want), path
    want = evaluate.mean_average_precision([dict(d) for p in maps for d in dets[p]], [dict(g) for p in maps for g in gt[p]])
    assert accuracy == {k: float(v) for k, v in want.items()} and set(accuracy) == {"boat", "human", "animal", "wheel", "mAP"}
    with open(os.path.join("model", "test_accuracy.json")) as f:
        assert f.read() == json.dumps(accuracy, indent=4)
    plain = evaluate.evaluate_scans(net, data_test[:1], "plain", labels=False)[2]
    assert np.array_equal(W.decode_bgr(open(plain[0], "rb").read()), W.paint(maps["scans/panel_a.png"].copy(), [p[1:] for p in D.outlines(D.DETS[:2], D.WHITE)]))
