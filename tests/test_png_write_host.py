"""The device-free half of the PNG writer and of the prediction maps: png.assemble (chunked deflate on host threads behind one zlib
header) on streams made by png_cases.filter_rows, read back by the tests' own decoder (png_write_cases.decode) and by png.parse;
the NumPy painter of png_write_cases against hand-written pixel sets; what imwrite / encode_device refuse before any device work;
RADNet.write_predictions with a stub painter and a stub encoder; the library's exports.  No device needed."""
import json
import os
import zlib

import numpy as np
import pytest

import png_cases as K
import png_write_cases as W
from faster_rcnn import png, utils_io
from faster_rcnn import RADNet as R
from radnet_hip import lib as L


def streams():
    """(what, stream bytes, raw rows, width, height, colour type): RGB and grey, adaptive, random per row and each fixed filter."""
    rs = np.random.RandomState(5)
    out = []
    for what, h, w, ch, types in (("rgb adaptive", 9, 11, 3, "adaptive"), ("rgb random", 13, 7, 3, rs.randint(0, 5, 13)), ("grey adaptive", 6, 29, 1, "adaptive"),
                                  ("grey paeth", 5, 3, 1, 4), ("one byte", 1, 1, 1, 0), ("rgb smooth", 12, 40, 3, "adaptive")):
        raw = (W.filter_input("ramp", h, w, ch) if "smooth" in what else rs.randint(0, 256, (h, w, ch)).astype(np.uint8)).reshape(h, w * ch)
        lines, _ = K.filter_rows(raw, ch, types)
        out.append((what, lines.tobytes(), raw, w, h, 2 if ch == 3 else 0))
    return out


STREAMS = streams()


@pytest.mark.parametrize("case", STREAMS, ids=[s[0] for s in STREAMS])
def test_assemble_round_trips_whatever_the_chunking_and_the_threads(case):
    what, stream, raw, w, h, color_type = case
    files = set()
    for chunk_bytes in (1, 7, max(1, len(stream) - 1), len(stream) + 100):
        for workers in (1, 3):
            data = png.assemble(stream, w, h, color_type, 1, "rle", workers, chunk_bytes)
            d = W.decode(data)
            assert (d.width, d.height, d.color_type) == (w, h, color_type)
            assert d.stream == stream, (what, chunk_bytes, workers)                        # identical whatever chunk_bytes and workers
            assert np.array_equal(d.samples.reshape(h, -1), raw)
            assert d.kinds.count(b"IHDR") == 1 and d.kinds.count(b"IDAT") >= 1 and d.kinds.count(b"IEND") == 1
            img = png.parse(data)                                                          # the product's own reader
            assert img.stream == stream and (img.header.width, img.header.height, img.header.bit_depth, img.header.color_type) == (w, h, 8, color_type)
            assert data == png.assemble(stream, w, h, color_type, 1, "rle", 1, chunk_bytes), "the thread count changes the file"
            files.add(data)
    assert len(files) >= (2 if len(stream) > 1 else 1)                                     # the chunking does change the deflate pieces


@pytest.mark.parametrize("level", [0, 6])
@pytest.mark.parametrize("strategy", ["rle", "default", zlib.Z_HUFFMAN_ONLY])
def test_assemble_levels_and_strategies(level, strategy):
    for what, stream, raw, w, h, color_type in STREAMS:
        data = png.assemble(stream, w, h, color_type, level, strategy, 2, 50)
        d = W.decode(data)
        assert d.stream == stream and np.array_equal(d.samples.reshape(h, -1), raw), what
        assert png.parse(data).stream == stream


def test_assemble_defaults_and_the_zlib_header():
    what, stream, raw, w, h, color_type = STREAMS[0]
    data = png.assemble(stream, w, h, color_type)
    assert data == png.assemble(stream, w, h, color_type, 1, "rle", None, 1 << 20)
    (idat,) = [p for k, p in W.chunks(data) if k == b"IDAT"]
    assert idat[0] == 0x78 and (idat[0] * 256 + idat[1]) % 31 == 0 and not idat[1] & 0x20      # 32 KiB window, FCHECK, no preset dictionary
    assert int.from_bytes(idat[-4:], "big") == zlib.adler32(stream)
    for level in (-1, 0, 1, 2, 5, 6, 7, 9):                                                 # every level's header is a legal CMF / FLG pair
        head = png.assemble(stream, w, h, color_type, level)[8 + 25 + 8:][:2]
        assert head[0] == 0x78 and (head[0] * 256 + head[1]) % 31 == 0 and not head[1] & 0x20


def test_assemble_refuses():
    what, stream, raw, w, h, color_type = STREAMS[0]
    for kw in (dict(width=w + 1), dict(height=h - 1), dict(color_type=0), dict(color_type=6), dict(level=10), dict(chunk_bytes=0),
               dict(strategy="fastest"), dict(width=0)):
        args = dict(stream_bytes=stream, width=w, height=h, color_type=color_type, level=1, strategy="rle", workers=1, chunk_bytes=64)
        args.update(kw)
        with pytest.raises(ValueError, match="PNG"):
            png.assemble(**args)


def test_an_idat_that_would_not_fit_a_chunk_is_refused(monkeypatch):
    what, stream, raw, w, h, color_type = STREAMS[0]
    monkeypatch.setattr(png, "IDAT_MAX", 40)
    with pytest.raises(ValueError, match="IDAT"):
        png.assemble(stream, w, h, color_type)


def test_worker_counts_follow_the_rules_of_decode_device_many():
    assert [png._workers(p, None) for p in (1, 5, 8, 9, 500)] == [1, 5, 8, 8, 8]
    assert [png._workers(500, k) for k in (0, 1, 16, 17, 1000)] == [1, 1, 16, 16, 16]


# ---- the painter ---------------------------------------------------------------------------------------------------------------------
def painted(h, w, rects):
    """The set of (x, y) the painter changes on a zero image, and the image."""
    img = W.paint(np.zeros((h, w, 3), np.uint8), rects)
    ys, xs = np.nonzero(img.any(axis=2))
    return set(zip(xs.tolist(), ys.tolist())), img


def box(x1, y1, x2, y2):
    return {(x, y) for x in range(x1, x2 + 1) for y in range(y1, y2 + 1)}


def test_painter_against_hand_written_pixel_sets():
    c = (1, 2, 3)
    got, img = painted(12, 16, [(3, 2, 9, 7, 1) + c])
    assert got == box(3, 2, 9, 7) - box(4, 3, 8, 6)                                          # the one-pixel outline
    assert {tuple(v) for v in img[img.any(axis=2)].tolist()} == {c}
    assert painted(12, 16, [(3, 2, 9, 7, W.FILLED) + c])[0] == box(3, 2, 9, 7)
    assert painted(12, 16, [(3, 2, 9, 7, -8) + c])[0] == box(3, 2, 9, 7)                      # any negative thickness fills
    got, _ = painted(40, 50, [(10, 12, 30, 28, 8) + c])                                      # hw = 4: four pixels out, four pixels in
    assert got == box(6, 8, 34, 32) - box(15, 17, 25, 23)
    assert len(got) == 29 * 25 - 11 * 7
    got9, _ = painted(40, 50, [(10, 12, 30, 28, 9) + c])                                     # 9 // 2 is 4 too
    assert got9 == got
    assert painted(40, 50, [(30, 28, 10, 12, 8) + c])[0] == got                              # reversed corners, both
    assert painted(40, 50, [(30, 12, 10, 28, 8) + c])[0] == got                              # ... and one
    assert painted(12, 16, [(20, 3, 30, 8, 1) + c, (-9, -9, -2, -2, W.FILLED) + c, (2, 30, 9, 40, 8) + c])[0] == set()      # off the image
    got, _ = painted(12, 16, [(-3, -2, 4, 5, 1) + c])                                        # clipped: the far edges remain
    assert got == {(4, y) for y in range(0, 6)} | {(x, 5) for x in range(0, 5)}
    got, _ = painted(12, 16, [(14, 3, 25, 8, 8) + c])                                        # x1 - hw = 10: the outline reaches in
    assert got == box(10, 0, 15, 11)
    assert painted(12, 16, [(5, 2, 5, 9, 1) + c])[0] == box(5, 2, 5, 9)                        # degenerate: a line
    assert painted(12, 16, [(5, 4, 9, 8, 2) + c])[0] == box(4, 3, 10, 9) - box(7, 6, 7, 6)     # t = 2: hw = 1


def test_painter_paints_in_list_order():
    a, b = (2, 2, 9, 9, W.FILLED, 10, 20, 30), (5, 5, 12, 12, W.FILLED, 40, 50, 60)
    ab = W.paint(np.zeros((16, 16, 3), np.uint8), [a, b])
    ba = W.paint(np.zeros((16, 16, 3), np.uint8), [b, a])
    assert tuple(ab[6, 6]) == (40, 50, 60) and tuple(ba[6, 6]) == (10, 20, 30)
    assert tuple(ab[3, 3]) == tuple(ba[3, 3]) == (10, 20, 30) and tuple(ab[11, 11]) == tuple(ba[11, 11]) == (40, 50, 60)


def test_the_tests_decoder_reads_the_tests_encoder():
    """png_write_cases.decode is independent of the product: it reads what png_cases.encode writes, for every fixed filter."""
    rs = np.random.RandomState(3)
    for color_type, ch in ((2, 3), (0, 1)):
        samples = rs.randint(0, 256, (7, 9, ch))
        for filters in (0, 1, 2, 3, 4, "adaptive", np.random.RandomState(1)):
            d = W.decode(K.encode(samples, color_type, 8, filters=filters, idat_sizes=(3, 10)).data)
            assert np.array_equal(d.samples, samples)


# ---- refusals before any device work -----------------------------------------------------------------------------------------------------
def test_imwrite_and_encode_refuse_before_any_device_work(tmp_path):
    img = np.zeros((4, 5, 3), np.uint8)
    for name in ("map.jpg", "map.PNG.tif", "map"):
        with pytest.raises(ValueError, match="PNG"):
            utils_io.imwrite(str(tmp_path / name), img)
    with pytest.raises(ValueError, match="shape"):
        utils_io.imwrite(str(tmp_path / "map.png"), np.zeros((4, 5, 4), np.uint8))            # a 4-channel array
    with pytest.raises(ValueError, match="shape"):
        png.encode_device(np.zeros((4, 5, 1, 3), np.uint8))
    with pytest.raises(ValueError, match="empty"):
        png.encode_device(np.zeros((0, 5, 3), np.uint8))
    with pytest.raises(TypeError, match="uint8"):
        png.encode_device(np.zeros((4, 5, 3), np.float32))
    with pytest.raises(ValueError, match="filter"):
        png.encode_device(img, filter="best")
    with pytest.raises(ValueError, match="filter"):
        png.encode_device(img, filter=5)
    assert os.listdir(tmp_path) == []


# ---- write_predictions with stubs ------------------------------------------------------------------------------------------------------
class _Config:
    class_mapping = {"boat": 0, "human": 1, "animal": 2, "bg": 3}


DETS = [{'class': 'boat', 'prob': np.float32(0.5), 'x1': np.int64(10), 'y1': np.int64(20), 'x2': np.int64(50), 'y2': np.int64(60)},
        {'class': 'human', 'prob': 0.75, 'x1': 5, 'y1': 6, 'x2': 7, 'y2': 8},
        {'class': 'animal', 'prob': 0.25, 'x1': 70, 'y1': 30, 'x2': 90, 'y2': 45},
        {'class': 'wheel', 'prob': 1.0, 'x1': 1, 'y1': 2, 'x2': 3, 'y2': 4}]

PREDICTIONS_JSON = """[
    {
        "label": "boat",
        "confidence": 0.5,
        "x1": 10,
        "y1": 20,
        "x2": 50,
        "y2": 60
    },
    {
        "label": "human",
        "confidence": 0.75,
        "x1": 5,
        "y1": 6,
        "x2": 7,
        "y2": 8
    },
    {
        "label": "animal",
        "confidence": 0.25,
        "x1": 70,
        "y1": 30,
        "x2": 90,
        "y2": 45
    },
    {
        "label": "wheel",
        "confidence": 1.0,
        "x1": 1,
        "y1": 2,
        "x2": 3,
        "y2": 4
    }
]"""


def test_write_predictions_with_a_stub_painter_and_a_stub_encoder(tmp_path, monkeypatch):
    net = R.RADNet(_Config(), None, None, None)
    calls = []

    def draw(img, rects, inplace=False, ctx=None):                                            # stands in for the device painter
        calls.append(([tuple(r) for r in rects], inplace))
        return ("drawn", len(calls), img)

    def encode(img, **kw):
        assert img[0] == "drawn" and img[2] == "the map" and not kw
        return b"PNG %d" % img[1]

    monkeypatch.setattr(R, "draw_rects_device", draw)
    monkeypatch.setattr(png, "encode_device", encode)
    out_dir = tmp_path / "predictions"
    paths = net.write_predictions(DETS, "the map", str(out_dir))
    names = ["all_predictions.png", "boat_predictions.png", "human_predictions.png", "other_predictions.png", "predictions.json"]
    assert [os.path.basename(p) for p in paths] == names and sorted(os.listdir(out_dir)) == sorted(names)
    for k, name in enumerate(names[:4]):
        assert (out_dir / name).read_bytes() == b"PNG %d" % (k + 1)
    boxes = [(10, 20, 50, 60), (5, 6, 7, 8), (70, 30, 90, 45), (1, 2, 3, 4)]
    assert calls == [([b + (8, 255, 255, 255) for b in boxes], False),
                     ([boxes[0] + (8, 28, 26, 228)], False),
                     ([boxes[1] + (8, 184, 126, 55)], False),
                     ([b + (8, 0, 127, 255) for b in boxes[2:]], False)]
    text = (out_dir / "predictions.json").read_text()
    assert text == PREDICTIONS_JSON
    assert json.loads(text)[0] == {"label": "boat", "confidence": 0.5, "x1": 10, "y1": 20, "x2": 50, "y2": 60}


def test_draw_detections_selects_by_names_and_by_predicate(monkeypatch):
    net = R.RADNet(_Config(), None, None, None)
    seen = []
    monkeypatch.setattr(R, "draw_rects_device", lambda img, rects, inplace=False, ctx=None: seen.append((list(rects), inplace)) or img)
    assert net.draw_detections("img", DETS, classes=["human", "wheel"], color=(1, 2, 3), thickness=2, inplace=True) == "img"
    net.draw_detections("img", DETS, classes=lambda name: name.startswith("b"))
    net.draw_detections("img", [], classes=None)
    assert seen == [([(5, 6, 7, 8, 2, 1, 2, 3), (1, 2, 3, 4, 2, 1, 2, 3)], True), ([(10, 20, 50, 60, 8, 255, 255, 255)], False), ([], False)]


# ---- the library ---------------------------------------------------------------------------------------------------------------------------
def test_the_library_exports_both_entries_and_the_mirrors_match():
    declared = L.declared_symbols()
    lib = L.load_library()
    for name in ("radnet_png_filter_rows_u8", "radnet_draw_rects_u8"):
        assert name in declared and hasattr(lib, name)
    assert L.header_constant("RADNET_DRAW_RECT_BATCH") == 256
    assert R.RECT.itemsize == 32 and list(R.RECT.names) == ["x1", "y1", "x2", "y2", "thickness", "b", "g", "r"]
    assert png.FILTER_MODES == {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": 5}
