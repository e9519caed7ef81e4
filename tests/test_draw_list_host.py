"""The device-free half of the labelled prediction maps: the package's own font read through radnet_draw_glyph_rows; text_size
and label_bytes; the primitive list RADNet.draw_detections(labels=True) emits, with draw_list_device stubbed; which maps
write_predictions labels; the NumPy painter of draw_list_cases against the mistakes a kernel is likely to make; the library's
exports.  No device needed."""
import ctypes
import os

import numpy as np
import pytest

import draw_list_cases as D
from faster_rcnn import RADNet as R
from faster_rcnn import png
from radnet_hip import lib as L
from test_png_write_host import DETS

ERR_ARG = -1


def glyph(code):
    rows = (ctypes.c_uint8 * 8)(*([0xEE] * 8))
    rc = L.load_library().radnet_draw_glyph_rows(code, rows)
    return rc, bytes(rows)


@pytest.fixture(scope="module")
def font():
    out = {}
    for code in range(D.FIRST, D.LAST + 1):
        rc, rows = glyph(code)
        assert rc == 0, code
        out[code] = rows
    return out


def picture(rows):
    return ["".join("#" if (b >> (4 - c)) & 1 else "." for c in range(5)) for b in rows]


# ---- the font ----------------------------------------------------------------------------------------------------------------------------
def test_the_font_has_95_distinct_glyphs_of_five_columns(font):
    assert len(font) == 95
    assert all(len(rows) == 8 and all(b < 32 for b in rows) for rows in font.values())
    assert font[0x20] == bytes(8)
    assert all(any(rows) for code, rows in font.items() if code != 0x20)
    assert len(set(font.values())) == 95
    for code in list(range(ord("0"), ord("9") + 1)) + list(range(ord("A"), ord("Z") + 1)):
        assert font[code][7] == 0, chr(code)                                                  # nothing below the baseline
    for ch in "gjpqy":
        assert font[ord(ch)][7] != 0, ch


PICTURES = {
    "b": ["#....",
          "#....",
          "#.##.",
          "##..#",
          "#...#",
          "#...#",
          "####.",
          "....."],
    "o": [".....",
          ".....",
          ".###.",
          "#...#",
          "#...#",
          "#...#",
          ".###.",
          "....."],
    "a": [".....",
          ".....",
          ".###.",
          "....#",
          ".####",
          "#...#",
          ".####",
          "....."],
    "t": [".#...",
          ".#...",
          "###..",
          ".#...",
          ".#...",
          ".#..#",
          "..##.",
          "....."],
    ":": [".....",
          ".##..",
          ".##..",
          ".....",
          ".##..",
          ".##..",
          ".....",
          "....."],
    "9": [".###.",
          "#...#",
          "#...#",
          ".####",
          "....#",
          "...#.",
          ".##..",
          "....."],
    "7": ["#####",
          "....#",
          "...#.",
          "..#..",
          ".#...",
          ".#...",
          ".#...",
          "....."],
    " ": ["....."] * 8,
}


@pytest.mark.parametrize("ch", sorted(PICTURES))
def test_glyphs_equal_their_pictures(font, ch):
    assert picture(font[ord(ch)]) == PICTURES[ch]


def test_codes_outside_the_font_are_refused():
    for code in (0x1F, 0x7F, -1, 0, 256, 2 ** 31 - 1, -2 ** 31):
        rc, rows = glyph(code)
        assert rc == ERR_ARG and rows == bytes([0xEE] * 8), code                              # nothing is written
    assert L.load_library().radnet_draw_glyph_rows(0x41, None) == ERR_ARG
    assert glyph(0x20)[0] == 0 and glyph(0x7E)[0] == 0
    assert L.glyph_rows(ord("A")) == glyph(ord("A"))[1]
    with pytest.raises(L.RadnetError, match="0x7F"):
        L.glyph_rows(0x7F)


# ---- text_size and label_bytes -------------------------------------------------------------------------------------------------------------
def test_text_size_and_label_bytes():
    assert R.text_size("") == ((0, 21), 3) and R.text_size("", 1) == ((0, 7), 1)
    assert R.text_size("a") == ((15, 21), 3) and R.text_size("a", 1) == ((5, 7), 1) and R.text_size("a", 7) == ((35, 49), 7)
    assert R.text_size("boat: 50") == ((141, 21), 3) and R.text_size("boat: 50", 2) == ((94, 14), 2)
    assert R.label_bytes("") == b"" and R.label_bytes("boat: 50") == b"boat: 50" and R.label_bytes(" ~") == b" ~"
    assert R.label_bytes("båt") == b"b?t" and R.label_bytes("船: 7") == b"?: 7"        # one '?' per character that is not ASCII
    assert R.label_bytes("a\tb\x7f\n") == b"a?b??"                                             # control codes are not in the font either
    assert R.text_size("båt") == R.text_size("b?t") == ((51, 21), 3)
    assert all(D.FIRST <= c <= D.LAST for c in R.label_bytes("".join(chr(c) for c in range(0, 0x250))))


# ---- draw_detections(labels=True) with the device painter stubbed ------------------------------------------------------------------------
class _Config:
    class_mapping = {"boat": 0, "human": 1, "animal": 2, "bg": 3}


def stubs(monkeypatch):
    lists, rects = [], []
    monkeypatch.setattr(R, "draw_list_device", lambda img, prims, inplace=False, ctx=None: lists.append(([tuple(p) for p in prims], inplace)) or img)
    monkeypatch.setattr(R, "draw_rects_device", lambda img, rs, inplace=False, ctx=None: rects.append(([tuple(r) for r in rs], inplace)) or img)
    return lists, rects


def test_draw_detections_emits_the_references_four_steps_per_detection(monkeypatch):
    """DETS[0] is a boat at 0.5 from (10, 20) to (50, 60), DETS[1] a human at 0.75 from (5, 6) to (7, 8).  'boat: 50' has 8 characters:
    tw = 47 * 3 = 141, th = 21, baseline = 3, so the label box runs from (10 - 5, 20 + 3 - 5) to (10 + 141 + 5, 20 - 21 - 5); 'human: 75'
    has 9: tw = 53 * 3 = 159."""
    net = R.RADNet(_Config(), None, None, None)
    lists, rects = stubs(monkeypatch)
    assert net.draw_detections("img", DETS[:2], labels=True) == "img"
    assert rects == [] and lists == [([("rect", 10, 20, 50, 60, 8, 255, 255, 255),
                                       ("rect", 5, 18, 156, -6, 1, 0, 0, 0),
                                       ("rect", 5, 18, 156, -6, -1, 255, 255, 255),
                                       ("text", 10, 20, "boat: 50", 3, 0, 0, 0),
                                       ("rect", 5, 6, 7, 8, 8, 255, 255, 255),
                                       ("rect", 0, 4, 169, -20, 1, 0, 0, 0),
                                       ("rect", 0, 4, 169, -20, -1, 255, 255, 255),
                                       ("text", 5, 6, "human: 75", 3, 0, 0, 0)], False)]
    del lists[:]
    net.draw_detections("img", DETS[1:2], color=(1, 2, 3), thickness=2, labels=True, label_scale=1, inplace=True)
    assert lists == [([("rect", 5, 6, 7, 8, 2, 1, 2, 3), ("rect", 0, 2, 63, -6, 1, 0, 0, 0), ("rect", 0, 2, 63, -6, -1, 255, 255, 255),
                       ("text", 5, 6, "human: 75", 1, 0, 0, 0)], True)]
    assert all(type(v) in (int, str) for p in lists[0][0] for v in p)                          # no NumPy scalars reach the table


def test_draw_detections_with_labels_selects_by_classes(monkeypatch):
    net = R.RADNet(_Config(), None, None, None)
    lists, rects = stubs(monkeypatch)
    net.draw_detections("img", DETS, classes=["human", "wheel"], labels=True)
    net.draw_detections("img", DETS, classes=lambda name: name.startswith("b"), labels=True)
    net.draw_detections("img", DETS, classes=(), labels=True)
    texts = [[p[3] for p in prims if p[0] == "text"] for prims, _ in lists]
    assert texts == [["human: 75", "wheel: 100"], ["boat: 50"], []] and [len(prims) for prims, _ in lists] == [8, 4, 0]
    assert rects == []
    net.draw_detections("img", DETS[:1], labels=False)                                         # the default path is the rectangle painter's
    assert rects == [([(10, 20, 50, 60, 8, 255, 255, 255)], False)] and len(lists) == 3


def test_write_predictions_labels_the_all_and_other_maps_only(tmp_path, monkeypatch):
    net = R.RADNet(_Config(), None, None, None)
    calls = []
    monkeypatch.setattr(R, "draw_list_device", lambda img, prims, inplace=False, ctx=None: calls.append(("list", [tuple(p) for p in prims], inplace)) or len(calls))
    monkeypatch.setattr(R, "draw_rects_device", lambda img, rs, inplace=False, ctx=None: calls.append(("rects", [tuple(r) for r in rs], inplace)) or len(calls))
    monkeypatch.setattr(png, "encode_device", lambda img, **kw: b"PNG %d" % img)
    paths = net.write_predictions(DETS, "the map", str(tmp_path / "out"), labels=True, label_scale=2)
    assert [os.path.basename(p) for p in paths] == ["all_predictions.png", "boat_predictions.png", "human_predictions.png", "other_predictions.png",
                                                    "predictions.json"]
    assert [c[0] for c in calls] == ["list", "rects", "rects", "list"] and not any(c[2] for c in calls)
    assert [open(p, "rb").read() for p in paths[:4]] == [b"PNG 1", b"PNG 2", b"PNG 3", b"PNG 4"]
    assert [p[3:5] for p in calls[0][1] if p[0] == "text"] == [("boat: 50", 2), ("human: 75", 2), ("animal: 25", 2), ("wheel: 100", 2)]
    assert [p[3:5] for p in calls[3][1] if p[0] == "text"] == [("animal: 25", 2), ("wheel: 100", 2)]
    assert [p for p in calls[3][1] if p[0] == "rect"][0] == ("rect", 70, 30, 90, 45, 8, 0, 127, 255)
    assert calls[1][1] == [(10, 20, 50, 60, 8, 28, 26, 228)] and calls[2][1] == [(5, 6, 7, 8, 8, 184, 126, 55)]
    del calls[:]
    net.write_predictions(DETS, "the map", str(tmp_path / "plain"))                             # the default: no list at all
    assert [c[0] for c in calls] == ["rects"] * 4


# ---- the painter ---------------------------------------------------------------------------------------------------------------------------
def test_the_painter_against_hand_written_pixel_sets(font):
    img = D.paint_list(np.zeros((12, 16, 3), np.uint8), [("text", 2, 8, ":", 1, 1, 2, 3)], font)
    ys, xs = np.nonzero(img.any(axis=2))
    assert set(zip(xs.tolist(), ys.tolist())) == {(3, 2), (4, 2), (3, 3), (4, 3), (3, 5), (4, 5), (3, 6), (4, 6)}      # rows 1, 2, 4, 5 of ':' from y = 1
    assert {tuple(v) for v in img[img.any(axis=2)].tolist()} == {(1, 2, 3)}
    img = D.paint_list(np.zeros((12, 30, 3), np.uint8), [("text", 1, 7, "tt", 1, 9, 9, 9)], font)          # the second character starts 6 dots on
    assert np.array_equal(img[:, 7:12], img[:, 1:6]) and not img[:, 6].any() and not img[:, 12:].any()
    img = D.paint_list(np.zeros((20, 20, 3), np.uint8), [("text", 0, 14, "7", 2, 9, 9, 9)], font)           # scale 2: row 0 of '7' is 10 x 2 pixels
    assert img[0:2, 0:10].all() and not img[0:2, 10:].any() and not img[14:].any()
    img = D.paint_list(np.zeros((6, 20, 3), np.uint8), [("text", 0, 0, "g", 3, 9, 9, 9)], font)             # y = 0: only the descender row
    assert img[0:3, 3:12].all() and not img[3:].any() and not img[:, 12:].any() and not img[:, :3].any()
    img = D.paint_list(np.zeros((9, 9, 3), np.uint8), [("text", 1, 8, "", 1, 9, 9, 9)], font)
    assert not img.any()


def test_the_case_tables_tell_every_likely_mistake_from_the_contract(font):
    """Every mutant of the painter differs from the painter on at least one case of the table the GPU test runs."""
    h, w = D.SIZES[-1]
    base = np.random.RandomState(0).randint(0, 256, (h, w, 3)).astype(np.uint8)
    lists = D.text_lists(h, w)
    want = {name: D.paint_list(base.copy(), prims, font) for name, prims in lists.items()}
    for name in D.NOTHING:
        assert np.array_equal(want[name], base), name
    assert all(not np.array_equal(img, base) for name, img in want.items() if name not in D.NOTHING)
    for mutant in D.MUTANTS:
        caught = [name for name, prims in lists.items() if not np.array_equal(D.paint_list(base.copy(), prims, font, mutant), want[name])]
        assert caught, mutant
    prims = D.batch_list(257, 16, 40)
    assert len(prims) == 257 and not np.array_equal(D.paint_list(base[:16, :40].copy(), prims, font, "earlier wins"),
                                                     D.paint_list(base[:16, :40].copy(), prims, font))


def test_pack_lays_the_runs_out_one_after_the_other():
    rows, pool = D.pack([("rect", 1, 2, 3, 4, -1, 5, 6, 7), ("text", 8, 9, "ab", 3, 0, 0, 255), ("text", 0, 0, "", 1, 0, 0, 0), ("text", 1, 1, "c", 2, 1, 0, 0)],
                        pool=b"xyz")
    assert rows == [(0, 1, 2, 3, 4, -1, 0, 5 | 6 << 8 | 7 << 16), (1, 8, 9, 3, 0, 3, 2, 255 << 16), (1, 0, 0, 1, 0, 5, 0, 0), (1, 1, 1, 2, 0, 5, 1, 1)]
    assert pool == b"xyzabc"


# ---- the library ---------------------------------------------------------------------------------------------------------------------------
def test_the_library_exports_both_entries_and_the_mirrors_match():
    declared = L.declared_symbols()
    lib = L.load_library()
    for name in ("radnet_draw_list_u8", "radnet_draw_glyph_rows"):
        assert name in declared and hasattr(lib, name)
    assert R.PRIM.itemsize == 32 and list(R.PRIM.names) == ["kind", "x1", "y1", "x2", "y2", "a", "b", "bgr"]
    assert all(R.PRIM[k] == np.int32 for k in R.PRIM.names)
    assert L.header_constant("RADNET_PRIM_RECT") == R.PRIM_RECT == D.PRIM_RECT == 0
    assert L.header_constant("RADNET_PRIM_TEXT") == R.PRIM_TEXT == D.PRIM_TEXT == 1
    assert L.header_constant("RADNET_DRAW_TEXT_MAX_SCALE") == 64
    assert L.header_constant("RADNET_DRAW_RECT_BATCH") == 256
    assert (R.FONT_CAP_ROWS, R.FONT_ADVANCE) == (D.CAP_ROWS, D.ADVANCE) == (7, 6)
