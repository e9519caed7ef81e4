"""The device-free half of the scene painter: the NumPy painter of draw_scene_cases has the properties the contract states and its
case tables catch the mistakes a kernel is likely to make; radnet_draw_scene_check refuses what it must, naming the entry;
RADNet.scene_table packs what the cases' own pack() packs; figures.precision_recall_scene lays out the figure; evaluate_scans with
pr_plot=True writes one more file.  No device needed."""
import copy
import json
import os

import numpy as np
import pytest

import draw_list_cases as D
import draw_scene_cases as S
from faster_rcnn import RADNet as R
from faster_rcnn import evaluate, figures, utils_io
from radnet_hip import lib as L

ERR_ARG = -1
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def font():
    return {code: L.glyph_rows(code) for code in range(D.FIRST, D.LAST + 1)}


def noise(h, w, seed=0):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


# ---- the painter's properties --------------------------------------------------------------------------------------------------------
def test_swapping_the_endpoints_gives_the_same_set():
    rs = np.random.RandomState(1)
    for _ in range(200):
        x1, x2 = (int(v) for v in rs.randint(-5, 45, 2))
        y1, y2 = (int(v) for v in rs.randint(-5, 25, 2))
        t, dash = int(rs.randint(1, 6)), (None, (1, 1), (3, 2))[int(rs.randint(0, 3))]
        assert np.array_equal(S.line_mask(20, 40, x1, y1, x2, y2, t, dash), S.line_mask(20, 40, x2, y2, x1, y1, t, dash)), (x1, y1, x2, y2, t, dash)


def test_a_thin_line_moves_at_most_one_minor_step_per_major_step():
    rs = np.random.RandomState(2)
    for _ in range(200):
        x1, x2 = (int(v) for v in rs.randint(0, 40, 2))
        y1, y2 = (int(v) for v in rs.randint(0, 20, 2))
        mask = S.line_mask(20, 40, x1, y1, x2, y2, 1)
        if abs(x2 - x1) < abs(y2 - y1):
            mask, (x1, y1, x2, y2) = mask.T, (y1, x1, y2, x2)
        cols = np.arange(min(x1, x2), max(x1, x2) + 1)
        assert (mask.sum(axis=0)[cols] == 1).all() and mask.sum() == len(cols)            # one pixel per major step, none elsewhere
        centres = mask.argmax(axis=0)[cols]
        assert (np.abs(np.diff(centres)) <= 1).all()
        lo, hi = (y1, y2) if x1 <= x2 else (y2, y1)
        assert centres[0] == lo and centres[-1] == hi                                     # it starts and ends on its endpoints


def test_an_exact_half_rounds_up():
    mask = S.line_mask(4, 4, 0, 0, 2, 1, 1)
    assert [tuple(p) for p in np.argwhere(mask)] == [(0, 0), (1, 1), (1, 2)]             # (y, x): at x = 1 the centre 0.5 becomes 1
    mask = S.line_mask(4, 4, 0, 2, 2, 1, 1)                                               # downhill: 1.5 becomes 2, the larger row again
    assert [tuple(p) for p in np.argwhere(mask)] == [(1, 2), (2, 0), (2, 1)]


def test_a_horizontal_line_is_the_filled_rectangle_of_height_one():
    for x1, x2, y in ((3, 30, 5), (30, 3, 0), (-4, 50, 19), (7, 7, 7)):
        want = D.paint_list(np.zeros((20, 40, 3), np.uint8), [("rect", x1, y, x2, y, D.FILLED, 255, 255, 255)], {})[:, :, 0] == 255
        assert np.array_equal(S.line_mask(20, 40, x1, y, x2, y, 1), want)
    for t in (1, 2, 3, 4, 5):                                                             # t rows: (t - 1) / 2 above, t / 2 below
        rows = np.flatnonzero(S.line_mask(20, 40, 3, 10, 30, 10, t).any(axis=1))
        assert rows.tolist() == list(range(10 - (t - 1) // 2, 10 + t // 2 + 1)) and len(rows) == t


def test_the_dash_phase_is_the_images():
    mask = S.line_mask(3, 40, 3, 1, 33, 1, 1, (3, 2))
    assert np.flatnonzero(mask[1]).tolist() == [x for x in range(3, 34) if x % 5 < 3]
    mask = S.line_mask(40, 3, 1, 33, 1, 4, 1, (7, 5))
    assert np.flatnonzero(mask[:, 1]).tolist() == [y for y in range(4, 34) if y % 12 < 7]


def test_discs_and_rings():
    assert np.argwhere(S.disc_mask(9, 9, 4, 5, 0, S.FILLED)).tolist() == [[5, 4]]
    assert S.disc_mask(9, 9, 4, 4, 1, S.FILLED).sum() == 9                                # dx^2 + dy^2 <= 2: the 3 x 3 block
    for r in (1, 2, 3, 7):
        ring = S.disc_mask(31, 31, 15, 15, r, 1)
        assert np.array_equal(ring, S.disc_mask(31, 31, 15, 15, r, S.FILLED) & ~S.disc_mask(31, 31, 15, 15, r - 1, S.FILLED))
        assert ring[15, 15 + r] and ring[15 - r, 15] and not ring[15, 15]
    assert np.array_equal(S.disc_mask(31, 31, 15, 15, 1, 5), S.disc_mask(31, 31, 15, 15, 3, S.FILLED))      # r - hw < 1: no hole
    assert np.array_equal(S.disc_mask(31, 31, 15, 15, 3, 2), S.disc_mask(31, 31, 15, 15, 4, S.FILLED) & ~S.disc_mask(31, 31, 15, 15, 1, S.FILLED))


def test_opaque_rectangles_and_text_equal_the_list_painter(font):
    import png_write_cases as W
    for h, w in D.SIZES:
        for name, prims in D.text_lists(h, w).items():
            assert np.array_equal(S.paint_scene(noise(h, w), prims, font), D.paint_list(noise(h, w), prims, font)), (h, w, name)
    for name, rects in W.rect_lists(70, 130).items():
        prims = [("rect",) + tuple(r) for r in rects]
        assert np.array_equal(S.paint_scene(noise(70, 130), prims, font), D.paint_list(noise(70, 130), prims, font)), name
    prims = D.batch_list(257, 20, 45)
    assert np.array_equal(S.paint_scene(noise(20, 45), prims, font), D.paint_list(noise(20, 45), prims, font))


def test_the_mixing_rule(font):
    img = noise(4, 4, 3)
    for tau in S.TAUS:
        got = S.paint_scene(img.copy(), [("rect", 0, 0, 3, 3, S.FILLED, 10, 200, 255, {"transparency": tau})], font)
        want = (np.array([10, 200, 255]) * (255 - tau) + img.astype(np.int64) * tau + 127) // 255
        assert np.array_equal(got, want)
    assert np.array_equal(S.paint_scene(img.copy(), [("rect", 0, 0, 3, 3, S.FILLED, 1, 2, 3, {"transparency": 255})], font), img)
    a, b = ("rect", 0, 0, 3, 3, S.FILLED) + S.RED + ({"transparency": 102},), ("disc", 1, 1, 2, S.FILLED) + S.BLUE + ({"transparency": 60},)
    assert not np.array_equal(S.paint_scene(img.copy(), [a, b], font), S.paint_scene(img.copy(), [b, a], font))      # the order shows


def test_the_nothing_lists_paint_nothing(font):
    for h, w in S.SIZES:
        for name, prims in S.nothing_lists(h, w).items():
            assert np.array_equal(S.paint_scene(noise(h, w), prims, font), noise(h, w)), (h, w, name)
        for name, prims in S.all_lists(h, w).items():
            if name not in S.nothing_lists(h, w) and (h, w) == S.SIZES[-1] and name != "tau 255":
                assert not np.array_equal(S.paint_scene(noise(h, w), prims, font), noise(h, w)), name


@pytest.mark.parametrize("mutant", S.MUTANTS)
def test_every_mutant_is_caught_by_some_case(font, mutant):
    assert len(S.MUTANTS) >= 5
    caught = []
    for h, w in S.SIZES[1:]:
        for name, prims in S.all_lists(h, w).items():
            if not np.array_equal(S.paint_scene(noise(h, w), prims, font), S.paint_scene(noise(h, w), prims, font, mutant=mutant)):
                caught.append((h, w, name))
    assert caught, mutant
    prims = S.batch_list(257, 20, 45)
    assert not np.array_equal(S.paint_scene(noise(20, 45), prims, font), S.paint_scene(noise(20, 45), prims, font, mutant="earlier wins"))


# ---- radnet_draw_scene_check ---------------------------------------------------------------------------------------------------------
def table_of(rows):
    return np.array([tuple(r) for r in rows], np.int32).reshape(-1, 8)


def test_the_check_accepts_the_case_tables(font):
    rows, pool, _ = S.refusals()
    assert L.draw_scene_check(table_of(rows), pool) == (0, -2, "")                         # nothing reported
    for h, w in S.SIZES:
        for name, prims in S.all_lists(h, w).items():
            r, p = S.pack(prims)
            assert L.draw_scene_check(table_of(r), p)[0] == 0, name
    for what, prims in S.accepted():
        r, p = S.pack(prims)
        assert L.draw_scene_check(table_of(r), p) == (0, -2, ""), what
    r, p = S.pack(S.batch_list(257, 20, 45))
    assert L.draw_scene_check(table_of(r), p)[0] == 0


def test_the_check_refuses_and_names_the_entry():
    rows, pool, cases = S.refusals()
    assert len(cases) >= 25
    for what, table, chars, entry in cases:
        rc, bad, msg = L.draw_scene_check(table_of(table), chars)
        assert rc == ERR_ARG and bad == entry and ("entry %d " % entry) in msg and msg.startswith("draw_scene: "), (what, bad, msg)
    # the first bad entry is the one named
    table = [list(r) for r in rows]
    table[4][5], table[2][5] = 0, 0
    assert L.draw_scene_check(table_of(table), pool)[1] == 2


def test_the_check_and_its_arguments():
    rows, pool, _ = S.refusals()
    t = table_of(rows)
    assert L.draw_scene_check(t, pool, count=0) == (0, -2, "")
    assert L.draw_scene_check(None, None, count=0) == (0, -2, "")
    assert L.draw_scene_check(None, pool, count=3)[:2] == (ERR_ARG, -1)
    assert L.draw_scene_check(t, pool, count=-1)[:2] == (ERR_ARG, -1)
    assert L.draw_scene_check(t, pool, n_chars=-1)[:2] == (ERR_ARG, -1)
    assert L.draw_scene_check(t, None, n_chars=7)[:2] == (ERR_ARG, -1)
    assert L.draw_scene_check(t, pool, n_chars=6)[:2] == (ERR_ARG, 5)                       # the last run no longer fits
    assert L.draw_scene_check(t[:1], None) == (0, -2, "")                                  # no text, no pool
    lib = L.load_library()                                                                 # null outputs are allowed
    bad = table_of(rows)
    bad[0, 5] = 0
    assert lib.radnet_draw_scene_check(bad.ctypes.data, len(bad), pool, len(pool), None, None, 0) == ERR_ARG
    import ctypes
    msg, index = ctypes.create_string_buffer(b"\xEE" * 12, 12), ctypes.c_int32(-9)
    assert lib.radnet_draw_scene_check(bad.ctypes.data, len(bad), pool, len(pool), ctypes.byref(index), msg, 8) == ERR_ARG
    assert index.value == 0 and msg.raw[:8] == b"draw_sc\0" and msg.raw[8:] == b"\xEE" * 4  # cut at msg_cap, nothing beyond it


def test_the_header_states_the_constants():
    assert L.header_constant("RADNET_PRIM_LINE") == S.PRIM_LINE == R.PRIM_LINE and L.header_constant("RADNET_PRIM_DISC") == S.PRIM_DISC == R.PRIM_DISC
    assert L.header_constant("RADNET_DRAW_SCENE_MAX_COORD") == S.MAX_COORD == 1 << 24
    lib = L.load_library()
    assert {"radnet_draw_scene_u8", "radnet_draw_scene_check", "radnet_grey3_u8"} <= set(L.declared_symbols())
    assert all(hasattr(lib, n) for n in ("radnet_draw_scene_u8", "radnet_draw_scene_check", "radnet_grey3_u8"))


# ---- RADNet.scene_table ----------------------------------------------------------------------------------------------------------------
def test_scene_table_packs_what_the_cases_pack():
    for prims in ([p for _, ps in sorted(S.all_lists(67, 342).items()) for p in ps], S.GOOD, S.batch_list(257, 20, 45)):
        table, chars = R.scene_table(prims)
        rows, pool = S.pack(prims)
        assert table.dtype == R.PRIM and table.view(np.int32).reshape(-1, 8).tolist() == [list(r) for r in rows] and chars.tobytes() == pool
    table, chars = R.scene_table([])
    assert len(table) == 0 and len(chars) == 0
    for bad, match in (([("circle", 1, 2, 3)], "entry 0"), ([S.GOOD[0], ("rect", 1, 1, 2, 2, 1, 0, 0, 0, {"dash": (1, 1)})], "entry 1"),
                       ([("line", 0, 0, 1, 1, 1, 0, 0, 0, {"dash": (0, 1)})], "dash"), ([("line", 0, 0, 1, 1, 1, 0, 0, 0, {"dash": (1, 65536)})], "dash"),
                       ([("disc", 0, 0, 1, 1, 0, 0, 0, {"transparency": 256})], "transparency"), ([("disc", 0, 0, 1, 1, 0, 0, 0, {"alpha": 1})], "options"),
                       ([("disc", 0, 0, 1, 1, 0, 0, 256)], "colour")):
        with pytest.raises(ValueError, match=match):
            R.scene_table(bad)


# ---- the precision/recall figure ---------------------------------------------------------------------------------------------------------
def golden_curves():
    with open(os.path.join(GOLD, "voc_ap.json")) as f:
        o = json.load(f)["objects"][0]
    curves = {key: evaluate.calc_class_ap(o["T"][key], o["P"][key]) for key in o["T"]}
    curves["an empty class"] = evaluate.calc_class_ap([], [])
    curves["one point"] = evaluate.calc_class_ap([1], [0.7])
    return curves


def on_canvas(p, n, font_scale):
    p, _ = S.split(p)
    if p[0] == "text":
        width = max(0, 6 * len(p[3]) - 1) * p[4]
        return p[4] == font_scale and 0 <= p[1] and p[1] + width <= n and 0 <= p[2] - 7 * p[4] and p[2] + p[4] <= n
    if p[0] == "line":
        return all(p[5] <= v < n - p[5] for v in p[1:5])
    return all(0 <= v < n for v in p[1:5])


@pytest.mark.parametrize("size", [1200, 300])
def test_precision_recall_scene(size):
    curves = golden_curves()
    assert len(curves) == 8 and all(len(c[2]) > 2 for k, c in curves.items() if k not in ("an empty class", "one point"))
    prims = figures.precision_recall_scene(curves, 0.123456, size)
    lay = figures.figure_layout(size)
    assert prims == figures.precision_recall_scene(copy.deepcopy(curves), 0.123456, size)      # a function of its arguments
    assert all(on_canvas(p, size, lay["scale"]) for p in prims), [p for p in prims if not on_canvas(p, size, lay["scale"])][:3]
    table, chars = R.scene_table(prims)
    assert L.draw_scene_check(table.view(np.int32).reshape(-1, 8), chars.tobytes())[0] == 0
    texts = [p[3] for p in prims if p[0] == "text"]
    keys = sorted(curves)
    assert texts.count("mAP: 12.35 %") == 1 and texts.count("Recall (TP / TP + FN)") == 1 and texts.count("Precision (TP / TP + FP)") == 1
    assert [t for t in texts if t[:3] in ("0.0", "0.2", "0.4", "0.6", "0.8", "1.0")] == [v for k in range(6) for v in ["%.1f" % (k / 5)] * 2]
    assert texts[-len(keys):] == [key + ": " + "{0:.2f}".format(100 * curves[key][0]) + " %" for key in keys]
    assert "an empty class: 0.00 %" in texts and len(set(texts[-len(keys):])) == len(keys)
    nx, ny = lay["x1"] - lay["x0"] + 1, lay["y1"] - lay["y0"] + 1
    assert ("rect", lay["x0"], lay["y0"], lay["x1"], lay["y1"], lay["frame"], 0, 0, 0) in prims

    def pixels(xs, ys):                                                                       # the issue's mapping, restated
        pts = [(lay["x0"] + int(np.floor(np.float64(x) * (nx - 1) + 0.5)), lay["y1"] - int(np.floor(np.float64(y) * (ny - 1) + 0.5))) for x, y in zip(xs, ys)]
        return [p for k, p in enumerate(pts) if k == 0 or p != pts[k - 1]]

    for k, key in enumerate(keys):
        colour = figures.COLOUR_CYCLE[k]
        mine = [p for p in prims if p[0] == "line" and tuple(S.split(p)[0][6:9]) == colour]
        solid, dashed = [p for p in mine if not S.split(p)[1]][:-1], [p for p in mine if S.split(p)[1]]      # the last solid one is the legend's sample
        assert all(S.split(p)[1] == {"dash": lay["dash"]} for p in dashed) and all(p[5] == lay["thickness"] for p in mine)
        ap, precision, recall, interp_precision, interp_recall = curves[key]
        for entries, xs, ys in ((solid, recall, precision), (dashed, interp_recall, interp_precision)):
            pts = pixels(xs, ys)
            if len(pts) == 0:
                assert entries == []
                continue
            chain = [tuple(entries[0][1:3])] + [tuple(e[3:5]) for e in entries]
            assert chain == (pts if len(pts) > 1 else pts * 2), key                          # one polyline, through every distinct pixel in order
            assert all(a != b for a, b in zip(entries[:-1], entries[1:]))
            assert len(pts) == 1 or all(e[1:3] != e[3:5] for e in entries)
    assert figures.COLOUR_CYCLE[0] == (0xb4, 0x77, 0x1f) and figures.COLOUR_CYCLE[9] == (0xcf, 0xbe, 0x17) and len(set(figures.COLOUR_CYCLE)) == 10


def test_the_scene_stays_short_for_a_pooled_test_set():
    rs = np.random.RandomState(5)
    curves = {}
    for k in range(12):                                                                       # more classes than colours: the cycle wraps
        n = 30000
        curves["class %02d" % k] = evaluate.calc_class_ap(list((rs.random_sample(n) < 0.6).astype(int)), list(rs.random_sample(n)))
    prims = figures.precision_recall_scene(curves, 0.5)
    # 30000 points per curve; from detection k on a step moves precision by less than 1 / k, under a pixel once k passes the 924 rows
    # of the axes, and recall never goes back: a few entries per pixel column, "a few thousand" per polyline instead of 30000
    assert len(prims) < 12 * 2 * 3000 and sum(p[0] == "line" for p in prims) > 12 * 100
    assert [S.split(p)[0][6:9] for p in prims if p[0] == "line"][-1] == figures.COLOUR_CYCLE[11 % 10]
    assert figures.precision_recall_scene({}, float("nan"), 300)[-1][0] == "rect"            # no class: the axes alone, no legend
    with pytest.raises(ValueError):
        figures.figure_layout(50)


def test_the_label_view_scenes():
    class C:
        anchor_box_scales, anchor_box_ratios, rpn_stride = [32, 64], [[1, 1], [1, 2], [2, 1]], 16
    A = 6
    regr = np.zeros((1, 5, 7, 8 * A))
    regr[0, 1, 2, 4 * 4:4 * 4 + 4] = 1                                                       # anchor 4: scale 64, ratio (1, 2), at row 1, column 2
    regr[0, 3, 0, 0:4] = 1                                                                   # anchor 0: scale 32, ratio (1, 1), at row 3, column 0
    regr[0, 1, 2, 4 * A + 3] = 0.25
    prims = figures.positive_anchor_scene([None, regr], C, 2)
    assert prims == [("disc", 32, 16, 3, -1, 227, 206, 166), ("rect", 32 - 32, 16 - 64, 32 + 32, 16 + 64, 2, 227, 206, 166),
                     ("disc", 0, 48, 3, -1, 138, 223, 178), ("rect", -16, 32, 16, 64, 2, 138, 223, 178)]
    assert figures.positive_anchor_scene([None, regr], C, 0) == []
    boxes = [{'x1': 3, 'y1': 4, 'x2': 30.9, 'y2': 20, 'class': 'boat'}, {'x1': 1, 'y1': 1, 'x2': 5, 'y2': 5}]
    assert figures.ground_truth_scene(boxes) == [("rect", 3, 4, 30, 20, 3, 28, 26, 227, {"transparency": 102}), ("rect", 1, 1, 5, 5, 3, 28, 26, 227, {"transparency": 102})]
    assert figures.ground_truth_scene(boxes[:1], alpha=1.0)[0][-1] == {"transparency": 0}
    with pytest.raises(ValueError):
        figures.ground_truth_scene(boxes, alpha=1.5)
    assert [c[0] for c in figures.COLORMAP][2] == (153, 154, 251) and len(figures.COLORMAP) == 5


# ---- evaluate_scans(pr_plot=True), the device work stubbed --------------------------------------------------------------------------------
import test_evaluate_scans_host as E      # noqa: E402  (its records, detections and stub network; nothing of it is changed)


def run_scans(tmp_path, monkeypatch, **kw):
    log = []
    monkeypatch.setattr(utils_io, "get_image", lambda path, types, random_type=False, to_host=True: ("map", path))
    monkeypatch.setattr(utils_io, "imwrite", lambda path, img, **k: log.append(("write", path, img, k)) or True)
    monkeypatch.setattr(figures, "precision_recall_figure", lambda curves, mAP, **k: log.append(("figure", curves, mAP, k)) or ("figure", sorted(curves)))
    return evaluate.evaluate_scans(E._Net([]), copy.deepcopy(E.RECORDS), str(tmp_path), **kw), log


def test_evaluate_scans_with_the_plot(tmp_path, monkeypatch):
    (accuracy, elapsed, paths), log = run_scans(tmp_path / "with", monkeypatch, pr_plot=True)
    (plain_accuracy, _, plain_paths), plain_log = run_scans(tmp_path / "plain", monkeypatch)
    assert [os.path.relpath(p, tmp_path / "with") for p in paths] == [os.path.relpath(p, tmp_path / "plain") for p in plain_paths] + [os.path.join("viz", "precision_recall.png")]
    assert os.path.isdir(tmp_path / "with" / "viz") and not os.path.exists(tmp_path / "plain" / "viz")
    assert [e[0] for e in plain_log] == ["write"] * 3 and [e[0] for e in log] == ["write"] * 3 + ["figure", "write"]
    assert log[-1][1:3] == (paths[-1], ("figure", ["animal", "boat", "human"]))
    # the same numbers as without the plot, and as the JSON: one matching of the pooled lists
    assert accuracy == plain_accuracy and all(type(v) is float for v in accuracy.values())
    assert (tmp_path / "with" / "test_accuracy.json").read_text() == (tmp_path / "plain" / "test_accuracy.json").read_text() == json.dumps(accuracy, indent=4)
    _, curves, mAP, kw = log[-2]
    assert list(curves) == ["animal", "boat", "human"] and float(mAP) == accuracy["mAP"] and kw == {}
    assert all(float(curves[k][0]) == accuracy[k] and len(curves[k]) == 5 for k in curves)
    assert sorted(os.listdir(tmp_path / "plain")) == ["test", "test_accuracy.json"] and sorted(os.listdir(tmp_path / "with")) == ["test", "test_accuracy.json", "viz"]
    (_, _, paths2), log2 = run_scans(tmp_path / "enc", monkeypatch, pr_plot=True, deflate="device", huffman="fixed")
    assert log2[-1][3] == dict(deflate="device", huffman="fixed") and log[-1][3] == {}
