"""The device-free half of the score-map pictures: radnet_heat_check accepts the case tables of tests/heat_cases.py and refuses one
table per bound, naming the entry and the field; RADNet.heat_table packs 32-byte entries; figures.heat_lut, figures.to_levels and
figures.score_map_scene; the placements of a scan are tile_windows' rectangles; and the case tables catch five mistakes a painter is
likely to make.  No device needed."""
import numpy as np
import pytest

import heat_cases as H
from faster_rcnn import RADNet as R
from faster_rcnn import figures
from radnet_hip import lib as L

ERR_ARG = -1


# ---- radnet_heat_check ------------------------------------------------------------------------------------------------------------------
def test_heat_check_accepts_the_case_tables():
    tables, pool = H.paint_tables()
    for (h, w) in H.SIZES:
        for name, places in tables.items():
            rc, bad, msg = L.heat_check(R.heat_table(places), len(pool), h, w)
            assert (rc, bad, msg) == (0, -2, ""), (name, msg)
    good, pool_len, _ = H.refused_tables()
    assert L.heat_check(R.heat_table(good), pool_len, 21, 37)[0] == 0                      # everything at its bound
    assert L.heat_check(None, 0, 1, 1) == (0, -2, "")                                       # count 0: a valid no-op
    assert L.heat_check(R.heat_table(good), pool_len, 21, 37, count=0)[0] == 0


def test_heat_check_refuses_one_table_per_bound():
    good, pool_len, cases = H.refused_tables()
    assert len({field for _, _, _, _, _, _, field in cases}) == 7                           # every field of a placement
    for what, places, n, h, w, entry, field in cases:
        rc, bad, msg = L.heat_check(R.heat_table(places), n, h, w)
        assert rc == ERR_ARG and bad == entry, (what, rc, bad, msg)
        assert ("entry %d " % entry) in msg and (" %s = " % field) in msg, (what, msg)
    table = R.heat_table(good)
    for what, args, kw in (("a negative count", (table, pool_len, 21, 37), dict(count=-1)), ("a null table", (None, pool_len, 21, 37), dict(count=2)),
                           ("a negative pool", (table, -1, 21, 37), {}), ("h = 0", (table, pool_len, 0, 37), {}), ("w = 0", (table, pool_len, 21, 0), {})):
        rc, bad, msg = L.heat_check(*args, **kw)
        assert rc == ERR_ARG and bad == -1 and msg, what
    first_bad = [list(r) for r in good]
    first_bad[1][4], first_bad[2][2] = 0, 0                                                 # the first bad entry is the one named
    assert L.heat_check(R.heat_table(first_bad), pool_len, 21, 37)[1] == 1


def test_heat_table_packs_32_byte_entries():
    assert R.HEAT_PLACE.itemsize == 32 and R.HEAT_PLACE.fields["offset"][1] == 24
    t = R.heat_table([(-7, 4, 15, 9, 5, 4, 2 ** 40 + 3), (1, 2, 3, 4, 5, 6, 7)])
    assert t.shape == (2,) and t.view(np.uint8).size == 64
    assert t.view(np.int32).reshape(2, 8)[:, :6].tolist() == [[-7, 4, 15, 9, 5, 4], [1, 2, 3, 4, 5, 6]]
    assert t.view(np.int64).reshape(2, 4)[:, 3].tolist() == [2 ** 40 + 3, 7]
    assert R.heat_table([]).shape == (0,)
    with pytest.raises(ValueError, match="entry 1 "):
        R.heat_table([(1, 2, 3, 4, 5, 6, 7), (1, 2, 3, 4, 5, 6)])


# ---- the colour table and the level rule ---------------------------------------------------------------------------------------------------
def luma(c):
    return 1868 * int(c[0]) + 9617 * int(c[1]) + 4899 * int(c[2])


def test_heat_lut():
    grey = figures.heat_lut([(0, 0, 0, 0), (255, 255, 255, 255)])
    assert grey.dtype == np.uint8 and grey.tolist() == [[i, i, i] for i in range(256)]
    lut = figures.heat_lut()
    assert lut.dtype == np.uint8 and lut.shape == (256, 3)
    anchors = figures.HEAT_ANCHORS
    assert [tuple(lut[a[0]]) for a in anchors] == [tuple(a[1:]) for a in anchors]
    lumas = [luma(lut[a[0]]) for a in anchors]
    assert all(b > a for a, b in zip(lumas[:-1], lumas[1:])), lumas
    two = figures.heat_lut([(0, 10, 0, 200), (4, 20, 3, 100), (255, 20, 3, 100)])           # the rounding of the integer rule
    assert two[:5].tolist() == [[10, 0, 200], [(10 * 3 + 20 + 2) // 4, (3 + 2) // 4, (600 + 100 + 2) // 4], [15, 2, 150], [(10 + 60 + 2) // 4, (9 + 2) // 4, (200 + 300 + 2) // 4],
                                [20, 3, 100]]
    for bad in ([(0, 0, 0, 0)], [(1, 0, 0, 0), (255, 1, 1, 1)], [(0, 0, 0, 0), (254, 1, 1, 1)], [(0, 0, 0, 0), (9, 1, 1, 1), (9, 2, 2, 2), (255, 3, 3, 3)],
                [(0, 0, 0, 0), (255, 256, 0, 0)]):
        with pytest.raises(ValueError):
            figures.heat_lut(bad)


def test_to_levels_is_the_level_rule_of_the_cases():
    for M, first, count, outside in H.level_cases():
        pred = H.level_case(M, first, count, np.inf if outside == "inf" else np.nan)
        with np.errstate(invalid="ignore"):
            s = np.fmax.reduce(pred[:, first:first + count], axis=1)
        got = figures.to_levels(s)
        assert got.dtype == np.uint8 and np.array_equal(got, H.levels(pred, H.LEVEL_LD, M, first, count)), (M, first, count, outside)
    k = np.arange(256)
    assert np.array_equal(figures.to_levels(k / 255.0), k) and np.array_equal(figures.to_levels((k + 0.499) / 255.0), k)
    assert figures.to_levels([np.nan, np.inf, -np.inf, -0.0, 2.0, 0.5 / 255 - 1e-6, 0.5 / 255 + 1e-6]).tolist() == [0, 255, 0, 0, 255, 0, 1]
    assert figures.to_levels(np.zeros((3, 4))).shape == (3, 4)


def test_the_level_cases_hold_what_they_promise():
    seen = set()
    for M, first, count, outside in H.level_cases():
        pred = H.level_case(M, first, count, np.inf if outside == "inf" else np.nan)
        win = pred[:, first:first + count]
        rest = np.delete(pred, np.arange(first, first + count), axis=1)
        assert (np.isposinf(rest) if outside == "inf" else np.isnan(rest)).all() and rest.size
        want = H.levels(pred, H.LEVEL_LD, M, first, count)
        if M > 1:
            assert np.isnan(win[M // 2]).all() and want[M // 2] == 0
        if M == 1000:
            assert np.isnan(win).any() and np.isposinf(win).any() and np.isneginf(win).any() and (win < 0).any() and (win > 1).any()
            seen.update(want.tolist())
    assert {0, 1, 254, 255} <= seen and len(seen) > 200


# ---- the placements of a scan -----------------------------------------------------------------------------------------------------------------
def test_the_placements_of_a_scan_are_the_windows_of_predict():
    class C:
        max_n_tiles_train, tile_size, tile_overlap, include_full_img = 1, 400, 250, True
    img = np.zeros((700, 900, 3), np.uint8)
    work, offs = R.tile_windows(img, C)
    sizes = [(19, 19)] * 9 + [(19, 25)]
    places, total = R.score_map_places(work, sizes)
    assert [p[:4] for p in places[:9]] == [(x0, y0, 400, 400) for y0 in (0, 250, 300) for x0 in (0, 250, 500)] and places[9][:4] == (0, 0, 900, 700)
    assert [p[:2] for p in places] == offs and [p[:4] for p in places] == [(win.x0, win.y0, win.ww, win.wh) for win in work]
    assert [p[4:6] for p in places] == [(19, 19)] * 9 + [(25, 19)]                           # (mw, mh): columns first
    assert [p[6] for p in places] == [361 * k for k in range(10)] and total == 9 * 361 + 19 * 25
    assert L.heat_check(R.heat_table(places), total, 700, 900)[0] == 0
    maps = R.ScoreMaps(np.arange(total, dtype=np.int64).astype(np.uint8), places, (700, 900))
    assert maps.shape == (700, 900) and maps.places == places
    C.include_full_img = False
    assert R.score_map_places(R.tile_windows(img, C)[0], sizes[:9]) == (places[:9], 9 * 361)


# ---- the figure's layout ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (38, 63), (63, 38)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("size", [600, 300, 1200])
def test_score_map_scene_keeps_the_aspect_ratio_inside_the_canvas(shape, size):
    mh, mw = shape
    scene = figures.score_map_scene(shape, "anchor 7", size)
    x0, y0, w, h = scene["map"]
    bx0, by0, bw, bh = scene["bar"]
    assert scene["size"] == size and w >= 1 and h >= 1
    assert abs(w * mh - h * mw) <= max(mw, mh)                                              # w / h = mw / mh up to one pixel's rounding
    assert max(w, h) >= size // 2                                                            # and it fills the axes area along one side
    assert 0 < x0 and x0 + w < bx0 and bx0 + bw < size and 0 < y0 and y0 + h < size and (by0, bh) == (y0, h)
    table, chars = R.scene_table(scene["prims"])
    assert L.draw_scene_check(table, bytes(chars))[0] == 0
    for p in scene["prims"]:                                                                 # nothing leaves the canvas
        if p[0] in ("rect", "line"):
            assert 0 <= min(p[1], p[3]) and max(p[1], p[3]) < size and 0 <= min(p[2], p[4]) and max(p[2], p[4]) < size, p
        else:
            (tw, th), base = R.text_size(p[3], p[4])
            assert p[0] == "text" and 0 <= p[1] and p[1] + tw <= size and 0 <= p[2] - th and p[2] + base <= size, p
    labels = [p[3] for p in scene["prims"] if p[0] == "text"]
    assert labels == ["0.0", "0.2", "0.4", "0.6", "0.8", "1.0", "anchor 7"]
    ticks = [p for p in scene["prims"] if p[0] == "line"]
    assert ticks[0][2] == y0 + h - 1 and ticks[-1][2] == y0                                  # 0.0 at the bar's bottom row, 1.0 at its top
    assert [p[3] for p in figures.score_map_scene(shape, "", size)["prims"] if p[0] == "text"] == labels[:-1]


def test_score_map_scene_refuses_what_it_cannot_lay_out():
    for shape, size in (((0, 3), 600), ((3, 0), 600), ((3, 3), 100)):
        with pytest.raises(ValueError):
            figures.score_map_scene(shape, "", size)


# ---- the cases catch a wrong painter ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", H.MUTANTS)
def test_a_mutant_painter_is_caught(mutant):
    tables, pool = H.paint_tables()
    luts = H.luts()
    caught = []
    for (h, w), name, tau, min_level, lut in H.paint_cases():
        buf = H.canvas(h, w, seed=h)
        want = H.expected(buf, h, w, pool, tables[name], luts[lut], tau, min_level)
        if not np.array_equal(H.expected(buf, h, w, pool, tables[name], luts[lut], tau, min_level, mutant), want):
            caught.append(name)
            if len(set(caught)) >= 2:
                break
    assert caught, mutant


def test_the_painter_has_the_properties_the_contract_states():
    tables, pool = H.paint_tables()
    luts = H.luts()
    h, w = H.SIZES[0]
    buf = H.canvas(h, w, seed=1)
    for name, places in tables.items():
        for tau, min_level in ((0, 0), (102, 1), (255, 0)):
            want = H.expected(buf, h, w, pool, places, luts["random"], tau, min_level)
            assert np.array_equal(want[:, 3 * w:], buf[:, 3 * w:])                          # the padding stays
            assert np.array_equal(H.expected(buf, h, w, pool, places[::-1], luts["random"], tau, min_level), want), name      # order-free
            if tau == 255 or name in ("none", "wholly outside"):
                assert np.array_equal(want, buf), (name, tau)
            elif tau == 0 and min_level == 0:
                assert not np.array_equal(want, buf), name
    # min_level 255 keeps only the cells at 255; 0 keeps every held pixel
    places = tables["two: 5x4 and 1x1"]
    img = H.paint(np.zeros((h, w, 3), np.uint8), pool, places, luts["grey"] | 1, 0, 0)
    assert int((img[:, :, 0] > 0).sum()) == 20 * 10 + 8 * 6
    cells = pool[places[0][6]:places[0][6] + 20].reshape(4, 5)
    img = H.paint(np.zeros((h, w, 3), np.uint8), pool, places[:1], luts["grey"], 0, 255)
    rows_per_cell = np.bincount((np.arange(10) * 4) // 10, minlength=4)                      # 10 rows over 4 cells: 3, 2, 3, 2
    assert rows_per_cell.tolist() == [3, 2, 3, 2]
    assert int((img[:, :, 0] == 255).sum()) == int(((cells == 255) * rows_per_cell[:, None]).sum()) * 4
    assert set(np.unique(img)) <= {0, 255}
