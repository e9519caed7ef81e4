"""Shared cases of the ordered draw list's tests (radnet_draw_list_u8).  Imports nothing from the product.
  paint_list(img, prims, font): the contract of include/radnet_hip.h as a plain loop over the list, written from the contract and
    not from the kernel: rectangles go through png_write_cases.paint, a text run is one boolean mask built dot by dot.  `font` maps a
    character code to its 8 row bytes (the tests read it through radnet_draw_glyph_rows).  `mutant` names one of MUTANTS, the
    mistakes a kernel is likely to make; the host test checks that the case tables tell every one of them from the contract.
  pack(prims): the list as rows of radnet_prim's eight integers plus the character pool.
  The case tables: text lists per image size, lists around the batch boundaries, the detections of the prediction maps.
A primitive is ("rect", x1, y1, x2, y2, thickness, b, g, r) or ("text", x, y, string, scale, b, g, r)."""
import numpy as np

import png_write_cases as W

FILLED = W.FILLED
WHITE, RED, BLUE, BLACK = W.WHITE, W.RED, W.BLUE, (0, 0, 0)
PRIM_RECT, PRIM_TEXT = 0, 1
COLS, ROWS, CAP_ROWS, ADVANCE = 5, 8, 7, 6
FIRST, LAST = 0x20, 0x7E
SIZES = [(1, 1), (3, 5), (9, 33), (67, 342)]        # (h, w); 9 x 33: one pixel past a tile of 8 rows x 32 columns in both directions
MUTANTS = ("gap column painted", "descender row dropped", "rows flipped", "character from dx / (5s)", "earlier wins")


def codes(text):
    return text if isinstance(text, bytes) else text.encode("ascii")


def text_mask(h, w, x, y, run, s, font, mutant=None):
    """The pixels a run paints: dot (c, r) of character k covers x + (6k + c) s .. + s - 1 by y - 7s + r s .. + s - 1."""
    def clip(lo, hi, n):
        return slice(min(max(lo, 0), n), min(max(hi + 1, 0), n))

    mask = np.zeros((h, w), bool)
    advance = 5 if mutant == "character from dx / (5s)" else ADVANCE
    for k, code in enumerate(codes(run)):
        rows = list(font[code])
        assert len(rows) == ROWS
        if mutant == "rows flipped":
            rows = rows[::-1]
        if mutant == "descender row dropped":
            rows[ROWS - 1] = 0
        for r in range(ROWS):
            dots = [(rows[r] >> (COLS - 1 - c)) & 1 for c in range(COLS)]
            if mutant == "gap column painted":
                dots.append(dots[-1])
            for c, dot in enumerate(dots):
                if dot:
                    px, py = x + (advance * k + c) * s, y - CAP_ROWS * s + r * s
                    mask[clip(py, py + s - 1, h), clip(px, px + s - 1, w)] = True
    return mask


def paint_list(img, prims, font, mutant=None):
    """radnet_draw_list_u8's contract on a [h][w][3] array, in place, entry by entry in list order."""
    h, w = img.shape[:2]
    for p in (list(prims)[::-1] if mutant == "earlier wins" else prims):
        if p[0] == "rect":
            W.paint(img, [tuple(p[1:])])
        else:
            _, x, y, run, s, b, g, r = p
            img[text_mask(h, w, x, y, run, s, font, mutant)] = (b, g, r)
    return img


def pack(prims, pool=b""):
    """(rows, pool): one (kind, x1, y1, x2, y2, a, b, bgr) per primitive; the runs are appended to `pool` one after the other."""
    rows, pool = [], bytearray(pool)
    for p in prims:
        if p[0] == "rect":
            _, x1, y1, x2, y2, t, b, g, r = p
            rows.append((PRIM_RECT, x1, y1, x2, y2, t, 0, b | g << 8 | r << 16))
        else:
            _, x, y, run, s, b, g, r = p
            rows.append((PRIM_TEXT, x, y, s, 0, len(pool), len(codes(run)), b | g << 8 | r << 16))
            pool += codes(run)
    return rows, bytes(pool)


def printable(n, start=0):
    """n printable codes, cycling through all of them but the space."""
    return bytes(0x21 + (start + i) % 94 for i in range(n))


ALL_CODES = bytes(range(FIRST, LAST + 1))
NOTHING = ("wholly outside", "n = 0", "far away")      # the lists that must leave the image as it was, at every size


def text_lists(h, w):
    """{name: prims} for an h x w image: each scale; a run wider than a tile and one wider than the image; a run clipped at each
    edge; runs wholly outside on each side (the nearest positions that paint nothing); only the descender row visible; an empty run;
    text and filled rectangles in both orders; two overlapping runs; coordinates at the ends of int32."""
    out = {}
    for s in (1, 2, 3, 7):
        out["scale %d" % s] = [("text", 2, 7 * s + 1, "boat: 97", s) + WHITE, ("text", w // 3, h // 2, "gy,;", s) + RED]
    out["wider than a tile"] = [("text", 1, 9, "a run of more than thirty-two pixels", 1) + BLUE]
    out["wider than the image"] = [("text", -21, h // 2 + 3, printable((w + 60) // 12 + 4), 2) + RED]
    out["clipped left"] = [("text", -7, 16, "clip", 2) + RED]
    out["clipped right"] = [("text", w - 9, 16, "clip", 2) + BLUE]
    out["clipped top"] = [("text", 5, 6, "Clip", 2) + WHITE]
    out["clipped bottom"] = [("text", 5, h + 4, "Clipg", 2) + RED]
    out["clipped all round"] = [("text", -9, h + 5, printable(w // 40 + 2, 30), 64) + BLUE]
    # "away" at scale 2 is (6 * 4 - 1) * 2 = 46 pixels wide and 16 high, its descender row is [y, y + 1]
    out["wholly outside"] = [("text", -46, 10, "away", 2) + RED, ("text", w, 10, "away", 2) + RED, ("text", 3, -2, "gway", 2) + RED,
                             ("text", 3, h + 14, "away", 2) + RED]
    out["one pixel inside"] = [("text", -45, 14, "awaM", 2) + RED, ("text", w - 1, 10, "Mway", 2) + BLUE, ("text", 3, -1, "gway", 2) + WHITE,
                               ("text", 3, h + 13, "Tway", 2) + RED]
    out["only the descender row"] = [("text", 1, 0, "gjpqy,", 3) + WHITE]
    out["n = 0"] = [("text", 3, 5, "", 2) + WHITE, ("text", 0, 0, b"", 64) + RED]
    out["text over a filled rectangle"] = [("rect", 2, 2, w - 3, h - 3, FILLED) + BLUE, ("text", 4, 12, "over", 1) + WHITE]
    out["a filled rectangle over text"] = [("text", 4, 12, "under", 1) + WHITE, ("rect", 9, 2, w // 2, 8, FILLED) + BLUE]
    out["outline over text over fill"] = [("rect", 0, 0, 40, 20, FILLED) + WHITE, ("text", 3, 17, "Mg", 2) + BLACK, ("rect", 6, 6, 30, 16, 3) + RED]
    out["overlapping runs"] = [("text", 3, 16, "first", 2) + RED, ("text", 5, 17, "second", 2) + BLUE]
    out["far away"] = [("text", -2 ** 31, 5, "far", 64) + RED, ("text", 2 ** 31 - 1, 2 ** 31 - 1, "far", 64) + RED, ("text", 3, -2 ** 31, "far", 64) + RED,
                       ("text", 2 ** 31 - 1, 5, "far", 1) + RED, ("text", 3, 2 ** 31 - 1, "far", 1) + RED]
    out["a run from the left end of int32"] = [("text", -2 ** 31, 5, "far", 1) + RED, ("text", 2, 8, "near", 1) + WHITE]
    return out


def batch_list(count, h, w, batch=256):
    """`count` entries on an h x w image (at least 16 x 40) of which the ones on both sides of every batch boundary cover the same
    pixels: around entry k * batch a filled rectangle, a run on it and another run on that, in colours that tell them apart; the rest
    is small rectangles and one-character runs all over the image."""
    rs = np.random.RandomState(count)
    prims = []
    for k in range(count):
        colour = (k % 251, (7 * k) % 256, 255 - k % 256)
        if k % 2:
            x, y = int(rs.randint(-3, w)), int(rs.randint(-3, h))
            prims.append(("rect", x, y, x + int(rs.randint(0, 9)), y + int(rs.randint(0, 5)), (1, FILLED, 2)[k % 3]) + colour)
        else:
            prims.append(("text", int(rs.randint(-3, w)), int(rs.randint(0, h + 8)), printable(1, k), 1 + k % 2) + colour)
    for edge in range(batch, count + 1, batch):
        for k, p in ((edge - 2, ("rect", 4, 2, 36, 14, FILLED) + RED), (edge - 1, ("text", 6, 12, "Wg#", 1) + WHITE), (edge, ("text", 7, 12, "M@y", 1) + BLUE),
                     (edge + 1, ("rect", 20, 0, 24, 15, 1) + BLACK)):
            if 0 <= k < count:
                prims[k] = p
    return prims


# ---- the detections of the prediction maps (those of tests/test_gpu_png_write.py) and their hand-built lists ------------------------------
DETS = [{'class': 'boat', 'prob': np.float32(0.91), 'x1': np.int64(10), 'y1': np.int64(20), 'x2': np.int64(70), 'y2': np.int64(60)},
        {'class': 'human', 'prob': 0.75, 'x1': 50, 'y1': 40, 'x2': 100, 'y2': 90},
        {'class': 'animal', 'prob': 0.25, 'x1': 90, 'y1': 5, 'x2': 126, 'y2': 45},
        {'class': 'wheel', 'prob': 1.0, 'x1': -4, 'y1': 70, 'x2': 30, 'y2': 99}]
LABELS = ["boat: 91", "human: 75", "animal: 25", "wheel: 100"]        # '{}: {}'.format(class, int(100 * prob))


def labelled(dets, labels, colour, scale=3, thickness=8):
    """predict.py:107-115 per detection, with the metrics of the issue: tw = (6 n - 1) scale, th = 7 scale, baseline = scale."""
    prims = []
    for d, label in zip(dets, labels):
        x1, y1, x2, y2 = int(d['x1']), int(d['y1']), int(d['x2']), int(d['y2'])
        tw, th, baseline = (6 * len(label) - 1) * scale, 7 * scale, scale
        prims.append(("rect", x1, y1, x2, y2, thickness) + tuple(colour))
        prims.append(("rect", x1 - 5, y1 + baseline - 5, x1 + tw + 5, y1 - th - 5, 1) + BLACK)
        prims.append(("rect", x1 - 5, y1 + baseline - 5, x1 + tw + 5, y1 - th - 5, FILLED) + WHITE)
        prims.append(("text", x1, y1, label, scale) + BLACK)
    return prims


def outlines(dets, colour, thickness=8):
    return [("rect", int(d['x1']), int(d['y1']), int(d['x2']), int(d['y2']), thickness) + tuple(colour) for d in dets]
