"""Shared cases of the scene painter's tests (radnet_draw_scene_u8).  Imports nothing from the product.
  paint_scene(img, prims, font): the contract of include/radnet_hip.h as a plain loop over the list, written from the contract and not
    from the kernel: every entry is one boolean mask over the whole image (NumPy int64 and floor division), mixed into the running
    image.  `mutant` names one of MUTANTS, the mistakes a kernel is likely to make; the host test checks that the case tables tell
    every one of them from the contract.
  pack(prims): the list as rows of radnet_prim's eight int32 plus the character pool.
  The case tables: lines, discs, transparency, lists around the batch boundaries, the lists that paint nothing, the refusals.
A primitive is draw_list_cases' ("rect", x1, y1, x2, y2, thickness, b, g, r) or ("text", x, y, string, scale, b, g, r), or
("line", x1, y1, x2, y2, t, b, g, r) or ("disc", cx, cy, radius, t, b, g, r); each may end in a dict {"dash": (on, off),
"transparency": 0..255}."""
import numpy as np

import draw_list_cases as D

FILLED = D.FILLED
WHITE, RED, BLUE, BLACK, GREEN = D.WHITE, D.RED, D.BLUE, D.BLACK, (40, 200, 60)
PRIM_RECT, PRIM_TEXT, PRIM_LINE, PRIM_DISC = 0, 1, 2, 3
MAX_COORD = 1 << 24
SIZES = [(1, 1), (7, 31), (9, 33), (67, 342)]       # (h, w); 7 x 31 and 9 x 33: one pixel short of and past a tile of 8 rows x 32 columns
TAUS = [0, 1, 102, 254, 255]
MUTANTS = ("rounds half down", "dash phase from the segment start", "d2 <= r2", "blends with the original pixel", "earlier wins")


def split(p):
    """(the primitive without its options, the options)."""
    return (tuple(p[:-1]), p[-1]) if isinstance(p[-1], dict) else (tuple(p), {})


def rect_mask(h, w, x1, y1, x2, y2, t):
    ys, xs = np.arange(h, dtype=np.int64)[:, None], np.arange(w, dtype=np.int64)[None, :]
    x1, x2, y1, y2 = min(x1, x2), max(x1, x2), min(y1, y2), max(y1, y2)
    hw = t // 2 if t > 0 else 0
    mask = (xs >= x1 - hw) & (xs <= x2 + hw) & (ys >= y1 - hw) & (ys <= y2 + hw)
    if t > 0:
        mask &= ~((xs > x1 + hw) & (xs < x2 - hw) & (ys > y1 + hw) & (ys < y2 - hw))
    return mask


def line_mask(h, w, x1, y1, x2, y2, t, dash=None, mutant=None):
    """x-major when |dx| >= |dy|; the y-major case is the x-major one of the transposed image."""
    if abs(x2 - x1) < abs(y2 - y1):
        return line_mask(w, h, y1, x1, y2, x2, t, dash, mutant).T
    (xa, ya), (xb, yb) = sorted([(x1, y1), (x2, y2)])[:2] if x1 != x2 else ((x1, y1), (x2, y2))
    ys, xs = np.arange(h, dtype=np.int64)[:, None], np.arange(w, dtype=np.int64)[None, :]
    if xa == xb:
        yc = np.full((1, w), ya, np.int64)
    else:
        num = 2 * (xs - xa) * (yb - ya) + (xb - xa)
        if mutant == "rounds half down":
            num = num - 1
        yc = ya + num // (2 * (xb - xa))                # NumPy's // is floor division
    mask = (xs >= xa) & (xs <= xb) & (ys >= yc - (t - 1) // 2) & (ys <= yc + t // 2)
    if dash is not None:
        on, off = dash
        phase = (xs - xa if mutant == "dash phase from the segment start" else xs) % (on + off)      # NumPy's % is floormod
        mask &= phase < on
    return mask


def disc_mask(h, w, cx, cy, r, t, mutant=None):
    ys, xs = np.arange(h, dtype=np.int64)[:, None], np.arange(w, dtype=np.int64)[None, :]
    d2 = (xs - cx) ** 2 + (ys - cy) ** 2

    def inside(rho):
        return d2 <= (rho * rho if mutant == "d2 <= r2" else rho * rho + rho)

    if t < 0:
        return inside(r)
    hw = t // 2
    return inside(r + hw) & ~inside(r - hw - 1) if r - hw >= 1 else inside(r + hw)


def mask_of(h, w, p, font, mutant=None):
    p, opts = split(p)
    if p[0] == "rect":
        return rect_mask(h, w, *p[1:6])
    if p[0] == "text":
        return D.text_mask(h, w, p[1], p[2], p[3], p[4], font)
    if p[0] == "line":
        return line_mask(h, w, *p[1:6], dash=opts.get("dash"), mutant=mutant)
    assert p[0] == "disc", p
    return disc_mask(h, w, *p[1:5], mutant=mutant)


def paint_scene(img, prims, font, mutant=None):
    """radnet_draw_scene_u8's contract on a [h][w][3] array, in place, entry by entry in list order."""
    h, w = img.shape[:2]
    original = img.copy()
    for p in (list(prims)[::-1] if mutant == "earlier wins" else prims):
        mask = mask_of(h, w, p, font, mutant)
        q, opts = split(p)
        tau = opts.get("transparency", 0)
        c = np.array(q[-3:], np.int64)
        d = (original if mutant == "blends with the original pixel" else img)[mask].astype(np.int64)
        img[mask] = ((c * (255 - tau) + d * tau + 127) // 255).astype(np.uint8)
    return img


def int32(v):
    return v - (1 << 32) if v >= 1 << 31 else v


def pack(prims, pool=b""):
    """(rows, pool): one (kind, x1, y1, x2, y2, a, b, bgr) per primitive, every value an int32."""
    rows, pool = [], bytearray(pool)
    for p in prims:
        p, opts = split(p)
        b, g, r = p[-3:]
        bgr = int32(b | g << 8 | r << 16 | opts.get("transparency", 0) << 24)
        if p[0] == "rect":
            rows.append((PRIM_RECT,) + p[1:6] + (0, bgr))
        elif p[0] == "text":
            run = D.codes(p[3])
            rows.append((PRIM_TEXT, p[1], p[2], p[4], 0, len(pool), len(run), bgr))
            pool += run
        elif p[0] == "line":
            on, off = opts.get("dash", (0, 0))
            rows.append((PRIM_LINE,) + p[1:6] + (int32(on | off << 16), bgr))
        else:
            rows.append((PRIM_DISC, p[1], p[2], p[3], 0, p[4], 0, bgr))
    return rows, bytes(pool)


# ---- lines -----------------------------------------------------------------------------------------------------------------------------
def line_lists(h, w):
    """{name: prims} for an h x w image."""
    out = {}
    out["horizontal"] = [("line", 2, h // 2, w - 3, h // 2, 1) + WHITE]
    out["vertical"] = [("line", w // 2, 1, w // 2, h - 2, 1) + RED]
    out["diagonal down"] = [("line", 1, 1, 1 + min(h, w), 1 + min(h, w), 1) + BLUE]
    out["diagonal up"] = [("line", 0, h - 1, h - 1, 0, 1) + WHITE, ("line", w - 1, h - 1, w - h, 0, 2) + RED]
    out["shallow"] = [("line", 0, 2, w - 1, 2 + h // 3, 1) + RED, ("line", 3, h - 2, w - 2, h - 2 - h // 5, 1) + BLUE]
    out["steep"] = [("line", 3, 0, 3 + h // 4, h - 1, 1) + WHITE, ("line", w // 2, h - 1, w // 2 - h // 3, 0, 1) + RED]
    out["exact halves"] = [("line", 4, 4, 14, 9, 1) + WHITE, ("line", 4, 20, 14, 15, 1) + RED, ("line", 30, 2, 35, 12, 1) + BLUE,
                           ("line", 40, 12, 45, 2, 2) + WHITE, ("line", 0, 0, 2, 1, 1) + RED]
    out["reversed"] = [("line", w - 1, 2 + h // 3, 0, 2, 1) + RED, ("line", 3 + h // 4, h - 1, 3, 0, 1) + WHITE]
    out["a point"] = [("line", w // 2, h // 2, w // 2, h // 2, 1) + WHITE, ("line", 0, 0, 0, 0, 4) + RED, ("line", w - 1, h - 1, w - 1, h - 1, 5) + BLUE]
    for t in (1, 2, 3, 4, 5):
        out["thickness %d" % t] = [("line", 2, 3, w - 5, h - 4, t) + WHITE, ("line", w // 3, 0, w // 3 + 2, h - 1, t) + RED,
                                   ("line", 1, h // 2, w - 2, h // 2, t) + BLUE, ("line", w - 4, h - 2, w - 4, 1, t) + GREEN]
    for on, off in ((1, 1), (3, 2), (7, 5)):            # across the tile edges at x = 32, 64, ... and y = 8, 16, ...
        dash = {"dash": (on, off)}
        out["dash %d %d" % (on, off)] = [("line", 1, 5, w - 2, 5, 1) + WHITE + (dash,), ("line", 30, 1, 30, h - 1, 2) + RED + (dash,),
                                         ("line", 2, 2, w - 3, h - 2, 3) + BLUE + (dash,), ("line", w // 2, h - 1, w // 2 + h // 2, 0, 1) + GREEN + (dash,)]
    # two pieces of one dashed polyline meet at (40, 9): the phase is the image's, not the piece's
    out["dashed polyline"] = [("line", 3, 3, 40, 9, 1) + WHITE + ({"dash": (3, 2)},), ("line", 40, 9, 90, 4, 1) + WHITE + ({"dash": (3, 2)},)]
    out["a dash with bit 31"] = [("line", 0, 1, w - 1, 1, 1) + RED + ({"dash": (2, 0x8001)},)]
    out["partly off"] = [("line", -9, -4, w // 2, h // 2, 2) + WHITE, ("line", w - 4, h // 2, w + 30, h + 11, 3) + RED,
                         ("line", -5, h - 1, w + 5, h - 1, 5) + BLUE, ("line", 0, -40, 2, h + 40, 1) + GREEN]
    out["ends at the bound"] = [("line", -MAX_COORD, -MAX_COORD, MAX_COORD, MAX_COORD, 3) + WHITE, ("line", MAX_COORD, 5, -MAX_COORD, h - 3, 2) + RED,
                                ("line", 3, MAX_COORD, w // 2, -MAX_COORD, 1) + BLUE + ({"dash": (3, 2)},),
                                ("line", -MAX_COORD, h // 2, MAX_COORD, h // 2, 1) + GREEN + ({"dash": (7, 5)},),
                                ("line", MAX_COORD, MAX_COORD, MAX_COORD, MAX_COORD, 5) + RED]
    return out


# ---- discs -----------------------------------------------------------------------------------------------------------------------------
def disc_lists(h, w):
    out = {}
    for r in (0, 1, 3, 40):
        out["filled %d" % r] = [("disc", w // 2, h // 2, r, FILLED) + WHITE, ("disc", 2, 3, r, FILLED) + RED]
        for t in (1, 2, 5):                             # r = 0 and 1 at t = 5, r = 0 at t = 2: r - hw < 1, no hole
            out["ring %d of %d" % (r, t)] = [("disc", w // 2, h // 2, r, t) + BLUE, ("disc", w - 3, 1, r, t) + RED]
    out["centre off the image"] = [("disc", -2, -1, 3, FILLED) + WHITE, ("disc", w + 1, h // 2, 3, 2) + RED, ("disc", w // 2, h + 38, 40, 1) + BLUE,
                                   ("disc", -100, h // 2, 102, 5) + GREEN]
    out["ring around a disc"] = [("disc", 20, 4, 3, FILLED) + RED, ("disc", 20, 4, 5, 1) + WHITE, ("disc", 20, 4, 3, 1) + BLUE]
    out["at the bound"] = [("disc", 0, 0, MAX_COORD, 1) + RED, ("disc", MAX_COORD, 3, MAX_COORD, 5) + WHITE, ("disc", -MAX_COORD, -MAX_COORD, 0, FILLED) + BLUE]
    return out


# ---- transparency ----------------------------------------------------------------------------------------------------------------------
def translucent_lists(h, w):
    out = {}
    for tau in TAUS:
        o = {"transparency": tau}
        out["tau %d" % tau] = [("rect", 1, 1, w - 2, h - 2, 3) + RED + (o,), ("line", 0, 0, w - 1, h - 1, 2) + WHITE + (o,),
                               ("disc", w // 3, h // 2, 3, FILLED) + BLUE + (o,), ("text", 2, 8, "tau", 1) + GREEN + (o,)]
    out["three kinds overlapping"] = [("rect", 2, 1, 40, 7, FILLED) + RED + ({"transparency": 102},),
                                      ("disc", 12, 4, 6, FILLED) + BLUE + ({"transparency": 60},),
                                      ("line", 0, 4, 44, 5, 3) + WHITE + ({"transparency": 200},)]
    out["opaque under translucent"] = [("rect", 0, 0, 20, 6, FILLED) + WHITE, ("disc", 10, 3, 5, FILLED) + BLACK + ({"transparency": 128},),
                                       ("text", 1, 7, "Mg", 1) + RED + ({"transparency": 30},)]
    out["translucent under opaque"] = [("disc", 10, 3, 5, FILLED) + BLACK + ({"transparency": 128},), ("line", 0, 3, 25, 3, 1) + GREEN]
    return out


def nothing_lists(h, w):
    """The lists that must leave the image as it was, at every size."""
    return {"no entries": [],
            "lines wholly outside": [("line", -10, -5, -1, -1, 1) + RED, ("line", w, 0, w + 5, h, 1) + RED, ("line", -3, -1, w + 3, -1, 1) + RED,
                                     ("line", -3, h, w + 3, h, 1) + RED, ("line", 0, -2, w, -2, 2) + RED, ("line", -2, 0, -2, h, 3) + RED,
                                     ("line", w + 2, -5, w + 2, h + 5, 4) + RED + ({"dash": (1, 1)},)],
            "discs wholly outside": [("disc", -5, -5, 3, FILLED) + RED, ("disc", -4, 0, 3, FILLED) + RED, ("disc", w + 3, h - 1, 3, 1) + RED,
                                     ("disc", w // 2, h // 2, 2000, 1) + RED, ("disc", w // 2, h // 2, 3000, 5) + RED + ({"transparency": 9},)],
            "far away": [("line", MAX_COORD, MAX_COORD, MAX_COORD - 9, MAX_COORD, 5) + RED, ("disc", -MAX_COORD, 0, 77, 3) + RED,
                         ("line", -MAX_COORD, -MAX_COORD, -MAX_COORD, MAX_COORD, 1) + RED]}


def all_lists(h, w):
    out = {}
    for table in (line_lists, disc_lists, translucent_lists, nothing_lists):
        out.update(table(h, w))
    return out


def batch_list(count, h, w, batch=256):
    """`count` entries of all four kinds on an h x w image (at least 16 x 40), a third of them translucent; the entries on both sides
    of every batch boundary cover the same pixels and mix, so an order lost at the boundary shows."""
    rs = np.random.RandomState(count)
    prims = []
    for k in range(count):
        colour = (k % 251, (7 * k) % 256, 255 - k % 256)
        o = ({"transparency": (60, 102, 200)[k % 9 // 3]},) if k % 3 == 0 else ()
        x, y = int(rs.randint(-3, w)), int(rs.randint(-3, h))
        if k % 4 == 0:
            prims.append(("rect", x, y, x + int(rs.randint(0, 9)), y + int(rs.randint(0, 5)), (1, FILLED, 2)[k % 3]) + colour + o)
        elif k % 4 == 1:
            prims.append(("text", x, y + 5, D.printable(1, k).decode("ascii"), 1 + k % 2) + colour + o)
        elif k % 4 == 2:
            dash = {"dash": (2, 1)} if k % 8 == 2 else {}
            dash.update(o[0] if o else {})
            prims.append(("line", x, y, x + int(rs.randint(-9, 10)), y + int(rs.randint(-6, 7)), 1 + k % 3) + colour + ((dash,) if dash else ()))
        else:
            prims.append(("disc", x, y, int(rs.randint(0, 5)), (FILLED, 1, 2)[k % 3]) + colour + o)
    for edge in range(batch, count + 1, batch):
        for k, p in ((edge - 2, ("rect", 4, 2, 36, 14, FILLED) + RED + ({"transparency": 90},)), (edge - 1, ("disc", 14, 8, 7, FILLED) + WHITE + ({"transparency": 120},)),
                     (edge, ("line", 2, 8, 38, 9, 3) + BLUE + ({"transparency": 150},)), (edge + 1, ("text", 7, 12, "M@y", 1) + BLACK + ({"transparency": 40},))):
            if 0 <= k < count:
                prims[k] = p
    return prims


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
GOOD = [("rect", 2, 2, 9, 9, 8, 1, 2, 3), ("text", 3, 12, "ok: 1", 1, 255, 0, 255), ("line", 1, 1, 20, 9, 2, 9, 9, 9, {"dash": (3, 2)}),
        ("disc", 8, 8, 4, FILLED, 0, 0, 0), ("disc", 15, 10, 5, 2, 7, 7, 7, {"transparency": 99}), ("text", 1, 18, "gy", 1, 9, 9, 9)]
FIELDS = ("kind", "x1", "y1", "x2", "y2", "a", "b", "bgr")
BEYOND = MAX_COORD + 1


def refusals():
    """(rows, pool, [(what, table, pool, the entry the message must name)]) on GOOD: every table is refused, `rows` itself is not."""
    rows, pool = pack(GOOD)
    assert rows[1][5:7] == (0, 5) and rows[5][5:7] == (5, 2) and len(pool) == 7

    def entry(i, **fields):
        t = [list(r) for r in rows]
        for k, v in fields.items():
            t[i][FIELDS.index(k)] = v
        return t

    def byte(k, v):
        p = bytearray(pool)
        p[k] = v
        return bytes(p)

    cases = [("an unknown kind", entry(3, kind=4), pool, 3), ("a negative kind", entry(0, kind=-1), pool, 0), ("a rectangle of thickness 0", entry(0, a=0), pool, 0),
             ("scale 0", entry(1, x2=0), pool, 1), ("scale 65", entry(5, x2=65), pool, 5), ("y2 on a text entry", entry(5, y2=1), pool, 5),
             ("a negative offset", entry(1, a=-1), pool, 1), ("a negative length", entry(5, b=-1), pool, 5), ("a run past the pool", entry(5, b=3), pool, 5),
             ("offset + length past int32", entry(1, a=2 ** 31 - 1, b=2 ** 31 - 1), pool, 1), ("a control code", rows, byte(2, 0x1F), 1),
             ("DEL", rows, byte(6, 0x7F), 5),
             ("a line of thickness 0", entry(2, a=0), pool, 2), ("a line of thickness -1", entry(2, a=-1), pool, 2),
             ("a dash with on = 0", entry(2, b=3 << 16), pool, 2), ("a dash with off = 0", entry(2, b=3), pool, 2),
             ("a line's x1 beyond the bound", entry(2, x1=BEYOND), pool, 2), ("a line's y1 beyond the bound", entry(2, y1=-BEYOND), pool, 2),
             ("a line's x2 beyond the bound", entry(2, x2=-BEYOND), pool, 2), ("a line's y2 beyond the bound", entry(2, y2=2 ** 31 - 1), pool, 2),
             ("a disc of thickness 0", entry(3, a=0), pool, 3), ("a negative radius", entry(4, x2=-1), pool, 4), ("y2 on a disc", entry(3, y2=1), pool, 3),
             ("b on a disc", entry(4, b=1), pool, 4), ("a disc's centre x beyond the bound", entry(3, x1=BEYOND), pool, 3),
             ("a disc's centre y beyond the bound", entry(4, y1=-2 ** 31), pool, 4), ("a radius beyond the bound", entry(3, x2=BEYOND), pool, 3)]
    return rows, pool, cases


def accepted():
    """Tables at the edge of what is allowed: [(what, prims)]."""
    return [("colour bits 24..31 on every kind", [tuple(split(p)[0]) + ({"transparency": 255 - 20 * k},) for k, p in enumerate(GOOD)]),
            ("coordinates at the bound", [("line", MAX_COORD, -MAX_COORD, -MAX_COORD, MAX_COORD, 1) + RED, ("disc", -MAX_COORD, MAX_COORD, MAX_COORD, 1) + RED]),
            ("the longest dash", [("line", 0, 0, 9, 0, 1) + RED + ({"dash": (0xFFFF, 0xFFFF)},)]),
            ("rectangles and text beyond the lines' bound", [("rect", -2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1, 1) + RED, ("text", 2 ** 31 - 1, -2 ** 31, "far", 64) + RED])]
