"""Shared cases of the tiled PNG reconstruction tests (radnet_png_unfilter_tiles_u8, unfilter="tiles"): the case table and a NumPy
model of the tile geometry include/radnet_hip.h states.  Imports nothing from the product; the constants are the caller's.

The model writes down, from the stated geometry alone,
  * which bytes tile (band b, block c) owns: of row b * 64 + l the pixels [c * T - l, (c + 1) * T - l) inside [0, P);
  * which bytes it reads and does not own: what the PNG predictors take -- the pixel to the left, the one above, the one above-left --
    of every pixel it owns, minus the pixels it owns itself;
  * the sweep of a tile, d = c + 2 * b, and the counts bands = ceil(R / 64), blocks = ceil((P + 63) / T), sweeps = blocks + 2 (bands - 1).
`run` executes given sweeps in order, the tiles of a sweep in a caller-given permutation; a tile reads every byte it does not own from
a snapshot taken before its sweep, so an order among the tiles of one sweep can matter only through a byte two of them touch.  The
expected bytes of a case are the raw rows it was filtered from (png_cases.filter_rows), never anything the code under test made."""
import collections

import numpy as np

import png_cases as K

ROWS = 64

Geometry = collections.namedtuple("Geometry", "rows pixels tile_pixels bands blocks sweeps")


def geometry(rows, pixels, tile_pixels):
    bands = -(-rows // ROWS)
    blocks = -(-(pixels + 63) // tile_pixels)
    return Geometry(rows, pixels, tile_pixels, bands, blocks, blocks + 2 * (bands - 1))


def sweep_of(band, block):
    return block + 2 * band


def tiles_by_sweep(geo, sweep_rule=sweep_of, blocks=None):
    """[sweep] -> the (band, block) pairs on it, bands ascending; blocks: another number of column blocks than the geometry's."""
    blocks = geo.blocks if blocks is None else blocks
    out = collections.defaultdict(list)
    for band in range(geo.bands):
        for block in range(blocks):
            out[sweep_rule(band, block)].append((band, block))
    return [sorted(out[d]) for d in range(max(out) + 1)]


def owned(geo, band, block):
    """bool [rows][pixels]: the pixels tile (band, block) owns."""
    mask = np.zeros((geo.rows, geo.pixels), bool)
    for lane in range(ROWS):
        r = band * ROWS + lane
        if r >= geo.rows:
            break
        lo, hi = block * geo.tile_pixels - lane, (block + 1) * geo.tile_pixels - lane
        mask[r, max(lo, 0):max(min(hi, geo.pixels), 0)] = True
    return mask


def read_not_owned(mask):
    """bool [rows][pixels]: the pixels inside the segment a tile with the ownership `mask` reads and does not own (left, above and
    above-left of each owned pixel; what falls outside the segment is zero by the PNG rules and no tile's)."""
    reads = np.zeros_like(mask)
    reads[:, :-1] |= mask[:, 1:]                   # the pixel to the left of an owned one
    reads[:-1, :] |= mask[1:, :]                   # above
    reads[:-1, :-1] |= mask[1:, 1:]                # above-left
    return reads & ~mask


def _paeth(a, b, c):
    pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def run_tile(state, types, mask):
    """The owned pixels of one tile reconstructed from `state` ([1 + rows][1 + pixels][bpp] int64 with a zero row on top and a zero pixel
    column at the left: the snapshot of its sweep), so that a neighbour the tile owns is its own fresh value and every other
    neighbour the snapshot's.  The order is by anti-diagonals r + p (all pixels of one at once): the three neighbours of a pixel lie
    on the two diagonals before its own.  Returns (row indices, pixel indices, values) of the owned pixels."""
    loc = state.copy()
    rr, pp = np.nonzero(mask)
    ft = np.asarray(types, np.int64)[rr][:, None]
    diagonal = rr + pp
    for d in np.unique(diagonal):
        at = diagonal == d
        r, p, f = rr[at], pp[at], ft[at]
        a, b, c = loc[r + 1, p], loc[r, p + 1], loc[r, p]
        pred = np.select([f == 1, f == 2, f == 3, f == 4], [a, b, (a + b) >> 1, _paeth(a, b, c)], 0)
        loc[r + 1, p + 1] = (loc[r + 1, p + 1] + pred) & 255
    return rr, pp, loc[rr + 1, pp + 1]


def run(lines, bpp, geo, sweeps, order):
    """The scanlines [rows][1 + rowbytes] reconstructed by the tiles of `sweeps` ([sweep] -> list of (band, block)), sweep after sweep;
    order(d, n) gives the permutation in which the n tiles of sweep d run.  Returns the data bytes [rows][rowbytes]."""
    rows, n = lines.shape[0], lines.shape[1] - 1
    assert rows == geo.rows and n == geo.pixels * bpp
    state = np.zeros((rows + 1, geo.pixels + 1, bpp), np.int64)
    state[1:, 1:] = lines[:, 1:].reshape(rows, geo.pixels, bpp)
    for d, tiles in enumerate(sweeps):
        snapshot = state.copy()
        for k in order(d, len(tiles)):
            rr, pp, values = run_tile(snapshot, lines[:, 0], owned(geo, *tiles[k]))
            state[rr + 1, pp + 1] = values
    return state[1:, 1:].reshape(rows, n).astype(np.uint8)


def in_order(d, n):
    return range(n)


def reversed_order(d, n):
    return range(n - 1, -1, -1)


def shuffled_order(seed):
    rs = np.random.RandomState(seed)
    return lambda d, n: rs.permutation(n)


# ---- the case table ---------------------------------------------------------------------------------------------------------------
ROW_COUNTS = (1, 63, 64, 65, 128, 129)
BPPS = (1, 2, 3, 4, 6, 8)
FILTER_KINDS = (0, 1, 2, 3, 4, "mix")


def pixel_counts(tile_pixels):
    t = tile_pixels
    return tuple(sorted({1, 2, 62, 63, 64, 65, t - 63, t - 1, t, t + 1, 2 * t + 1}))


def shapes(tile_pixels):
    """Every (rows, pixels) of the table: the row counts around one band and two, the widths around the lane skew and the block."""
    return [(r, p) for r in ROW_COUNTS for p in pixel_counts(tile_pixels)]


def model_cases(tile_pixels):
    """(rows, pixels, bpp, filter kind) the model is run on: a cover of the row counts, widths, bpp values and filter kinds by a few
    small cases (the executor is Python, pixel by pixel)."""
    t = tile_pixels
    return [(1, 1, 1, 4), (63, 2, 8, 3), (64, 65, 2, "mix"), (65, 63, 3, 4), (65, t + 1, 1, 4), (128, t - 63, 4, "mix"), (129, t - 1, 6, 3),
            (129, 2 * t + 1, 1, "mix"), (70, t, 3, 2), (130, 64, 3, 4), (5, 2 * t + 1, 2, 1), (66, 62, 1, 0)]


def draw_segment(rs, rows, pixels, bpp, kind):
    """(filtered scanlines [rows][1 + pixels * bpp] uint8, raw rows [rows][pixels * bpp] uint8) of a seeded case.  The samples are
    drawn from a few values around 0 / 128 / 255 so that Paeth's ties and Average's 9-bit sum occur often."""
    raw = rs.choice(np.array([0, 1, 2, 3, 127, 128, 129, 253, 254, 255], np.uint8), size=(rows, pixels * bpp))
    types = rs.randint(0, 5, rows) if kind == "mix" else kind
    lines, _ = K.filter_rows(raw, bpp, types)
    return lines, raw
