"""Shared cases of the PNG writer's and the rectangle painter's tests.  Imports nothing from the product.
  decode(data): an independent PNG decoder for the writer's output (8 bits per sample, colour type 0 or 2, not interlaced): walks
    the chunks and checks every CRC, inflates the concatenated IDAT data with zlib.decompress (which also checks the Adler-32 and
    that the stream ends), and unfilters per the PNG specification, row by row.
  paint(img, rects): the contract of radnet_draw_rects_u8 (include/radnet_hip.h) as a plain loop over the list, with slices.
  The case tables: sizes and inputs of the filter kernel, rectangle lists of the draw kernel."""
import collections
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
Decoded = collections.namedtuple("Decoded", "width height color_type stream samples kinds")      # samples: [h][w][channels] as stored

FILLED = -1


def chunks(data):
    """[(type, payload)] of a file; asserts the signature, every length and every CRC, and that nothing follows IEND."""
    assert data[:8] == SIGNATURE
    pos, out = 8, []
    while pos < len(data):
        length, kind = struct.unpack(">I4s", data[pos:pos + 8])
        payload = data[pos + 8:pos + 8 + length]
        assert len(payload) == length, "truncated %r chunk" % kind
        (crc,) = struct.unpack(">I", data[pos + 8 + length:pos + 12 + length])
        assert crc == zlib.crc32(kind + payload), "CRC of the %r chunk" % kind
        out.append((kind, payload))
        pos += 12 + length
    assert pos == len(data) and out[-1][0] == b"IEND"
    return out


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def unfilter(stream, h, rowbytes, bpp):
    """Reconstruction per the specification: [h][rowbytes] raw bytes of a stream of h rows of 1 + rowbytes bytes.  None, Sub and Up
    are whole-row NumPy operations; Average and Paeth walk the row byte by byte."""
    lines = np.frombuffer(stream, np.uint8).reshape(h, 1 + rowbytes)
    raw = np.zeros((h + 1, rowbytes + bpp), np.int64)      # row 0 and the first bpp columns: the zeros above and left of the image
    for r in range(h):
        ft, x = int(lines[r, 0]), lines[r, 1:].astype(np.int64)
        cur, up = raw[r + 1], raw[r]
        if ft == 0:
            cur[bpp:] = x
        elif ft == 1:
            for k in range(bpp):
                cur[bpp + k::bpp] = np.cumsum(x[k::bpp]) & 255
        elif ft == 2:
            cur[bpp:] = (x + up[bpp:]) & 255
        elif ft == 3:
            for i in range(rowbytes):
                cur[bpp + i] = (x[i] + ((cur[i] + up[bpp + i]) >> 1)) & 255
        elif ft == 4:
            for i in range(rowbytes):
                cur[bpp + i] = (x[i] + _paeth(int(cur[i]), int(up[bpp + i]), int(up[i]))) & 255
        else:
            raise AssertionError("filter type %d in row %d" % (ft, r))
    return raw[1:, bpp:].astype(np.uint8)


def decode(data):
    """Decoded(width, height, color_type, the inflated stream, samples [h][w][channels] in the file's channel order, chunk types)."""
    cs = chunks(bytes(data))
    kinds = [k for k, _ in cs]
    assert kinds[0] == b"IHDR" and kinds.count(b"IHDR") == 1 and kinds.count(b"IEND") == 1 and kinds.count(b"IDAT") >= 1
    assert set(kinds) == {b"IHDR", b"IDAT", b"IEND"}
    width, height, depth, color_type, compression, filt, interlace = struct.unpack(">IIBBBBB", cs[0][1])
    assert (depth, compression, filt, interlace) == (8, 0, 0, 0) and color_type in (0, 2)
    channels = 3 if color_type == 2 else 1
    stream = zlib.decompress(b"".join(p for k, p in cs if k == b"IDAT"))      # raises on a bad Adler-32 or an unfinished stream
    assert len(stream) == height * (1 + width * channels)
    samples = unfilter(stream, height, width * channels, channels).reshape(height, width, channels)
    return Decoded(width, height, color_type, stream, samples, kinds)


def decode_bgr(data):
    """The image cv2.imdecode(data, IMREAD_COLOR) returns for the writer's files: [h][w][3] in B, G, R order, grey replicated."""
    d = decode(data)
    return np.repeat(d.samples, 3, axis=2) if d.color_type == 0 else np.ascontiguousarray(d.samples[:, :, ::-1])


# ---- the rectangle contract ----------------------------------------------------------------------------------------------------------
def paint(img, rects):
    """radnet_draw_rects_u8's contract on a [h][w][3] array, in place, in list order: rects of (x1, y1, x2, y2, thickness, b, g, r)."""
    h, w = img.shape[:2]

    def clip(lo, hi, n):                           # the slice of [lo, hi] inside [0, n)
        return slice(min(max(lo, 0), n), min(max(hi + 1, 0), n))

    for x1, y1, x2, y2, t, b, g, r in rects:
        x1, x2, y1, y2 = min(x1, x2), max(x1, x2), min(y1, y2), max(y1, y2)
        hw = t // 2 if t > 0 else 0
        mask = np.zeros((h, w), bool)
        mask[clip(y1 - hw, y2 + hw, h), clip(x1 - hw, x2 + hw, w)] = True
        if t > 0:                                  # strictly inside (x1 + hw, x2 - hw) x (y1 + hw, y2 - hw) stays
            mask[clip(y1 + hw + 1, y2 - hw - 1, h), clip(x1 + hw + 1, x2 - hw - 1, w)] = False
        img[mask] = (b, g, r)
    return img


# ---- case tables -----------------------------------------------------------------------------------------------------------------------
# (h, w): one byte; one row; one column; tiny; rows of 255 and 258 bytes around a 256-thread sweep (3 channels); more than 1024 bytes
# per row and more rows than a wave
FILTER_SIZES = [(1, 1), (1, 5), (5, 1), (3, 2), (2, 85), (2, 86), (67, 342)]
FILTER_MODES = [0, 1, 2, 3, 4, 5]                  # 5: adaptive
FILTER_INPUTS = ["noise", "ramp", "constant", "flat", "columns"]


def filter_input(kind, h, w, channels, seed=0):
    """[h][w][channels] uint8: noise; a smooth ramp with a band of equal rows (Sub, Up and Paeth all win somewhere); an image of zeros (all five sums tie in
    every row: type 0); a flat non-zero image (Up and Paeth tie below row 0: type 2); an image whose columns are constant."""
    rs = np.random.RandomState(seed + 1000 * h + w)
    if kind == "noise":
        out = rs.randint(0, 256, (h, w, channels))
    elif kind == "ramp":
        y, x = np.mgrid[0:h, 0:w]
        planes = [(3 * x + 2 * y), (x * x // 7 + 5 * y), (2 * x + y * y // 3 + (x * y) // 5)]
        out = np.stack(planes[:channels], axis=2) + (rs.randint(0, 2, (h, w, channels)) if h * w > 64 else 0)
        out[h // 3:2 * h // 3] = out[h // 3]        # a band of equal rows: Up leaves zeros there
    elif kind == "constant":
        out = np.zeros((h, w, channels), np.int64)
    elif kind == "flat":
        out = np.full((h, w, channels), 77)
    elif kind == "columns":
        out = np.broadcast_to(rs.randint(0, 256, (1, w, channels)), (h, w, channels))
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(out & 255).astype(np.uint8)


def stream_rows(img):
    """The raw scanlines of an image as the writer stores them: [h][w * channels], B, G, R read as R, G, B."""
    img = img if img.ndim == 3 else img[:, :, None]
    return np.ascontiguousarray(img[:, :, ::-1]).reshape(img.shape[0], -1)


WHITE, RED, BLUE = (255, 255, 255), (28, 26, 228), (184, 126, 55)


def rect_lists(h, w):
    """{name: rects} for an h x w image: each thickness; overlaps in both orders; clipping at each edge; wholly outside; degenerate;
    reversed corners."""
    a, b = (5, 6, w // 2 + 3, h // 2 + 2), (w // 3, h // 4, w - 7, h - 5)
    out = {}
    for t in (1, 8, 9, FILLED):
        out["t=%d" % t] = [a + (t,) + WHITE, (w // 2, h // 3, w // 2 + 17, h // 3 + 21, t) + RED]
    out["overlap a then b"] = [a + (8,) + RED, b + (FILLED,) + BLUE, a + (1,) + WHITE]
    out["overlap b then a"] = [a + (1,) + WHITE, b + (FILLED,) + BLUE, a + (8,) + RED]
    out["clipped left"] = [(-3, 10, 12, 30, 9) + RED]
    out["clipped right"] = [(w - 6, 10, w + 20, 30, 8) + RED]
    out["clipped top"] = [(10, -2, 40, 9, 8) + BLUE, (20, -30, 30, 3, FILLED) + WHITE]
    out["clipped bottom"] = [(10, h - 3, 40, h + 9, 9) + BLUE]
    out["clipped all round"] = [(-3, -3, w + 2, h + 2, 8) + WHITE, (0, 0, w - 1, h - 1, 1) + RED]      # a frame of two pixels, its rim red
    out["outline wider than the image"] = [(-40, -40, w + 40, h + 40, 8) + RED]                 # paints nothing
    out["wholly outside"] = [(w + 10, 5, w + 30, 20, 8) + RED, (-40, -40, -20, -20, FILLED) + RED, (5, h + 5, 20, h + 9, 1) + RED,
                             (5, -9, 20, -5, 9) + WHITE]
    out["just outside, thickness reaches in"] = [(w + 2, 5, w + 30, 20, 8) + RED, (5, -3, 20, -1, 9) + WHITE]
    out["degenerate"] = [(20, 5, 20, 40, 1) + WHITE, (30, 5, 30, 40, 8) + RED, (40, 20, 40, 20, FILLED) + BLUE, (5, 50, 45, 50, 9) + BLUE]
    out["reversed corners"] = [(w // 2, h // 2, 4, 3, 8) + RED, (w - 4, 9, w // 2, h - 9, 1) + WHITE, (30, h - 2, 9, h // 2, FILLED) + BLUE]
    out["huge coordinates"] = [(-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1) + RED, (3, 3, 2 ** 31 - 1, 9, 1) + WHITE,
                               (-2 ** 31, 12, 2 ** 31 - 1, 14, FILLED) + BLUE]
    return out
