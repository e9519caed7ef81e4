"""Shared cases of the PNG tests: an independent encoder written from the PNG specification (forward filters in vectorised NumPy --
a filtered byte depends on raw bytes only --, a chosen filter type per row, sub-byte packing, the Adam7 split, zlib.compress and
zlib.crc32) and a NumPy statement of the expansion rules (what cv2.imdecode(buf, IMREAD_COLOR) makes of each colour type).
Imports nothing from the product.  Expected output = expand(source samples); product output = decode of encode(source samples)."""
import collections
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
LEGAL = [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16), (6, 8), (6, 16)]
ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))      # x0, y0, dx, dy

Encoded = collections.namedtuple("Encoded", "data stream passes")      # file bytes, filtered scanline stream, pass tuples


def chunk(kind, payload=b""):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload))


def ihdr(width, height, depth, color_type, interlace=0, compression=0, filt=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, depth, color_type, compression, filt, interlace))


def pack_rows(samples, depth):
    """[h][w][channels] samples -> [h][rowbytes] bytes: 16-bit big-endian, 8-bit as they are, smaller depths MSB first."""
    h = samples.shape[0]
    flat = np.asarray(samples).reshape(h, -1)
    if depth == 16:
        out = np.empty((h, flat.shape[1], 2), np.uint8)
        out[:, :, 0] = flat >> 8
        out[:, :, 1] = flat & 255
        return out.reshape(h, -1)
    if depth == 8:
        return flat.astype(np.uint8)
    bits = ((flat[:, :, None].astype(np.int64) >> np.arange(depth - 1, -1, -1)) & 1).astype(np.uint8).reshape(h, -1)
    return np.packbits(bits, axis=1)               # pads the last byte with zero bits


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(raw, bpp, types):
    """Forward filters: raw [h][rowbytes] uint8, types [h] in 0..4 (or 'adaptive': per row the type with the smallest sum of
    absolute signed residuals) -> ([h][1 + rowbytes] filtered scanlines, the types)."""
    h, n = raw.shape
    x = raw.astype(np.int64)
    a = np.zeros_like(x)
    a[:, bpp:] = x[:, :n - bpp] if n > bpp else 0
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[:, bpp:] = b[:, :n - bpp] if n > bpp else 0
    forms = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - _paeth(a, b, c)]) & 255      # [5][h][n]
    if isinstance(types, str):
        assert types == "adaptive"
        signed = np.where(forms > 127, 256 - forms, forms).sum(axis=2)
        types = np.argmin(signed, axis=0)
    types = np.broadcast_to(np.asarray(types, np.int64), (h,))
    out = np.empty((h, 1 + n), np.uint8)
    out[:, 0] = types
    out[:, 1:] = forms[types, np.arange(h)]
    return out, types


def pass_list(width, height, interlace):
    out = []
    for x0, y0, dx, dy in (ADAM7 if interlace else ((0, 0, 1, 1),)):
        pw, ph = -(-(width - x0) // dx), -(-(height - y0) // dy)
        if pw > 0 and ph > 0:
            out.append((x0, y0, dx, dy, pw, ph))
    return out


def encode(samples, color_type, depth, filters=0, interlace=False, palette=None, trns=None, idat_sizes=None, level=6, extra=()):
    """samples: [h][w][channels] unsigned integers below 2 ** depth (palette indices for colour type 3).
    filters: one type for every row, 'adaptive', or a RandomState (one random type per row).  palette: [n][3] R, G, B.
    trns: payload of a tRNS chunk placed before IDAT.  idat_sizes: sizes of the leading IDAT chunks (the rest goes in a last one).
    extra: chunks inserted after IHDR as they are."""
    samples = np.asarray(samples)
    if samples.ndim == 2:
        samples = samples[:, :, None]
    h, w, ch = samples.shape
    assert ch == CHANNELS[color_type] and (color_type, depth) in LEGAL
    bpp = max(1, ch * depth // 8)
    stream, passes = [], []
    offset = 0
    for x0, y0, dx, dy, pw, ph in pass_list(w, h, interlace):
        raw = pack_rows(samples[y0::dy, x0::dx], depth)
        assert raw.shape == (ph, (pw * ch * depth + 7) // 8)
        types = filters.randint(0, 5, size=ph) if isinstance(filters, np.random.RandomState) else filters
        lines, _ = filter_rows(raw, bpp, types)
        passes.append((x0, y0, dx, dy, pw, ph, raw.shape[1], offset))
        stream.append(lines.tobytes())
        offset += lines.size
    stream = b"".join(stream)
    z = zlib.compress(stream, level)
    parts = [SIGNATURE, ihdr(w, h, depth, color_type, 1 if interlace else 0)]
    parts.extend(extra)
    if palette is not None:
        parts.append(chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes()))
    if trns is not None:
        parts.append(chunk(b"tRNS", bytes(trns)))
    for size in (idat_sizes or ()):
        parts.append(chunk(b"IDAT", z[:size]))
        z = z[size:]
    parts.append(chunk(b"IDAT", z))
    parts.append(chunk(b"IEND"))
    return Encoded(b"".join(parts), stream, passes)


def expand(samples, color_type, depth, palette=None):
    """The image cv2.imdecode(buf, IMREAD_COLOR) returns for these source samples: uint8 [h][w][3] in B, G, R order."""
    samples = np.asarray(samples)
    if samples.ndim == 2:
        samples = samples[:, :, None]
    s = samples.astype(np.int64)
    if color_type == 3:
        table = np.zeros((256, 3), np.uint8)       # an index beyond the PLTE length gives 0
        pal = np.asarray(palette, np.uint8)
        table[:len(pal)] = pal[:, ::-1]
        return table[s[:, :, 0]]
    if depth == 16:
        s = s >> 8                                 # strip_16: the high byte
    elif depth < 8:
        s = s * {1: 255, 2: 85, 4: 17}[depth]
    if color_type in (0, 4):                       # grey (alpha dropped) on three channels
        return np.repeat(s[:, :, :1], 3, axis=2).astype(np.uint8)
    return s[:, :, 2::-1].astype(np.uint8)         # R, G, B (alpha dropped) -> B, G, R


def draw(rng, h, w, color_type, depth, kind="full"):
    """Source samples: kind 'low' from {0, 1, 2, 3} (Paeth ties are frequent), 'high' from 128..255 per byte (Average's 9-bit sum,
    wrap-around), 'full' the whole range."""
    ch = CHANNELS[color_type]
    top = 1 << depth
    if kind == "low":
        s = rng.randint(0, min(4, top), size=(h, w, ch))
        return s | (s << 8) if depth == 16 else s
    if kind == "high":
        if depth == 16:
            return (rng.randint(128, 256, size=(h, w, ch)) << 8) | rng.randint(128, 256, size=(h, w, ch))
        return rng.randint(top // 2, top, size=(h, w, ch))
    return rng.randint(0, top, size=(h, w, ch))
