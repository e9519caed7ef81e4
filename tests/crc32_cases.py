"""A model of radnet_crc32_segments (include/radnet_hip.h, csrc/crc32_rule.h) written from the three identities alone, the case table
its tests share, and five mutants of the model that named cases must catch.  NumPy only: no device, no library.

CRC-32 as zlib sums it: P = 0xEDB88320, reflected (bit 31 of a register is the coefficient of x^0).  pure(B) is the register after
the bytes B from init 0 without the final xor; products are taken mod P:
    pure(A || B) = pure(A) * x^(8 |B|) ^ pure(B)
    pure(0^k || B) = pure(B)
    zlib.crc32(B, c0) = pure(B) ^ (c0 ^ 0xFFFFFFFF) * x^(8 |B|) ^ 0xFFFFFFFF
The model cuts a segment as THE GRAIN RULE says -- a tail behind the last 16-byte boundary, grains of 16 bytes and spans of 256 grains
counted backwards from it -- and joins the pieces with the first identity, so it is the kernels' arithmetic in the kernels' order."""
import functools
import zlib

import numpy as np

POLY = 0xEDB88320
ONE = 0x80000000           # x^0
X8 = 0x00800000            # x^8
GRAIN = 16
SPAN_GRAINS = 256
SPAN = GRAIN * SPAN_GRAINS
IDAT = zlib.crc32(b"IDAT")
MUTANTS = ("non_reflected", "no_init_fold", "power_off_by_one", "reversed_combine", "no_final_xor")
# the case (by name) that has to tell each mutant from zlib.crc32
CAUGHT_BY = {"non_reflected": "noise_17_init0_at0", "no_init_fold": "zeros_17_idat_at0", "power_off_by_one": "noise_4097_init0_at0",
             "reversed_combine": "first_bit_4097_init0_at0", "no_final_xor": "noise_0_init0_at0"}


def times(a, b, poly=POLY):
    """a * b mod P, elementwise on uint32 arrays (or scalars): 32 shift / xor steps."""
    a, b = np.broadcast_arrays(np.asarray(a, np.uint32), np.asarray(b, np.uint32))
    b, p = b.copy(), np.zeros(a.shape, np.uint32)
    for i in range(31, -1, -1):
        p ^= b * ((a >> np.uint32(i)) & np.uint32(1))
        b = (b >> np.uint32(1)) ^ (np.uint32(poly) * (b & np.uint32(1)))
    return p


def times_int(a, b, poly=POLY):
    """times() on two Python ints."""
    p = 0
    for i in range(31, -1, -1):
        if (a >> i) & 1:
            p ^= b
        b = (b >> 1) ^ (poly if b & 1 else 0)
    return p


@functools.lru_cache(maxsize=None)
def shift(nbytes, poly=POLY):
    """x^(8 nbytes) mod P by squaring (Python ints)."""
    r, b, e = ONE, X8, max(int(nbytes), 0)
    while e:
        if e & 1:
            r = times_int(r, b, poly)
        b = times_int(b, b, poly)
        e >>= 1
    return r


def byte_table(poly=POLY):
    """table[v]: the register v (below 256) after eight steps."""
    t = np.arange(256, dtype=np.uint32)
    for _ in range(8):
        t = (t >> np.uint32(1)) ^ (np.uint32(poly) * (t & np.uint32(1)))
    return t


def pure_rows(rows, poly=POLY):
    """pure() of every row of a [k][m] uint8 array, from init 0: byte by byte through the table, all rows at once."""
    table, v = byte_table(poly), np.zeros(rows.shape[0], np.uint32)
    for j in range(rows.shape[1]):
        v = table[(v ^ rows[:, j]) & np.uint32(0xff)] ^ (v >> np.uint32(8))
    return v


def cut(at, length):
    """(grains, spans, tail) of a segment whose first byte stands `at` bytes behind a 16-byte boundary."""
    end = at + length
    aligned_end = end - end % GRAIN
    if aligned_end <= at:
        return 0, 0, length
    grains = -(-(aligned_end - at) // GRAIN)
    return grains, -(-grains // SPAN_GRAINS), end - aligned_end


def model(data, init=0, at=0, mutant=None):
    """zlib.crc32(data, init) by grains, spans and the fold; `at` as in cut().  mutant: one of MUTANTS, or None for the real thing."""
    assert mutant is None or mutant in MUTANTS
    poly = 0x04C11DB7 if mutant == "non_reflected" else POLY
    data = np.frombuffer(bytes(data), np.uint8)
    grains, spans, tail = cut(at, len(data))
    body = data[:len(data) - tail]
    # grains from the body's end: zeros in front cost nothing, so the body is padded to whole spans and every unit's weight is a constant
    padded = np.zeros(spans * SPAN, np.uint8)
    padded[len(padded) - len(body):] = body
    sums = pure_rows(padded.reshape(-1, GRAIN), poly).reshape(spans, SPAN_GRAINS)      # [span from the front][grain from the front]
    back = 1 if mutant == "power_off_by_one" else 0
    weights = np.array([shift(max(GRAIN * i - back, 0), poly) for i in range(SPAN_GRAINS)], np.uint32)      # of the unit i units in front of the end
    grain_w = weights if mutant == "reversed_combine" else weights[::-1]
    part = np.bitwise_xor.reduce(times(sums, grain_w[None, :], poly), axis=1)[::-1] if spans else np.zeros(0, np.uint32)   # part[e]: e spans in front of the end
    # the spans of one segment: lane t takes e = t, t + 256, ... by Horner's rule, then its own distance
    stride = shift(SPAN * SPAN_GRAINS, poly)
    span_w = [shift(SPAN * t, poly) for t in range(min(spans, SPAN_GRAINS))]
    v = 0
    for t in range(min(spans, SPAN_GRAINS)):
        lane = 0
        for e in reversed(range(t, spans, SPAN_GRAINS)):
            lane = times_int(lane, stride, poly) ^ int(part[e])
        v ^= times_int(lane, span_w[t], poly)
    table = byte_table(poly)
    for byte in data[len(data) - tail:].tolist():
        v = int(table[(v ^ byte) & 0xff]) ^ (v >> 8)
    if mutant != "no_init_fold":
        v ^= times_int(init ^ 0xFFFFFFFF, shift(len(data), poly), poly)
    return v if mutant == "no_final_xor" else v ^ 0xFFFFFFFF


def content(kind, length, seed=0):
    """The bytes of a case: zeros (pure = 0: only the init fold speaks), ff, first_bit / last_bit (one set bit in the first / last
    byte), noise."""
    out = np.zeros(length, np.uint8)
    if kind == "ff":
        out[:] = 0xff
    elif kind == "first_bit" and length:
        out[0] = 0x80
    elif kind == "last_bit" and length:
        out[-1] = 0x01
    elif kind == "noise":
        out = np.random.RandomState(1000 + seed + length % 997).randint(0, 256, size=length).astype(np.uint8)
    else:
        assert kind in ("zeros", "first_bit", "last_bit"), kind
    return out


CONTENTS = ("zeros", "ff", "first_bit", "last_bit", "noise")
INITS = {"init0": 0, "initff": 0xFFFFFFFF, "idat": IDAT, "rand": 0x9E3779B9}
SMALL = (0, 1, 3, 4, 15, 16, 17)                                         # round the grain G = 16: G - 1, G, G + 1 are among them
EDGES = (SPAN - 1, SPAN, SPAN + 1, 2 * SPAN + 5)                         # one workgroup's span +- 1, two spans + 5
DEEP = SPAN * SPAN_GRAINS + 3 * SPAN + 21                                # more than 256 spans: every level up to Horner's rule; 1.01 MiB
MISALIGN = (1, 3, 7, 13)


def cases():
    """(name, kind, length, init, at): `at` is the misalignment of the segment's first byte against a 16-byte boundary."""
    out = []
    for length in SMALL:
        for kind in CONTENTS:
            for iname, init in INITS.items():
                out.append(("%s_%d_%s_at0" % (kind, length, iname), kind, length, init, 0))
    for length in SMALL + EDGES:
        for at in MISALIGN:
            out.append(("noise_%d_idat_at%d" % (length, at), "noise", length, IDAT, at))
    for length in EDGES:
        for kind in CONTENTS:
            out.append(("%s_%d_init0_at0" % (kind, length), kind, length, 0, 0))
        out.append(("noise_%d_rand_at0" % length, "noise", length, INITS["rand"], 0))
    for kind, iname in zip(CONTENTS, ("rand", "idat", "init0", "initff", "idat")):
        out.append(("%s_%d_%s_at0" % (kind, DEEP, iname), kind, DEEP, INITS[iname], 0))
    out.append(("noise_%d_rand_at13" % DEEP, "noise", DEEP, INITS["rand"], 13))
    assert len({c[0] for c in out}) == len(out)
    return out


SEGMENT = np.dtype([("offset", np.int64), ("length", np.int64), ("init", np.uint32), ("expect", np.uint32)])      # radnet_crc32_segment
