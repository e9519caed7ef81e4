"""The many-stream inflate's contract (include/radnet_hip.h, "THE BOUNDARY RULE") in plain Python, and the batches its tests share.
Nothing here restates a decoder: every function is the one-stream model of tests/inflate_cases.py (I) or tests/inflate_lz_cases.py
(Z) applied to ONE stream's own bytes -- a slice that ends where the stream ends, so nothing behind it can be read -- and shifted by
8 * z_offset bits and out_offset bytes.  Imports nothing from the product.
  Batch: the common buffer z, the table [(z_offset, n, out_offset, expected)], out_len, the streams, and a tally that proves the
    batch reaches the branch it is for.
  find_many / measure_many / chains / emit_rle_many / emit_lz_many: the five entries and the per-stream host chain.
  MUTANTS: deliberate mistakes (keyword switches of the functions above); CAUGHT_BY names the batch that catches each.
  batches(): the case table, built once."""
import functools
import zlib

import numpy as np

import inflate_cases as I
import inflate_lz_cases as Z

PAST_END = I.PAST_END
MUTANTS = ("find_no_boundary", "measure_no_boundary", "emit_no_boundary", "unshifted_end", "clamp_at_zero")
NO_SRC = 0xFFFFFFFF      # a local source table's prefill: no position has it (out_len < 2^31)


class Batch:
    """z: the common buffer (streams, gaps, whatever fills them); table: [(z_offset, n, out_offset, expected)]; streams: [(name, the
    stream's own bytes, the data it inflates to or None)]."""

    def __init__(self, name, pieces, tally=None):
        """pieces: [("stream", name, z bytes, expected, data or None, output gap in front) | ("gap", bytes)] in buffer order."""
        self.name, self.table, self.streams, self.tally = name, [], [], dict(tally or {})
        z, out = bytearray(), 0
        for p in pieces:
            if p[0] == "gap":
                z += p[1]
                continue
            _, sname, sz, expected, data, out_gap = p
            out += out_gap
            self.table.append((len(z), len(sz), out, expected))
            self.streams.append((sname, bytes(sz), data))
            z += sz
            out += expected
        self.z, self.out_len = bytes(z), out + 5      # five bytes of output behind the last stream belong to nobody

    def stream_of(self, bit):
        """The index of the stream whose bytes hold the global bit, or None for a bit in a gap or outside the buffer."""
        for k, (zo, n, _, _) in enumerate(self.table):
            if 8 * zo <= bit < 8 * (zo + n):
                return k
        return None

    def own(self, k, no_boundary=False):
        """What stream k may read: its own n bytes.  MUTANT *_no_boundary: everything up to the end of the buffer."""
        zo, n, _, _ = self.table[k]
        return self.z[zo:] if no_boundary else self.z[zo:zo + n]


def find_many(b, find_no_boundary=False):
    """radnet_inflate_find_blocks_many: the sorted global candidates -- per stream, I.find_blocks on the stream alone from its bit 16."""
    out = []
    for k, (zo, n, _, _) in enumerate(b.table):
        out += [8 * zo + p for p in I.find_blocks(b.own(k, find_no_boundary), 16) if p < 8 * n]      # a bit of stream k, whatever was read
    return sorted(out)


def measure_many(b, starts, lz, measure_no_boundary=False, unshifted_end=False):
    """radnet_inflate_rle_measure_many (lz: radnet_inflate_lz_measure_many): the records of the units at the global `starts`."""
    M = Z if lz else I
    out = []
    for s in starts:
        k = b.stream_of(s)
        if k is None:
            out.append(M.unit_record(s, PAST_END))
            continue
        shift = 8 * b.table[k][0]
        rec = list(M.decode_unit(b.own(k, measure_no_boundary), s - shift))
        rec[0] = s
        if rec[5] == I.OK and not unshifted_end:                      # MUTANT unshifted_end: end_bit stays the stream's own
            rec[1] += shift
        out.append(tuple(rec))
    return out


def chains(b, units, lz):
    """The host chain per stream on its slice of the records (sorted by start), bits shifted back, links shifted forward:
    [(code, bad_unit, global links)] per stream."""
    M = Z if lz else I
    out = []
    for k, (zo, n, oo, expected) in enumerate(b.table):
        local = []
        for u in units:
            if 8 * zo <= u[0] < 8 * (zo + n):
                u = list(u)
                u[0] -= 8 * zo
                if u[5] == I.OK:
                    u[1] -= 8 * zo
                local.append(tuple(u))
        code, bad, links, _ = M.chain(local, 16, n, expected) if local else (M.CHAIN_NO_START, -1, [], 0)
        out.append((code, bad, [(off + oo, start + 8 * zo, nbytes, prev) for off, start, nbytes, prev in links]))
    return out


def _local_links(b, k, links, no_boundary):
    """The links whose start bit stream k holds, in the stream's own bits and output positions; one that begins outside the
    stream's output writes nothing and is dropped.  MUTANT emit_no_boundary: the output's end is the common buffer's."""
    zo, n, oo, expected = b.table[k]
    room = b.out_len - oo if no_boundary else expected
    mine = [(off - oo, start - 8 * zo, nbytes, prev) for off, start, nbytes, prev in links if b.stream_of(start) == k]
    return [l for l in mine if 0 <= l[0] <= room], room


def emit_rle_many(b, links, fill, emit_no_boundary=False):
    """radnet_inflate_rle_emit_many: the common output, prefilled with `fill`."""
    out = np.full(b.out_len, fill, np.uint8)
    for k, (zo, n, oo, expected) in enumerate(b.table):
        mine, room = _local_links(b, k, links, emit_no_boundary)
        if mine:
            out[oo:oo + room] = np.frombuffer(I.emit(b.own(k, emit_no_boundary), mine, room, fill), np.uint8)
    return out


def emit_lz_many(b, links, fill, fill_src, emit_no_boundary=False, clamp_at_zero=False):
    """radnet_inflate_lz_emit_many: (buf, src) of the common output, prefilled; src holds absolute positions."""
    buf, src = np.full(b.out_len, fill, np.uint8), np.full(b.out_len, fill_src, np.uint32)
    for k, (zo, n, oo, expected) in enumerate(b.table):
        mine, room = _local_links(b, k, links, emit_no_boundary)
        if not mine:
            continue
        if clamp_at_zero:                                             # MUTANT clamp_at_zero: positions are absolute from the start, so
            shifted = [(off + oo, start, nbytes, prev) for off, start, nbytes, prev in mine]      # only a source below 0 is replaced
            lbuf, lsrc = Z.emit(b.own(k, emit_no_boundary), shifted, oo + room, fill, NO_SRC)
            lbuf, lsrc, base = lbuf[oo:], lsrc[oo:], 0
        else:
            lbuf, lsrc = Z.emit(b.own(k, emit_no_boundary), mine, room, fill, NO_SRC)
            base = oo
        written = lsrc != NO_SRC
        buf[oo:oo + room] = lbuf
        src[oo:oo + room] = np.where(written, lsrc.astype(np.int64) + base, fill_src).astype(np.uint32)
    return buf, src


def clamped(b, links):
    """How many source entries of `links` the clamp replaces: those where clamping at 0 and at out_offset differ."""
    a = emit_lz_many(b, links, 0, 0)[1]
    c = emit_lz_many(b, links, 0, 0, clamp_at_zero=True)[1]
    return int((a != c).sum())


# ---- the case table ------------------------------------------------------------------------------------------------------------------
def _stream(name, z, data=None, expected=None, out_gap=0):
    return ("stream", name, bytes(z), len(data) if expected is None else expected, data, out_gap)


def _noise(rs, n):
    return rs.randint(0, 256, n).astype(np.uint8).tobytes()


@functools.lru_cache(maxsize=1)
def base_streams():
    """The six streams of the plain batches: 1 byte; the deflate model's dynamic stream; a stored stream that buries the headers of
    the last one; level 6 with far matches; 300 bytes; memLevel 1 (blocks of 128 symbols, units on every bit phase)."""
    rs = np.random.RandomState(5)
    c = I.cases()
    buried = _noise(rs, 700) + c["b memlevel 1"].z[:3000] + _noise(rs, 300)
    out = [(n, c[n].z, c[n].data) for n in ("f 1 bytes", "g deflate model dynamic")]
    out.append(("stored with buried headers", zlib.compress(buried, 0), buried))
    out += [(n, c[n].z, c[n].data) for n in ("i level 6", "f 300 bytes", "b memlevel 1")]
    return out


def _plain(name, gap, rs):
    pieces = [("gap", _noise(rs, gap))] if gap else []
    for k, (sname, z, data) in enumerate(base_streams()):
        pieces.append(_stream(sname, z, data, out_gap=gap % 4 if k else 0))
        if gap:
            pieces.append(("gap", _noise(rs, gap)))
    return Batch(name, pieces)


def _cut_batches():
    """(a) and (b): the memLevel 1 stream cut in the middle of its 5th dynamic header, and in the middle of the unit behind it; the
    rest of the stream stands in the gap behind the cut, so a reader without the boundary goes on as if nothing had happened."""
    rs = np.random.RandomState(6)
    c = I.cases()
    zb, small, lz6 = c["b memlevel 1"].z, c["f 300 bytes"], c["i level 6"]
    starts = I.true_dynamic_starts(zb)
    start, after = starts[4], starts[5]
    status, header_end, _, _ = I.parse_dynamic(zb, start + 3, 8 * len(zb))
    assert status == I.OK and header_end - start > 64
    out = []
    for name, cut_bit in (("a cut in a header", (start + header_end) // 2), ("b cut in a unit", (header_end + after) // 2)):
        cut = cut_bit // 8
        tally = dict(cut_bits=8 * cut, unit_start=start, header_end=header_end, unit_end=after)
        out.append(Batch(name, [_stream(small.name, small.z, small.data), ("gap", _noise(rs, 3)),
                                _stream("b memlevel 1, cut", zb[:cut], None, expected=2000, out_gap=2), ("gap", zb[cut:cut + 900]),
                                _stream(lz6.name, lz6.z, lz6.data, out_gap=1)], tally))
    return out


def _reach_batch():
    """(c): four-valued noise at memLevel 1 -- small units that reach into those in front of them -- behind a neighbour, with 0 and 15
    bytes between them.  Its tests chain it honestly and also hand-make links that put a LATER unit at the stream's out_offset."""
    rs = np.random.RandomState(8)
    low = rs.randint(0, 4, 6000).astype(np.uint8).tobytes()
    z = Z._deflate(low, mem=1)
    c = I.cases()
    first = c["g deflate model dynamic"]
    return Batch("c reach in front of the stream", [_stream(first.name, first.z, first.data), _stream("noise small", z, low),
                                                    ("gap", _noise(rs, 15)), _stream("f 2 bytes", c["f 2 bytes"].z, c["f 2 bytes"].data, out_gap=15)])


@functools.lru_cache(maxsize=1)
def batches():
    """{name: Batch}.  "gap 0" / "gap 1" / "gap 15": the six base streams back to back, 1 and 15 bytes of noise apart (and in front
    of the first and behind the last); "a cut in a header", "b cut in a unit", "c reach in front of the stream": see above."""
    rs = np.random.RandomState(9)
    out = [_plain("gap %d" % g, g, rs) for g in (0, 1, 15)] + _cut_batches() + [_reach_batch()]
    return {b.name: b for b in out}


CAUGHT_BY = {"find_no_boundary": "a cut in a header", "measure_no_boundary": "b cut in a unit", "emit_no_boundary": "a cut in a header",
             "unshifted_end": "gap 1", "clamp_at_zero": "c reach in front of the stream"}


@functools.lru_cache(maxsize=None)
def model(name, lz):
    """(candidates, starts, unit records, per-stream chains, all links) of a batch, computed once and shared."""
    b = batches()[name]
    cands = find_many(b)
    starts = sorted(set(cands) | {8 * zo + 16 for zo, _, _, _ in b.table})
    units = measure_many(b, starts, lz)
    per_stream = chains(b, units, lz)
    ok = (Z if lz else I).CHAIN_OK
    links = [l for code, _, ls in per_stream if code == ok for l in ls]
    return cands, starts, units, per_stream, links


def hand_links(name):
    """Links no chain gives, for the emit entries.  (a): the cut stream's unit whose header straddles the cut, with room for all
    it would write had it not been cut -- it must write nothing.  (a) and (b): a link of the FIRST stream, put 3 bytes in front of
    the end of that stream's output, that asks for 4000 -- it must stop there.  (c): the noise stream's first unit that reaches, put
    at the stream's own out_offset, so that its first far match points in front of the stream.  (A unit that fails in the middle
    of its tokens is in none of them: how much of it is written before it stops is not part of the contract.)"""
    b = batches()[name]
    if name.startswith(("a ", "b ")):
        zo, n, oo, expected = b.table[1]
        fzo, fn, foo, fexp = b.table[0]
        over = [(foo + fexp - 3, 8 * fzo + 16, 4000, 0)]
        return [(oo, 8 * zo + b.tally["unit_start"], 1500, 0)] + over if name.startswith("a ") else over
    zo, n, oo, expected = b.table[1]
    units = model(name, True)[2]
    far = [u for u in units if 8 * zo <= u[0] < 8 * (zo + n) and u[5] == I.OK and u[7] > 0]
    return [(oo, far[0][0], far[0][2], 0)]
