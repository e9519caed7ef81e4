"""The device inflate for ANY stream (include/radnet_hip.h, "far matches by pointer jumping") in plain Python, and the cases its tests
share.  The bit reader, the header rule, the code tables and the block search are tests/inflate_cases.py's; the unit decoder is this
file's own, because that one does not read a distance's extra bits.
  decode_unit / measure: one unit with its distances whole -- its record (UNIT_FIELDS), its tokens.
  chain: radnet_inflate_lz_chain.   emit: buf and src as radnet_inflate_lz_emit leaves them in prefilled buffers.
  resolve: the pointer jumping of radnet_inflate_lz_resolve, one launch at a time, all entries at once (Jacobi; the kernel works in
    place and may be done sooner, never later).   gather: radnet_inflate_lz_gather.   inflate: the whole path, or the reason it refuses.
  MUTANTS: deliberate mistakes (keyword switches of the functions above) that the tests must catch.
  cases(): the case table, built once."""
import functools
import struct
import zlib

import numpy as np

import deflate_cases as D
import inflate_cases as I
from inflate_cases import _table, find_blocks, parse_dynamic, peek

MAX_SYMBOLS = I.MAX_SYMBOLS
OK, BAD_HEADER, BAD_CODE, NOT_RLE, STORED_MISMATCH, PAST_END, TOO_LONG = range(7)
FINAL = 1
CHAIN_OK, CHAIN_NO_START, CHAIN_BAD_UNIT, CHAIN_LEAD_MATCH, CHAIN_LENGTH, CHAIN_TRAILER, CHAIN_REACH = range(7)
CHAIN_NAMES = I.CHAIN_NAMES + ("a match that reaches in front of the stream",)
UNIT_FIELDS = ("start_bit", "end_bit", "out_bytes", "symbols", "blocks", "status", "flags", "reach", "far_matches", "reserved")
MUTANTS = ("no_mod", "no_distance_extra", "reach_from_end", "reach_off_by_one", "gather_before_flat")
# RFC 1951, 3.2.5: (first distance, extra bits) of the distance symbols 0..29
DISTANCE_TABLE = []
for _s in range(30):
    _eb = 0 if _s < 4 else (_s - 2) >> 1
    DISTANCE_TABLE.append(((DISTANCE_TABLE[-1][0] + (1 << DISTANCE_TABLE[-1][1])) if _s else 1, _eb))
assert DISTANCE_TABLE[29] == (24577, 13) and DISTANCE_TABLE[16] == (257, 7)


def distance_symbol(distance):
    """(symbol, extra bits, extra value) of a match distance 1..32768."""
    for s in range(29, -1, -1):
        first, eb = DISTANCE_TABLE[s]
        if distance >= first:
            assert distance - first < 1 << eb
            return s, eb, distance - first
    raise ValueError("no distance symbol for %d" % distance)


def bound(n):
    """ceil(log2(max(n, 2))): the rounds that flatten any table emit writes."""
    return (max(n, 2) - 1).bit_length()


def unit_record(start, status=OK, end=0, out_bytes=0, symbols=0, blocks=0, flags=0, reach=0, far=0):
    if status != OK:
        return (start, 0, 0, 0, 0, status, 0, 0, 0, 0)
    return (start, end, out_bytes, symbols, blocks, OK, flags, reach, far, 0)


def decode_unit(z, start, cap=MAX_SYMBOLS, tokens=None, no_distance_extra=False, reach_from_end=False):
    """The record (UNIT_FIELDS) of the unit that begins at bit `start`; its tokens (("lit", byte), ("match", length, distance),
    ("stored", bytes)) are appended to `tokens` if given."""
    nbits = 8 * len(z)
    if start >= nbits:
        return unit_record(start, PAST_END)
    pos, symbols, blocks, produced, flags, reach, far = start, 0, 0, 0, 0, 0, 0
    while True:
        v = peek(z, pos)
        pos += 3
        if pos > nbits:
            return unit_record(start, PAST_END)
        bfinal, btype = v & 1, (v >> 1) & 3
        if btype == 0:
            pos = (pos + 7) & ~7
            v = peek(z, pos)
            pos += 32
            n = v & 0xffff
            if pos > nbits:
                return unit_record(start, PAST_END)
            if n != (v >> 16) ^ 0xffff:
                return unit_record(start, STORED_MISMATCH)
            at = pos >> 3
            pos += 8 * n
            if pos > nbits:
                return unit_record(start, PAST_END)
            produced += n
            if tokens is not None:
                tokens.append(("stored", bytes(z[at:at + n])))
        elif btype == 3:
            return unit_record(start, BAD_HEADER)
        else:
            llen, dlen = I.FIXED_LLEN, I.FIXED_DLEN
            if btype == 2:
                status, pos, llen, dlen = parse_dynamic(z, pos, nbits)
                if status != OK:
                    return unit_record(start, status)
            table, dtable = _table(llen), _table(dlen)
            while True:
                if symbols >= cap:
                    return unit_record(start, TOO_LONG)
                e = table[peek(z, pos) & 0x7fff]
                if not e:
                    return unit_record(start, PAST_END if pos + 15 > nbits else BAD_CODE)
                sym = e & 511
                pos += e >> 9
                if pos > nbits:
                    return unit_record(start, PAST_END)
                symbols += 1
                if sym < 256:
                    produced += 1
                    if tokens is not None:
                        tokens.append(("lit", sym))
                    continue
                if sym == 256:
                    break
                if sym >= 286:
                    return unit_record(start, BAD_CODE)
                first, eb = D.LENGTH_TABLE[sym - 257]
                length = first + (peek(z, pos) & ((1 << eb) - 1))
                pos += eb
                if pos > nbits:
                    return unit_record(start, PAST_END)
                e = dtable[peek(z, pos) & 0x7fff]
                if not e:
                    return unit_record(start, PAST_END if pos + 15 > nbits else BAD_CODE)
                pos += e >> 9
                if pos > nbits:
                    return unit_record(start, PAST_END)
                if (e & 511) >= 30:
                    return unit_record(start, BAD_CODE)
                first, eb = DISTANCE_TABLE[e & 511]
                distance = first + (0 if no_distance_extra else peek(z, pos) & ((1 << eb) - 1))      # MUTANT no_distance_extra: the extra bits are passed over
                pos += eb
                if pos > nbits:
                    return unit_record(start, PAST_END)
                reach = max(reach, distance - (produced + length if reach_from_end else produced))      # MUTANT reach_from_end: measured from behind the match
                far += distance != 1
                produced += length
                if tokens is not None:
                    tokens.append(("match", length, distance))
        blocks += 1
        if bfinal:
            flags |= FINAL
            break
        if pos + 3 <= nbits and (peek(z, pos) >> 1) & 3 == 2:
            break
    return unit_record(start, OK, pos, produced, symbols, blocks, flags, reach, far)


def measure(z, starts, cap=MAX_SYMBOLS, **mutant):
    z = bytes(z)
    return [decode_unit(z, s, cap, **mutant) for s in starts]


def chain(units, first_bit, n, expected, reach_off_by_one=False):
    """radnet_inflate_lz_chain: (code, bad_unit, links [(out_offset, start_bit, out_bytes, 0)], false_count)."""
    starts = {u[0]: i for i, u in enumerate(units)}
    bit, total, came_from, links = first_bit, 0, -1, []
    while True:
        i = starts.get(bit)
        if i is None:
            return CHAIN_NO_START, came_from, links, 0
        start, end, out_bytes, _, _, status, flags, reach, _, _ = units[i]
        if status != OK:
            return CHAIN_BAD_UNIT, i, links, 0
        if reach > total + (1 if reach_off_by_one else 0):             # MUTANT reach_off_by_one: one byte in front of the stream passes
            return CHAIN_REACH, i, links, 0
        links.append((total, start, out_bytes, 0))
        total += out_bytes
        if flags & FINAL:
            if total != expected:
                return CHAIN_LENGTH, i, links, 0
            if (end + 7) // 8 + 4 != n:
                return CHAIN_TRAILER, i, links, 0
            return CHAIN_OK, -1, links, len(units) - len(links)
        if end <= bit:
            return CHAIN_BAD_UNIT, i, links, 0
        came_from, bit = i, end


def emit(z, links, out_len, fill=0, fill_src=0, no_mod=False, **mutant):
    """(buf uint8[out_len], src uint32[out_len]) as radnet_inflate_lz_emit leaves buffers prefilled with `fill` and `fill_src`."""
    z = bytes(z)
    buf, src = np.full(out_len, fill, np.uint8), np.full(out_len, fill_src, np.uint32)
    decode = {k: v for k, v in mutant.items() if k in ("no_distance_extra", "reach_from_end")}
    for offset, start, out_bytes, _ in links:
        tokens = []
        decode_unit(z, start, tokens=tokens, **decode)
        p, stop = offset, max(offset, min(offset + out_bytes, out_len))
        for t in tokens:
            if t[0] == "match":
                length, dist = t[1], t[2]
                j = np.arange(max(0, min(length, stop - p)), dtype=np.int64)
                from_ = p - dist + (j if no_mod else j % dist)         # MUTANT no_mod: a run points at its own bytes, one after the other
                src[p:p + len(j)] = np.where(from_ < 0, p + j, from_)
                p += length
            else:
                data = np.frombuffer(bytes([t[1]]) if t[0] == "lit" else t[1], np.uint8)
                k = max(0, min(len(data), stop - p))
                buf[p:p + k] = data[:k]
                src[p:p + k] = np.arange(p, p + k)
                p += len(data)
    return buf, src


def resolve_round(src):
    """One launch of radnet_inflate_lz_resolve with every entry read before any is written: (the new table, entries rewritten)."""
    src = np.asarray(src, np.uint32)
    i = np.arange(len(src), dtype=np.int64)
    s = src.astype(np.int64)
    lower = s < i
    t = src[np.where(lower, s, 0)].astype(np.int64)
    jump = lower & (t < s)
    return np.where(jump, t, s).astype(np.uint32), int(jump.sum())


def resolve(src):
    """(the flat table, the rounds that rewrote an entry)."""
    rounds = 0
    while True:
        nxt, changed = resolve_round(src)
        if not changed:
            return np.asarray(src, np.uint32), rounds
        src, rounds = nxt, rounds + 1


def gather(buf, src):
    """radnet_inflate_lz_gather: buf[i] = buf[src[i]] where src[i] < i."""
    buf = np.asarray(buf, np.uint8)
    i = np.arange(len(buf), dtype=np.int64)
    s = np.asarray(src).astype(np.int64)
    lower = s < i
    return np.where(lower, buf[np.where(lower, s, 0)], buf)


def inflate(z, expected, cap=MAX_SYMBOLS, **mutant):
    """The whole path on a zlib stream: (bytes or None, reason or None, dict(candidates, false_candidates, units, blocks, rounds,
    far_units))."""
    z = bytes(z)
    stats = dict(candidates=0, false_candidates=0, units=0, blocks=0, rounds=0, far_units=0)
    if len(z) < 7 or not I.zlib_header_ok(z):
        return None, "zlib header", stats
    cands = find_blocks(z, 16)
    starts = sorted(set(cands) | {16})
    decode = {k: v for k, v in mutant.items() if k in ("no_distance_extra", "reach_from_end")}
    units = measure(z, starts, cap, **decode)
    stats["candidates"] = len(cands)
    code, bad, links, false_count = chain(units, 16, len(z), expected, reach_off_by_one=mutant.get("reach_off_by_one", False))
    if code != CHAIN_OK:
        why = "chain: " + CHAIN_NAMES[code]
        if code == CHAIN_BAD_UNIT:
            why += " (%s)" % I.STATUS_NAMES[units[bad][5]]
        return None, why, stats
    by_start = {u[0]: u for u in units}
    stats.update(false_candidates=false_count, units=len(links), blocks=sum(by_start[l[1]][4] for l in links),
                 far_units=sum(by_start[l[1]][8] > 0 for l in links))
    buf, src = emit(z, links, expected, no_mod=mutant.get("no_mod", False), **decode)
    flat, stats["rounds"] = resolve(src)
    out = gather(buf, src if mutant.get("gather_before_flat") else flat).tobytes()      # MUTANT gather_before_flat: the bytes of a match are not there yet
    if zlib.adler32(out) != struct.unpack(">I", z[-4:])[0]:
        return None, "adler", stats
    return out, None, stats


# ---- the case table ------------------------------------------------------------------------------------------------------------------
def _deflate(data, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, mem, strategy)
    return c.compress(data) + c.flush()


def hand_stream(lead=32768):
    """(zlib stream, data): ONE final fixed-code block, assembled by hand, of `lead` literals and then matches zlib never emits itself
    or that strain the source rule: length 258 at distance 32768 (the last value of distance symbol 29), length 10 at distance 24577
    (its first), length 258 at distance 2 and at distance 257, a literal and a run of 3.  With lead = 32768 the first match copies
    from byte 0; with one literal fewer it reaches one byte in front of the stream."""
    rs = np.random.RandomState(77)
    lengths, codes = D.fixed_code()
    w, data = D.BitWriter(), bytearray()
    w.put(3, 3)                                                       # BFINAL 1, BTYPE 01

    def lit(v):
        w.code(codes[v], lengths[v])
        data.append(v)

    def match(length, distance):
        s, eb, extra = D.length_symbol(length)
        w.code(codes[s], lengths[s])
        w.put(extra, eb)
        s, eb, extra = distance_symbol(distance)
        w.code(s, 5)
        w.put(extra, eb)
        for _ in range(length):
            data.append(data[-distance] if distance <= len(data) else 0x33)      # the twin: no such byte; its Adler-32 fits no buffer's fill
    for v in rs.randint(0, 256, lead).tolist():
        lit(v)
    for length, distance in ((258, 32768), (10, 24577), (258, 2), (258, 257)):
        match(length, distance)
    lit(200)
    match(3, 1)
    w.code(codes[256], lengths[256])
    w.pad()
    return b"\x78\x01" + w.bytes() + struct.pack(">I", zlib.adler32(bytes(data))), bytes(data)


Case = I.Case
REACH_REASON = "chain: " + CHAIN_NAMES[CHAIN_REACH]
# what this project refuses and zlib does not: a unit above the symbol cap, bytes between the final block and the Adler-32
OWN_REFUSALS = ("h unit cap", "j bytes behind the final block")
FROM_RLE = I.ELIGIBLE + ("h unit cap", "i level 6", "i distance 2", "j flipped bit", "j truncated", "j bytes behind the final block", "j wrong adler",
                         "k incomplete header")


@functools.lru_cache(maxsize=1)
def cases():
    """{name: Case(name, z, data, expected, reason, corrupt)}; reason None for a stream the device path takes.  The cases of
    tests/inflate_cases.py (its run-length streams, which must give the same bytes here; its level-6 and distance-2 streams, now
    taken; its unit above the cap and its corrupt streams, still refused) and: four-valued noise at level 6 and memLevel 1 (85 units,
    every one reaching thousands of bytes into those in front of it) and in a 512-byte window; noise, zeros, random bytes and noise
    again at memLevel 2 and with the fixed code; 200,000 zeros (one literal and runs); a period of 256; 1, 2 and 300 bytes at level
    6; the hand-assembled stream and its twin that reaches one byte in front of the stream."""
    out = []
    for name in FROM_RLE:
        c, k = I.cases()[name], Case()
        k.name, k.z, k.data, k.expected, k.corrupt = c.name, c.z, c.data, c.expected, c.corrupt
        k.reason = None if name in ("i level 6", "i distance 2") else c.reason
        out.append(k)
    rs = np.random.RandomState(1)
    low = rs.randint(0, 4, (120, 481)).astype(np.uint8).tobytes()
    mix = low[:20000] + bytes(70000) + rs.randint(0, 256, 70000).astype(np.uint8).tobytes() + low[:20000]
    out.append(I._case("noise memlevel 1", _deflate(low, mem=1)))
    out.append(I._case("noise window 512", _deflate(low, wbits=9)))
    out.append(I._case("mix memlevel 2", _deflate(mix, mem=2)))
    out.append(I._case("mix fixed", _deflate(mix, strategy=zlib.Z_FIXED)))
    out.append(I._case("zeros", _deflate(bytes(200000))))
    out.append(I._case("period 256", _deflate(bytes(range(256)) * 300)))
    for n in (1, 2, 300):
        out.append(I._case("level 6, %d bytes" % n, _deflate(low[:n])))
    z, data = hand_stream()
    out.append(I._case("hand far", z, data=data))
    z, data = hand_stream(32767)
    out.append(I._case("hand far twin", z, data=None, expected=len(data), reason=REACH_REASON, corrupt=True))
    return {c.name: c for c in out}


ELIGIBLE = tuple(n for n in I.ELIGIBLE) + ("i level 6", "i distance 2", "noise memlevel 1", "noise window 512", "mix memlevel 2", "mix fixed", "zeros",
                                           "period 256", "level 6, 1 bytes", "level 6, 2 bytes", "level 6, 300 bytes", "hand far")
# the rounds a sweep over all entries at once (Jacobi) needs on these streams, counted once and pinned; the kernel, in place, needs
# no more: after r rounds an entry points 2^r links up its path or at the root, whichever values of the others it read
ROUNDS = {"i level 6": 5, "noise memlevel 1": 5, "noise window 512": 7, "mix memlevel 2": 9, "mix fixed": 9, "zeros": 10, "period 256": 9}
CAUGHT_BY = {"no_mod": "zeros", "no_distance_extra": "hand far", "reach_from_end": "hand far twin", "reach_off_by_one": "hand far twin",
             "gather_before_flat": "noise memlevel 1"}


def idat_of(data):
    """(the chunks in front of the first IDAT, the joined IDAT payloads) of a PNG file."""
    pos, head, idat = 8, [], b""
    while pos < len(data):
        length, kind = struct.unpack(">I4s", data[pos:pos + 8])
        if kind == b"IDAT":
            idat += data[pos + 8:pos + 8 + length]
        elif kind != b"IEND":
            head.append(data[pos:pos + 12 + length])
        pos += 12 + length
    return head, idat


@functools.lru_cache(maxsize=1)
def png_files():
    """[(what, file bytes)] the end-to-end test decodes, as png_cases.encode writes them at level 6: every legal colour type and
    depth at 13x17, plain and Adam7, with random filter types; 120x160 four-valued RGB noise with adaptive filters, and that file
    with its IDAT stream deflated again at memLevel 1 (blocks of 128 symbols that reach into each other)."""
    import png_cases as K
    rs = np.random.RandomState(31)
    out = []
    for color, depth in K.LEGAL:
        for interlace in (False, True):
            pal = rs.randint(0, 256, (1 << min(depth, 8), 3)) if color == 3 else None
            enc = K.encode(K.draw(rs, 13, 17, color, depth), color, depth, filters=rs, interlace=interlace, palette=pal, idat_sizes=(3, 1, 40) if interlace else None)
            out.append(("colour type %d, depth %d%s" % (color, depth, ", Adam7" if interlace else ""), enc.data))
    enc = K.encode(K.draw(np.random.RandomState(5), 120, 160, 2, 8, "low").astype(np.uint8), 2, 8, filters="adaptive")
    out.append(("low noise", enc.data))
    head, idat = idat_of(enc.data)
    z = _deflate(zlib.decompress(idat), mem=1)
    out.append(("low noise, memlevel 1", b"".join([K.SIGNATURE] + head + [K.chunk(b"IDAT", z), K.chunk(b"IEND")])))
    return out


@functools.lru_cache(maxsize=None)
def model(name):
    """inflate() of a case, computed once and shared: (bytes or None, reason, stats)."""
    c = cases()[name]
    return inflate(c.z, c.expected)


@functools.lru_cache(maxsize=None)
def model_units(name):
    """(starts, unit records) of a case, computed once and shared."""
    c = cases()[name]
    starts = sorted(set(find_blocks(c.z, 16)) | {16})
    return starts, measure(c.z, starts)


@functools.lru_cache(maxsize=None)
def model_buffers(name, fill, fill_src):
    """(links, buf after emit, src after emit, flat src, rounds, buf after gather) of a case whose chain is accepted, in buffers of
    `expected` entries prefilled with the sentinels; computed once, shared and never written."""
    c = cases()[name]
    code, _, links, _ = chain(model_units(name)[1], 16, len(c.z), c.expected)
    assert code == CHAIN_OK, name
    buf, src = emit(c.z, links, c.expected, fill, fill_src)
    flat, rounds = resolve(src)
    out = gather(buf, flat)
    for a in (buf, src, flat, out):
        a.setflags(write=False)
    return links, buf, src, flat, rounds, out
