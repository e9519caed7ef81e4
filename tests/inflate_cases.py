"""The device inflate's contract (include/radnet_hip.h, "THE READING RULE") in plain Python, and the cases its tests share.  Imports
nothing from the product but, lazily, the writers whose streams case (g) reads.
  peek / parse_dynamic: RFC 1951's bit order and zlib's acceptance rule for a dynamic block header, with the order of the checks
    the kernels keep (a position beyond the stream ends the parse before the value is looked at).
  find_blocks: the rule at every bit offset (a NumPy sieve for BTYPE, the counts and the code-length code's Kraft sum, then the
    exact rule on what is left).
  decode_unit / measure / emit: one unit -- consecutive blocks up to the next dynamic header or the final block --, its record, its bytes.
  chain: radnet_inflate_chain.   inflate: the whole path, or the reason it refuses.
  MUTANTS: deliberate mistakes (keyword switches of the functions above) that the tests must catch.
  cases(): the case table, built once."""
import functools
import struct
import zlib

import numpy as np

import deflate_cases as D

MAX_SYMBOLS = 1 << 18
OK, BAD_HEADER, BAD_CODE, NOT_RLE, STORED_MISMATCH, PAST_END, TOO_LONG = range(7)
STATUS_NAMES = ("ok", "bad header", "bad code", "not run-length", "stored length mismatch", "ran past the stream", "unit too long")
FINAL, LEAD_MATCH, LAST_KNOWN = 1, 2, 4
CHAIN_OK, CHAIN_NO_START, CHAIN_BAD_UNIT, CHAIN_LEAD_MATCH, CHAIN_LENGTH, CHAIN_TRAILER = range(6)
CHAIN_NAMES = ("ok", "an end bit that is no measured start", "a unit that did not decode", "a match with nothing in front of it",
               "the inflated length differs", "the final block does not end 4 bytes before the stream's end")
UNIT_FIELDS = ("start_bit", "end_bit", "out_bytes", "symbols", "blocks", "status", "flags", "last_byte")
MUTANTS = ("end_off_by_one", "no_inherit", "no_stored_tail", "accept_incomplete", "ignore_distance")
FIXED_LLEN = tuple([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DLEN = tuple([5] * 32)


def peek(z, pos):
    """32 bits of the stream from bit `pos` on, zero beyond it."""
    b = pos >> 3
    return (int.from_bytes(z[b:b + 5], "little") >> (pos & 7)) & 0xffffffff


def parse_dynamic(z, pos, nbits, accept_incomplete=False):
    """The dynamic block header behind BFINAL and BTYPE: (status, position behind it, literal/length lengths [288], distance lengths [32])."""
    v = peek(z, pos)
    pos += 14
    if pos > nbits:
        return PAST_END, pos, None, None
    nlen, ndist, ncode = 257 + (v & 31), 1 + ((v >> 5) & 31), 4 + ((v >> 10) & 15)
    if nlen > 286 or ndist > 30:
        return BAD_HEADER, pos, None, None
    cl = [0] * 19
    for i in range(ncode):
        cl[D.CODE_LENGTH_ORDER[i]] = peek(z, pos) & 7
        pos += 3
    if pos > nbits:
        return PAST_END, pos, None, None
    if sum(128 >> v for v in cl if v) != 128:
        return BAD_HEADER, pos, None, None
    codes = D.canonical_codes(cl)
    lookup = {(l, D.reverse_bits(c, l)): s for s, (l, c) in enumerate(zip(cl, codes)) if l}
    total, lens, prev = nlen + ndist, [], 0
    while len(lens) < total:
        v = peek(z, pos)
        for l in range(1, 8):
            sym = lookup.get((l, v & ((1 << l) - 1)))
            if sym is not None:
                break
        else:
            return BAD_HEADER, pos, None, None
        pos += l
        if pos > nbits:
            return PAST_END, pos, None, None
        rep, val = 1, sym
        if sym >= 16:
            if sym == 16 and not lens:
                return BAD_HEADER, pos, None, None
            eb = 2 if sym == 16 else 3 if sym == 17 else 7
            rep = (11 if sym == 18 else 3) + (peek(z, pos) & ((1 << eb) - 1))
            pos += eb
            if pos > nbits:
                return PAST_END, pos, None, None
            val = prev if sym == 16 else 0
            if len(lens) + rep > total:
                return BAD_HEADER, pos, None, None
        prev = val
        lens += [val] * rep
    llen, dlen = lens[:nlen], lens[nlen:]
    if not llen[256]:
        return BAD_HEADER, pos, None, None
    complete = lambda ls: D.kraft(ls) == 1 << 15 or [v for v in ls if v] == [1]      # noqa: E731
    if not complete(llen) and not accept_incomplete:              # MUTANT accept_incomplete: an incomplete literal/length code passes
        return BAD_HEADER, pos, None, None
    if any(dlen) and not complete(dlen):
        return BAD_HEADER, pos, None, None
    return OK, pos, tuple(llen + [0] * (288 - nlen)), tuple(dlen + [0] * (32 - ndist))


def find_blocks(z, first_bit, **mutant):
    """The sorted bit offsets at which a dynamic block header that zlib accepts begins."""
    z = bytes(z)
    nbits = 8 * len(z)
    bits = np.concatenate([np.unpackbits(np.frombuffer(z, np.uint8), bitorder="little"), np.zeros(96, np.uint8)]).astype(np.int32)
    p = np.arange(first_bit, nbits)
    field = lambda at, width: sum(bits[p + at + k] << k for k in range(width))      # noqa: E731
    keep = (field(1, 2) == 2) & (field(3, 5) <= 29) & (field(8, 5) <= 29)
    p = p[keep]
    ncode = 4 + field(13, 4)
    kraft = np.zeros(len(p), np.int64)
    for i in range(19):
        l = np.where(i < ncode, field(17 + 3 * i, 3), 0)
        kraft += np.where(l > 0, 128 >> l, 0)
    out = []
    for q in p[kraft == 128].tolist():
        if parse_dynamic(z, q + 3, nbits, **mutant)[0] == OK:
            out.append(q)
    return out


@functools.lru_cache(maxsize=64)
def _table(lens):
    """[symbol | length << 9] by the 15 bits that follow in the stream, 0 where no code word begins them."""
    t = np.zeros(1 << 15, np.int32)
    for s, (l, c) in enumerate(zip(lens, D.canonical_codes(lens))):
        if l:
            t[D.reverse_bits(c, l)::1 << l] = s | (l << 9)
    return t.tolist()


def unit_record(start, status=OK, end=0, out_bytes=0, symbols=0, blocks=0, flags=0, last=0):
    if status != OK:
        return (start, 0, 0, 0, 0, status, 0, 0)
    return (start, end, out_bytes, symbols, blocks, OK, flags, last if flags & LAST_KNOWN else 0)


def decode_unit(z, start, cap=MAX_SYMBOLS, out=None, prev=0, tokens=None, end_off_by_one=False, no_stored_tail=False, ignore_distance=False,
                accept_incomplete=False):
    """The record (UNIT_FIELDS) of the unit that begins at bit `start`; its bytes are appended to `out` (a bytearray) and its tokens
    (("lit", byte), ("match", length), ("stored", bytes), ("eob", btype)) to `tokens` if given."""
    nbits = 8 * len(z)
    if start >= nbits:
        return unit_record(start, PAST_END)
    pos, symbols, blocks, produced, flags, last, seen = start, 0, 0, 0, 0, 0, False
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
            src = pos >> 3
            pos += 8 * n
            if pos > nbits:
                return unit_record(start, PAST_END)
            if n:
                prev = last = z[src + n - 1]
                flags, seen, produced = flags | LAST_KNOWN, True, produced + n
                if out is not None:
                    out += z[src:src + n]
            if tokens is not None:
                tokens.append(("stored", bytes(z[src:src + n])))
        elif btype == 3:
            return unit_record(start, BAD_HEADER)
        else:
            llen, dlen = FIXED_LLEN, FIXED_DLEN
            if btype == 2:
                status, pos, llen, dlen = parse_dynamic(z, pos, nbits, accept_incomplete)
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
                    prev = last = sym
                    flags, seen, produced = flags | LAST_KNOWN, True, produced + 1
                    if out is not None:
                        out.append(sym)
                    if tokens is not None:
                        tokens.append(("lit", sym))
                    continue
                if sym == 256:
                    if tokens is not None:
                        tokens.append(("eob", btype))
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
                if (e & 511) != 0 and not ignore_distance:            # MUTANT ignore_distance: every match is taken for distance 1
                    return unit_record(start, NOT_RLE)
                if not seen:
                    seen, flags = True, flags | LEAD_MATCH
                produced += length
                if out is not None:
                    out += bytes([prev]) * length
                if tokens is not None:
                    tokens.append(("match", length))
        blocks += 1
        if bfinal:
            flags |= FINAL
            break
        if pos + 3 <= nbits and (peek(z, pos) >> 1) & 3 == 2:
            break
        if no_stored_tail:                                            # MUTANT no_stored_tail: a stored or fixed block is left to the next unit
            break
    return unit_record(start, OK, pos + (1 if end_off_by_one else 0), produced, symbols, blocks, flags, last)      # MUTANT end_off_by_one


def measure(z, starts, cap=MAX_SYMBOLS, **mutant):
    """The records of the units that begin at `starts`."""
    z = bytes(z)
    return [decode_unit(z, s, cap, **mutant) for s in starts]


def chain(units, first_bit, n, expected, no_inherit=False):
    """radnet_inflate_chain: (code, bad_unit, links [(out_offset, start_bit, out_bytes, prev_byte)], false_count)."""
    starts = {u[0]: i for i, u in enumerate(units)}
    bit, total, came_from, links, have_prev, prev = first_bit, 0, -1, [], False, 0
    while True:
        i = starts.get(bit)
        if i is None:
            return CHAIN_NO_START, came_from, links, 0
        start, end, out_bytes, _, _, status, flags, last = units[i]
        if status != OK:
            return CHAIN_BAD_UNIT, i, links, 0
        if flags & LEAD_MATCH and not have_prev:
            return CHAIN_LEAD_MATCH, i, links, 0
        links.append((total, start, out_bytes, prev if have_prev else 0))
        total += out_bytes
        if flags & LAST_KNOWN:
            prev, have_prev = last, True
        elif no_inherit:                                              # MUTANT no_inherit: a unit without a known byte hands on nothing
            prev = 0
        if flags & FINAL:
            if total != expected:
                return CHAIN_LENGTH, i, links, 0
            if (end + 7) // 8 + 4 != n:
                return CHAIN_TRAILER, i, links, 0
            return CHAIN_OK, -1, links, len(units) - len(links)
        if end <= bit:
            return CHAIN_BAD_UNIT, i, links, 0
        came_from, bit = i, end


def emit(z, links, out_len, fill=0, **mutant):
    """The bytes radnet_inflate_rle_emit writes into a buffer of out_len bytes prefilled with `fill`."""
    z, out = bytes(z), bytearray([fill]) * out_len
    for offset, start, out_bytes, prev in links:
        got = bytearray()
        decode_unit(z, start, out=got, prev=prev, **{k: v for k, v in mutant.items() if k != "no_inherit"})
        got = got[:max(0, min(out_bytes, out_len - offset))]
        out[offset:offset + len(got)] = got
    return bytes(out)


def zlib_header_ok(z):
    """CM 8, a window of at most 32 KiB, FCHECK, no preset dictionary."""
    return len(z) >= 2 and z[0] & 15 == 8 and z[0] >> 4 <= 7 and (z[0] * 256 + z[1]) % 31 == 0 and not z[1] & 32


def inflate(z, expected, cap=MAX_SYMBOLS, **mutant):
    """The whole path on a zlib stream: (bytes or None, reason or None, dict(candidates, false_candidates, units, blocks))."""
    z = bytes(z)
    stats = dict(candidates=0, false_candidates=0, units=0, blocks=0)
    if len(z) < 7 or not zlib_header_ok(z):
        return None, "zlib header", stats
    find = {k: v for k, v in mutant.items() if k == "accept_incomplete"}
    cands = find_blocks(z, 16, **find)
    starts = sorted(set(cands) | {16})
    units = measure(z, starts, cap, **{k: v for k, v in mutant.items() if k != "no_inherit"})
    stats["candidates"] = len(cands)
    code, bad, links, false_count = chain(units, 16, len(z), expected, **{k: v for k, v in mutant.items() if k == "no_inherit"})
    if code != CHAIN_OK:
        why = "chain: " + CHAIN_NAMES[code]
        if code == CHAIN_BAD_UNIT:
            why += " (%s)" % STATUS_NAMES[units[bad][5]]
        return None, why, stats
    by_start = {u[0]: u for u in units}
    stats.update(false_candidates=false_count, units=len(links), blocks=sum(by_start[l[1]][4] for l in links))
    out = emit(z, links, expected, **mutant)
    if zlib.adler32(out) != struct.unpack(">I", z[-4:])[0]:
        return None, "adler", stats
    return out, None, stats


def true_dynamic_starts(z):
    """The bit offsets of the dynamic blocks of a zlib stream, by a straight walk from bit 16 (every block, no speculation)."""
    z, pos, out = bytes(z), 16, []
    nbits = 8 * len(z)
    while True:
        v = peek(z, pos)
        if (v >> 1) & 3 == 2:
            out.append(pos)
        # one block: a unit cut behind every block
        rec = decode_unit(z, pos, no_stored_tail=True, ignore_distance=True)
        assert rec[5] == OK, (pos, STATUS_NAMES[rec[5]])
        if rec[6] & FINAL:
            return out
        pos = rec[1]
        assert pos < nbits


# ---- the case table ------------------------------------------------------------------------------------------------------------------
def rgb_panel_stream(h=300, w=401):
    """The Sub-filtered stream of an RGB panel: smooth shading with flat regions and a little noise (D.panel_stream in three channels)."""
    rs = np.random.RandomState(7)
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([(x // 7 * (c + 1) + (y // 5) * 3 + (rs.randint(0, 3, (h, w)) * (rs.rand(h, w) < 0.2))) & 255 for c in range(3)], axis=2)
    img[h // 4:h // 2, w // 3:] = (200, 90, 10)
    img = img.astype(np.uint8)
    lines = np.empty((h, 1 + 3 * w), np.uint8)
    lines[:, 0] = 1
    lines[:, 1:4] = img[:, 0]
    lines[:, 4:] = (img[:, 1:] - img[:, :-1]).reshape(h, -1)
    return lines.tobytes()


def _deflate(data, level=1, mem=8, strategy=zlib.Z_RLE):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, mem, strategy)
    return c.compress(data) + c.flush()


def fixed_literals(count):
    """One final fixed-code block of `count` literals below 144 (8-bit codes 0x30 + v, most significant bit first), no two equal
    neighbours: (zlib stream, data)."""
    data = ((np.arange(count) * 37) % 143).astype(np.uint8)
    codes = np.unpackbits((data + 0x30)[:, None], axis=1)             # most significant bit first, as the stream takes a code
    bits = np.concatenate([np.array([1, 1, 0], np.uint8), codes.reshape(-1), np.zeros(7, np.uint8)])
    body = np.packbits(bits, bitorder="little").tobytes()
    return b"\x78\x01" + body + struct.pack(">I", zlib.adler32(data.tobytes())), data.tobytes()


def recode_fixed(z, far_match=None):
    """(zlib stream, data): the tokens of the zlib stream z written again as ONE final fixed-code block; match number far_match gets
    distance 2 (symbol 1) instead of distance 1, and the data is what that inflates to."""
    tokens, pos, z = [], 16, bytes(z)
    while True:
        rec = decode_unit(z, pos, tokens=tokens)
        assert rec[5] == OK
        if rec[6] & FINAL:
            break
        pos = rec[1]
    lengths, codes = D.fixed_code()
    w, matches, data = D.BitWriter(), 0, bytearray()
    w.put(3, 3)                                                       # BFINAL 1, BTYPE 01
    for kind, v in tokens:
        if kind == "lit":
            w.code(codes[v], lengths[v])
            data.append(v)
        elif kind == "match":
            s, eb, extra = D.length_symbol(v)
            w.code(codes[s], lengths[s])
            w.put(extra, eb)
            far = 2 if matches == far_match else 1
            w.code(far - 1, 5)
            matches += 1
            for _ in range(v):
                data.append(data[-far])
        elif kind == "stored":
            for b in v:
                w.code(codes[b], lengths[b])
            data += v
    assert far_match is None or matches > far_match
    w.code(codes[256], lengths[256])
    w.pad()
    return b"\x78\x01" + w.bytes() + struct.pack(">I", zlib.adler32(bytes(data))), bytes(data)


def incomplete_header_stream():
    """A final dynamic block whose literal/length code is INCOMPLETE (literal 0: 1 bit, end-of-block: 2 bits; Kraft sum 3/4) and is
    otherwise well formed: zlib refuses it ("invalid literal/lengths set").  Followed by zero bytes so that nothing ends early."""
    lengths = [0] * 286
    lengths[0], lengths[256] = 1, 2
    header, nbits = D.dynamic_header(lengths)
    return b"\x78\x01" + bytes([header[0] | 1]) + header[1:] + bytes(64)


Case = type("Case", (), {})


def _case(name, z, data=None, reason=None, **extra):
    c = Case()
    c.name, c.z, c.reason = name, bytes(z), reason
    c.corrupt = bool(extra.pop("corrupt", False))
    c.data = zlib.decompress(c.z) if data is None and reason is None and not c.corrupt else data
    c.expected = len(c.data) if c.data is not None else extra.pop("expected", 0)
    for k, v in extra.items():
        setattr(c, k, v)
    return c


@functools.lru_cache(maxsize=1)
def cases():
    """{name: Case(name, z, data, expected, reason)}: reason None for a stream the device path takes (data = what it inflates to), else
    the reason inflate() gives; every stream is small.
    (a) a 300x401 RGB panel, Sub on every row, level 1 / Z_RLE / memLevel 8; (b) 30 KB at memLevel 1: blocks of 128 symbols, ends on
    every bit phase; (c) a sync flush at the very start (the first block is stored), one in the middle and a full flush; (d) level 0:
    70 KB of stored blocks whose payload holds the first 60,000 compressed bytes of (a), valid headers the chain never visits; (e) 200 KB
    of one byte at memLevel 1: units of matches alone; (f) 1, 2 and 300 bytes; (g) the deflate model's dynamic and fixed streams (and,
    in package_cases, png.assemble's); (h) one fixed block of more than MAX_SYMBOLS literals; (i) level 6, and the tokens of (b) written
    again with the fixed code (a dynamic header of (b) has no code for another distance) with one match at distance 2; (j) a flipped
    bit, a truncated stream, bytes behind the final block, a wrong Adler-32; (k) a header with an incomplete literal/length code."""
    rs = np.random.RandomState(23)
    noise = lambda n: rs.randint(0, 256, n).astype(np.uint8).tobytes()      # noqa: E731
    out = []
    panel, grey = rgb_panel_stream(), D.panel_stream()
    za = _deflate(panel)
    out.append(_case("a cv2-like", za))
    zb = _deflate(grey[:30000], mem=1)
    out.append(_case("b memlevel 1", zb))
    c = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    zc = c.flush(zlib.Z_SYNC_FLUSH) + c.compress(grey[:40000]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(grey[40000:70000]) + c.flush(zlib.Z_FULL_FLUSH)
    zc += c.compress(grey[70000:]) + c.flush()
    out.append(_case("c flushes", zc))
    out.append(_case("d stored with buried headers", zlib.compress(noise(6000) + za[:60000] + noise(4000), 0)))
    out.append(_case("e long runs", _deflate(b"\x5a" * 200000, mem=1)))
    for n in (1, 2, 300):
        out.append(_case("f %d bytes" % n, _deflate(grey[1000:1000 + n])))
    small = grey[:3 * 401 * 40 // 3][:402 * 60]
    out.append(_case("g deflate model dynamic", D.zlib_stream(small, 8192, 4096, "dynamic")))
    out.append(_case("g deflate model fixed", D.zlib_stream(small, 8192, 4096, "fixed")))
    zh, data = fixed_literals(MAX_SYMBOLS + 40)
    out.append(_case("h unit cap", zh, data=data, reason="chain: a unit that did not decode (unit too long)"))
    z6 = zlib.compress(grey[:20000], 6)
    out.append(_case("i level 6", z6, data=grey[:20000], reason="chain: a unit that did not decode (not run-length)"))
    (zfar, far), (znear, near) = recode_fixed(zb, far_match=5), recode_fixed(zb)
    assert zlib.decompress(zfar) == far != near and zlib.decompress(znear) == near == grey[:30000]
    out.append(_case("i distance 2", zfar, data=far, reason="chain: a unit that did not decode (not run-length)"))
    flipped = bytearray(za)
    flipped[len(za) // 3] ^= 0x10
    out.append(_case("j flipped bit", flipped, expected=len(panel), reason=None, data=None, corrupt=True))
    out.append(_case("j truncated", za[:-1000], expected=len(panel), data=None, corrupt=True))
    out.append(_case("j bytes behind the final block", za + b"behind", data=panel, reason="chain: " + CHAIN_NAMES[CHAIN_TRAILER]))
    out.append(_case("j wrong adler", za[:-1] + bytes([za[-1] ^ 1]), expected=len(panel), data=None, reason="adler", corrupt=True))
    out.append(_case("k incomplete header", incomplete_header_stream(), expected=10, data=None, corrupt=True,
                     reason="chain: a unit that did not decode (bad header)"))
    return {c.name: c for c in out}


def package_cases():
    """Case (g), the package's own host writer: the IDAT payload of png.assemble for a small Sub-filtered grey panel, cut into several
    pieces (each ends in a sync flush: units with stored tails)."""
    from faster_rcnn import png
    stream = D.panel_stream(60, 401)
    data = png.assemble(stream, 401, 60, 0, chunk_bytes=5000, workers=1)
    pos, idat = 8, b""
    while pos < len(data):
        length, kind = struct.unpack(">I4s", data[pos:pos + 8])
        if kind == b"IDAT":
            idat += data[pos + 8:pos + 8 + length]
        pos += 12 + length
    return {"g png.assemble": _case("g png.assemble", idat)}


ELIGIBLE = ("a cv2-like", "b memlevel 1", "c flushes", "d stored with buried headers", "e long runs", "f 1 bytes", "f 2 bytes", "f 300 bytes",
            "g deflate model dynamic", "g deflate model fixed")


@functools.lru_cache(maxsize=None)
def model(name):
    """inflate() of a case, computed once and shared: (bytes or None, reason, stats)."""
    c = {**cases(), **(package_cases() if name == "g png.assemble" else {})}[name]
    return inflate(c.z, c.expected)


@functools.lru_cache(maxsize=None)
def model_units(name):
    """(sorted candidates, starts, unit records) of a case, computed once and shared."""
    c = cases()[name]
    cands = find_blocks(c.z, 16)
    starts = sorted(set(cands) | {16})
    return cands, starts, measure(c.z, starts)
