"""The device deflate's contract (include/radnet_hip.h, "THE TOKEN RULE") in plain Python, and the cases its tests share.  Imports
nothing from the product.
  tokens / histogram: the tokeniser -- chunks, tiles, maximal runs, literal + 258-matches + rest -- and the symbol counts it gives.
  BitWriter, canonical_codes, fixed_code, dynamic_header / parse_header: RFC 1951's bit order, code numbering, fixed code and the
    simplest dynamic header (and its inverse, a parser that reads ANY dynamic header back to its lengths).
  limited_lengths: a length-limited Huffman code by package-merge, independent of the product's Huffman-and-repair builder.
  piece / pieces / zlib_stream: a chunk's deflate block with the sync flush, all of them, and the zlib stream round them.
  adler_parts / adler_combine: the per-chunk sums radnet_deflate_rle_scan_u8 writes and the Adler-32 the host makes of them.
  MUTANTS: deliberate mistakes (keyword switches of the functions above) that the tests must catch.
  streams(chunk, tile): the case table."""
import struct
import zlib

import numpy as np

SYMBOLS, EOB, MAX_BITS = 286, 256, 15
# RFC 1951, 3.2.5: (first length, extra bits) of the length symbols 257..285
LENGTH_TABLE = [(3, 0), (4, 0), (5, 0), (6, 0), (7, 0), (8, 0), (9, 0), (10, 0), (11, 1), (13, 1), (15, 1), (17, 1), (19, 2), (23, 2), (27, 2), (31, 2),
                (35, 3), (43, 3), (51, 3), (59, 3), (67, 4), (83, 4), (99, 4), (115, 4), (131, 5), (163, 5), (195, 5), (227, 5), (258, 0)]
CODE_LENGTH_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
MUTANTS = ("cut259", "rest2_match", "lsb_codes", "no_sync", "adler_no_length")


def length_symbol(length):
    """(symbol, extra bits, extra value) of a match length 3..258."""
    if length == 258:
        return 285, 0, 0
    for k in range(len(LENGTH_TABLE) - 2, -1, -1):
        first, extra_bits = LENGTH_TABLE[k]
        if length >= first:
            if length - first >= 1 << extra_bits:
                break
            return 257 + k, extra_bits, length - first
    raise ValueError("no length symbol for a match of %d bytes" % length)


def run_tokens(value, length, cut259=False, rest2_match=False):
    """The tokens of one run inside a tile: ("lit", byte) and ("match", length)."""
    if cut259 and length > 259:                        # MUTANT: the run is cut every 259 bytes instead of being coded as one
        out = []
        for s in range(0, length, 259):
            out += run_tokens(value, min(259, length - s), rest2_match=rest2_match)
        return out
    out = [("lit", value)] + [("match", 258)] * ((length - 1) // 258)
    rest = (length - 1) % 258
    if rest >= 3 or (rest2_match and rest == 2):       # MUTANT: a rest of 2 as a match, which deflate cannot code
        out.append(("match", rest))
    else:
        out += [("lit", value)] * rest
    return out


def tokens(data, chunk, tile, **mutant):
    """[tokens of chunk 0, tokens of chunk 1, ...] of a byte string."""
    data = np.frombuffer(bytes(data), np.uint8)
    out = []
    for c0 in range(0, len(data), chunk):
        piece, toks = data[c0:c0 + chunk], []
        for t0 in range(0, len(piece), tile):
            t = piece[t0:t0 + tile]
            starts = np.concatenate([[0], np.flatnonzero(t[1:] != t[:-1]) + 1, [len(t)]])
            for s, e in zip(starts[:-1].tolist(), starts[1:].tolist()):
                toks += run_tokens(int(t[s]), e - s, **mutant)
        out.append(toks)
    return out


def histogram(data, chunk, tile):
    """The 286 counts radnet_deflate_rle_scan_u8 adds up: every token's literal/length symbol and one end-of-block per chunk."""
    hist = np.zeros(SYMBOLS, np.int64)
    for toks in tokens(data, chunk, tile):
        for kind, v in toks:
            hist[v if kind == "lit" else length_symbol(v)[0]] += 1
        hist[EOB] += 1
    return hist


class BitWriter:
    """RFC 1951, 3.1.1: bits fill a byte from its least significant end; put() takes a value least significant bit first, code()
    a Huffman code most significant bit first."""

    def __init__(self):
        self.done, self.acc, self.held, self.n = bytearray(), 0, 0, 0      # whole bytes written; the bits behind them; how many; all bits

    def put(self, value, bits):
        assert 0 <= value < (1 << bits) or bits == 0
        self.acc |= value << self.held
        self.held += bits
        self.n += bits
        if self.held >= 1024:                          # keep the integer short: the whole bytes move out
            whole = self.held // 8
            self.done += (self.acc & ((1 << (8 * whole)) - 1)).to_bytes(whole, "little")
            self.acc >>= 8 * whole
            self.held -= 8 * whole

    def code(self, code, bits, lsb_codes=False):
        self.put(code if lsb_codes else reverse_bits(code, bits), bits)      # MUTANT lsb_codes: not reversed

    def pad(self):
        self.put(0, -self.n % 8)

    def bytes(self):
        return bytes(self.done) + self.acc.to_bytes((self.held + 7) // 8, "little")


def reverse_bits(value, bits):
    return int(("{:0%db}" % bits).format(value)[::-1], 2) if bits else 0


def canonical_codes(lengths):
    """RFC 1951, 3.2.2: the code of every symbol from the lengths alone (0 where the length is 0)."""
    lengths = [int(v) for v in lengths]
    count = [0] * (MAX_BITS + 2)
    for v in lengths:
        count[v] += 1
    count[0] = 0
    nxt, code = [0] * (MAX_BITS + 2), 0
    for bits in range(1, MAX_BITS + 1):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = []
    for v in lengths:
        out.append(nxt[v] if v else 0)
        nxt[v] += 1 if v else 0
    return out


def kraft(lengths):
    """The Kraft sum of the non-zero lengths times 2^15: exactly 2^15 for a complete code."""
    return sum(1 << (MAX_BITS - int(v)) for v in lengths if v)


def limited_lengths(hist, max_bits=MAX_BITS):
    """Optimal code lengths of at most max_bits for the symbols with a count (two at least), by package-merge: max_bits rounds of
    pairing the cheapest items; a symbol's length is the number of the 2n - 2 cheapest items of the last round that hold it."""
    leaves = sorted((int(w), [s]) for s, w in enumerate(hist) if w > 0)
    assert 2 <= len(leaves) <= 1 << max_bits
    cur = list(leaves)
    for _ in range(max_bits - 1):
        merged = [(cur[i][0] + cur[i + 1][0], cur[i][1] + cur[i + 1][1]) for i in range(0, len(cur) - 1, 2)]
        cur = sorted(leaves + merged, key=lambda item: item[0])
    lengths = [0] * len(hist)
    for _, members in cur[:2 * len(leaves) - 2]:
        for s in members:
            lengths[s] += 1
    return lengths


def fixed_code():
    """(lengths, codes) of RFC 1951, 3.2.6 for the 286 symbols that occur; the codes are numbered over all 288 of the alphabet."""
    lengths = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
    return lengths[:SYMBOLS], canonical_codes(lengths)[:SYMBOLS]


def dynamic_header(lengths):
    """(bytes, bits) of the simplest dynamic block header for 286 literal/length lengths and the one-bit distance code: BFINAL 0,
    BTYPE 10, HLIT 29, HDIST 0, HCLEN 15, a code-length code of 4 bits for each of 0..15, every length as such a 4-bit code."""
    assert len(lengths) == SYMBOLS
    w = BitWriter()
    w.put(0, 1)
    w.put(2, 2)
    w.put(SYMBOLS - 257, 5)
    w.put(0, 5)
    w.put(15, 4)
    for s in CODE_LENGTH_ORDER:
        w.put(4 if s < 16 else 0, 3)
    for v in list(lengths) + [1]:
        w.code(int(v), 4)
    return w.bytes(), w.n


def fixed_header():
    return b"\x02", 3                                  # BFINAL 0, BTYPE 01


class BitReader:
    def __init__(self, data):
        self.acc, self.pos = int.from_bytes(bytes(data), "little"), 0

    def take(self, bits):
        v = (self.acc >> self.pos) & ((1 << bits) - 1)
        self.pos += bits
        return v

    def symbol(self, lengths):
        """One symbol of the canonical code with these lengths."""
        codes = canonical_codes(lengths)
        code = 0
        for bits in range(1, MAX_BITS + 1):
            code = (code << 1) | self.take(1)
            for s, v in enumerate(lengths):
                if v == bits and codes[s] == code:
                    return s
        raise ValueError("no symbol")


def parse_header(data, nbits):
    """A dynamic block header back to (bfinal, literal/length lengths, distance lengths); reads symbols 16..18 too.  Asserts that the
    header ends after nbits bits and that its code-length code is complete."""
    r = BitReader(data)
    bfinal, btype = r.take(1), r.take(2)
    assert btype == 2
    hlit, hdist, hclen = r.take(5) + 257, r.take(5) + 1, r.take(4) + 4
    cl = [0] * 19
    for s in CODE_LENGTH_ORDER[:hclen]:
        cl[s] = r.take(3)
    assert sum(1 << (7 - v) for v in cl if v) == 1 << 7
    out = []
    while len(out) < hlit + hdist:
        s = r.symbol(cl)
        if s < 16:
            out.append(s)
        elif s == 16:
            out += [out[-1]] * (3 + r.take(2))
        elif s == 17:
            out += [0] * (3 + r.take(3))
        else:
            out += [0] * (11 + r.take(7))
    assert len(out) == hlit + hdist and r.pos == nbits
    return bfinal, out[:hlit], out[hlit:]


def piece(toks, lengths, codes, header, header_nbits, dist_nbits, last, lsb_codes=False, no_sync=False):
    """The bytes of one chunk's deflate block: header, tokens, end-of-block, then the sync flush (or, last, BFINAL and padding)."""
    w = BitWriter()
    w.put(int.from_bytes(header, "little") & ((1 << header_nbits) - 1) & ~1 | (1 if last else 0), header_nbits)
    as_put = [c if lsb_codes else reverse_bits(c, n) for c, n in zip(codes, lengths)]      # MUTANT lsb_codes: not reversed
    for kind, v in toks:
        if kind == "lit":
            assert lengths[v], "literal %d has no code" % v
            w.put(as_put[v], lengths[v])
        else:
            s, extra_bits, extra = length_symbol(v)
            assert lengths[s], "length symbol %d has no code" % s
            w.put(as_put[s], lengths[s])
            w.put(extra, extra_bits)
            w.put(0, dist_nbits)
    w.put(as_put[EOB], lengths[EOB])
    if not last and not no_sync:                       # MUTANT no_sync: the pieces are byte aligned but nothing says so to inflate
        w.put(0, 3)
        w.pad()
        w.put(0xFFFF0000, 32)
    w.pad()
    return w.bytes()


def pieces(data, chunk, tile, lengths, header, header_nbits, dist_nbits, codes=None, **mutant):
    codes = canonical_codes(lengths) if codes is None else codes
    tok = {k: mutant[k] for k in ("cut259", "rest2_match") if k in mutant}
    enc = {k: mutant[k] for k in ("lsb_codes", "no_sync") if k in mutant}
    all_toks = tokens(data, chunk, tile, **tok)
    return [piece(t, lengths, codes, header, header_nbits, dist_nbits, c == len(all_toks) - 1, **enc) for c, t in enumerate(all_toks)]


def adler_parts(data, chunk):
    """[[sum(byte), sum((len - i) * byte)] per chunk], exact."""
    data = np.frombuffer(bytes(data), np.uint8).astype(np.uint64)
    out = []
    for c0 in range(0, len(data), chunk):
        p = data[c0:c0 + chunk]
        out.append([int(p.sum()), int((p * np.arange(len(p), 0, -1, dtype=np.uint64)).sum())])
    return out


def adler_combine(parts, n, chunk, adler_no_length=False):
    a, b = 1, n
    for c, (s1, s2) in enumerate(parts):
        behind = n - min(n, (c + 1) * chunk)           # the bytes of the stream behind this chunk: each sees the chunk's sum once more
        a += s1
        b += s2 + (0 if adler_no_length else behind * s1)      # MUTANT: the chunks summed as if each stood at the end
    return ((b % 65521) << 16) | (a % 65521)


def zlib_stream(data, chunk, tile, huffman="dynamic", lengths=None, header=None, **mutant):
    """78 01, the pieces, the Adler-32.  huffman "dynamic": the model's own package-merge code and header unless lengths (and
    header = (bytes, bits)) are given; "fixed": the fixed code."""
    codes = None
    if huffman == "fixed":
        (lengths, codes), (hdr, nbits), dist = fixed_code(), fixed_header(), 5
    else:
        lengths = limited_lengths(histogram(data, chunk, tile)) if lengths is None else list(lengths)
        (hdr, nbits), dist = dynamic_header(lengths) if header is None else header, 1
    enc = {k: v for k, v in mutant.items() if k != "adler_no_length"}
    body = b"".join(pieces(data, chunk, tile, lengths, hdr, nbits, dist, codes, **enc))
    adler = adler_combine(adler_parts(data, chunk), len(data), chunk, mutant.get("adler_no_length", False))
    return b"\x78\x01" + body + struct.pack(">I", adler)


def inflate(stream):
    """(bytes, eof, unused_data) of a zlib stream through zlib.decompressobj()."""
    d = zlib.decompressobj()
    out = d.decompress(stream) + d.flush()
    return out, d.eof, d.unused_data


# ---- the case table ------------------------------------------------------------------------------------------------------------------
RUNS = (1, 2, 3, 4, 258, 259, 260, 261, 262, 517)
# what the rule gives for one run of each length, written out by hand: l = the literal, a number = a match of that length
RUN_TOKENS = {1: "l", 2: "l l", 3: "l l l", 4: "l 3", 258: "l 257", 259: "l 258", 260: "l 258 l", 261: "l 258 l l", 262: "l 258 3",
              517: "l 258 258"}


def panel_stream(h=300, w=401):
    """The Sub-filtered stream of a grey panel: smooth shading with flat regions (runs of zeros) and a little noise."""
    rs = np.random.RandomState(5)
    y, x = np.mgrid[0:h, 0:w]
    img = (x // 7 + (y // 5) * 3 + (rs.randint(0, 3, (h, w)) * (rs.rand(h, w) < 0.2))) & 255
    img[h // 4:h // 2, w // 3:] = 200
    img = img.astype(np.uint8)
    lines = np.empty((h, 1 + w), np.uint8)
    lines[:, 0] = 1
    lines[:, 1] = img[:, 0]
    lines[:, 2:] = img[:, 1:] - img[:, :-1]
    return lines.tobytes()


def streams(chunk, tile):
    """{name: bytes}: the lengths round a tile and a chunk, runs of every length the rule tells apart, runs across a tile and a
    chunk boundary, every byte value, zeros, noise, a histogram whose Huffman tree is deeper than 15."""
    rs = np.random.RandomState(11)
    noise = lambda n: rs.randint(0, 256, n).astype(np.uint8).tobytes()      # noqa: E731
    mixed = lambda n: (rs.randint(0, 4, n) * (rs.rand(n) < 0.3)).astype(np.uint8).tobytes()      # noqa: E731  zeros with short interruptions
    out = {}
    for name, n in (("1", 1), ("tile-1", tile - 1), ("tile", tile), ("tile+1", tile + 1), ("chunk-1", chunk - 1), ("chunk", chunk),
                    ("chunk+1", chunk + 1), ("2chunk+3", 2 * chunk + 3)):
        out["mixed " + name] = mixed(n)
    out["runs"] = b"".join(bytes([7 + k]) * L + bytes([200 + k]) for k, L in enumerate(RUNS))
    # a run of 600 over the first tile boundary, one of 1000 over the chunk boundary, one that fills a tile and more
    straddle = bytearray(noise(chunk + 3 * tile))
    straddle[tile - 300:tile + 300] = bytes([9]) * 600
    straddle[chunk - 500:chunk + 500] = bytes([0]) * 1000
    straddle[5 * tile - 10:6 * tile + 10] = bytes([255]) * (tile + 20)
    out["straddle"] = bytes(straddle)
    out["all byte values"] = bytes(range(256)) + bytes(v for v in range(256) for _ in range(3)) + bytes(range(255, -1, -1))
    out["zeros"] = bytes(chunk + tile + 5)
    out["noise"] = noise(chunk + 77)
    # Fibonacci counts: 24 symbols whose unlimited Huffman tree is 23 deep
    fib, skew = [1, 1], bytearray()
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    for k, f in enumerate(fib):
        skew += bytes([k, 255 - k]) * ((f + 1) // 2)     # pairs, so that no runs form and the counts stay skewed
    out["skewed"] = bytes(skew)
    out["panel"] = panel_stream()
    return out
