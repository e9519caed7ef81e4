"""The device LZ deflate's contract (include/radnet_hip.h, "THE LZ TOKEN RULE") in plain Python, and the cases its tests share.
Imports nothing from the product; the bit writer, the length table, the code builders and the Adler parts are deflate_cases'.
  RULE: the rule's constants as the header states them (the tests read the header and pass what they read).
  hashes / chunk_tokens / tokens: the candidates (distance 1, distance `near`, the hash candidate out of earlier groups), their
    lengths, acceptance, choice and the greedy parse from every tile's start.
  token_table / histograms: what radnet_deflate_lz_scan_u8 writes.
  distance_symbol, DISTANCE_TABLE (RFC 1951 3.2.5, written out by hand), dynamic_header / piece / pieces / zlib_stream.
  stream_bits / choose / chosen_stream: the size of either rule's stream from its counts, and the rule that is emitted.
  MUTANTS: deliberate mistakes (keyword switches of the functions above) that the tests must catch, each by a named case.
  streams(chunk, tile): the case table, {name: (bytes, near)}."""
import struct

import numpy as np

import deflate_cases as D

RULE = dict(group=256, far_min=10, far_min2=12, far_d=4096)
WINDOW, MAX_MATCH, DIST_SYMBOLS = 32768, 258, 30
# RFC 1951, 3.2.5: (first distance, extra bits) of the distance symbols 0..29
DISTANCE_TABLE = [(1, 0), (2, 0), (3, 0), (4, 0), (5, 1), (7, 1), (9, 2), (13, 2), (17, 3), (25, 3), (33, 4), (49, 4), (65, 5), (97, 5), (129, 6), (193, 6),
                  (257, 7), (385, 7), (513, 8), (769, 8), (1025, 9), (1537, 9), (2049, 10), (3073, 10), (4097, 11), (6145, 11), (8193, 12), (12289, 12),
                  (16385, 13), (24577, 13)]
MUTANTS = ("far32769", "no_tile_cut", "own_group", "dist_msb", "tie_larger")
LITERAL = 1 << 31


def distance_symbol(distance):
    """(symbol, extra bits, extra value) of a match distance 1..32768."""
    for k in range(DIST_SYMBOLS - 1, -1, -1):
        first, extra_bits = DISTANCE_TABLE[k]
        if distance >= first:
            if distance - first >= 1 << extra_bits:
                break
            return k, extra_bits, distance - first
    raise ValueError("no distance symbol for a distance of %d" % distance)


def hashes(a):
    """H(x) of every position x with x + 4 <= len(a): ((little-endian u32 at x) * 2654435761 mod 2^32) >> 17."""
    if len(a) < 4:
        return np.zeros(0, np.int64)
    b = a.astype(np.uint64)
    word = b[:-3] | (b[1:-2] << np.uint64(8)) | (b[2:-1] << np.uint64(16)) | (b[3:] << np.uint64(24))
    return (((word * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(17)).astype(np.int64)


def _run_lengths(a, d):
    """run[p] = the number of i >= 0 with a[p + j] == a[p + j - d] for all j <= i (0 for p < d)."""
    n = len(a)
    run = np.zeros(n + 1, np.int64)
    if n > d:
        eq = np.zeros(n, bool)
        eq[d:] = a[d:] == a[:-d]
        stop = np.append(np.flatnonzero(~eq), n)       # the first unequal position at or behind p; n: none
        run[:n] = stop[np.searchsorted(stop, np.arange(n), side="left")] - np.arange(n)
    return run


def chunk_tokens(a, tile, near, rule=RULE, far32769=False, no_tile_cut=False, own_group=False, tie_larger=False):
    """The tokens of one chunk (a uint8 array): ("lit", byte) and ("match", length, distance)."""
    n, group = len(a), rule["group"]
    raw = a.tobytes()
    h = hashes(a).tolist()
    run1 = _run_lengths(a, 1)
    run_near = _run_lengths(a, near) if near > 1 else None
    head, inserted = {}, 0                             # hash -> the greatest position of the groups in front of the current one
    toks = []
    for t0 in range(0, n, tile):
        p, tile_end = t0, min(n, t0 + tile)
        while p < tile_end:
            room = min(MAX_MATCH, (n if no_tile_cut else tile_end) - p)      # MUTANT no_tile_cut: the length runs into the next tile
            upto = p if own_group else p - p % group                         # MUTANT own_group: every earlier position is a source
            for q in range(inserted, min(upto, len(h))):
                head[h[q]] = q
            inserted = max(inserted, min(upto, len(h)))
            best = (0, 0)                              # length, distance
            cands = []
            if p >= 1:
                cands.append((1, min(int(run1[p]), room), 3))
            if near > 1 and p >= near:
                cands.append((near, min(int(run_near[p]), room), 3))
            if p < len(h) and h[p] in head:
                q = head[h[p]]
                d = p - q
                if d <= WINDOW + (1 if far32769 else 0):                     # MUTANT far32769: one beyond deflate's window
                    length = 0
                    while length < room and raw[q + length] == raw[p + length]:
                        length += 1
                    cands.append((d, length, rule["far_min"] if d <= rule["far_d"] else rule["far_min2"]))
            for d, length, least in cands:
                if length >= least:
                    better = d > best[1] if tie_larger else d < best[1]      # MUTANT tie_larger
                    if length > best[0] or (length == best[0] and better):
                        best = (length, d)
            if best[0]:
                toks.append(("match", best[0], best[1]))
                p += best[0]
            else:
                toks.append(("lit", raw[p]))
                p += 1
    return toks


def tokens(data, chunk, tile, near, rule=RULE, **mutant):
    """[tokens of chunk 0, tokens of chunk 1, ...] of a byte string."""
    data = np.frombuffer(bytes(data), np.uint8)
    return [chunk_tokens(data[c0:c0 + chunk], tile, near, rule, **mutant) for c0 in range(0, len(data), chunk)]


def token_table(all_toks, n):
    """radnet_deflate_lz_scan_u8's table: per byte 0 (covered), 1 << 31 (a literal) or 1 << 31 | length << 16 | distance - 1."""
    table, p = np.zeros(n, np.uint32), 0
    for toks in all_toks:
        for t in toks:
            if t[0] == "lit":
                table[p] = LITERAL
                p += 1
            else:
                table[p] = LITERAL | (t[1] << 16) | (t[2] - 1)
                p += t[1]
    assert p == n
    return table


def histograms(all_toks):
    """(286 literal/length counts with one end-of-block per chunk, 30 distance counts)."""
    ll, dist = np.zeros(D.SYMBOLS, np.int64), np.zeros(DIST_SYMBOLS, np.int64)
    for toks in all_toks:
        for t in toks:
            if t[0] == "lit":
                ll[t[1]] += 1
            else:
                ll[D.length_symbol(t[1])[0]] += 1
                dist[distance_symbol(t[2])[0]] += 1
        ll[D.EOB] += 1
    return ll, dist


def counts(all_toks, near):
    """(matches, far matches): all matches, and those at a distance other than 1 and `near`."""
    m = [t for toks in all_toks for t in toks if t[0] == "match"]
    return len(m), sum(1 for t in m if t[2] not in (1, near))


def distance_weights(hist_d):
    """The distance counts a code is built from: with fewer than two used symbols, symbol 0 (or 1) joins them."""
    w = [int(v) for v in hist_d]
    used = [s for s, v in enumerate(w) if v]
    if len(used) == 0:
        w[0] = w[1] = 1
    elif len(used) == 1:
        w[1 if used[0] == 0 else 0] = 1
    return w


def model_lengths(hist_ll, hist_d):
    """The model's own codes (package-merge) for both alphabets."""
    ll = [int(v) for v in hist_ll]
    if sum(1 for v in ll if v) < 2:
        ll[0 if ll[0] == 0 else 1] = 1
    return D.limited_lengths(ll), D.limited_lengths(distance_weights(hist_d))


def dynamic_header(len_ll, len_d):
    """(bytes, bits) of the block header: BFINAL 0, BTYPE 10, HLIT 29, HDIST 29, HCLEN 15, a code-length code of 4 bits for each of
    0..15, then the 286 + 30 lengths as such 4-bit codes: 74 + 316 * 4 = 1338 bits."""
    assert len(len_ll) == D.SYMBOLS and len(len_d) == DIST_SYMBOLS
    w = D.BitWriter()
    w.put(0, 1)
    w.put(2, 2)
    w.put(D.SYMBOLS - 257, 5)
    w.put(DIST_SYMBOLS - 1, 5)
    w.put(15, 4)
    for s in D.CODE_LENGTH_ORDER:
        w.put(4 if s < 16 else 0, 3)
    for v in list(len_ll) + list(len_d):
        w.code(int(v), 4)
    return w.bytes(), w.n


def piece(toks, len_ll, codes_ll, len_d, codes_d, header, header_nbits, last, dist_msb=False):
    """The bytes of one chunk's deflate block: header, tokens, end-of-block, then the sync flush (or, last, BFINAL and padding)."""
    w = D.BitWriter()
    w.put(int.from_bytes(header, "little") & ((1 << header_nbits) - 1) & ~1 | (1 if last else 0), header_nbits)
    for t in toks:
        if t[0] == "lit":
            assert len_ll[t[1]], "literal %d has no code" % t[1]
            w.code(codes_ll[t[1]], len_ll[t[1]])
        else:
            s, extra_bits, extra = D.length_symbol(t[1])
            assert len_ll[s], "length symbol %d has no code" % s
            w.code(codes_ll[s], len_ll[s])
            w.put(extra, extra_bits)
            s, extra_bits, extra = distance_symbol(t[2])
            assert len_d[s], "distance symbol %d has no code" % s
            w.code(codes_d[s], len_d[s])
            w.put(D.reverse_bits(extra, extra_bits) if dist_msb else extra, extra_bits)      # MUTANT dist_msb
    w.code(codes_ll[D.EOB], len_ll[D.EOB])
    if not last:
        w.put(0, 3)
        w.pad()
        w.put(0xFFFF0000, 32)
    w.pad()
    return w.bytes()


def pieces(all_toks, len_ll, len_d, header, header_nbits, codes_ll=None, codes_d=None, **mutant):
    codes_ll = D.canonical_codes(len_ll) if codes_ll is None else codes_ll
    codes_d = D.canonical_codes(len_d) if codes_d is None else codes_d
    return [piece(t, len_ll, codes_ll, len_d, codes_d, header, header_nbits, c == len(all_toks) - 1, **mutant) for c, t in enumerate(all_toks)]


def zlib_stream(data, chunk, tile, near, rule=RULE, lengths=None, header=None, **mutant):
    """78 01, the LZ rule's pieces, the Adler-32.  lengths: (literal/length lengths, distance lengths), the model's own unless given;
    header (bytes, bits): the model's own unless given."""
    tok = {k: v for k, v in mutant.items() if k != "dist_msb"}
    enc = {k: v for k, v in mutant.items() if k == "dist_msb"}
    all_toks = tokens(data, chunk, tile, near, rule, **tok)
    len_ll, len_d = model_lengths(*histograms(all_toks)) if lengths is None else lengths
    hdr, nbits = dynamic_header(len_ll, len_d) if header is None else header
    body = b"".join(pieces(all_toks, len_ll, len_d, hdr, nbits, **enc))
    return b"\x78\x01" + body + struct.pack(">I", D.adler_combine(D.adler_parts(data, chunk), len(data), chunk))


def stream_bits(hist_ll, hist_d, len_ll, len_d, dist_nbits, header_nbits, chunks):
    """radnet_deflate_stream_bits: the bits of all headers, tokens and end-of-blocks (the flush and the padding to a byte are not
    counted: at most 7 bits a piece differ between two rules).  hist_d None: every match has the one distance code of dist_nbits
    bits (the run-length rule)."""
    bits = chunks * header_nbits
    for s, c in enumerate(hist_ll):
        bits += int(c) * (int(len_ll[s]) + (D.LENGTH_TABLE[s - 257][1] if s > 256 else 0))
    if hist_d is None:
        return bits + int(sum(int(c) for c in hist_ll[257:])) * dist_nbits
    for s, c in enumerate(hist_d):
        bits += int(c) * (int(len_d[s]) + DISTANCE_TABLE[s][1])
    return bits


def choose(bits_lz, bits_rle, chunks):
    """"lz" when its stream cannot be longer than run-length's even if every piece pads 7 bits more, else "rle" (ties included)."""
    return "lz" if bits_lz + 7 * chunks < bits_rle else "rle"


def chosen_stream(data, chunk, tile, near, rule=RULE):
    """(rule, zlib stream, bits_lz, bits_rle) with the model's own codes for both rules."""
    chunks = -(-len(data) // chunk)
    rle_hist = D.histogram(data, chunk, tile)
    rle_len = D.limited_lengths(rle_hist)
    bits_rle = stream_bits(rle_hist, None, rle_len, None, 1, D.dynamic_header(rle_len)[1], chunks)
    all_toks = tokens(data, chunk, tile, near, rule)
    hist_ll, hist_d = histograms(all_toks)
    len_ll, len_d = model_lengths(hist_ll, hist_d)
    bits_lz = stream_bits(hist_ll, hist_d, len_ll, len_d, 0, dynamic_header(len_ll, len_d)[1], chunks)
    which = choose(bits_lz, bits_rle, chunks)
    stream = zlib_stream(data, chunk, tile, near, rule) if which == "lz" else D.zlib_stream(data, chunk, tile)
    return which, stream, bits_lz, bits_rle


# ---- the case table ------------------------------------------------------------------------------------------------------------------
def rgb_panel_stream(h=200, w=300):
    """The Sub-filtered stream of an RGB panel: smooth shading whose channels differ, a flat patch, a little noise."""
    rs = np.random.RandomState(7)
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([(x // 3 + y // 4), (x // 5 + (y // 3) * 2), (x // 2 + y // 7) * 3], axis=2)
    img = (img + (rs.randint(0, 3, (h, w, 3)) * (rs.rand(h, w, 1) < 0.15))) & 255
    img[h // 4:h // 2, w // 3:] = (200, 90, 30)
    img = img.astype(np.uint8)
    lines = np.empty((h, 1 + 3 * w), np.uint8)
    lines[:, 0] = 1
    lines[:, 1:4] = img[:, 0]
    lines[:, 4:] = (img[:, 1:] - img[:, :-1]).reshape(h, -1)
    return lines.tobytes()


def period7_stream(n=140000):
    return (bytes([3, 141, 59, 26, 53, 58, 97]) * (n // 7 + 1))[:n]


def repeated_row_stream(rowbytes=1203, rows=100):
    return np.random.RandomState(3).randint(0, 256, rowbytes).astype(np.uint8).tobytes() * rows


def _collision():
    """Two different 4-byte keys with the same H, found by search (H has 15 bits: the first collision comes after a few hundred)."""
    seen = {}
    for v in range(1, 1 << 20):
        key = struct.pack("<I", v * 2246822519 & 0xFFFFFFFF)
        hv = int(hashes(np.frombuffer(key, np.uint8))[0])
        if hv in seen and seen[hv] != key:
            return seen[hv], key
        seen[hv] = key
    raise AssertionError("no collision")


def streams(chunk, tile, rule=RULE):
    """{name: (bytes, near)}.  Noise is the background wherever a case plants something, so that nothing else matches."""
    group, far_min, far_min2, far_d = rule["group"], rule["far_min"], rule["far_min2"], rule["far_d"]
    rs = np.random.RandomState(23)
    noise = lambda n: rs.randint(0, 256, n).astype(np.uint8).tobytes()      # noqa: E731
    mixed = lambda n: (rs.randint(0, 4, n) * (rs.rand(n) < 0.3)).astype(np.uint8).tobytes()      # noqa: E731
    out = {}
    for name, n in (("1", 1), ("2", 2), ("3", 3), ("4", 4), ("5", 5), ("tile-1", tile - 1), ("tile", tile), ("tile+1", tile + 1),
                    ("chunk-1", chunk - 1), ("chunk", chunk), ("chunk+1", chunk + 1), ("2chunk+3", 2 * chunk + 3)):
        out["mixed " + name] = (mixed(n), 3 if n % 2 else 1)

    def planted(n, *copies):
        """noise of n bytes with, for each (source, target, length), the bytes at source repeated at target"""
        b = bytearray(noise(n))
        for src, dst, length in copies:
            for i in range(length):                    # byte by byte: an overlapping copy repeats its period
                b[dst + i] = b[src + i]
        return bytes(b)

    # a far match that ends exactly on the tile end, and one the tile end cuts (40 bytes planted, 25 left in the tile); the sources
    # lie 300 back, so that hardly a position between can take their place in the table
    out["match ends on the tile end"] = (planted(3 * tile, (2 * tile - 340, 2 * tile - 40, 40)), 1)
    out["match cut by the tile end"] = (planted(3 * tile, (2 * tile - 325, 2 * tile - 25, 40)), 1)
    out["match of 258"] = (planted(2 * tile, (50, tile + 300, 258)), 1)
    out["match of 259"] = (planted(2 * tile, (50, tile + 300, 259)), 1)
    out["overlap distance 3 length 258"] = (planted(tile, (600, 603, 258)), 3)
    # a repeat of 40 bytes 100 back inside one group: the rule must not see it; the same repeat from the group before: it must
    g0 = 8 * group
    out["source in the own group only"] = (planted(tile, (g0 + 20, g0 + 120, 40)), 1)
    out["source in the group before"] = (planted(tile, (g0 - 60, g0 + 40, 40)), 1)
    ka, kb = _collision()
    b = bytearray(noise(tile))
    b[300:304], b[1500:1504], b[1504:1506 + far_min] = ka, kb, b[304:306 + far_min]
    out["equal hashes, different bytes"] = (bytes(b), 1)
    # a source exactly 32768 back and one 32769 back; both planted 60 bytes long, in one chunk
    out["source 32768 back"] = (planted(chunk, (1000, 1000 + 32768, 60)), 1)
    out["source 32769 back"] = (planted(chunk, (1000, 1000 + 32769, 60)), 1)
    out["repeat across a chunk boundary"] = (planted(chunk + tile, (chunk - 500, chunk + 300, 80)), 1)
    # a key that repeats in the last three bytes of a chunk (H is not defined there) and just in front of them
    out["keys in the last bytes of a chunk"] = (planted(chunk + 7, (200, chunk - 3, 3), (900, chunk - 7, 7), (40, chunk + 4, 3)), 1)
    # FAR_MIN bytes within FAR_D (accepted), FAR_MIN bytes one beyond FAR_D (refused), FAR_MIN2 bytes far beyond it (accepted)
    out["short far matches"] = (planted(4 * tile, (1700, 2000, far_min), (2 * tile + 2100 - far_d - 1, 2 * tile + 2100, far_min), (60, 3 * tile + 100, far_min2)), 1)
    # a tie: in a run of 600 the second match has the same length at distance 1, at distance 3 and from the group before
    b = bytearray(noise(tile))
    b[997:1000], b[1000:1600], b[1600] = bytes([1, 2, 3]), bytes([77]) * 600, 5
    out["tie between distance 1 and near"] = (bytes(b), 3)
    out["zeros"] = (bytes(chunk + tile + 5), 1)
    out["noise near 1"] = (noise(chunk + 77), 1)
    out["noise near 3"] = (noise(tile + 77), 3)
    out["all byte values"] = (bytes(range(256)) + bytes(v for v in range(256) for _ in range(3)) + bytes(range(255, -1, -1)), 3)
    out["panel"] = (D.panel_stream(), 1)
    out["rgb panel"] = (rgb_panel_stream(), 3)
    out["period 7"] = (period7_stream(), 1)
    out["repeated row"] = (repeated_row_stream(), 3)
    return out
