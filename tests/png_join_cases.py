"""The IDAT join (radnet_png_join_u8, include/radnet_hip.h) stated in NumPy, its case table and five mutants of the statement.

The model is written from the header, not from the kernel: out[dst_k + j] = file[src_k + j]; the work is cut into grains, the 16
bytes between two 16-byte boundaries of device memory clipped to [out, out + n); the piece of a byte p is the LAST k with
dst_k <= p.  It works on whole arrays (one searchsorted), so the 2 MiB case costs milliseconds.  The host tests hold it against
b"".join of the pieces, the device tests hold the kernel against it.

A case is a dict: name, file (uint8 array), table (PIECE rows), n, out_at and file_at (bytes behind a 16-byte boundary at which the
device test places the output and the file)."""
import numpy as np

PIECE = np.dtype([("src", np.int64), ("dst", np.int64), ("length", np.int64)])      # radnet_png_piece
GRAIN = 16
SPAN_GRAINS = 256
ALIGNMENTS = (0, 1, 3, 7, 13)
LENGTHS = (0, 1, 15, 16, 17, 4095, 4096, 4097, 8192)
MUTANTS = ("first_of_equal_dst", "src_rounded_to_4", "boundary_off_by_one", "last_grain_dropped", "dst_in_src_order")
UNWRITTEN = 0xEE      # what the model leaves in a byte it does not write (the mutant that drops a grain)


def content(size, seed):
    """Noise in the high nibble, the position in the low one: a source that is off by less than 16 shows in every byte, one that
    is off by more in 15 bytes of 16."""
    noise = np.random.RandomState(seed).randint(0, 256, size=size).astype(np.uint8)
    return (noise & 0xF0) | (np.arange(size) & 0x0F).astype(np.uint8)


def table_of(srcs, lengths):
    table = np.zeros(len(lengths), PIECE)
    table["src"], table["length"] = srcs, lengths
    table["dst"] = np.cumsum(table["length"]) - table["length"]
    return table


def joined(file, table):
    """The reference: the pieces one after the other."""
    return np.frombuffer(b"".join(file[int(s):int(s + l)].tobytes() for s, _, l in table.tolist()), np.uint8)


def model(file, table, n, out_at=0, mutant=None):
    """out[0 .. n) as the contract states it, for an output that stands out_at bytes behind a 16-byte boundary."""
    out = np.full(n, UNWRITTEN, np.uint8)
    if n == 0:
        return out
    src, dst, length = (table[f].astype(np.int64) for f in ("src", "dst", "length"))
    if mutant == "dst_in_src_order":
        order = np.argsort(src, kind="stable")
        in_order = np.cumsum(length[order]) - length[order]
        dst = np.empty_like(dst)
        dst[order] = in_order
        keep = np.argsort(dst, kind="stable")      # the bisection needs dst ascending
        src, dst, length = src[keep], dst[keep], length[keep]
    p = np.arange(n, dtype=np.int64)
    grain = (p + out_at) // GRAIN
    k = np.searchsorted(dst, p, side="right") - 1      # the last k with dst_k <= p
    if mutant == "first_of_equal_dst":
        k = np.searchsorted(dst, dst[k], side="left")      # the first of the pieces that share that dst: an empty one, if there is one
    if mutant == "boundary_off_by_one":
        # inside a grain, the byte a new piece starts with is still taken from the piece in front of it, one byte past its end
        starts = (p == dst[k]) & (p > 0) & (np.roll(grain, 1) == grain)
        k = np.where(starts, np.searchsorted(dst, np.maximum(p - 1, 0), side="right") - 1, k)
    at = src[k] + (p - dst[k])
    if mutant == "src_rounded_to_4":
        at = (src[k] & ~np.int64(3)) + (p - dst[k])
    out[:] = file[np.clip(at, 0, len(file) - 1)]
    if mutant == "last_grain_dropped" and (out_at + n) % GRAIN:
        out[grain == grain[-1]] = UNWRITTEN
    return out


def _case(name, lengths, gaps, seed, out_at=0, file_at=0, lead=8, tail=5, order=None, srcs=None):
    """Pieces of `lengths` laid into a file one after the other, `gaps` bytes between them (a chunk's CRC, length and type are 12),
    `lead` bytes in front and `tail` behind; order: a permutation of the src column; srcs: the src column itself."""
    lengths = np.asarray(lengths, np.int64)
    gaps = np.resize(np.asarray(gaps, np.int64), len(lengths))
    if srcs is None:
        srcs = lead + np.cumsum(lengths + gaps) - (lengths + gaps)
        size = int(lead + (lengths + gaps).sum() - (gaps[-1] if len(gaps) else 0) + tail)
        if order is not None:      # the same ranges of the file, in another order: the lengths move with them
            srcs, lengths = srcs[order], lengths[order]
    else:
        srcs = np.asarray(srcs, np.int64)
        size = int((srcs + lengths).max() + tail) if len(lengths) else lead + tail
    file = content(size, seed)
    table = table_of(srcs, lengths)
    return dict(name=name, file=file, table=table, n=int(lengths.sum()), out_at=out_at, file_at=file_at)


def cases():
    rs = np.random.RandomState(41)
    out = []
    # the lengths round the grain and the span with the 12-byte gaps of a file, at every alignment of the output and of the file
    for out_at, file_at in zip(ALIGNMENTS, (0, 13, 7, 3, 1)):
        out.append(_case("file gaps, out at %d, file at %d" % (out_at, file_at), LENGTHS, 12, 1, out_at, file_at))
    # odd gaps: src - dst takes every residue mod 16
    out.append(_case("odd gaps", LENGTHS * 2, np.arange(1, 19), 2, out_at=3, file_at=1, lead=1))
    out.append(_case("empty pieces first, last and a thousand in a row", [0, 0, 5, 100] + [0] * 1000 + [37, 4096, 0, 0], 12, 3, out_at=7))
    out.append(_case("empty pieces alone", [0] * 7, 12, 4))
    out.append(_case("the empty table", [], 12, 5))
    out.append(_case("three thousand small pieces", rs.randint(0, 41, size=3000), rs.randint(0, 20, size=3000), 6, out_at=13, file_at=3))
    out.append(_case("one long piece between tiny ones", [1, 1, 2 << 20, 1, 1], 12, 7, out_at=1, file_at=7))
    lengths = rs.randint(0, 300, size=200)
    out.append(_case("shuffled sources", lengths, 12, 8, out_at=3, order=rs.permutation(200)))
    lengths = rs.randint(0, 200, size=300)
    out.append(_case("overlapping sources", lengths, 0, 9, out_at=7, file_at=13, srcs=rs.randint(0, 5000, size=300)))
    out.append(_case("ends on the last byte of an odd file", [17, 4096, 33], 12, 10, out_at=13, file_at=1, lead=9, tail=0))
    assert len(out[-1]["file"]) % 2 == 1 and int(out[-1]["table"]["src"][-1] + out[-1]["table"]["length"][-1]) == len(out[-1]["file"])
    return out


# the case that tells each mutant from the model
CAUGHT_BY = {"first_of_equal_dst": "empty pieces first, last and a thousand in a row", "src_rounded_to_4": "odd gaps",
             "boundary_off_by_one": "three thousand small pieces", "last_grain_dropped": "file gaps, out at 1, file at 13",
             "dst_in_src_order": "shuffled sources"}
