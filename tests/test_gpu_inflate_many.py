"""The many-stream inflate entries (csrc/inflate_many.hip) through the C ABI against their Python model (tests/inflate_many_cases.py)
on its whole case table: the candidates of radnet_inflate_find_blocks_many as sorted sets, the unit records of the two measure
entries field for field, the common output of the two emit entries bit for bit in sentinel-prefilled buffers -- everything that
must NOT be written included: the gaps of the output, the neighbours, the margins, the compressed buffer itself --, the shared
resolve and gather on the common table, and the refusals, which launch nothing."""
import numpy as np
import pytest

import inflate_cases as I
import inflate_lz_cases as Z
import inflate_many_cases as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL, SENTINEL_SRC, MARGIN = 0xA5, 0xA5A5A5A5, 64
ERR_ARG, ERR_UNSUPPORTED = -1, -3
NAMES = sorted(M.batches())
STREAM = np.dtype([("z_offset", np.int64), ("n", np.int64), ("out_offset", np.int64), ("expected", np.int64)])


@pytest.fixture(scope="module")
def png():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    from faster_rcnn import png
    return png


@pytest.fixture(scope="module")
def ctx(png):
    from radnet_hip import runtime as rt
    return rt.default_context()


def last_error(ctx):
    msg = ctx.lib.radnet_last_error(ctx.h)
    return msg.decode() if msg else ""


def to_device(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


class Staged:
    """A batch on the device: z at an odd address with sentinels round it, the table on the host and on the device."""

    def __init__(self, b, offset=3):
        self.b, self.offset = b, offset
        self.zbuf = torch.full((offset + len(b.z) + MARGIN,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.zbuf[offset:offset + len(b.z)] = to_device(np.frombuffer(b.z, np.uint8))
        self.z = self.zbuf.data_ptr() + offset
        self.table = np.array(b.table, np.int64).view(STREAM).reshape(-1)
        self.table_dev = to_device(self.table)
        self.head = (self.z, len(b.z), self.table.ctypes.data, self.table_dev.data_ptr(), len(self.table))

    def untouched(self):
        got = self.zbuf.cpu().numpy()
        o, n = self.offset, len(self.b.z)
        return got[o:o + n].tobytes() == self.b.z and (got[:o] == SENTINEL).all() and (got[o + n:] == SENTINEL).all()


def find(ctx, s, cap):
    """(rc, the count, the candidates written, what stands behind them)."""
    found = torch.from_numpy(np.full(1 + cap + 8, SENTINEL_SRC, np.uint32).view(np.int32)).cuda()
    found[0] = 0
    rc = ctx.lib.radnet_inflate_find_blocks_many(ctx.h, *s.head, found.data_ptr() + 4, cap, found.data_ptr())
    ctx.sync()
    got = found.cpu().numpy().view(np.uint32)
    return rc, int(got[0]), got[1:1 + cap], got[1 + cap:]


def measure(ctx, png, s, starts, lz):
    dtype = png.INFLATE_LZ_UNIT if lz else png.INFLATE_UNIT
    table = np.zeros(len(starts) + 1, dtype)
    table.view(np.uint8)[:] = SENTINEL
    table["start_bit"][:len(starts)] = starts
    dev = to_device(table)
    entry = ctx.lib.radnet_inflate_lz_measure_many if lz else ctx.lib.radnet_inflate_rle_measure_many
    rc = entry(ctx.h, *s.head, dev.data_ptr(), len(starts))
    ctx.sync()
    got = dev.cpu().numpy().view(dtype)
    assert (got[len(starts):].view(np.uint8) == SENTINEL).all(), "written behind the unit table"
    return rc, [tuple(int(v) for v in u) for u in got[:len(starts)]]


class Buffers:
    """buf (uint8) and src (uint32) of n entries on the device, MARGIN sentinel entries in front of and behind each."""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * MARGIN,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.src = torch.from_numpy(np.full(n + 2 * MARGIN, SENTINEL_SRC, np.uint32).view(np.int32)).cuda()
        self.buf_ptr, self.src_ptr = self.buf.data_ptr() + MARGIN, self.src.data_ptr() + 4 * MARGIN

    def host(self):
        buf, src = self.buf.cpu().numpy(), self.src.cpu().numpy().view(np.uint32)
        for a, s in ((buf, SENTINEL), (src, SENTINEL_SRC)):
            assert (a[:MARGIN] == s).all(), "written in front of the buffer"
            assert (a[MARGIN + self.n:] == s).all(), "written behind the buffer"
        return buf[MARGIN:MARGIN + self.n], src[MARGIN:MARGIN + self.n]


def links_on_device(png, links):
    table = np.zeros(len(links), png.INFLATE_LINK)
    for k, (offset, start, out_bytes, prev) in enumerate(links):
        table[k] = (offset, start, out_bytes, prev, 0)
    return to_device(table)


def first_difference(a, b):
    return "first difference at entry %d" % int(np.flatnonzero(np.asarray(a) != np.asarray(b))[0])


def emit_rle(ctx, png, s, links):
    b, table = Buffers(s.b.out_len), links_on_device(png, links)
    rc = ctx.lib.radnet_inflate_rle_emit_many(ctx.h, *s.head, table.data_ptr(), len(links), b.buf_ptr, s.b.out_len)
    ctx.sync()
    assert rc == 0, last_error(ctx)
    buf, src = b.host()
    assert (src == SENTINEL_SRC).all()
    return buf


def emit_lz(ctx, png, s, links):
    b, table = Buffers(s.b.out_len), links_on_device(png, links)
    rc = ctx.lib.radnet_inflate_lz_emit_many(ctx.h, *s.head, table.data_ptr(), len(links), b.buf_ptr, b.src_ptr, s.b.out_len)
    ctx.sync()
    assert rc == 0, last_error(ctx)
    return b


@pytest.mark.parametrize("name", NAMES)
def test_find_measure_and_emit_match_the_model(ctx, png, name):
    b = M.batches()[name]
    s = Staged(b, 1 + 2 * (NAMES.index(name) % 4))
    cands, starts, _, _, _ = M.model(name, False)
    cap = len(cands) + 5
    rc, count, got, behind = find(ctx, s, cap)
    assert rc == 0, last_error(ctx)
    assert count == len(cands) and sorted(got[:count].tolist()) == cands, (name, count, len(cands))
    assert (got[count:] == SENTINEL_SRC).all() and (behind == SENTINEL_SRC).all(), "written behind the candidates"
    # a cap below the count: the count is whole, nothing stands behind the cap, what stands below it are candidates
    rc, count, got, behind = find(ctx, s, 3)
    assert rc == 0 and count == len(cands) and set(got.tolist()) <= set(cands) and (behind == SENTINEL_SRC).all()
    # the units: the candidates, every stream's bit 16, bits in the gaps and behind the buffer, and for the cut batches the unit at the cut
    extra = [8 * zo + 8 * n + 3 for zo, n, _, _ in b.table] + [8 * len(b.z) + 5, 8 * b.table[0][0] + 8]
    if "unit_start" in b.tally:
        extra.append(8 * b.table[1][0] + b.tally["unit_start"])
    probe = sorted(set(starts) | set(extra))
    for lz in (False, True):
        rc, records = measure(ctx, png, s, probe, lz)
        assert rc == 0, last_error(ctx)
        want = M.measure_many(b, probe, lz)
        fields = Z.UNIT_FIELDS if lz else I.UNIT_FIELDS
        for g, w in zip(records, want):
            assert g == w, (name, lz, dict(zip(fields, g)), dict(zip(fields, w)))
    # emit: the chained links of every stream whose chain is accepted
    links = M.model(name, False)[4]
    buf = emit_rle(ctx, png, s, links)
    want = M.emit_rle_many(b, links, SENTINEL)
    assert np.array_equal(buf, want), (name, first_difference(buf, want))
    links = M.model(name, True)[4]
    d = emit_lz(ctx, png, s, links)
    buf, src = d.host()
    want_buf, want_src = M.emit_lz_many(b, links, SENTINEL, SENTINEL_SRC)
    assert np.array_equal(src, want_src), (name, first_difference(src, want_src))
    assert np.array_equal(buf, want_buf), (name, first_difference(buf, want_buf))
    # the shared resolve and gather on the common table: the sentinels of the gaps are roots (>= their index) and stay
    rounds = Z.bound(b.out_len)
    changed = torch.zeros(rounds, dtype=torch.int32, device="cuda")
    assert ctx.lib.radnet_inflate_lz_resolve(ctx.h, d.src_ptr, b.out_len, rounds, changed.data_ptr()) == 0, last_error(ctx)
    assert ctx.lib.radnet_inflate_lz_gather(ctx.h, d.src_ptr, d.buf_ptr, b.out_len) == 0, last_error(ctx)
    ctx.sync()
    buf, src = d.host()
    flat, _ = Z.resolve(want_src)
    want_out = Z.gather(want_buf, flat)
    assert np.array_equal(src, flat) and np.array_equal(buf, want_out), name
    for (zo, n, oo, expected), (sname, _, data), (code, _, _) in zip(b.table, b.streams, M.model(name, True)[3]):
        if data is not None:
            assert code == Z.CHAIN_OK and buf[oo:oo + expected].tobytes() == data, (name, sname)
    assert s.untouched(), "the compressed buffer or its margins were written"


@pytest.mark.parametrize("name", ["a cut in a header", "b cut in a unit", "c reach in front of the stream"])
def test_hand_made_links_stay_inside_their_stream(ctx, png, name):
    b = M.batches()[name]
    s = Staged(b, 5)
    links = M.hand_links(name)
    if name.startswith("c "):
        assert M.clamped(b, links) > 0
    else:
        buf = emit_rle(ctx, png, s, links)
        want = M.emit_rle_many(b, links, SENTINEL)
        assert np.array_equal(buf, want), (name, first_difference(buf, want))
        oo, expected = b.table[0][2], b.table[0][3]
        assert (buf[oo + expected - 3:oo + expected] != SENTINEL).any() and (buf[oo + expected:] == SENTINEL).all()
    buf, src = emit_lz(ctx, png, s, links).host()
    want_buf, want_src = M.emit_lz_many(b, links, SENTINEL, SENTINEL_SRC)
    assert np.array_equal(src, want_src), (name, first_difference(src, want_src))
    assert np.array_equal(buf, want_buf), (name, first_difference(buf, want_buf))
    if name.startswith("c "):
        oo = b.table[1][2]
        written = src != SENTINEL_SRC
        assert written.any() and (src[written] >= oo).all(), "a source in front of the stream's own output"
    assert s.untouched()


def test_refused_arguments_launch_nothing(ctx, png):
    b = M.batches()["gap 1"]
    s = Staged(b)
    good = s.table
    links = M.model("gap 1", True)[4][:4]
    ltab = links_on_device(png, links)

    def tables(mutate):
        t = good.copy()
        mutate(t)
        return t, to_device(t)

    def swap(t):
        t[[1, 2]] = t[[2, 1]]

    def overlap_z(t):
        t["z_offset"][2] = t["z_offset"][1] + t["n"][1] - 1

    def overlap_out(t):
        t["out_offset"][2] = t["out_offset"][1] + t["expected"][1] - 1

    def outside_z(t):
        t["n"][-1] += 2                                                   # one byte of gap stands behind the last stream

    def short(t):
        t["n"][0] = 2

    cases = [(swap, ERR_ARG, "sorted"), (overlap_z, ERR_ARG, "overlaps"), (overlap_out, ERR_ARG, "overlaps"), (outside_z, ERR_ARG, "outside"),
             (short, ERR_ARG, "3 at least")]
    for mutate, code, word in cases:
        t, tdev = tables(mutate)
        head = (s.z, len(b.z), t.ctypes.data, tdev.data_ptr(), len(t))
        d = Buffers(b.out_len)
        found = torch.zeros(16, dtype=torch.int32, device="cuda")
        units = to_device(np.zeros(4, png.INFLATE_LZ_UNIT))
        rcs = [ctx.lib.radnet_inflate_find_blocks_many(ctx.h, *head, found.data_ptr() + 4, 8, found.data_ptr()),
               ctx.lib.radnet_inflate_rle_measure_many(ctx.h, *head, units.data_ptr(), 4),
               ctx.lib.radnet_inflate_lz_measure_many(ctx.h, *head, units.data_ptr(), 4),
               ctx.lib.radnet_inflate_rle_emit_many(ctx.h, *head, ltab.data_ptr(), len(links), d.buf_ptr, b.out_len)]
        assert word in last_error(ctx), (mutate.__name__, last_error(ctx))
        rcs.append(ctx.lib.radnet_inflate_lz_emit_many(ctx.h, *head, ltab.data_ptr(), len(links), d.buf_ptr, d.src_ptr, b.out_len))
        ctx.sync()
        assert rcs == [code] * 5, (mutate.__name__, rcs)
        buf, src = d.host()
        assert (buf == SENTINEL).all() and (src == SENTINEL_SRC).all() and not found.cpu().numpy().any() and not units.cpu().numpy().any()
    d = Buffers(b.out_len)
    head = s.head
    # the size limits, a count of 0 and one above the cap, null pointers, a misaligned device table, an output shorter than the table says
    assert ctx.lib.radnet_inflate_lz_emit_many(ctx.h, s.z, 1 << 29, *head[2:], ltab.data_ptr(), len(links), d.buf_ptr, d.src_ptr, b.out_len) == ERR_UNSUPPORTED
    assert ctx.lib.radnet_inflate_lz_emit_many(ctx.h, *head, ltab.data_ptr(), len(links), d.buf_ptr, d.src_ptr, 1 << 31) == ERR_UNSUPPORTED
    assert ctx.lib.radnet_inflate_lz_emit_many(ctx.h, *head[:4], 0, ltab.data_ptr(), len(links), d.buf_ptr, d.src_ptr, b.out_len) == ERR_ARG
    assert ctx.lib.radnet_inflate_lz_emit_many(ctx.h, *head[:4], png.INFLATE_MANY_MAX_STREAMS + 1, ltab.data_ptr(), len(links), d.buf_ptr, d.src_ptr, b.out_len) == ERR_ARG
    assert ctx.lib.radnet_inflate_lz_emit_many(ctx.h, *head, ltab.data_ptr(), len(links), d.buf_ptr, None, b.out_len) == ERR_ARG
    assert ctx.lib.radnet_inflate_lz_emit_many(ctx.h, *head, ltab.data_ptr(), 0, d.buf_ptr, d.src_ptr, b.out_len) == ERR_ARG
    assert ctx.lib.radnet_inflate_lz_emit_many(ctx.h, *head[:3], head[3] + 4, head[4], ltab.data_ptr(), len(links), d.buf_ptr, d.src_ptr, b.out_len) == ERR_ARG
    # an output shorter than the last stream's: the emit entries judge the table against the output they are given
    assert ctx.lib.radnet_inflate_rle_emit_many(ctx.h, *head, ltab.data_ptr(), len(links), d.buf_ptr, b.out_len - 6) == ERR_ARG and "outside" in last_error(ctx)
    assert ctx.lib.radnet_inflate_lz_emit_many(ctx.h, *head, ltab.data_ptr(), len(links), d.buf_ptr, d.src_ptr, b.out_len - 6) == ERR_ARG
    assert ctx.lib.radnet_inflate_rle_emit_many(ctx.h, *head, ltab.data_ptr(), len(links), d.buf_ptr, -1) == ERR_ARG
    assert ctx.lib.radnet_inflate_rle_emit_many(ctx.h, None, *head[1:], ltab.data_ptr(), len(links), d.buf_ptr, b.out_len) == ERR_ARG
    assert ctx.lib.radnet_inflate_find_blocks_many(ctx.h, *head, None, 8, d.src_ptr) == ERR_ARG
    assert ctx.lib.radnet_inflate_find_blocks_many(ctx.h, *head, d.src_ptr, -1, d.src_ptr) == ERR_ARG
    assert ctx.lib.radnet_inflate_rle_measure_many(ctx.h, *head, None, 4) == ERR_ARG
    assert ctx.lib.radnet_inflate_lz_measure_many(ctx.h, *head, d.src_ptr, 0) == ERR_ARG
    ctx.sync()
    buf, src = d.host()
    assert (buf == SENTINEL).all() and (src == SENTINEL_SRC).all() and s.untouched()
