"""The host half of the batched PNG decoder: radnet_png_plan_segments (csrc/png_plan.cpp) cuts a pass into segments that start on
row 0 or on a row of filter type 0 / 1.  Its properties over fixed and random filter columns; a NumPy check of the claim the
segments rest on (each reconstructed alone, zeros above its first row, gives the bytes of the whole pass reconstructed in one go);
the planner under AddressSanitizer + UBSan in a stand-alone program; DeviceImageLoader.prefetch's accounting with fake decoders.
No device needed."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import png_cases as K
from faster_rcnn import png, utils_io
from radnet_hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1


def plan(types, rowbytes=5, stream_offset=0, target_rows=0, cap=None):
    """The planner on a pass with the given filter-type column (the sample bytes are 0xEE: illegal as filter types, were they read
    as such): (count or error, table)."""
    types = np.asarray(types, np.uint8)
    lines = np.full((len(types), 1 + rowbytes), 0xEE, np.uint8)
    lines[:, 0] = types
    cap = len(types) if cap is None else cap
    table = np.zeros(max(cap, 1), png.SEGMENT)
    n = L.load_library().radnet_png_plan_segments(lines.ctypes.data, stream_offset, len(types), rowbytes, target_rows,
                                                  table.ctypes.data_as(ctypes.c_void_p), cap)
    return n, table[:max(n, 0)]


def first_rows(table):
    return np.concatenate([[0], np.cumsum(table["rows"])[:-1]])


def check_legal(types, table, rowbytes=5, stream_offset=0):
    types = np.asarray(types)
    assert (table["rows"] > 0).all() and int(table["rows"].sum()) == len(types)      # tile the rows exactly, in order
    firsts = first_rows(table)
    assert all(r == 0 or types[r] <= 1 for r in firsts)
    assert (table["rowbytes"] == rowbytes).all()
    assert np.array_equal(table["offset"], stream_offset + firsts * (1 + rowbytes))


COLUMNS = {
    "none": np.zeros(200, int), "sub": np.ones(200, int), "up": np.full(200, 2), "average": np.full(200, 3), "paeth": np.full(200, 4),
    "one_row": np.array([3]), "cut_every_65": np.where(np.arange(400) % 65 == 0, 1, 4), "cut_at_the_end": np.array([4] * 99 + [0]),
    "random": np.random.RandomState(0).randint(0, 5, 1000), "sparse_cuts": np.where(np.random.RandomState(1).rand(3000) < 0.02, 0, 2),
}


def test_the_constant_the_abi_mirror_and_the_binding():
    assert L.header_constant("RADNET_PNG_SEGMENT_TARGET_ROWS") == 64
    assert png.SEGMENT.itemsize == 16
    assert [(n, png.SEGMENT.fields[n][1]) for n in png.SEGMENT.names] == [("offset", 0), ("rows", 8), ("rowbytes", 12)]
    assert "radnet_png_plan_segments" in L.declared_symbols() and "radnet_png_unfilter_segments_u8" in L.declared_symbols()


@pytest.mark.parametrize("name", sorted(COLUMNS))
@pytest.mark.parametrize("target", [0, 1, 7, 64, 100])
def test_segments_tile_the_rows_and_start_on_legal_cuts(name, target):
    types = COLUMNS[name]
    n, table = plan(types, rowbytes=6, stream_offset=12345, target_rows=target)
    assert n == len(table) >= 1
    check_legal(types, table, 6, 12345)


def test_fixed_columns():
    for ft in (2, 3, 4):
        n, table = plan(np.full(200, ft))
        assert n == 1 and int(table["rows"][0]) == 200          # no legal cut: the pass is one segment, as without segments
    for ft in (0, 1):
        n, table = plan(np.full(200, ft))
        assert n == 4 and table["rows"].tolist() == [64, 64, 64, 8]
        n, table = plan(np.full(200, ft), target_rows=50)
        assert table["rows"].tolist() == [50, 50, 50, 50]
    n, table = plan([4])
    assert n == 1 and table["rows"].tolist() == [1]


def test_target_rows_is_honoured_when_legal_cuts_allow():
    rs = np.random.RandomState(5)
    for target in (0, 3, 16, 64):
        t = target or 64
        types = rs.randint(0, 5, 2000)
        n, table = plan(types, target_rows=target)
        check_legal(types, table)
        cuts = np.flatnonzero(types <= 1)
        for first, rows in zip(first_rows(table), table["rows"]):
            end = first + rows
            inside = cuts[(cuts > first) & (cuts <= first + t)]
            if first + t >= len(types):
                assert end == len(types)                           # the rest fits
            elif len(inside):
                assert end == inside[-1] and rows <= t             # the last legal cut within the target
            else:
                later = cuts[cuts > first + t]
                assert end == (later[0] if len(later) else len(types))      # none: the next legal cut
    types = np.where(np.arange(400) % 65 == 0, 1, 4)               # cuts 65 rows apart: a target of 64 cannot be kept
    assert plan(types)[1]["rows"].tolist() == [65] * 6 + [10]
    assert plan(types, target_rows=130)[1]["rows"].tolist() == [130, 130, 130, 10]


@pytest.mark.parametrize("name", sorted(COLUMNS))
def test_a_small_cap_merges_and_never_fails(name):
    types = COLUMNS[name]
    full, _ = plan(types, target_rows=8)
    for cap in sorted({1, 2, 3, max(full - 1, 1), full, full + 5}):
        n, table = plan(types, target_rows=8, cap=cap)
        assert n == min(cap, full)
        check_legal(types, table)


def test_errors():
    types = np.zeros(10, int)
    for bad_row in (0, 4, 9):
        bad = types.copy()
        bad[bad_row] = 5
        assert plan(bad)[0] == ERR_ARG
    bad[9] = 255
    assert plan(bad)[0] == ERR_ARG
    assert plan(types, cap=0)[0] == ERR_ARG and plan(types, stream_offset=-1)[0] == ERR_ARG and plan(types, target_rows=-1)[0] == ERR_ARG
    fn = L.load_library().radnet_png_plan_segments
    table = np.zeros(4, png.SEGMENT)
    lines = np.zeros((4, 3), np.uint8)
    out = table.ctypes.data_as(ctypes.c_void_p)
    assert fn(None, 0, 4, 2, 0, out, 4) == ERR_ARG and fn(lines.ctypes.data, 0, 4, 2, 0, None, 4) == ERR_ARG
    assert fn(lines.ctypes.data, 0, 0, 2, 0, out, 4) == ERR_ARG and fn(lines.ctypes.data, 0, 4, 0, 0, out, 4) == ERR_ARG
    assert not table.view(np.uint8).any()


# ---- the claim itself, in NumPy ---------------------------------------------------------------------------------------------------
def reconstruct(lines, bpp):
    """PNG specification section 9 on [rows][1 + rowbytes] filtered scanlines, the row above row 0 being zeros: the raw bytes."""
    rows, n = lines.shape[0], lines.shape[1] - 1
    out = np.zeros((rows, n), np.int64)
    above = np.zeros(n, np.int64)
    for r in range(rows):
        ft, x = int(lines[r, 0]), lines[r, 1:].astype(np.int64)
        cur = out[r]
        for i in range(n):
            a = cur[i - bpp] if i >= bpp else 0
            b = above[i]
            c = above[i - bpp] if i >= bpp else 0
            if ft == 0:
                p = 0
            elif ft == 1:
                p = a
            elif ft == 2:
                p = b
            elif ft == 3:
                p = (a + b) >> 1
            else:
                pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                p = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            cur[i] = (x[i] + p) & 255
        above = cur
    return out.astype(np.uint8)


@pytest.mark.parametrize("bpp", [1, 3, 4, 8])
def test_segments_reconstructed_alone_equal_the_pass_reconstructed_whole(bpp):
    rs = np.random.RandomState(bpp)
    rows, n = 40, 5 * bpp
    raw = rs.randint(0, 256, (rows, n)).astype(np.uint8)
    for filters in (0, 1, 2, 3, 4, rs.randint(0, 5, rows), "adaptive"):
        lines, types = K.filter_rows(raw, bpp, filters)
        whole = reconstruct(lines, bpp)
        assert np.array_equal(whole, raw)                          # the encoder and this decoder agree: `whole` is the truth
        for target in (1, 4, 64):
            table = np.zeros(rows, png.SEGMENT)
            cnt = L.load_library().radnet_png_plan_segments(lines.ctypes.data, 0, rows, n, target, table.ctypes.data_as(ctypes.c_void_p), rows)
            assert cnt >= 1
            check_legal(types, table[:cnt], n, 0)
            if isinstance(filters, int) and filters <= 1:
                assert cnt == -(-rows // target)
            got = np.concatenate([reconstruct(lines[f:f + r], bpp) for f, r in zip(first_rows(table[:cnt]), table["rows"][:cnt])])
            assert np.array_equal(got, whole), (filters if isinstance(filters, (int, str)) else "random", target)


def test_an_illegal_cut_does_change_the_bytes():
    """A control of this file's own `reconstruct`, not of the product (it runs no product code and passes without the feature): the
    check above can fail, because a segment cut in front of a Paeth row does not reconstruct to the pass's bytes."""
    raw = np.random.RandomState(2).randint(0, 256, (8, 12)).astype(np.uint8)
    lines, _ = K.filter_rows(raw, 3, 4)
    assert not np.array_equal(np.concatenate([reconstruct(lines[:4], 3), reconstruct(lines[4:], 3)]), raw)


def test_plan_segments_of_a_parsed_file():
    s = K.draw(np.random.RandomState(1), 150, 21, 2, 8)
    for interlace in (False, True):
        img = png.parse(K.encode(s, 2, 8, filters=np.random.RandomState(3), interlace=interlace).data)
        table = png.plan_segments(img, base_offset=4096)
        at = 0
        for p in img.passes:
            types = np.frombuffer(img.stream, np.uint8)[p.stream_offset::1 + p.rowbytes][:p.pass_h]
            n = int(np.searchsorted(np.cumsum(table["rows"][at:]), p.pass_h)) + 1
            check_legal(types, table[at:at + n], p.rowbytes, 4096 + p.stream_offset)
            at += n
        assert at == len(table)


# ---- the planner under sanitizers ---------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_planner_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "png_plan_sanitize")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "rock-art-radnet_amd", "csrc", "png_plan.cpp"),
           os.path.join(ROOT, "tests", "native", "png_plan_sanitize.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    # the sanitizer runtimes are linked statically: the program needs no place in the library list and the environment stays as it is
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


# ---- DeviceImageLoader.prefetch (fake decoders: the accounting alone) ------------------------------------------------------------
def test_prefetch_accounting(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    rs = np.random.RandomState(4)
    data = []
    for k in range(5):
        d = {"filepath": "maps/m%d.png" % k}
        for t in ("rgb", "topo"):
            path = utils_io.image_path(d["filepath"], t)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "wb") as f:
                f.write(K.encode(K.draw(rs, 10, 10 + k, 2, 8), 2, 8).data)
        data.append(d)
    batches, singles = [], []

    def blank(buf):
        return np.zeros(tuple(png.read_header(buf)[1::-1]) + (3,), np.uint8)

    def many(files):
        batches.append(len(files))
        return [blank(f) for f in files]

    def one(buf):
        singles.append(1)
        return blank(buf)

    pairs = [(d, t) for d in data for t in ("rgb", "topo")]
    loader = utils_io.DeviceImageLoader(cache_bytes=1 << 20, decode=one, decode_many=many)
    assert loader.prefetch(pairs + pairs[:3]) == 10 and batches == [10] and loader.prefetched == 10      # duplicates decode once
    got = [loader(d, t) for d, t in pairs]
    assert not singles and (loader.hits, loader.misses) == (10, 0)
    assert [g.shape for g in got] == [(10, 10 + k, 3) for k in range(5) for _ in range(2)]
    assert loader.prefetch(pairs) == 0 and batches == [10]                                               # all cached: nothing to do
    del batches[:], singles[:]
    # a cache of 1000 bytes: batches of decoded images within it (300 + 330 + 360 <= 1000 < + 390), least recently used evicted
    small = utils_io.DeviceImageLoader(cache_bytes=1000, decode=one, decode_many=many)
    rgb = [(d, "rgb") for d in data]
    assert small.prefetch(rgb) == 5 and batches == [3, 2] and small.used <= 1000
    small(*rgb[4])
    assert not singles and small.hits == 1
    small(*rgb[0])
    assert singles == [1] and small.misses == 1                                                          # evicted by the later batch
    # a cached pair named again moves to the recent end, so a later batch does not evict it first
    assert list(k[0] for k in small._lru) == [utils_io.image_path(rgb[i][0]["filepath"], "rgb") for i in (4, 0)]
    assert small.prefetch([rgb[4]]) == 0 and list(small._lru)[-1][0] == utils_io.image_path(rgb[4][0]["filepath"], "rgb")
    # only decode= customised: prefetch fills the cache through that decoder, file by file, so __call__ and prefetch agree
    del singles[:], batches[:]
    own = utils_io.DeviceImageLoader(cache_bytes=1 << 20, decode=one)
    assert own.prefetch(rgb) == 5 and len(singles) == 5 and not batches
    own(*rgb[2])
    assert len(singles) == 5 and (own.hits, own.misses) == (1, 0)
    batches[:] = [3, 2]
    off = utils_io.DeviceImageLoader(cache_bytes=0, decode=one, decode_many=many)
    assert off.prefetch(rgb) == 0 and batches == [3, 2]                                                  # nothing would be kept: nothing decoded
