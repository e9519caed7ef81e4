"""The host half of the many-stream inflate.  The Python model of the five entries (tests/inflate_many_cases.py) on its case table:
every batch carries a tally that proves it reaches the branch it is for, the model inflates every valid stream of every batch to
its data and leaves everything else at the sentinel, and each deliberate mistake (MUTANTS) is caught by the batch named for it.
radnet_inflate_streams_check (csrc/inflate_plan.cpp) through every refusal, and under AddressSanitizer + UBSan in a stand-alone
program.  The new keywords' mode errors, DeviceImageLoader(prefetch_modes=) with fake decoders, RADNet.png_many.  No device needed."""
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import inflate_cases as I
import inflate_lz_cases as Z
import inflate_many_cases as M
import png_cases as K
from faster_rcnn import png, utils_io
from radnet_hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED = -1, -3
SENTINEL, SENTINEL_SRC = 0xA5, 0xA5A5A5A5


# ---- the case table ------------------------------------------------------------------------------------------------------------------
def test_the_batches_reach_the_branches_they_are_for():
    batches = M.batches()
    for gap in (0, 1, 15):
        b = batches["gap %d" % gap]
        assert [s[0] for s in b.streams] == ["f 1 bytes", "g deflate model dynamic", "stored with buried headers", "i level 6", "f 300 bytes", "b memlevel 1"]
        assert 4 <= len(b.table) <= 6 and all(9 <= n <= 10000 for _, n, _, _ in b.table)
        ends = [zo + n for zo, n, _, _ in b.table]
        assert [b.table[k + 1][0] - ends[k] for k in range(5)] == [gap] * 5 and b.table[0][0] == gap and len(b.z) - ends[-1] == gap
        cands, starts, units, per_stream, links = M.model(b.name, True)
        # the stored stream buries valid dynamic headers: candidates the chain never visits; level 6 has matches at other distances
        zo, n, _, _ = b.table[2]
        buried = [c for c in cands if 8 * zo <= c < 8 * (zo + n)]
        chained = {l[1] for l in per_stream[2][2]}
        assert len(buried) >= 5 and not set(buried) & chained
        assert all(code == Z.CHAIN_OK for code, _, _ in per_stream)
        far = [u for u in units if b.stream_of(u[0]) == 3 and u[5] == I.OK]
        assert sum(u[8] for u in far) > 10
        rle = M.model(b.name, False)[3]
        assert [code for code, _, _ in rle] == [I.CHAIN_OK] * 3 + [I.CHAIN_BAD_UNIT] + [I.CHAIN_OK] * 2      # level 6 is not run-length
        # units begin on every bit phase, and with a gap that is not a multiple of 8 ... every global phase too
        assert {l[1] % 8 for l in links} == set(range(8))
    a, b = batches["a cut in a header"], batches["b cut in a unit"]
    assert a.tally["unit_start"] + 17 < a.tally["cut_bits"] < a.tally["header_end"], "the cut falls inside the dynamic header"
    assert b.tally["header_end"] < b.tally["cut_bits"] < b.tally["unit_end"], "the cut falls behind the header, inside the unit"
    for batch in (a, b):
        zo, n, _, _ = batch.table[1]
        assert 8 * n == batch.tally["cut_bits"] and batch.z[zo + n:zo + n + 900] == I.cases()["b memlevel 1"].z[n:n + 900], "the rest stands in the gap"
    start = 8 * a.table[1][0] + a.tally["unit_start"]
    assert start not in M.find_many(a) and start in M.find_many(a, find_no_boundary=True)
    start = 8 * b.table[1][0] + b.tally["unit_start"]
    assert start in M.find_many(b)
    assert M.measure_many(b, [start], False)[0][5] == M.measure_many(b, [start], True)[0][5] == I.PAST_END
    assert M.measure_many(b, [start], True, measure_no_boundary=True)[0][5] == I.OK
    c = batches["c reach in front of the stream"]
    links = M.hand_links(c.name)
    assert M.clamped(c, links) > 0, "sources that fall in front of the stream's out_offset"
    buf, src = M.emit_lz_many(c, links, SENTINEL, SENTINEL_SRC)
    oo = c.table[1][2]
    written = src != SENTINEL_SRC
    assert written.sum() == links[0][2] and (src[written] >= oo).all() and not written[:oo].any()
    low = M.emit_lz_many(c, links, SENTINEL, SENTINEL_SRC, clamp_at_zero=True)[1]
    assert (low[written] < oo).any(), "clamped at 0 the link reads the neighbour's bytes"


@pytest.mark.parametrize("name", sorted(M.batches()))
def test_the_model_inflates_every_valid_stream_and_nothing_else(name):
    b = M.batches()[name]
    owned = np.zeros(b.out_len, bool)
    for lz in (False, True):
        cands, starts, units, per_stream, links = M.model(name, lz)
        if lz:
            buf, src = M.emit_lz_many(b, links, SENTINEL, SENTINEL_SRC)
            flat, _ = Z.resolve(src)
            out = Z.gather(buf, flat)
        else:
            out = M.emit_rle_many(b, links, SENTINEL)
        owned[:] = False
        for (zo, n, oo, expected), (sname, sz, data), (code, _, _) in zip(b.table, b.streams, per_stream):
            alone = (Z if lz else I).inflate(sz, expected)
            assert (code == 0) == (alone[0] is not None or alone[1] == "adler"), (name, sname, lz, code, alone[1])
            if code == 0:
                assert out[oo:oo + expected].tobytes() == data, (name, sname, lz)
                owned[oo:oo + expected] = True
        assert (out[~owned] == SENTINEL).all(), (name, lz, "written outside the streams that chain")
        # every record is the stream's own, shifted: the stream alone gives the same candidates
        for (zo, n, _, _), (sname, sz, _) in zip(b.table, b.streams):
            assert [c - 8 * zo for c in cands if 8 * zo <= c < 8 * (zo + n)] == I.find_blocks(sz, 16), (name, sname)


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_every_mutant_of_the_model_is_caught(mutant):
    name = M.CAUGHT_BY[mutant]
    b = M.batches()[name]
    cands, starts, units, _, links = M.model(name, True)
    if mutant == "find_no_boundary":
        assert M.find_many(b, find_no_boundary=True) != cands
    elif mutant == "measure_no_boundary":
        probe = starts + [8 * b.table[1][0] + b.tally["unit_start"]]
        assert M.measure_many(b, probe, True, measure_no_boundary=True) != M.measure_many(b, probe, True)
        assert M.measure_many(b, probe, False, measure_no_boundary=True) != M.measure_many(b, probe, False)
    elif mutant == "unshifted_end":
        assert M.measure_many(b, starts, True, unshifted_end=True) != units
        assert M.measure_many(b, starts, False, unshifted_end=True) != M.model(name, False)[2]
    elif mutant == "emit_no_boundary":
        hand = M.hand_links(name)
        assert not np.array_equal(M.emit_rle_many(b, hand, SENTINEL, emit_no_boundary=True), M.emit_rle_many(b, hand, SENTINEL))
        got, want = M.emit_lz_many(b, hand, SENTINEL, SENTINEL_SRC, emit_no_boundary=True), M.emit_lz_many(b, hand, SENTINEL, SENTINEL_SRC)
        assert not np.array_equal(got[0], want[0]) and not np.array_equal(got[1], want[1])
    else:
        hand = M.hand_links(name)
        assert not np.array_equal(M.emit_lz_many(b, hand, SENTINEL, SENTINEL_SRC, clamp_at_zero=True)[1], M.emit_lz_many(b, hand, SENTINEL, SENTINEL_SRC)[1])
    assert set(M.CAUGHT_BY) == set(M.MUTANTS)


# ---- radnet_inflate_streams_check ---------------------------------------------------------------------------------------------------
def table_of(rows):
    return np.array(rows, np.int64).view(png.INFLATE_STREAM).reshape(-1)


def test_the_constant_the_abi_mirror_and_the_bindings():
    assert png.INFLATE_MANY_MAX_STREAMS == L.header_constant("RADNET_INFLATE_MANY_MAX_STREAMS") == 4096
    assert png.INFLATE_STREAM.itemsize == 32
    assert [(n, png.INFLATE_STREAM.fields[n][1]) for n in png.INFLATE_STREAM.names] == [("z_offset", 0), ("n", 8), ("out_offset", 16), ("expected", 24)]
    for name in ("radnet_inflate_streams_check", "radnet_inflate_find_blocks_many", "radnet_inflate_rle_measure_many", "radnet_inflate_lz_measure_many",
                 "radnet_inflate_rle_emit_many", "radnet_inflate_lz_emit_many"):
        assert name in L.declared_symbols(), name


def test_streams_check_accepts_the_batches_and_names_every_refusal():
    for b in M.batches().values():
        assert L.inflate_streams_check(table_of(b.table), len(b.z), b.out_len) == (0, -1, ""), b.name
    good = [(0, 9, 0, 1), (10, 100, 1, 0), (125, 3, 8, 40)]
    assert L.inflate_streams_check(table_of(good), 128, 48)[0] == 0

    def refused(rows, z_len=128, out_len=48, count=None):
        rc, bad, msg = L.inflate_streams_check(None if rows is None else table_of(rows), z_len, out_len, count)
        assert rc != 0 and msg.startswith("inflate streams: "), (rc, msg)
        return rc, bad, msg
    rc, bad, msg = refused([good[0], good[2], good[1]])
    assert (rc, bad) == (ERR_ARG, 2) and "not sorted" in msg                                      # unsorted
    rc, bad, msg = refused([good[0], (8, 100, 1, 0), good[2]])
    assert (rc, bad) == (ERR_ARG, 1) and "overlaps" in msg                                        # overlapping in z
    rc, bad, msg = refused([good[0], (10, 100, 1, 8), good[2]])
    assert (rc, bad) == (ERR_ARG, 2) and "overlaps" in msg                                        # overlapping in the output
    assert refused(good, z_len=127)[:2] == (ERR_ARG, 2) and "outside" in refused(good, z_len=127)[2]      # outside z
    assert refused(good, out_len=47)[:2] == (ERR_ARG, 2) and "outside" in refused(good, out_len=47)[2]    # outside the output
    assert refused([(0, 2, 0, 1)])[:2] == (ERR_ARG, 0)
    assert refused([(-1, 9, 0, 1)])[0] == refused([(0, 9, -1, 1)])[0] == refused([(0, 9, 0, -1)])[0] == ERR_ARG
    assert refused([(0, 9, 0, 1), (2 ** 63 - 2, 5, 1, 1)])[:2] == (ERR_ARG, 1)                    # no sum wraps
    rc, bad, msg = refused(good, z_len=1 << 29)
    assert (rc, bad) == (ERR_UNSUPPORTED, -1) and "2^29" in msg                                   # both size limits
    rc, bad, msg = refused(good, out_len=1 << 31)
    assert (rc, bad) == (ERR_UNSUPPORTED, -1) and "2^31" in msg
    assert L.inflate_streams_check(table_of(good), (1 << 29) - 1, (1 << 31) - 1)[0] == 0
    assert refused(good, count=0)[:2] == (ERR_ARG, -1)                                            # count 0 and count above the cap
    full = [(3 * k, 3, k, 1) for k in range(png.INFLATE_MANY_MAX_STREAMS + 1)]
    assert L.inflate_streams_check(table_of(full[:-1]), 3 * len(full), len(full))[0] == 0
    assert refused(full, 3 * len(full), len(full))[:2] == (ERR_ARG, -1)
    assert refused(None, count=3)[:2] == (ERR_ARG, -1)
    assert refused(good, z_len=-1)[0] == refused(good, out_len=-1)[0] == ERR_ARG


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
@pytest.mark.skipif(bool(os.environ.get("LD_PRELOAD")), reason="LD_PRELOAD is set: a sanitized program wants its runtime first")
def test_streams_check_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "inflate_streams_check_sanitize")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-pthread",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "rock-art-radnet_amd", "csrc", "inflate_plan.cpp"),
           os.path.join(ROOT, "tests", "native", "inflate_streams_check_sanitize.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


# ---- modes and accounting ------------------------------------------------------------------------------------------------------------
def test_the_modes_of_decode_device_many_are_check_modes():
    data = K.encode(K.draw(np.random.RandomState(2), 5, 7, 2, 8), 2, 8).data
    for kw in (dict(inflate="gpu"), dict(crc="disk"), dict(join="gpu"), dict(unfilter="tile"), dict(crc="device"), dict(join="device"),
               dict(inflate="host", crc="device", join="device"), dict(inflate="device", unfilter="bands")):
        with pytest.raises(ValueError) as want:
            png.check_modes(**kw)
        with pytest.raises(ValueError) as got:
            png.decode_device_many([data], **kw)
        assert str(got.value) == str(want.value), kw
        with pytest.raises(ValueError) as one:
            png.decode_device(data, **kw)
        assert str(one.value) == str(want.value), kw
    # beside the host inflate the refusal is also what the entry raised while it had no such keyword: a TypeError
    for kw in (dict(crc="device"), dict(join="device"), dict(inflate="host", crc="device", join="device")):
        with pytest.raises(TypeError) as old:
            png.decode_device_many([data], **kw)
        assert isinstance(old.value, ValueError) and type(old.value) is png.HostInflateModeError
    with pytest.raises(ValueError) as plain:
        png.decode_device_many([data], join="gpu")
    assert type(plain.value) is ValueError
    assert png.decode_device_many([], inflate="device-lz", crc="device", join="device") == []
    report = {}
    assert png.decode_device_many([], report=report) == [] and report == dict(files=[], batches=0, overflow=0)


def test_the_layout_of_a_batch():
    at = png.many_layout(3, 160)
    assert (at.streams, at.z, at.palettes, at.total) == (0, 96, 256, 256 + 3 * 768) and at.z % 16 == 0
    at = png.many_layout(5, 1008, pieces=7, crc_count=7, sums=True)
    assert at.z == 160 and at.palettes == 160 + 1008 and at.pad == at.palettes + 5 * 768 and at.pieces == (at.pad + 7) & ~7
    assert at.table == at.pieces + 7 * 24 and at.sums == at.table + 7 * 24 and at.result == at.sums + 28 and at.total == at.result + 8
    files = [bytes(40), bytes(33), bytes(5)]
    assert png._batches(files) == [[0, 1, 2]]


def test_prefetch_modes_accounting(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    rs = np.random.RandomState(4)
    data = []
    for k in range(3):
        d = {"filepath": "maps/m%d.png" % k}
        path = utils_io.image_path(d["filepath"], "rgb")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as f:
            f.write(K.encode(K.draw(rs, 6, 8 + k, 2, 8), 2, 8).data)
        data.append(d)
    pairs = [(d, "rgb") for d in data]
    paths = [utils_io.image_path(d["filepath"], "rgb") for d in data]
    calls = []

    def stub(files, **kw):
        calls.append(([f if isinstance(f, str) else "bytes" for f in files], kw))
        return [np.zeros(tuple(png.read_header(f)[1::-1]) + (3,), np.uint8) for f in files]
    monkeypatch.setattr(png, "decode_device_many", stub)
    assert utils_io.DeviceImageLoader().prefetch_modes is False
    # the default: prefetch is what it was, whatever the modes of __call__ are
    loader = utils_io.DeviceImageLoader(inflate="device-lz", crc="device", join="device")
    assert loader.prefetch(pairs) == 3 and calls == [(["bytes"] * 3, {})]
    del calls[:]
    loader = utils_io.DeviceImageLoader(inflate="device-lz", unfilter="tiles")
    assert loader.prefetch(pairs) == 3 and calls == [(["bytes"] * 3, dict(unfilter="tiles"))]
    del calls[:]
    # prefetch_modes: the modes go to decode_device_many; paths, not arrays, with join="device"
    loader = utils_io.DeviceImageLoader(inflate="device-lz", crc="device", join="device", prefetch_modes=True)
    assert loader.prefetch(pairs + pairs[:1]) == 3 and loader.prefetched == 3
    assert calls == [(paths, dict(unfilter="band", inflate="device-lz", crc="device", join="device"))]
    assert [loader(d, t).shape for d, t in pairs] == [(6, 8 + k, 3) for k in range(3)] and (loader.hits, loader.misses) == (3, 0)
    del calls[:]
    loader = utils_io.DeviceImageLoader(inflate="device", unfilter="tiles", prefetch_modes=True)
    assert loader.prefetch(pairs) == 3 and calls == [(["bytes"] * 3, dict(unfilter="tiles", inflate="device", crc="host", join="host"))]
    del calls[:]
    loader = utils_io.DeviceImageLoader(prefetch_modes=True)              # nothing to hand on: the call is the default's
    assert loader.prefetch(pairs) == 3 and calls == [(["bytes"] * 3, {})]
    del calls[:]
    # a caller's own decoders are called as they are
    own = []
    loader = utils_io.DeviceImageLoader(inflate="device", join="device", prefetch_modes=True, decode_many=lambda files: own.append(len(files)) or stub(files))
    assert loader.prefetch(pairs) == 3 and own == [3] and calls == [(["bytes"] * 3, {})]
    with pytest.raises(ValueError, match="needs inflate"):
        utils_io.DeviceImageLoader(join="device", prefetch_modes=True)


def test_png_many_is_off_by_default_and_reads_the_types_in_one_call(tmp_path, monkeypatch):
    from faster_rcnn.RADNet import RADNet
    assert RADNet.png_many is False
    monkeypatch.chdir(tmp_path)
    for t in ("grey", "topo"):
        os.makedirs(os.path.join("maps", t))
        with open(os.path.join("maps", t, "scan.png"), "wb") as f:
            f.write(K.encode(K.draw(np.random.RandomState(3), 4, 4, 2, 8), 2, 8).data)
    singles, batches = [], []
    monkeypatch.setattr(utils_io, "get_image", lambda path, kinds, **kw: singles.append((kinds, kw)) or "one")
    monkeypatch.setattr(png, "decode_device_many", lambda files, **kw: batches.append(([f if isinstance(f, str) else "bytes" for f in files], kw)) or ["many"] * len(files))
    monkeypatch.setattr(RADNet, "_takes_device_images", lambda self: True)
    monkeypatch.setattr(RADNet, "predict", lambda self, images: images)
    net = object.__new__(RADNet)
    net.C = types.SimpleNamespace(use_img_type=True, img_types=["grey", "topo"])
    assert net.predict_from_path("maps/scan.png") == ["one", "one"] and not batches and [k for k, _ in singles] == [["grey"], ["topo"]]
    net.png_many, net.png_inflate, net.png_join = True, "device-lz", "device"
    assert net.predict_from_path("maps/scan.png") == ["many", "many"] and len(singles) == 2
    assert batches == [([os.path.join("maps", "grey", "scan.png"), os.path.join("maps", "topo", "scan.png")],
                        dict(inflate="device-lz", unfilter="band", crc="host", join="device"))]
    net.png_join = "host"
    net.predict_from_path("maps/scan.png")
    assert batches[1] == (["bytes", "bytes"], dict(inflate="device-lz", unfilter="band", crc="host", join="host"))
    net.C.img_types = ["grey"]                                            # one type: nothing to batch
    assert net.predict_from_path("maps/scan.png") == ["one"] and len(batches) == 2
    net.C = types.SimpleNamespace(use_img_type=False, img_types=["grey", "topo"])
    assert net.predict_from_path("maps/scan.png") == ["one"] and len(batches) == 2
