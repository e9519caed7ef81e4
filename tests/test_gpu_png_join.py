"""The IDAT join on the device: radnet_png_join_u8 through the C ABI (csrc/png_join.hip) against the model of tests/png_join_cases.py
-- the output between sentinels at its case's byte address, the file at its own, the file and the table compared after the call --,
the refusals; then join="device" of png.decode_device, utils_io.get_image and the loader against the defaults, good files and
corrupt ones."""
import numpy as np
import pytest

import png_cases as K
import png_join_cases as JC
from test_gpu_crc32 import idat_chunks, outcome, read_files, recompressed      # noqa: F401  (read_files: the fixture of the four files)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = 0xA5
ERR_ARG = -1
GUARD = 64                       # sentinel bytes in front of and behind every buffer


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


def guarded(payload, at=0):
    """`payload` between sentinels in device memory, its first byte `at` bytes behind a 16-byte boundary: (tensor, offset of the
    payload, the host copy)."""
    host = np.full(GUARD + 16 + len(payload) + GUARD, SENTINEL, np.uint8)
    dev = torch.from_numpy(host).cuda()
    start = GUARD + (at - (dev.data_ptr() + GUARD)) % 16
    host[start:start + len(payload)] = payload
    dev.copy_(torch.from_numpy(host))
    return dev, start, host


def run(ctx, file, table, n, out_at=0, file_at=0, count=None, file_len=None, handle=True, null=(), table_shift=0):
    """One call: (rc, message, out[0 .. n) or None, True when nothing but out[0 .. n) was written -- and, after a refusal, nothing
    at all).  null: names among file, host, dev, out passed as null pointers; table_shift: bytes added to the device table's address."""
    count = len(table) if count is None else count
    file_len = len(file) if file_len is None else file_len
    buf, f0, buf_host = guarded(file, file_at)
    rows = np.zeros(max(len(table), 1) + 1, JC.PIECE)
    rows[:len(table)] = table
    table_dev, t0, table_was = guarded(rows.view(np.uint8))
    out, o0, out_was = guarded(np.full(max(n, 0), SENTINEL, np.uint8), out_at)
    assert (buf.data_ptr() + f0) % 16 == file_at and (out.data_ptr() + o0) % 16 == out_at and (table_dev.data_ptr() + t0) % 8 == 0
    ptr = dict(file=buf.data_ptr() + f0, host=rows.ctypes.data, dev=table_dev.data_ptr() + t0 + table_shift, out=out.data_ptr() + o0)
    for name in null:
        ptr[name] = None
    rc = ctx.lib.radnet_png_join_u8(ctx.h if handle else None, ptr["file"], file_len, ptr["host"], ptr["dev"], count, ptr["out"], n)
    msg = ctx.lib.radnet_last_error(ctx.h)
    ctx.sync()
    got = out.cpu().numpy()
    written = np.zeros(len(got), bool)
    if rc == 0:
        written[o0:o0 + n] = True
    clean = (np.array_equal(buf.cpu().numpy(), buf_host) and np.array_equal(table_dev.cpu().numpy(), table_was)
             and np.array_equal(got[~written], out_was[~written]))
    return rc, (msg.decode() if msg else ""), (got[o0:o0 + n].copy() if rc == 0 else None), clean


CASES = JC.cases()
BY_NAME = {c["name"]: c for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_every_case_equals_the_model(ctx, case):
    want = JC.model(case["file"], case["table"], case["n"], case["out_at"])
    rc, msg, got, clean = run(ctx, case["file"], case["table"], case["n"], case["out_at"], case["file_at"])
    assert rc == 0, msg
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
    assert clean                                          # the sentinels round the output, the file and the table


def test_every_alignment_of_the_output_against_every_alignment_of_the_file(ctx):
    case = BY_NAME["odd gaps"]
    want = JC.joined(case["file"], case["table"])
    for out_at in JC.ALIGNMENTS + (15,):
        for file_at in JC.ALIGNMENTS:
            rc, msg, got, clean = run(ctx, case["file"], case["table"], case["n"], out_at, file_at)
            assert rc == 0 and np.array_equal(got, want) and clean, (out_at, file_at, msg)


def test_outputs_shorter_than_a_grain(ctx):
    file = JC.content(64, 31)
    for n in (1, 2, 15, 16, 17):
        for out_at in (0, 1, 15):
            table = JC.table_of([3, 40], [n // 2, n - n // 2])
            rc, msg, got, clean = run(ctx, file, table, n, out_at, 5)
            assert rc == 0 and np.array_equal(got, JC.model(file, table, n, out_at)) and clean, (n, out_at, msg)


def test_the_mutants_cases_run_on_the_device(ctx):
    """The cases that tell the model's five mutants from the model are among those above; here by name, so that a renamed case shows."""
    for mutant in JC.MUTANTS:
        case = BY_NAME[JC.CAUGHT_BY[mutant]]
        rc, msg, got, clean = run(ctx, case["file"], case["table"], case["n"], case["out_at"], case["file_at"])
        assert rc == 0 and clean and not np.array_equal(got, JC.model(case["file"], case["table"], case["n"], case["out_at"], mutant=mutant)), mutant
        assert np.array_equal(got, JC.joined(case["file"], case["table"])), mutant


def test_nothing_to_write_launches_nothing(ctx):
    file = JC.content(40, 32)
    empty = JC.table_of([0, 40, 7], [0, 0, 0])
    for table, null in ((empty, ()), (empty, ("file", "out", "dev")), (JC.table_of([], []), ()), (JC.table_of([], []), ("file", "host", "dev", "out"))):
        rc, msg, got, clean = run(ctx, file, table, 0, 3, 1, null=null)
        assert rc == 0 and clean, msg


def test_refusals_launch_nothing(ctx):
    file = JC.content(200, 33)
    good = JC.table_of([10, 100, 30], [50, 0, 70])

    def refused(table=good, n=120, say="png_join", **kw):
        rc, msg, got, clean = run(ctx, file, table, n, 3, 7, **kw)
        assert rc == ERR_ARG and clean, (rc, msg, kw)
        assert say in msg, msg
    for name in ("file", "host", "dev", "out"):
        refused(null=(name,), say="null pointer")
    refused(count=-1, say="-1 pieces")
    refused(file_len=-1, say="a file of -1 bytes")
    refused(n=-1, say="an output of -1 bytes")
    refused(table_shift=4, say="8-byte aligned")
    refused(n=119, say="passes the output")
    refused(n=121, say="the pieces hold 120 bytes")
    refused(file_len=99, say="piece 1")
    for row, field, value in ((0, "src", -1), (2, "length", -1), (2, "src", 131), (0, "length", 191), (1, "src", (1 << 63) - 1), (2, "length", (1 << 63) - 1),
                              (1, "dst", 49), (2, "dst", 51)):
        t = good.copy()
        t[field][row] = value
        refused(t, say="piece %d" % row)
    rc, msg, got, clean = run(ctx, file, good, 120, handle=False)
    assert rc == ERR_ARG and clean
    # the output inside the file's buffer, in front of it and reaching in, behind it and starting inside
    both = torch.from_numpy(np.concatenate([file, np.full(200, SENTINEL, np.uint8)])).cuda()
    table_dev = torch.from_numpy(good.view(np.uint8)).cuda()
    base = both.data_ptr()
    for file_at, out_at in ((0, 40), (100, 0), (0, 199), (100, 99)):
        rc = ctx.lib.radnet_png_join_u8(ctx.h, base + file_at, 200, good.ctypes.data, table_dev.data_ptr(), 3, base + out_at, 120)
        assert rc == ERR_ARG and b"overlaps" in ctx.lib.radnet_last_error(ctx.h), (file_at, out_at)
    rc = ctx.lib.radnet_png_join_u8(ctx.h, base, 200, good.ctypes.data, table_dev.data_ptr(), 3, base + 200, 120)      # side by side: legal
    ctx.sync()
    after = both.cpu().numpy()
    assert rc == 0 and np.array_equal(after[:200], file) and np.array_equal(after[200:320], JC.joined(file, good)) and (after[320:] == SENTINEL).all()
    rc, msg, got, clean = run(ctx, file, good, 120, 3, 7)                 # and the context still works
    assert rc == 0 and clean and np.array_equal(got, JC.joined(file, good))


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def split_trailer(data, rle):
    """`data` recompressed, its first IDAT chunk 1 byte long and its trailer split over chunks of 1, 0 and 2 bytes behind the rest."""
    whole = recompressed(data, (), rle=rle)
    (start, end), = idat_chunks(whole)
    z = whole[start:end]
    cuts = [z[:1], z[1:-3], z[-3:-2], b"", z[-2:]]
    return whole[:start - 8] + b"".join(K.chunk(b"IDAT", c) for c in cuts) + K.chunk(b"IEND")


NAMES = ["one idat", "many idat", "a zero-length idat", "zero-length first and 8-byte ones", "a 1-byte first idat and a split trailer"]


@pytest.mark.parametrize("inflate", ["device", "device-lz"])
@pytest.mark.parametrize("name", NAMES)
def test_the_reader_gives_the_same_image_and_the_same_errors(png, read_files, inflate, name):
    if name == NAMES[-1]:
        data = split_trailer(read_files["one idat"][0], rle=inflate == "device")
        chunks = idat_chunks(data)
        assert [e - s for s, e in chunks][0] == 1 and [e - s for s, e in chunks][-3:] == [1, 0, 2]
    else:
        source, sizes = read_files[name]
        data = recompressed(source, sizes, rle=inflate == "device")
        chunks = idat_chunks(data)
        assert len(chunks) == len(sizes) + 1
    want = png.decode_device(data)
    plain = {}
    assert torch.equal(png.decode_device(data, inflate=inflate, report=plain), want) and "join" not in plain and plain["path"] == "device"
    for crc in png.CRC_MODES:
        for unfilter in ("band", "tiles"):
            report = {}
            got = png.decode_device(data, inflate=inflate, crc=crc, unfilter=unfilter, join="device", report=report)
            assert torch.equal(got, want), (name, crc, unfilter, report)
            assert report["path"] == "device" and report["join"] == "device" and report["reason"] is None, report
            assert report.get("crc") == ("device" if crc == "device" else None), report
    # one flipped payload byte, one flipped CRC field: in the largest chunk and in the first one (which may be empty)
    big = max(range(len(chunks)), key=lambda k: chunks[k][1] - chunks[k][0])
    spoiled = [(big, chunks[big][0] + (chunks[big][1] - chunks[big][0]) // 2), (big, chunks[big][1] + 3), (0, chunks[0][1])]
    for k, at in spoiled:
        bad = bytearray(data)
        bad[at] ^= 0x04
        bad = bytes(bad)
        expected = outcome(lambda: png.decode_device(bad))
        assert expected[0] == "ValueError" and "CRC mismatch in the b'IDAT' chunk" in expected[1]
        for crc in png.CRC_MODES:
            report = {}
            assert outcome(lambda: png.decode_device(bad, inflate=inflate, crc=crc, join="device", report=report)) == expected
            assert report["path"] == "host" and report["join"] == "host", (name, k, crc, report)
            if crc == "device":
                assert report["crc"] == "host" and report["reason"] == "crc: IDAT chunk %d" % k, (name, k, report)
            else:
                assert report["reason"].startswith("container: PNG: CRC mismatch in the b'IDAT' chunk"), (name, k, report)
    with pytest.raises(ValueError, match="not inflate=\"host\""):
        png.decode_device(data, join="device")


def test_get_image_and_the_loader_pass_the_option_on(png, tmp_path, monkeypatch):
    from faster_rcnn import utils_io
    rs = np.random.RandomState(61)
    data = recompressed(K.encode(K.draw(rs, 30, 40, 2, 8, "low"), 2, 8, filters="adaptive").data, (5, 0, 9))
    (tmp_path / "maps" / "grey").mkdir(parents=True)
    (tmp_path / "maps" / "grey" / "scan.png").write_bytes(data)
    monkeypatch.chdir(tmp_path)
    want = png.decode_device(data)
    path = "maps/scan.png"                                                # image_path: maps/<type>/scan.png
    seen = []
    real = png.decode_device
    monkeypatch.setattr(png, "decode_device", lambda buf, **kw: seen.append(kw) or real(buf, **kw))
    got = utils_io.get_image(path, ["grey"], to_host=False, inflate="device", join="device")
    assert torch.equal(got, want)
    assert np.array_equal(utils_io.get_image(path, ["grey"], inflate="device-lz", crc="device", join="device"), want.cpu().numpy())
    with pytest.raises(ValueError, match="not inflate=\"host\""):
        utils_io.get_image(path, ["grey"], join="device")
    loader = utils_io.DeviceImageLoader(inflate="device", join="device")
    assert torch.equal(loader(dict(filepath=path), "grey"), want) and loader.misses == 1
    assert seen == [dict(inflate="device", join="device"), dict(inflate="device-lz", crc="device", join="device"), dict(inflate="host", join="device"),
                    dict(inflate="device", join="device")]
