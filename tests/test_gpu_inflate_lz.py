"""The device inflate for any stream against its Python model (tests/inflate_lz_cases.py) over whole sentinel-prefilled buffers: the
unit records of radnet_inflate_lz_measure, buf and src after radnet_inflate_lz_emit, src after radnet_inflate_lz_resolve, buf after
radnet_inflate_lz_gather, each with the sentinels in front of and behind it and the stream at an odd device address; resolve and
gather on a hostile table; what the entries refuse; png.decode_device(inflate="device-lz") byte for byte against the default on every
colour type and depth as other tools write them, with report["path"] == "device" asserted (a test that passes through the fallback
proves nothing); the fallbacks with their reasons; "device" and the default unchanged; get_image and predict_from_path."""
import copy
import os
import zlib

import numpy as np
import pytest

import inflate_lz_cases as Z
import png_cases as K

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL, SENTINEL_SRC, MARGIN = 0xA5, 0xA5A5A5A5, 64
ERR_ARG, ERR_UNSUPPORTED = -1, -3
NAMES = sorted(Z.cases())


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


def upload(data, offset=0):
    """(buffer, pointer): the bytes on the device at `offset` of an allocation, sentinels round them."""
    buf = torch.full((offset + len(data) + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    buf[offset:offset + len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    return buf, buf.data_ptr() + offset


def measure(ctx, png, z, ptr, starts):
    """(rc, the records as tuples): one sentinel record stands behind the table."""
    table = np.zeros(len(starts) + 1, png.INFLATE_LZ_UNIT)
    table.view(np.uint8)[:] = SENTINEL
    table["start_bit"][:len(starts)] = starts
    dev = torch.from_numpy(table.view(np.uint8).copy()).cuda()
    rc = ctx.lib.radnet_inflate_lz_measure(ctx.h, ptr, len(z), dev.data_ptr(), len(starts))
    ctx.sync()
    got = dev.cpu().numpy().view(png.INFLATE_LZ_UNIT)
    assert (got[len(starts):].view(np.uint8) == SENTINEL).all(), "written behind the unit table"
    return rc, [tuple(int(v) for v in u) for u in got[:len(starts)]]


class Buffers:
    """buf (uint8) and src (uint32) of n entries on the device, MARGIN sentinel entries in front of and behind each."""

    def __init__(self, n, buf=None, src=None):
        self.n = n
        self.buf = torch.full((n + 2 * MARGIN,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.src = torch.from_numpy(np.full(n + 2 * MARGIN, SENTINEL_SRC, np.uint32).view(np.int32)).cuda()
        if buf is not None:
            self.buf[MARGIN:MARGIN + n] = torch.from_numpy(np.asarray(buf, np.uint8).copy()).cuda()
        if src is not None:
            self.src[MARGIN:MARGIN + n] = torch.from_numpy(np.asarray(src, np.uint32).view(np.int32).copy()).cuda()
        self.buf_ptr, self.src_ptr = self.buf.data_ptr() + MARGIN, self.src.data_ptr() + 4 * MARGIN

    def host(self):
        """(buf, src) of the n entries, after checking the sentinels round them."""
        buf, src = self.buf.cpu().numpy(), self.src.cpu().numpy().view(np.uint32)
        for a, s in ((buf, SENTINEL), (src, SENTINEL_SRC)):
            assert (a[:MARGIN] == s).all(), "written in front of the buffer"
            assert (a[MARGIN + self.n:] == s).all(), "written behind the buffer"
        return buf[MARGIN:MARGIN + self.n], src[MARGIN:MARGIN + self.n]


def links_on_device(png, links):
    table = np.zeros(len(links), png.INFLATE_LINK)
    for k, (offset, start, out_bytes, prev) in enumerate(links):
        table[k] = (offset, start, out_bytes, prev, 0)
    return torch.from_numpy(table.view(np.uint8).copy()).cuda()


def resolve(ctx, b, n, rounds):
    """(rc, the counters): `rounds` launches; a sentinel stands behind the counters."""
    changed = torch.zeros(rounds + 1, dtype=torch.int32, device="cuda")
    changed[rounds] = -1
    rc = ctx.lib.radnet_inflate_lz_resolve(ctx.h, b.src_ptr, n, rounds, changed.data_ptr())
    ctx.sync()
    got = changed.cpu().numpy()
    assert got[rounds] == -1, "written behind the counters"
    return rc, got[:rounds].tolist()


def first_difference(a, b):
    return "first difference at entry %d" % int(np.flatnonzero(np.asarray(a) != np.asarray(b))[0])


# ---- the kernels against the model -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_measure_emit_resolve_and_gather_match_the_model(ctx, png, name):
    c = Z.cases()[name]
    starts, units = Z.model_units(name)
    offset = 1 + 2 * (NAMES.index(name) % 4)                           # 1, 3, 5, 7 bytes off an aligned address
    zbuf, ptr = upload(c.z, offset)
    rc, records = measure(ctx, png, c.z, ptr, starts)
    assert rc == 0, last_error(ctx)
    for got_u, want_u in zip(records, units):
        assert got_u == want_u, (name, dict(zip(Z.UNIT_FIELDS, got_u)), dict(zip(Z.UNIT_FIELDS, want_u)))
    code = Z.chain(units, 16, len(c.z), c.expected)[0]
    assert (code == Z.CHAIN_OK) == (c.reason in (None, "adler")) or c.corrupt, name
    if code == Z.CHAIN_OK:
        links, want_buf, want_src, want_flat, want_rounds, want_out = Z.model_buffers(name, SENTINEL, SENTINEL_SRC)
        n, table = c.expected, links_on_device(png, links)
        b = Buffers(n)
        rc = ctx.lib.radnet_inflate_lz_emit(ctx.h, ptr, len(c.z), table.data_ptr(), len(links), b.buf_ptr, b.src_ptr, n)
        ctx.sync()
        assert rc == 0, last_error(ctx)
        buf, src = b.host()
        assert np.array_equal(src, want_src), (name, first_difference(src, want_src))
        assert np.array_equal(buf, want_buf), (name, first_difference(buf, want_buf))
        rounds = Z.bound(n)
        rc, changed = resolve(ctx, b, n, rounds)
        assert rc == 0, last_error(ctx)
        buf, src = b.host()
        assert np.array_equal(src, want_flat), (name, first_difference(src, want_flat))
        assert np.array_equal(buf, want_buf), "resolve wrote the bytes"
        busy = [r for r, k in enumerate(changed) if k]
        assert busy == list(range(len(busy))) and len(busy) <= want_rounds <= rounds, (name, changed, want_rounds)
        assert ctx.lib.radnet_inflate_lz_gather(ctx.h, b.src_ptr, b.buf_ptr, n) == 0, last_error(ctx)
        ctx.sync()
        buf, src = b.host()
        assert np.array_equal(buf, want_out), (name, first_difference(buf, want_out))
        assert np.array_equal(src, want_flat), "gather wrote the table"
        if c.reason is None and not c.corrupt:
            assert buf.tobytes() == c.data
        # a short output cuts the units there and nothing is written behind it, in either array
        short = n - min(n, 5)
        b = Buffers(n)
        assert ctx.lib.radnet_inflate_lz_emit(ctx.h, ptr, len(c.z), table.data_ptr(), len(links), b.buf_ptr, b.src_ptr, short) == 0
        ctx.sync()
        buf, src = b.host()
        assert np.array_equal(src[:short], want_src[:short]) and (src[short:] == SENTINEL_SRC).all(), name
        assert np.array_equal(buf[:short], want_buf[:short]) and (buf[short:] == SENTINEL).all(), name
    assert bytes(zbuf.cpu().numpy()[offset:offset + len(c.z)]) == c.z, "the stream was written"


def test_units_entered_anywhere_measure_like_the_model(ctx, png):
    """Starts that are no block starts at all -- every 499th bit of the memLevel 1 noise stream and the bits round its end: garbage
    decodes to the model's record, whatever its status."""
    z = Z.cases()["noise memlevel 1"].z
    starts = sorted(set(range(16, 8 * len(z), 499)) | set(range(8 * len(z) - 40, 8 * len(z))))
    zbuf, ptr = upload(z, 3)
    rc, records = measure(ctx, png, z, ptr, starts)
    assert rc == 0, last_error(ctx)
    want = Z.measure(z, starts)
    assert records == want, [(dict(zip(Z.UNIT_FIELDS, g)), dict(zip(Z.UNIT_FIELDS, w))) for g, w in zip(records, want) if g != w][:3]
    assert len({u[5] for u in want}) >= 3 and Z.NOT_RLE not in {u[5] for u in want}, "several statuses are met, never not-run-length"


def test_resolve_and_gather_on_a_hostile_table(ctx):
    """Random entries, entries beyond the table, entries above their index: resolve reads and writes nothing outside the table, only
    ever lowers an entry that lies below its index, and ends at the model's flat table; gather reads nothing outside either."""
    rs = np.random.RandomState(44)
    n = 5 * 256 + 37
    i = np.arange(n)
    src = rs.randint(0, n, n).astype(np.uint32)                        # anything inside the table, above or below the index
    below = rs.rand(n) < 0.6
    src[below] = (i[below] * rs.rand(int(below.sum()))).astype(np.uint32)      # long chains of entries below their index
    wild = rs.rand(n) < 0.1
    src[wild] = rs.randint(n, 1 << 32, int(wild.sum()), dtype=np.int64).astype(np.uint32)      # beyond the table, up to 2^32 - 1
    src[7], src[n - 1] = 0xFFFFFFFF, n
    data = rs.randint(0, 256, n).astype(np.uint8)
    want_flat, want_rounds = Z.resolve(src)
    assert want_rounds >= 3 and (src > i).any() and (src >= n).any() and (src < i).any()
    b = Buffers(n, data, src)
    rc, changed = resolve(ctx, b, n, 1)
    assert rc == 0, last_error(ctx)
    buf, once = b.host()
    roots = src >= i
    assert np.array_equal(once[roots], src[roots]), "an entry at or above its index was written"
    assert (once[~roots] <= src[~roots]).all() and (once[~roots] < i[~roots]).all() and changed[0] == int((once != src).sum()) > 0
    rc, changed = resolve(ctx, b, n, Z.bound(n))
    assert rc == 0 and changed[-1] == 0, changed
    buf, flat = b.host()
    assert np.array_equal(flat, want_flat), first_difference(flat, want_flat)
    assert np.array_equal(buf, data), "resolve wrote the bytes"
    assert ctx.lib.radnet_inflate_lz_gather(ctx.h, b.src_ptr, b.buf_ptr, n) == 0
    ctx.sync()
    buf, flat = b.host()
    assert np.array_equal(buf, Z.gather(data, want_flat)) and np.array_equal(flat, want_flat)


def test_refused_arguments_launch_nothing(ctx, png):
    lib = ctx.lib
    z = Z.cases()["level 6, 300 bytes"].z
    n = len(z)
    zbuf, ptr = upload(z)
    units = torch.full((80,), SENTINEL, dtype=torch.uint8, device="cuda")
    for what, args, code in (("null stream", (None, n, units.data_ptr(), 1), ERR_ARG), ("null table", (ptr, n, None, 1), ERR_ARG), ("no units", (ptr, n, units.data_ptr(), 0), ERR_ARG),
                             ("n = 2", (ptr, 2, units.data_ptr(), 1), ERR_ARG), ("n = 2^29", (ptr, 1 << 29, units.data_ptr(), 1), ERR_UNSUPPORTED)):
        assert lib.radnet_inflate_lz_measure(ctx.h, *args) == code and last_error(ctx), what
    assert lib.radnet_inflate_lz_measure(None, ptr, n, units.data_ptr(), 1) == ERR_ARG
    links = links_on_device(png, [(0, 16, 300, 0)])
    b = Buffers(300, np.arange(300) % 251, np.maximum(np.arange(300), 2) - 2)      # a table resolve and gather would rewrite
    good = (ptr, n, links.data_ptr(), 1, b.buf_ptr, b.src_ptr, 300)
    for what, change, code in (("null stream", {0: None}, ERR_ARG), ("n = 2", {1: 2}, ERR_ARG), ("null table", {2: None}, ERR_ARG), ("no units", {3: 0}, ERR_ARG),
                               ("null output", {4: None}, ERR_ARG), ("null sources", {5: None}, ERR_ARG), ("a negative length", {6: -1}, ERR_ARG),
                               ("n = 2^29", {1: 1 << 29}, ERR_UNSUPPORTED), ("2^31 bytes", {6: 1 << 31}, ERR_UNSUPPORTED)):
        args = tuple(change.get(k, v) for k, v in enumerate(good))
        assert lib.radnet_inflate_lz_emit(ctx.h, *args) == code and last_error(ctx), what
    assert lib.radnet_inflate_lz_emit(None, *good) == ERR_ARG
    changed = torch.zeros(40, dtype=torch.int32, device="cuda")
    good = (b.src_ptr, 300, 4, changed.data_ptr())
    top = png_constant("RADNET_INFLATE_LZ_MAX_ROUNDS")
    for what, change, code in (("null table", {0: None}, ERR_ARG), ("a negative length", {1: -1}, ERR_ARG), ("no rounds", {2: 0}, ERR_ARG),
                               ("too many rounds", {2: top + 1}, ERR_ARG), ("null counters", {3: None}, ERR_ARG), ("2^31 entries", {1: 1 << 31}, ERR_UNSUPPORTED)):
        args = tuple(change.get(k, v) for k, v in enumerate(good))
        assert lib.radnet_inflate_lz_resolve(ctx.h, *args) == code and last_error(ctx), what
    assert lib.radnet_inflate_lz_resolve(None, *good) == ERR_ARG
    good = (b.src_ptr, b.buf_ptr, 300)
    for what, change, code in (("null table", {0: None}, ERR_ARG), ("null bytes", {1: None}, ERR_ARG), ("a negative length", {2: -1}, ERR_ARG),
                               ("2^31 bytes", {2: 1 << 31}, ERR_UNSUPPORTED)):
        args = tuple(change.get(k, v) for k, v in enumerate(good))
        assert lib.radnet_inflate_lz_gather(ctx.h, *args) == code and last_error(ctx), what
    assert lib.radnet_inflate_lz_gather(None, *good) == ERR_ARG
    assert lib.radnet_inflate_lz_resolve(ctx.h, b.src_ptr, 0, 4, changed.data_ptr()) == 0 and lib.radnet_inflate_lz_gather(ctx.h, b.src_ptr, b.buf_ptr, 0) == 0
    ctx.sync()
    buf, src = b.host()
    assert np.array_equal(buf, np.arange(300) % 251) and np.array_equal(src, np.maximum(np.arange(300), 2) - 2)
    assert (units.cpu().numpy() == SENTINEL).all() and (changed.cpu().numpy() == 0).all()
    assert lib.radnet_inflate_lz_emit(ctx.h, ptr, n, links.data_ptr(), 1, b.buf_ptr, b.src_ptr, 300) == 0      # and the arguments they were derived from pass
    assert lib.radnet_inflate_lz_resolve(ctx.h, b.src_ptr, 300, Z.bound(300), changed.data_ptr()) == 0 and lib.radnet_inflate_lz_gather(ctx.h, b.src_ptr, b.buf_ptr, 300) == 0
    ctx.sync()
    assert b.host()[0].tobytes() == Z.cases()["level 6, 300 bytes"].data


def png_constant(name):
    from radnet_hip import lib as L
    return L.header_constant(name)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def wrap(z, expected):
    """A one-row 8-bit grey PNG whose IDAT stream is z: 1 + width = expected bytes."""
    return b"".join([K.SIGNATURE, K.ihdr(expected - 1, 1, 8, 0), K.chunk(b"IDAT", z), K.chunk(b"IEND")])


def outcome(f):
    try:
        return "image", f().cpu().numpy()
    except ValueError as e:
        return "ValueError", str(e)


def same_outcome(a, b):
    return a[0] == b[0] and (np.array_equal(a[1], b[1]) if a[0] == "image" else a[1] == b[1])


def test_files_as_other_tools_write_them_decode_on_the_device(png):
    for what, data in Z.png_files():
        report = {}
        got = png.decode_device(data, inflate="device-lz", report=report)
        want = png.decode_device(data)
        assert report["path"] == "device" and report["reason"] is None, (what, report)
        assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got, want), what
        assert set(report) == {"path", "reason", "candidates", "false_candidates", "units", "blocks", "reconstruction", "rounds", "far_units"}, report
        assert report["units"] >= 1 and report["blocks"] >= report["units"] and 0 <= report["far_units"] <= report["units"]
        _, idat = Z.idat_of(data)
        expected = len(zlib.decompress(idat))
        model = Z.inflate(idat, expected)[2]
        assert (report["units"], report["blocks"], report["far_units"], report["candidates"]) == (model["units"], model["blocks"], model["far_units"], model["candidates"])
        assert report["rounds"] <= model["rounds"] <= Z.bound(expected)
        if what == "low noise, memlevel 1":
            assert report["units"] > 50 and report["far_units"] > 0, report
        if what == "low noise":
            assert report["far_units"] > 0
            as_array = png.decode_device(np.frombuffer(data, np.uint8), inflate="device-lz")     # the bytes as np.fromfile gives them
            assert torch.equal(as_array, want)


def test_run_length_files_decode_the_same_in_both_device_modes(png):
    rs = np.random.RandomState(5)
    img = K.draw(rs, 120, 160, 2, 8, "low").astype(np.uint8)
    dev = torch.from_numpy(np.ascontiguousarray(img[:, :, ::-1])).cuda()
    for kw in (dict(), dict(deflate="device"), dict(chunk_bytes=5000)):
        data = png.encode_device(dev, **kw)
        a, b = {}, {}
        got = png.decode_device(data, inflate="device-lz", report=a)
        assert a["path"] == "device" and a["far_units"] == 0 and torch.equal(got, dev), (kw, a)
        assert torch.equal(png.decode_device(data, inflate="device", report=b), dev) and b["path"] == "device"
        assert {k: a[k] for k in b} == b and set(a) - set(b) == {"rounds", "far_units"}, (a, b)


@pytest.mark.parametrize("name", ["h unit cap", "j flipped bit", "j truncated", "j bytes behind the final block", "j wrong adler", "k incomplete header",
                                  "hand far twin"])
def test_what_the_device_cannot_take_goes_to_the_host_path(png, name):
    c = Z.cases()[name]
    data = wrap(c.z, c.expected)
    want = outcome(lambda: png.decode_device(data))
    report = {}
    got = outcome(lambda: png.decode_device(data, inflate="device-lz", report=report))
    assert same_outcome(got, want), (name, got[0], want[0], got[1] if got[0] != "image" else "", want[1] if want[0] != "image" else "")
    assert report["path"] == "host" and report["reason"] == Z.model(name)[1], (name, report)
    assert report["reason"] == c.reason or c.reason is None
    assert report["units"] == 0 and report["reconstruction"] is None and report["rounds"] == 0 and report["far_units"] == 0
    assert (want[0] == "image") == (name in ("h unit cap", "j bytes behind the final block")), (name, want)


def test_other_fallbacks_the_run_length_mode_and_the_default(png):
    rs = np.random.RandomState(8)
    samples = K.draw(rs, 40, 50, 2, 8, "low")                           # four values: level 6 finds matches at every distance
    enc = K.encode(samples, 2, 8, filters=rs)
    report = {}
    got = png.decode_device(enc.data, inflate="device-lz", report=report)
    assert report["path"] == "device" and report["far_units"] > 0 and np.array_equal(got.cpu().numpy(), K.expand(samples, 2, 8)), report
    report = {}
    same = png.decode_device(enc.data, inflate="device", report=report)   # the run-length mode refuses the file as before
    assert report["path"] == "host" and "not run-length" in report["reason"] and torch.equal(same, got), report
    assert "rounds" not in report and "far_units" not in report
    report = {}
    want = png.decode_device(enc.data, report=report)                    # the default: the host path, nothing searched
    assert report == dict(path="host", reason=None, candidates=0, false_candidates=0, units=0, blocks=0, reconstruction=None)
    assert torch.equal(want, got)
    # a broken container and a filter type above 4: the default's exception
    broken = bytearray(enc.data)
    broken[len(broken) - 30] ^= 1
    lines = bytearray(enc.stream)
    lines[151 * 3] = 5
    type5 = b"".join([K.SIGNATURE, K.ihdr(50, 40, 8, 2), K.chunk(b"IDAT", zlib.compress(bytes(lines), 6)), K.chunk(b"IEND")])
    for what, data, reason in (("CRC", bytes(broken), "container: "), ("filter type 5", type5, "a filter type above 4")):
        want = outcome(lambda: png.decode_device(data))
        report = {}
        got = outcome(lambda: png.decode_device(data, inflate="device-lz", report=report))
        assert same_outcome(got, want) and want[0] == "ValueError" and report["path"] == "host" and report["reason"].startswith(reason), (what, report, got[0], want[0])
    with pytest.raises(ValueError, match="\"host\", \"device\" or \"device-lz\""):
        png.decode_device(enc.data, inflate="gpu")


def test_get_image_and_predict_from_path_reach_the_new_path(png, tmp_path, monkeypatch):
    from faster_rcnn import models as M
    from faster_rcnn import utils_io
    from faster_rcnn.base_models import resnet50 as base
    from faster_rcnn.config import Config
    from faster_rcnn.RADNet import RADNet
    from oracle import dense
    Cc = Config()
    Cc.img_size = 300
    ms = M.build_models(Cc, weights=copy.deepcopy(dense.init_params(seed=3)), workload="predict")
    rnet = RADNet(Cc, ms[3], ms[4], base.preprocess)
    Cc.tile_size, Cc.tile_overlap, Cc.include_full_img, Cc.use_img_type = 400, 250, True, False
    Cc.img_types = ["blended_grey"]
    rnet.bbox_threshold, rnet.device_tail, rnet.device_resident = 0.0, True, True
    y, x = np.mgrid[0:420, 0:460]
    img = np.stack([(x // 9 + y // 7 * 3 + c * 40) & 255 for c in range(3)], axis=2).astype(np.uint8)      # level 6 finds far matches in it
    os.makedirs(tmp_path / "blended_grey")
    (tmp_path / "blended_grey" / "scan.png").write_bytes(K.encode(img[:, :, ::-1], 2, 8, filters="adaptive").data)
    monkeypatch.chdir(tmp_path.parent)
    rel = tmp_path.name + "/scan.png"
    reports, decode = [], png.decode_device

    def watched(data, ctx=None, inflate="host", report=None):
        report = {} if report is None else report
        reports.append((inflate, report))
        return decode(data, ctx, inflate, report)
    monkeypatch.setattr(png, "decode_device", watched)
    assert np.array_equal(utils_io.get_image(rel, Cc.img_types, inflate="device-lz"), img)
    on_device = utils_io.get_image(rel, Cc.img_types, to_host=False, inflate="device-lz")
    assert on_device.is_cuda and np.array_equal(on_device.cpu().numpy(), img)
    assert [(i, r["path"], r["far_units"] > 0) for i, r in reports] == [("device-lz", "device", True)] * 2
    with pytest.raises(ValueError, match="device-lz"):
        utils_io.get_image(rel, Cc.img_types, inflate="lz")
    del reports[:]
    want = rnet.predict_from_path(rel)
    assert [(i, r["path"]) for i, r in reports] == [("host", "host")]
    rnet.png_inflate = "device-lz"
    got = rnet.predict_from_path(rel)
    assert [(i, r["path"]) for i, r in reports[1:]] == [("device-lz", "device")]
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert list(a) == list(b) and all(type(a[k]) is type(b[k]) and np.array_equal(a[k], b[k]) for k in a), (a, b)
