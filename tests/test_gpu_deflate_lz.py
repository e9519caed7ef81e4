"""The device LZ deflate against its Python model (tests/deflate_lz_cases.py), byte for byte, over sentinel-filled buffers:
radnet_deflate_lz_scan_u8's token table, both histograms and Adler parts, radnet_deflate_lz_emit_u8's pieces and sizes,
radnet_deflate_pack's packed bytes -- with the stream at 0, 1, 3, 7 and 13 bytes behind a 16-byte boundary; what the entries refuse;
png.encode_device(deflate="device-lz") read back by the host inflate, the device LZ inflate and the tests' own decoder, never longer
than deflate="device", and byte-equal to it where run-length wins."""
import zlib

import numpy as np
import pytest

import deflate_cases as D
import deflate_lz_cases as Z
import png_write_cases as W

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = 0xA5
ERR_ARG, ERR_UNSUPPORTED = -1, -3


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


@pytest.fixture(scope="module")
def cut(png):
    from radnet_hip import lib as L
    return L.header_constant("RADNET_DEFLATE_CHUNK"), L.header_constant("RADNET_DEFLATE_TILE")


@pytest.fixture(scope="module")
def rule(png):
    from radnet_hip import lib as L
    return dict(group=L.header_constant("RADNET_DEFLATE_LZ_GROUP"), far_min=L.header_constant("RADNET_DEFLATE_LZ_FAR_MIN"),
                far_min2=L.header_constant("RADNET_DEFLATE_LZ_FAR_MIN2"), far_d=L.header_constant("RADNET_DEFLATE_LZ_FAR_D"))


@pytest.fixture(scope="module")
def streams(cut, rule):
    return Z.streams(cut[0], cut[1], rule)


NAMES = sorted(Z.streams(65536, 4096))                                 # the names do not depend on the cut
# the stream starts this far off a 16-byte boundary: the byte-wise loads
MISALIGNED = {"mixed tile+1": 1, "mixed 2chunk+3": 3, "rgb panel": 7, "match cut by the tile end": 13, "mixed 5": 1, "source 32768 back": 3, "panel": 13}


def last_error(ctx):
    msg = ctx.lib.radnet_last_error(ctx.h)
    return msg.decode() if msg else ""


def upload(data, offset=0):
    """(buffer, pointer): the bytes on the device at `offset` of an allocation, sentinels round them."""
    buf = torch.full((offset + len(data) + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    buf[offset:offset + len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    return buf, buf.data_ptr() + offset


def scan(ctx, data, near, chunk, offset=0, hists=None):
    """(rc, token table, hist_ll [286], hist_d [30], parts [chunks][2], the table on the device) with the guards behind all four checked."""
    chunks, n = -(-len(data) // chunk), len(data)
    buf, ptr = upload(data, offset)
    tokens = torch.full((n + 8,), -1, dtype=torch.int32, device="cuda")
    hists = torch.zeros(286 + 2 + 30 + 2, dtype=torch.int32, device="cuda") if hists is None else hists
    hists[286:288] = -1
    hists[318:] = -1
    parts = torch.full((2 * chunks + 2,), -1, dtype=torch.int64, device="cuda")
    rc = ctx.lib.radnet_deflate_lz_scan_u8(ctx.h, ptr, n, near, tokens.data_ptr(), hists.data_ptr(), hists.data_ptr() + 288 * 4, parts.data_ptr())
    ctx.sync()
    t, h, p = tokens.cpu().numpy(), hists.cpu().numpy(), parts.cpu().numpy()
    assert (t[n:] == -1).all() and (h[286:288] == -1).all() and (h[318:] == -1).all() and (p[2 * chunks:] == -1).all(), "written behind a table"
    assert bytes(buf.cpu().numpy()[offset:offset + n]) == data, "the stream was written"
    return rc, t[:n].view(np.uint32), h[:286].view(np.uint32), h[288:318].view(np.uint32), p[:2 * chunks].view(np.uint64).reshape(chunks, 2), tokens


def emit(ctx, data, tokens, chunk, code_ll, code_d, header, nbits, offset=0, extra_cap=0):
    """(rc, [piece bytes], sizes, the piece buffer, piece_cap): every byte of the buffer behind a piece's size must be the sentinel."""
    chunks = -(-len(data) // chunk)
    cap = int(ctx.lib.radnet_deflate_lz_piece_cap(code_ll.ctypes.data, code_d.ctypes.data, nbits)) + extra_cap
    buf, ptr = upload(data, offset)
    pieces = torch.full((chunks * cap + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    sizes = torch.full((chunks + 2,), -1, dtype=torch.int32, device="cuda")
    hdr = np.frombuffer(header, np.uint8)
    rc = ctx.lib.radnet_deflate_lz_emit_u8(ctx.h, ptr, len(data), tokens.data_ptr(), code_ll.ctypes.data, code_d.ctypes.data, hdr.ctypes.data, nbits,
                                           pieces.data_ptr(), cap, sizes.data_ptr())
    ctx.sync()
    got, s = pieces.cpu().numpy(), sizes.cpu().numpy()
    assert (s[chunks:] == -1).all() and (got[chunks * cap:] == SENTINEL).all(), "written behind the sizes or the pieces"
    out = []
    if rc == 0:
        for c in range(chunks):
            assert 0 < s[c] <= cap, (c, s[c], cap)
            out.append(bytes(got[c * cap:c * cap + s[c]]))
            assert (got[c * cap + s[c]:(c + 1) * cap] == SENTINEL).all(), "piece %d: bytes behind its size were written" % c
    return rc, out, s[:chunks], pieces, cap


def pack(ctx, pieces, cap, sizes):
    count, want = len(sizes), int(np.asarray(sizes, np.int64).sum())
    sizes_dev = torch.from_numpy(np.asarray(sizes, np.int32).copy()).cuda()
    out = torch.full((want + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    total = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    rc = ctx.lib.radnet_deflate_pack(ctx.h, pieces.data_ptr(), cap, sizes_dev.data_ptr(), count, out.data_ptr(), want, total.data_ptr())
    ctx.sync()
    got, t = out.cpu().numpy(), total.cpu().numpy()
    assert t[1] == -1 and (got[want:] == SENTINEL).all(), "written behind the total or the packed bytes"
    return rc, bytes(got[:want]), int(t[0])


# ---- the two entries against the model --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_scan_emit_and_pack_match_the_model(ctx, png, cut, rule, streams, name):
    (data, near), offset = streams[name], MISALIGNED.get(name, 0)
    want_toks = Z.tokens(data, cut[0], cut[1], near, rule)
    rc, table, hist_ll, hist_d, parts, tokens = scan(ctx, data, near, cut[0], offset)
    assert rc == 0, last_error(ctx)
    want_table = Z.token_table(want_toks, len(data))
    if not np.array_equal(table, want_table):
        at = int(np.flatnonzero(table != want_table)[0])
        pytest.fail("%s: the token table differs first at byte %d: 0x%08x, the model has 0x%08x" % (name, at, table[at], want_table[at]))
    want_ll, want_d = Z.histograms(want_toks)
    assert np.array_equal(hist_ll, want_ll) and np.array_equal(hist_d, want_d), name
    assert parts.tolist() == D.adler_parts(data, cut[0]), name
    adler = png.adler32_of_parts(parts, len(data))
    assert adler == zlib.adler32(data)
    code_ll, code_d, header, nbits = png.huffman_codes_lz(hist_ll, hist_d)
    len_ll, len_d = [int(v) for v in code_ll["length"]], [int(v) for v in code_d["length"]]
    want = Z.pieces(want_toks, len_ll, len_d, header, nbits, [int(v) for v in code_ll["bits"]], [int(v) for v in code_d["bits"]])
    rc, got, sizes, pieces, cap = emit(ctx, data, tokens, cut[0], code_ll, code_d, header, nbits, offset, extra_cap=len(data) % 2)      # odd pieces too
    assert rc == 0, last_error(ctx)
    assert sizes.tolist() == [len(p) for p in want], name
    for c, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, "piece %d differs first at byte %d" % (c, next(i for i in range(len(w)) if g[i] != w[i])))
    rc, packed, total = pack(ctx, pieces, cap, sizes)
    assert rc == 0 and total == len(packed) and packed == b"".join(want), name
    out, eof, unused = D.inflate(b"\x78\x01" + packed + adler.to_bytes(4, "big"))
    assert out == data and eof and unused == b"", name
    chunks = -(-len(data) // cut[0])
    assert 8 * len(packed) - 35 * (chunks - 1) - 7 * chunks <= png.stream_bits(hist_ll, code_ll, nbits, chunks, hist_d, code_d) <= 8 * len(packed) - 35 * (chunks - 1)


def test_scan_adds_to_the_histograms_it_is_given(ctx, cut, rule, streams):
    data, near = streams["rgb panel"]
    want_ll, want_d = Z.histograms(Z.tokens(data, cut[0], cut[1], near, rule))
    hists = torch.zeros(320, dtype=torch.int32, device="cuda")
    for times in (1, 2):
        rc, _, hist_ll, hist_d, _, _ = scan(ctx, data, near, cut[0], hists=hists)
        assert rc == 0 and np.array_equal(hist_ll, times * want_ll) and np.array_equal(hist_d, times * want_d)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_leave_the_buffers_untouched(ctx, png, cut, rule):
    lib, data = ctx.lib, (bytes(range(200)) * 3 + bytes(range(40)) * 4)
    n = len(data)
    buf, ptr = upload(data)
    tokens = torch.full((n + 8,), 7, dtype=torch.int32, device="cuda")
    hist_ll = torch.full((286,), 7, dtype=torch.int32, device="cuda")
    hist_d = torch.full((30,), 7, dtype=torch.int32, device="cuda")
    parts = torch.full((2,), 7, dtype=torch.int64, device="cuda")
    good = dict(stream=ptr, n=n, near=3, tokens=tokens.data_ptr(), ll=hist_ll.data_ptr(), d=hist_d.data_ptr(), parts=parts.data_ptr())

    def call_scan(handle=True, **kw):
        a = dict(good, **kw)
        return lib.radnet_deflate_lz_scan_u8(ctx.h if handle else None, a["stream"], a["n"], a["near"], a["tokens"], a["ll"], a["d"], a["parts"])

    for what, kw, code in (("null stream", dict(stream=None), ERR_ARG), ("null table", dict(tokens=None), ERR_ARG), ("null literal counts", dict(ll=None), ERR_ARG),
                           ("null distance counts", dict(d=None), ERR_ARG), ("null parts", dict(parts=None), ERR_ARG), ("n = 0", dict(n=0), ERR_ARG),
                           ("n < 0", dict(n=-5), ERR_ARG), ("near = 0", dict(near=0), ERR_ARG), ("near = 32769", dict(near=32769), ERR_ARG),
                           ("a misaligned table", dict(tokens=tokens.data_ptr() + 4), ERR_ARG), ("n = 2^32", dict(n=1 << 32), ERR_UNSUPPORTED)):
        assert call_scan(**kw) == code and last_error(ctx), what
    assert call_scan(handle=False) == ERR_ARG
    ctx.sync()
    assert (tokens.cpu().numpy() == 7).all() and (hist_ll.cpu().numpy() == 7).all() and (hist_d.cpu().numpy() == 7).all() and (parts.cpu().numpy() == 7).all()
    hist_ll.zero_()
    hist_d.zero_()
    assert call_scan() == 0 and call_scan(near=32768) == 0                                    # the bounds themselves pass
    ctx.sync()
    hist_ll.zero_()
    hist_d.zero_()
    assert call_scan() == 0
    ctx.sync()
    want_toks = Z.tokens(data, cut[0], cut[1], 3, rule)
    assert np.array_equal(tokens.cpu().numpy()[:n].view(np.uint32), Z.token_table(want_toks, n))

    code_ll, code_d, header, nbits = png.huffman_codes_lz(hist_ll.cpu().numpy().view(np.uint32), hist_d.cpu().numpy().view(np.uint32))
    cap = int(lib.radnet_deflate_lz_piece_cap(code_ll.ctypes.data, code_d.ctypes.data, nbits))
    pieces = torch.full((cap,), SENTINEL, dtype=torch.uint8, device="cuda")
    sizes = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    hdr = np.frombuffer(header, np.uint8)

    def call(stream=ptr, n=n, table=tokens.data_ptr(), ll=code_ll, d=code_d, h=hdr.ctypes.data, nbits=nbits, out=pieces.data_ptr(), cap=cap, sz=sizes.data_ptr(),
             handle=True):
        return lib.radnet_deflate_lz_emit_u8(ctx.h if handle else None, stream, n, table, ll.ctypes.data if ll is not None else None,
                                             d.ctypes.data if d is not None else None, h, nbits, out, cap, sz)

    def edited(code, **fields):
        c = code.copy()
        for name, (s, v) in fields.items():
            c[name][s] = v
        return c

    for what, kw, code in (("null stream", dict(stream=None), ERR_ARG), ("null table", dict(table=None), ERR_ARG), ("null literal code", dict(ll=None), ERR_ARG),
                           ("null distance code", dict(d=None), ERR_ARG), ("null header", dict(h=None), ERR_ARG), ("null pieces", dict(out=None), ERR_ARG),
                           ("null sizes", dict(sz=None), ERR_ARG), ("n = 0", dict(n=0), ERR_ARG), ("a misaligned table", dict(table=tokens.data_ptr() + 8), ERR_ARG),
                           ("a literal length of 16", dict(ll=edited(code_ll, length=(65, 16))), ERR_ARG),
                           ("literal bits beyond the length", dict(ll=edited(code_ll, bits=(280, 0x8000))), ERR_ARG),
                           ("no end-of-block", dict(ll=edited(code_ll, length=(256, 0), bits=(256, 0))), ERR_ARG),
                           ("a distance length of 16", dict(d=edited(code_d, length=(2, 16))), ERR_ARG),
                           ("distance bits beyond the length", dict(d=edited(code_d, bits=(2, 0x8000))), ERR_ARG),
                           ("a short piece_cap", dict(cap=cap - 1), ERR_ARG), ("a header of 2 bits", dict(nbits=2), ERR_ARG),
                           ("a header of 2049 bits", dict(nbits=2049), ERR_ARG), ("n = 2^32", dict(n=1 << 32), ERR_UNSUPPORTED)):
        assert call(**kw) == code and last_error(ctx), what
    assert call(handle=False) == ERR_ARG
    ctx.sync()
    assert (pieces.cpu().numpy() == SENTINEL).all() and (sizes.cpu().numpy() == -1).all()
    assert call() == 0                                                                      # and the arguments they were derived from pass
    ctx.sync()
    size = int(sizes.cpu().numpy()[0])
    want = Z.pieces(want_toks, [int(v) for v in code_ll["length"]], [int(v) for v in code_d["length"]], header, nbits)
    assert bytes(pieces.cpu().numpy()[:size]) == want[0]


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def rgb_picture(h=200, w=300):
    """Smooth shading whose channels differ, a flat patch, a texture that repeats every 64 columns and every 8 rows: far matches."""
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([x // 3 + y // 4, x // 5 + (y // 3) * 2, (x // 2 + y // 7) * 3], axis=2) & 255
    rs = np.random.RandomState(9)
    img[h // 2:, :, :] = np.tile(rs.randint(0, 256, (8, 64, 3)), (h // 16 + 1, w // 64 + 1, 1))[:h - h // 2, :w]
    img[h // 8:h // 4, w // 3:] = (200, 90, 30)
    return img.astype(np.uint8)


def grey_picture(h=300, w=401):
    rs = np.random.RandomState(10)
    img = np.tile(rs.randint(0, 256, (6, 50)), (h // 6 + 1, w // 50 + 1))[:h, :w]
    img[:h // 3] = W.filter_input("ramp", h // 3, w, 1)[:, :, 0]
    return img.astype(np.uint8)


@pytest.mark.parametrize("name", ["300x401 grey", "200x300 rgb"])
def test_encode_device_lz_round_trips_and_is_never_longer(png, name):
    img = grey_picture() if name.endswith("grey") else rgb_picture()
    dev = torch.from_numpy(img).cuda()
    report = {}
    data = png.encode_device(dev, deflate="device-lz", report=report)
    rle_file, host_file = png.encode_device(dev, deflate="device"), png.encode_device(dev)
    assert isinstance(data, bytes) and len(data) <= len(rle_file), (len(data), len(rle_file))
    assert report["rule"] == "lz" and report["bits_lz"] + 7 < report["bits_rle"] and report["matches"] >= report["far_matches"] > 0, report
    want = img if img.ndim == 3 else np.repeat(img[:, :, None], 3, axis=2)
    back_host = png.decode_device(data, inflate="host")
    lz_report = {}
    back_device = png.decode_device(data, inflate="device-lz", report=lz_report)
    assert lz_report["path"] == "device", lz_report
    own = W.decode_bgr(data)
    assert back_host.is_cuda and torch.equal(back_host, torch.from_numpy(want).cuda()) and torch.equal(back_device, back_host) and np.array_equal(own, want)
    d = W.decode(data)
    assert d.kinds == [b"IHDR", b"IDAT", b"IEND"] and d.color_type == (2 if img.ndim == 3 else 0)
    assert d.stream == W.decode(host_file).stream                                           # exactly the filtered stream of the host path
    assert png.encode_device(dev, deflate="device-lz", crc="device") == data               # the sum made on the device: the same bytes
    assert png.encode_device(img, deflate="device-lz") == data                             # a NumPy input; deterministic
    # and the file is the model's: the IDAT payload byte for byte
    from radnet_hip import lib as L
    chunk, tile = L.header_constant("RADNET_DEFLATE_CHUNK"), L.header_constant("RADNET_DEFLATE_TILE")
    toks = Z.tokens(d.stream, chunk, tile, 3 if img.ndim == 3 else 1)
    code_ll, code_d, header, nbits = png.huffman_codes_lz(*Z.histograms(toks))
    body = b"".join(Z.pieces(toks, [int(v) for v in code_ll["length"]], [int(v) for v in code_d["length"]], header, nbits))
    idat = [p for k, p in W.chunks(data) if k == b"IDAT"][0]
    assert idat == b"\x78\x01" + body + zlib.adler32(d.stream).to_bytes(4, "big")
    assert (report["matches"], report["far_matches"]) == Z.counts(toks, 3 if img.ndim == 3 else 1)
    assert torch.equal(dev.cpu(), torch.from_numpy(img)), "the input was written"


def test_noise_takes_the_run_length_branch_and_equals_deflate_device(png):
    for shape in ((64, 97), (40, 50, 3)):
        img = np.random.RandomState(4).randint(0, 256, shape).astype(np.uint8)
        dev = torch.from_numpy(img).cuda()
        report = {}
        data = png.encode_device(dev, deflate="device-lz", report=report)
        assert report["rule"] == "rle" and report["bits_lz"] + 7 >= report["bits_rle"], report
        assert data == png.encode_device(dev, deflate="device")
        assert png.encode_device(dev, deflate="device-lz", crc="device") == data
        assert np.array_equal(W.decode_bgr(data), img if img.ndim == 3 else np.repeat(img[:, :, None], 3, axis=2))


def test_defaults_and_deflate_device_are_untouched_by_a_report(png):
    img = rgb_picture(40, 60)
    dev = torch.from_numpy(img).cuda()
    for kw in (dict(), dict(deflate="device"), dict(deflate="device", huffman="fixed")):
        report = {}
        assert png.encode_device(dev, report=report, **kw) == png.encode_device(dev, **kw) and report == {}


def test_imwrite_and_write_predictions_on_the_device(png, tmp_path):
    from faster_rcnn import RADNet as R
    from faster_rcnn import utils_io

    class _Config:
        class_mapping = {"boat": 0, "human": 1, "animal": 2, "bg": 3}

    img = rgb_picture(96, 128)
    dev = torch.from_numpy(img).cuda()
    path, report = tmp_path / "map.png", {}
    assert utils_io.imwrite(path, dev, deflate="device-lz", report=report) is True
    assert path.read_bytes() == png.encode_device(dev, deflate="device-lz") and np.array_equal(W.decode_bgr(path.read_bytes()), img)
    assert report["rule"] in ("lz", "rle") and set(report) == {"rule", "bits_lz", "bits_rle", "matches", "far_matches"}
    dets = [{'class': 'boat', 'prob': 0.9, 'x1': 10, 'y1': 20, 'x2': 70, 'y2': 60}, {'class': 'human', 'prob': 0.7, 'x1': 50, 'y1': 40, 'x2': 100, 'y2': 90}]
    net = R.RADNet(_Config(), None, None, None)
    rle = net.write_predictions(dets, dev, str(tmp_path / "rle"), deflate="device")
    lz = net.write_predictions(dets, dev, str(tmp_path / "lz"), deflate="device-lz", crc="device")
    for a, b in zip(rle[:4], lz[:4]):
        fa, fb = open(a, "rb").read(), open(b, "rb").read()
        assert W.decode(fa).stream == W.decode(fb).stream and len(fb) <= len(fa), a
        assert np.array_equal(W.decode_bgr(fb), png.decode_device(fb).cpu().numpy()), a
    assert open(rle[4]).read() == open(lz[4]).read()
    with pytest.raises(ValueError, match="fixed"):
        net.write_predictions(dets, dev, str(tmp_path / "bad"), deflate="device-lz", huffman="fixed")
