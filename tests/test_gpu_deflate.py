"""The device deflate against its Python model (tests/deflate_cases.py), byte for byte: radnet_deflate_rle_scan_u8's counts and Adler
parts, radnet_deflate_rle_emit_u8's pieces and sizes in a sentinel-filled buffer, radnet_deflate_pack's packed bytes and total --
for the dynamic code of radnet_deflate_build_code, the fixed code and a forced table with a 1-bit and a 15-bit code side by side;
what the entries refuse; png.encode_device(deflate="device") read back by png.decode_device and by the tests' own decoder, and the
defaults unchanged."""
import zlib

import numpy as np
import pytest

import deflate_cases as D
import png_cases as K
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
def streams(cut):
    return D.streams(*cut)


NAMES = sorted(D.streams(65536, 4096))                                 # the names do not depend on the cut
MISALIGNED = {"mixed tile+1": 1, "straddle": 3, "noise": 7, "panel": 13}      # the stream starts this far off a 16-byte boundary: the byte-wise tile load


def last_error(ctx):
    msg = ctx.lib.radnet_last_error(ctx.h)
    return msg.decode() if msg else ""


def upload(data, offset=0):
    """(buffer, pointer): the bytes on the device at `offset` of an allocation, sentinels round them."""
    buf = torch.full((offset + len(data) + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    buf[offset:offset + len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    return buf, buf.data_ptr() + offset


def scan(ctx, data, chunk, offset=0, hist=None):
    """(rc, hist [286], parts [chunks][2]) with the guards behind both checked."""
    chunks = -(-len(data) // chunk)
    buf, ptr = upload(data, offset)
    hist = torch.zeros(286 + 4, dtype=torch.int32, device="cuda") if hist is None else hist
    hist[286:] = -1
    parts = torch.full((2 * chunks + 2,), -1, dtype=torch.int64, device="cuda")
    rc = ctx.lib.radnet_deflate_rle_scan_u8(ctx.h, ptr, len(data), hist.data_ptr(), parts.data_ptr())
    ctx.sync()
    h, p = hist.cpu().numpy(), parts.cpu().numpy()
    assert (h[286:] == -1).all() and (p[2 * chunks:] == -1).all(), "written behind the histogram or the parts"
    assert bytes(buf.cpu().numpy()[offset:offset + len(data)]) == data, "the stream was written"
    return rc, h[:286].view(np.uint32), p[:2 * chunks].view(np.uint64).reshape(chunks, 2)


def emit(ctx, png, data, chunk, hc, offset=0, extra_cap=0):
    """(rc, [piece bytes], sizes, the piece buffer, piece_cap): every byte of the buffer behind a piece's size must be the sentinel."""
    chunks = -(-len(data) // chunk)
    cap = int(ctx.lib.radnet_deflate_piece_cap(hc.code.ctypes.data, hc.header_nbits, hc.dist_nbits)) + extra_cap
    buf, ptr = upload(data, offset)
    pieces = torch.full((chunks * cap + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    sizes = torch.full((chunks + 2,), -1, dtype=torch.int32, device="cuda")
    header = np.frombuffer(hc.header, np.uint8)
    rc = ctx.lib.radnet_deflate_rle_emit_u8(ctx.h, ptr, len(data), hc.code.ctypes.data, header.ctypes.data, hc.header_nbits, hc.dist_nbits,
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


def pack(ctx, pieces, cap, sizes, out_cap=None):
    """(rc, the packed bytes up to out_cap, total): behind min(total, out_cap) nothing may be written."""
    count, want = len(sizes), int(np.asarray(sizes, np.int64).sum())
    out_cap = want if out_cap is None else out_cap
    sizes_dev = torch.from_numpy(np.asarray(sizes, np.int32).copy()).cuda()
    out = torch.full((out_cap + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    total = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    rc = ctx.lib.radnet_deflate_pack(ctx.h, pieces.data_ptr(), cap, sizes_dev.data_ptr(), count, out.data_ptr(), out_cap, total.data_ptr())
    ctx.sync()
    got, t = out.cpu().numpy(), total.cpu().numpy()
    assert t[1] == -1 and (got[min(want, out_cap):] == SENTINEL).all(), "written behind the total or the packed bytes"
    return rc, bytes(got[:min(want, out_cap)]), int(t[0])


def model_pieces(data, cut, hc):
    lengths = [int(v) for v in hc.code["length"]]
    codes = [int(v) for v in hc.code["bits"]]
    return D.pieces(data, cut[0], cut[1], lengths, hc.header, hc.header_nbits, hc.dist_nbits, codes)


# ---- the three entries against the model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_scan_emit_and_pack_match_the_model(ctx, png, cut, streams, name):
    data, offset = streams[name], MISALIGNED.get(name, 0)
    rc, hist, parts = scan(ctx, data, cut[0], offset)
    assert rc == 0, last_error(ctx)
    assert np.array_equal(hist, D.histogram(data, *cut)), name
    assert parts.tolist() == D.adler_parts(data, cut[0]), name
    adler = png.adler32_of_parts(parts, len(data))
    assert adler == zlib.adler32(data)
    for mode, hc in (("dynamic", png.huffman_code(hist)), ("fixed", png.fixed_code())):
        want = model_pieces(data, cut, hc)
        rc, got, sizes, pieces, cap = emit(ctx, png, data, cut[0], hc, offset, extra_cap=1 if mode == "fixed" else 0)      # odd pieces too
        assert rc == 0, last_error(ctx)
        assert sizes.tolist() == [len(p) for p in want], (name, mode)
        for c, (g, w) in enumerate(zip(got, want)):
            assert g == w, (name, mode, "piece %d differs first at byte %d" % (c, next(i for i in range(len(w)) if g[i] != w[i])))
        rc, packed, total = pack(ctx, pieces, cap, sizes)
        assert rc == 0 and total == len(packed) and packed == b"".join(want), (name, mode)
        out, eof, unused = D.inflate(b"\x78\x01" + packed + adler.to_bytes(4, "big"))
        assert out == data and eof and unused == b"", (name, mode)


def test_scan_adds_to_the_histogram_it_is_given(ctx, cut, streams):
    data = streams["runs"]
    hist = torch.zeros(286 + 4, dtype=torch.int32, device="cuda")
    for times in (1, 2):
        rc, got, _ = scan(ctx, data, cut[0], hist=hist)
        assert rc == 0 and np.array_equal(got, times * D.histogram(data, *cut))


def forced_table(png):
    """A complete code with lengths 1, 2, ..., 14, 15, 15: literal 0 in one bit beside the literals 255 and 1 in fifteen, the match
    lengths 3..16 and 258, end-of-block."""
    symbols = [0, 285, 257, 258, 259, 260, 261, 262, 263, 264, 265, 266, 267, 256, 255, 1]
    lengths = [0] * 286
    for s, n in zip(symbols, list(range(1, 16)) + [15]):
        lengths[s] = n
    assert D.kraft(lengths) == 1 << 15
    code = np.zeros(286, png.DEFLATE_CODE)
    code["length"], code["bits"] = lengths, D.canonical_codes(lengths)
    header, nbits = D.dynamic_header(lengths)
    return png.HuffmanCode(code, header, nbits, 1)


def forced_stream(chunk, tile):
    """Blocks of 512 bytes (so that no run crosses a tile) that use only what the forced table codes: 0 / 255 alternating -- 1 and 15
    bits, a word boundary crossed at every offset --, zero runs whose rests are 3..16 or 258, the literal 1."""
    block = bytes([0, 255]) * 40 + bytes(259) + b"\xff" + bytes(17) + b"\xff" + bytes(4) + b"\xff\x01\xff" + bytes(7) + b"\xff\x01" + bytes([0, 255]) * 69
    assert len(block) == 512 and tile % 512 == 0
    return block * ((chunk + 2 * tile) // 512) + bytes([0, 255, 0, 255, 1])


def test_a_forced_table_with_a_one_bit_and_a_fifteen_bit_code(ctx, png, cut):
    hc, data = forced_table(png), forced_stream(*cut)
    hist = D.histogram(data, *cut)
    assert all(hc.code["length"][s] for s in range(286) if hist[s]) and hist[0] and hist[255] and hist[1] and hist[285] and hist[267]
    want = model_pieces(data, cut, hc)
    assert len(want) == 2 and len(want[0]) > cut[0] // 4                                       # thousands of words, sixteen tiles
    for offset in (0, 5):
        rc, got, sizes, pieces, cap = emit(ctx, png, data, cut[0], hc, offset)
        assert rc == 0, last_error(ctx)
        assert sizes.tolist() == [len(p) for p in want] and got == want
    rc, packed, total = pack(ctx, pieces, cap, sizes)
    assert rc == 0 and packed == b"".join(want) and total == len(packed)
    out, eof, unused = D.inflate(b"\x78\x01" + packed + zlib.adler32(data).to_bytes(4, "big"))      # the table is legal: zlib reads it
    assert out == data and eof and unused == b""


def test_pack_cuts_at_the_capacity_and_still_reports_the_total(ctx, png, cut, streams):
    data = streams["mixed 2chunk+3"]
    hc = png.fixed_code()
    rc, got, sizes, pieces, cap = emit(ctx, png, data, cut[0], hc)
    whole = b"".join(got)
    for out_cap in (len(whole) - 1, len(got[0]) + 5, len(got[0]), 3, 0):
        rc, packed, total = pack(ctx, pieces, cap, sizes, out_cap)
        assert rc == 0 and total == len(whole) and packed == whole[:out_cap], out_cap


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_leave_the_buffers_untouched(ctx, png, cut):
    lib, data = ctx.lib, bytes(range(200)) * 3
    n = len(data)
    buf, ptr = upload(data)
    hist = torch.full((286,), 7, dtype=torch.int32, device="cuda")
    parts = torch.full((2,), 7, dtype=torch.int64, device="cuda")
    for what, args, code in (("null stream", (None, n, hist.data_ptr(), parts.data_ptr()), ERR_ARG), ("null histogram", (ptr, n, None, parts.data_ptr()), ERR_ARG),
                             ("null parts", (ptr, n, hist.data_ptr(), None), ERR_ARG), ("n = 0", (ptr, 0, hist.data_ptr(), parts.data_ptr()), ERR_ARG),
                             ("n < 0", (ptr, -5, hist.data_ptr(), parts.data_ptr()), ERR_ARG),
                             ("n = 2^32", (ptr, 1 << 32, hist.data_ptr(), parts.data_ptr()), ERR_UNSUPPORTED)):
        assert lib.radnet_deflate_rle_scan_u8(ctx.h, *args) == code and last_error(ctx), what
    assert lib.radnet_deflate_rle_scan_u8(None, ptr, n, hist.data_ptr(), parts.data_ptr()) == ERR_ARG
    ctx.sync()
    assert (hist.cpu().numpy() == 7).all() and (parts.cpu().numpy() == 7).all()

    good = png.fixed_code()
    cap = int(lib.radnet_deflate_piece_cap(good.code.ctypes.data, 3, 5))
    pieces = torch.full((cap,), SENTINEL, dtype=torch.uint8, device="cuda")
    sizes = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    header = np.frombuffer(good.header, np.uint8)

    def call(stream=ptr, n=n, code=good.code, hdr=header.ctypes.data, nbits=3, dist=5, out=pieces.data_ptr(), cap=cap, sz=sizes.data_ptr(), handle=True):
        return lib.radnet_deflate_rle_emit_u8(ctx.h if handle else None, stream, n, code.ctypes.data if code is not None else None, hdr, nbits, dist, out, cap, sz)

    def edited(**fields):
        c = good.code.copy()
        for name, (s, v) in fields.items():
            c[name][s] = v
        return c

    for what, kw, code in (("null stream", dict(stream=None), ERR_ARG), ("null code", dict(code=None), ERR_ARG), ("null header", dict(hdr=None), ERR_ARG),
                           ("null pieces", dict(out=None), ERR_ARG), ("null sizes", dict(sz=None), ERR_ARG), ("n = 0", dict(n=0), ERR_ARG),
                           ("a length of 16", dict(code=edited(length=(65, 16))), ERR_ARG), ("bits beyond the length", dict(code=edited(bits=(280, 0x100))), ERR_ARG),
                           ("no end-of-block", dict(code=edited(length=(256, 0), bits=(256, 0))), ERR_ARG), ("a short piece_cap", dict(cap=cap - 1), ERR_ARG),
                           ("a header of 2 bits", dict(nbits=2), ERR_ARG), ("a header of 2049 bits", dict(nbits=2049), ERR_ARG),
                           ("a distance code of 16 bits", dict(dist=16), ERR_ARG), ("a negative distance code", dict(dist=-1), ERR_ARG),
                           ("n = 2^32", dict(n=1 << 32), ERR_UNSUPPORTED)):
        assert call(**kw) == code and last_error(ctx), what
    assert call(handle=False) == ERR_ARG
    ctx.sync()
    assert (pieces.cpu().numpy() == SENTINEL).all() and (sizes.cpu().numpy() == -1).all()
    assert call() == 0                                                                      # and the arguments they were derived from pass
    ctx.sync()
    size = int(sizes.cpu().numpy()[0])
    assert bytes(pieces.cpu().numpy()[:size]) == model_pieces(data, cut, good)[0]

    out = torch.full((64,), SENTINEL, dtype=torch.uint8, device="cuda")
    total = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    one = torch.tensor([size], dtype=torch.int32, device="cuda")
    for what, args, code in (("null pieces", (None, cap, one.data_ptr(), 1, out.data_ptr(), 64, total.data_ptr()), ERR_ARG),
                             ("null sizes", (pieces.data_ptr(), cap, None, 1, out.data_ptr(), 64, total.data_ptr()), ERR_ARG),
                             ("null output", (pieces.data_ptr(), cap, one.data_ptr(), 1, None, 64, total.data_ptr()), ERR_ARG),
                             ("null total", (pieces.data_ptr(), cap, one.data_ptr(), 1, out.data_ptr(), 64, None), ERR_ARG),
                             ("no pieces", (pieces.data_ptr(), cap, one.data_ptr(), 0, out.data_ptr(), 64, total.data_ptr()), ERR_ARG),
                             ("piece_cap 0", (pieces.data_ptr(), 0, one.data_ptr(), 1, out.data_ptr(), 64, total.data_ptr()), ERR_ARG),
                             ("a negative capacity", (pieces.data_ptr(), cap, one.data_ptr(), 1, out.data_ptr(), -1, total.data_ptr()), ERR_ARG),
                             ("65537 pieces", (pieces.data_ptr(), cap, one.data_ptr(), 65537, out.data_ptr(), 64, total.data_ptr()), ERR_UNSUPPORTED)):
        assert lib.radnet_deflate_pack(ctx.h, *args) == code and last_error(ctx), what
    assert lib.radnet_deflate_pack(None, pieces.data_ptr(), cap, one.data_ptr(), 1, out.data_ptr(), 64, total.data_ptr()) == ERR_ARG
    ctx.sync()
    assert (out.cpu().numpy() == SENTINEL).all() and total.cpu().numpy()[0] == -1


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pictures():
    return {"1x1 grey": W.filter_input("noise", 1, 1, 1)[:, :, 0], "1x7 grey": W.filter_input("ramp", 1, 7, 1)[:, :, 0],
            "5x3 rgb": W.filter_input("noise", 5, 3, 3), "300x401 grey": W.filter_input("ramp", 300, 401, 1)[:, :, 0],
            "300x401 rgb": W.filter_input("ramp", 300, 401, 3)}


@pytest.mark.parametrize("huffman", ["dynamic", "fixed"])
def test_encode_device_on_the_device_round_trips(png, pictures, cut, huffman):
    for name, img in pictures.items():
        dev = torch.from_numpy(img).cuda()
        host_file = png.encode_device(dev)
        data = png.encode_device(dev, deflate="device", huffman=huffman)
        assert isinstance(data, bytes), name                                                    # (a tiny image's fixed-code file can equal zlib's)
        want = img if img.ndim == 3 else np.repeat(img[:, :, None], 3, axis=2)
        back = png.decode_device(data)
        assert back.is_cuda and torch.equal(back, torch.from_numpy(want).cuda()), name
        assert np.array_equal(W.decode_bgr(data), want), name
        d = W.decode(data)
        assert d.kinds == [b"IHDR", b"IDAT", b"IEND"] and d.color_type == (2 if img.ndim == 3 else 0)
        assert d.stream == W.decode(host_file).stream, name                                   # exactly the stream the host path deflates
        # and the file is the model's: the IDAT payload byte for byte
        idat = [p for k, p in W.chunks(data) if k == b"IDAT"][0]
        lengths = None if huffman == "fixed" else [int(v) for v in png.huffman_code(D.histogram(d.stream, *cut)).code["length"]]
        assert idat == D.zlib_stream(d.stream, cut[0], cut[1], huffman, lengths=lengths), name
        assert png.encode_device(img, deflate="device", huffman=huffman) == data              # a NumPy input; deterministic
        assert torch.equal(dev.cpu(), torch.from_numpy(img)), "the input was written"


def test_encode_device_defaults_are_the_host_path_of_before(png, pictures, ctx):
    for name, img in pictures.items():
        dev = torch.from_numpy(img).cuda()
        h, w = img.shape[:2]
        channels = 1 if img.ndim == 2 else 3
        stream = torch.empty(h * (1 + w * channels), dtype=torch.uint8, device="cuda")
        ctx.call("radnet_png_filter_rows_u8", dev, h, w, channels, w * channels, 5, stream)
        ctx.sync()
        want = png.assemble(stream.cpu().numpy(), w, h, 2 if channels == 3 else 0)
        assert png.encode_device(dev) == want == png.encode_device(dev, deflate="host", huffman="dynamic"), name
        lines, _ = K.filter_rows(W.stream_rows(img), channels, "adaptive")
        assert want == png.assemble(lines.tobytes(), w, h, 2 if channels == 3 else 0), name


def test_imwrite_and_write_predictions_on_the_device(png, tmp_path):
    from faster_rcnn import RADNet as R
    from faster_rcnn import utils_io

    class _Config:
        class_mapping = {"boat": 0, "human": 1, "animal": 2, "bg": 3}

    img = W.filter_input("ramp", 96, 128, 3)
    dev = torch.from_numpy(img).cuda()
    path = tmp_path / "map.png"
    assert utils_io.imwrite(path, dev, deflate="device") is True
    assert path.read_bytes() == png.encode_device(dev, deflate="device") and np.array_equal(W.decode_bgr(path.read_bytes()), img)
    dets = [{'class': 'boat', 'prob': 0.9, 'x1': 10, 'y1': 20, 'x2': 70, 'y2': 60}, {'class': 'human', 'prob': 0.7, 'x1': 50, 'y1': 40, 'x2': 100, 'y2': 90}]
    net = R.RADNet(_Config(), None, None, None)
    host = net.write_predictions(dets, dev, str(tmp_path / "host"))
    device = net.write_predictions(dets, dev, str(tmp_path / "device"), deflate="device", huffman="fixed")
    for a, b in zip(host[:4], device[:4]):
        fa, fb = open(a, "rb").read(), open(b, "rb").read()
        assert W.decode(fa).stream == W.decode(fb).stream and np.array_equal(W.decode_bgr(fb), png.decode_device(fb).cpu().numpy()), a
    assert open(host[4]).read() == open(device[4]).read()
