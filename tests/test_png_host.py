"""The host half of the PNG reader (faster_rcnn/png.py: container, CRC, inflate, pass geometry, errors) against the independent
encoder of tests/png_cases.py, and faster_rcnn/utils_io.py (get_image pinned by the reference's own function through
tests/golden/get_image.json, predict_from_path through fake models, DeviceImageLoader's LRU accounting).  No device needed."""
import json
import os
import struct
import zlib

import numpy as np
import pytest

import png_cases as K
from conftest import GOLDEN
from faster_rcnn import png, utils_io

SIZES = [(1, 1), (2, 3), (5, 5), (8, 8), (9, 9), (17, 3)]      # width, height


def _samples(w, h, color_type, depth, seed=0):
    return K.draw(np.random.RandomState(seed), h, w, color_type, depth)


def _palette(n, seed=1):
    return np.random.RandomState(seed).randint(0, 256, size=(n, 3)).astype(np.uint8)


@pytest.mark.parametrize("color_type,depth", K.LEGAL)
@pytest.mark.parametrize("interlace", [False, True])
def test_header_and_parse_on_every_legal_format(color_type, depth, interlace, tmp_path):
    w, h = 13, 7
    pal = _palette(1 << min(depth, 8)) if color_type == 3 else None
    enc = K.encode(_samples(w, h, color_type, depth), color_type, depth, filters=np.random.RandomState(3), interlace=interlace, palette=pal)
    want = (w, h, depth, color_type, 1 if interlace else 0)
    assert tuple(png.read_header(enc.data)) == want
    assert tuple(png.read_header(enc.data[:33])) == want                 # the first 33 bytes are all it reads
    path = tmp_path / "x.png"
    path.write_bytes(enc.data)
    assert tuple(png.read_header(str(path))) == want and tuple(png.read_header(path)) == want
    img = png.parse(enc.data)
    assert tuple(img.header) == want
    assert isinstance(img.stream, bytes) and img.stream == enc.stream
    assert [tuple(p) for p in img.passes] == enc.passes
    assert img.bpp == max(1, K.CHANNELS[color_type] * depth // 8)
    assert img.palette.shape == (256, 3) and img.palette.dtype == np.uint8


@pytest.mark.parametrize("w,h", SIZES)
def test_pass_geometry(w, h):
    one = png.parse(K.encode(_samples(w, h, 2, 8), 2, 8).data)
    assert [tuple(p) for p in one.passes] == [(0, 0, 1, 1, w, h, 3 * w, 0)]
    for color_type, depth in ((2, 8), (3, 4), (0, 16), (0, 1)):
        pal = _palette(16) if color_type == 3 else None
        enc = K.encode(_samples(w, h, color_type, depth), color_type, depth, filters=4, interlace=True, palette=pal)
        img = png.parse(enc.data)
        bits = K.CHANNELS[color_type] * depth
        want, offset = [], 0
        for x0, y0, dx, dy in K.ADAM7:                                   # restated here: ceil((W - x0) / dx) x ceil((H - y0) / dy)
            pw = len(range(x0, w, dx))
            ph = len(range(y0, h, dy))
            if pw == 0 or ph == 0:
                continue                                                 # an empty pass occupies no bytes
            rowbytes = (pw * bits + 7) // 8
            want.append((x0, y0, dx, dy, pw, ph, rowbytes, offset))
            offset += ph * (1 + rowbytes)
        assert [tuple(p) for p in img.passes] == want == enc.passes
        assert len(img.stream) == offset == len(enc.stream)
        assert sum(p.pass_w * p.pass_h for p in img.passes) == w * h
    n_passes = {(1, 1): 1, (2, 3): 4, (5, 5): 7, (8, 8): 7, (9, 9): 7, (17, 3): 6}[(w, h)]
    assert len(png.parse(K.encode(_samples(w, h, 2, 8), 2, 8, interlace=True).data).passes) == n_passes


def test_palette_padding_and_bgr_order():
    pal = np.array([[1, 2, 3], [10, 20, 30], [255, 0, 128]], np.uint8)      # R, G, B in the file
    img = png.parse(K.encode(np.zeros((2, 2, 1), np.int64), 3, 2, palette=pal).data)
    assert np.array_equal(img.palette[:3], pal[:, ::-1])
    assert not img.palette[3:].any()
    rgb = png.parse(K.encode(_samples(3, 3, 2, 8), 2, 8, palette=pal).data)      # PLTE on a truecolour file: a suggestion, kept out of the pixels
    assert np.array_equal(rgb.palette[:3], pal[:, ::-1])
    assert not png.parse(K.encode(_samples(3, 3, 2, 8), 2, 8).data).palette.any()


def _file(parts):
    return K.SIGNATURE + b"".join(parts)


def test_errors_name_their_cause():
    good = K.encode(_samples(6, 5, 2, 8), 2, 8, filters=np.random.RandomState(0))
    png.parse(good.data)
    png.parse(good.data + b"trailing bytes after IEND are ignored")

    with pytest.raises(ValueError, match="signature"):
        png.parse(b"\x89PNX" + good.data[4:])
    with pytest.raises(ValueError, match="signature"):
        png.read_header(b"GIF89a" + good.data[6:])

    at = good.data.index(b"IDAT") + 4 + 3                                # one bit of the IDAT payload
    flipped = bytearray(good.data)
    flipped[at] ^= 0x10
    with pytest.raises(ValueError, match="CRC"):
        png.parse(bytes(flipped))
    broken_ihdr = bytearray(good.data)
    broken_ihdr[20] ^= 1                                                 # inside the IHDR payload
    with pytest.raises(ValueError, match="CRC"):
        png.read_header(bytes(broken_ihdr))

    z = zlib.compress(good.stream)
    with pytest.raises(ValueError, match="IHDR"):
        png.parse(_file([K.chunk(b"IDAT", z), K.chunk(b"IEND")]))
    with pytest.raises(ValueError, match="IHDR"):
        png.parse(_file([K.chunk(b"gAMA", struct.pack(">I", 45455)), K.ihdr(6, 5, 8, 2), K.chunk(b"IDAT", z), K.chunk(b"IEND")]))

    for color_type, depth in ((2, 4), (3, 16), (4, 2), (6, 1), (0, 3), (1, 8), (5, 8), (7, 8)):
        with pytest.raises(ValueError, match="colour type"):
            png.parse(_file([K.ihdr(6, 5, depth, color_type), K.chunk(b"IDAT", z), K.chunk(b"IEND")]))
        with pytest.raises(ValueError, match="colour type"):
            png.read_header(_file([K.ihdr(6, 5, depth, color_type)]))

    idx = K.encode(np.zeros((5, 6, 1), np.int64), 3, 8, palette=_palette(4))
    no_plte = idx.data[:33] + idx.data[idx.data.index(b"IDAT") - 4:]
    with pytest.raises(ValueError, match="(?i)palette"):
        png.parse(no_plte)

    with pytest.raises(ValueError, match="truncated"):
        png.parse(_file([K.ihdr(6, 5, 8, 2), K.chunk(b"IDAT", zlib.compress(good.stream[:-1])), K.chunk(b"IEND")]))
    with pytest.raises(ValueError, match="truncated"):
        png.parse(_file([K.ihdr(6, 5, 8, 2), K.chunk(b"IDAT", z[:len(z) // 2]), K.chunk(b"IEND")]))      # the zlib stream itself cut short
    with pytest.raises(ValueError, match="over-long"):
        png.parse(_file([K.ihdr(6, 5, 8, 2), K.chunk(b"IDAT", zlib.compress(good.stream + b"\0")), K.chunk(b"IEND")]))
    with pytest.raises(ValueError, match="truncated"):
        png.parse(good.data[:-12])                                       # no IEND
    with pytest.raises(ValueError, match="truncated"):
        png.parse(good.data[:len(good.data) // 2])

    for row in (0, 2, 4):
        bad = bytearray(good.stream)
        bad[row * (1 + 18)] = 5
        with pytest.raises(ValueError, match="filter type"):
            png.parse(_file([K.ihdr(6, 5, 8, 2), K.chunk(b"IDAT", zlib.compress(bytes(bad))), K.chunk(b"IEND")]))
    lace = K.encode(_samples(9, 9, 0, 8), 0, 8, interlace=True)
    bad = bytearray(lace.stream)
    bad[lace.passes[-1][-1]] = 200                                       # first filter byte of the last pass
    with pytest.raises(ValueError, match="filter type"):
        png.parse(_file([K.ihdr(9, 9, 8, 0, interlace=1), K.chunk(b"IDAT", zlib.compress(bytes(bad))), K.chunk(b"IEND")]))


def test_idat_chunks_are_concatenated_and_ancillary_chunks_skipped():
    s = _samples(11, 4, 6, 8)
    whole = K.encode(s, 6, 8, filters=3)
    split = K.encode(s, 6, 8, filters=3, idat_sizes=[1, 1, 5, 0, 7], trns=None,
                     extra=[K.chunk(b"gAMA", struct.pack(">I", 45455)), K.chunk(b"tEXt", b"Comment\0made by a test")])
    assert split.data.count(b"IDAT") == 6
    assert png.parse(split.data).stream == png.parse(whole.data).stream == whole.stream


# ---- utils_io ------------------------------------------------------------------------------------------------------------------

def test_get_image_follows_the_reference(monkeypatch):
    with open(os.path.join(GOLDEN, "get_image.json")) as f:
        cases = json.load(f)["cases"]
    assert len(cases) >= 12
    opened = []
    monkeypatch.setattr(np, "fromfile", lambda path, dtype=None: opened.append(path) or np.zeros(1, np.uint8))
    monkeypatch.setattr(png, "imdecode_color", lambda buf: "host image")
    monkeypatch.setattr(png, "decode_device", lambda buf: "device image")
    for c in cases:
        for to_host in (True, False):
            # NumPy's global stream, the default, as the reference draws; and a private RandomState at the same position
            np.random.seed(c["seed"])
            got = utils_io.get_image(c["img_path"], list(c["types"]), random_type=c["random_type"], to_host=to_host)
            assert got == ("host image" if to_host else "device image")
            assert opened.pop() == c["opened"], c
            assert np.random.random() == c["next_uniform"], c
            rs = np.random.RandomState(c["seed"])
            utils_io.get_image(c["img_path"], list(c["types"]), c["random_type"], rng=rs)
            assert opened.pop() == c["opened"] and rs.random_sample() == c["next_uniform"], c
    assert {c["random_type"] for c in cases} == {True, False} and {len(c["types"]) for c in cases} == {2, 3, 5}
    assert any(c["img_path"].startswith("/") for c in cases) and any(c["img_path"].count("/") > 1 for c in cases)


def test_image_size_and_load_image(tmp_path, monkeypatch):
    os.makedirs(tmp_path / "depth")
    enc = K.encode(_samples(31, 9, 0, 4), 0, 4)
    (tmp_path / "depth" / "a.png").write_bytes(enc.data)
    assert utils_io.image_size(str(tmp_path / "depth" / "a.png")) == (31, 9)
    seen = []
    monkeypatch.setattr(png, "imdecode_color", lambda buf: seen.append(bytes(buf)) or "decoded")
    monkeypatch.chdir(tmp_path.parent)
    rel = tmp_path.name + "/a.png"                                        # the type becomes path component 1
    assert utils_io.load_image({"filepath": rel}, "depth") == "decoded"
    assert seen == [enc.data]


def test_predict_from_path_equals_predict_on_the_same_arrays(monkeypatch):
    from faster_rcnn import rpn
    from faster_rcnn.config import Config
    from faster_rcnn.RADNet import RADNet
    from oracle import glue
    from test_oracle_glue import fake_detector

    class FakeDet:
        def __init__(self):
            self._f = fake_detector(7, 2, [])

        def predict(self, inputs):
            return self._f(inputs[1])

    class FakeRPN:
        def predict(self, X):
            h, w = glue.resnet50_feat_len(X.shape[1]), glue.resnet50_feat_len(X.shape[2])
            rs = np.random.RandomState(8 + int(abs(float(X.sum()))) % 1000)
            n = h * w * 12
            cls = (rs.permutation(n).astype(np.float32) / np.float32(n)).reshape(1, h, w, 12)
            return [cls, (rs.standard_normal((1, h, w, 48)) * 2.0).astype(np.float32), rs.standard_normal((1, h, w, 8)).astype(np.float32)]

    # the two device calls of predict's host path, restated by the oracle, and a seeded array per file in place of the decoder
    monkeypatch.setattr(rpn, "rpn_to_roi", lambda Y1, Y2, Cc, overlap_thresh=0.7: glue.rpn_to_roi(Y1, Y2, Cc, True, 300, overlap_thresh))
    monkeypatch.setattr(rpn, "non_max_suppression_fast", lambda b, p, overlap_thresh=0.9, max_boxes=300: glue.greedy_nms(b, p, overlap_thresh, max_boxes))
    opened = []
    monkeypatch.setattr(np, "fromfile", lambda path, dtype=None: opened.append(path) or np.frombuffer(path.encode(), np.uint8))

    def decoded(buf):
        return np.random.RandomState(zlib.crc32(bytes(buf))).randint(0, 256, (240, 240, 3)).astype(np.uint8)

    monkeypatch.setattr(png, "imdecode_color", decoded)
    Cc = Config()
    Cc.img_size, Cc.tile_size, Cc.tile_overlap = 160, 160, 80            # tiles arrive at network size: no resize
    Cc.img_types = ["blended_grey", "depth"]
    net = RADNet(Cc, FakeRPN(), FakeDet(), lambda x: x - np.float32(100.0))
    for use_img_type, types in ((False, ["blended_grey"]), (True, ["blended_grey", "depth"])):
        Cc.use_img_type = use_img_type
        del opened[:]
        got = net.predict_from_path("maps/panel.png")
        assert opened == ["maps/%s/panel.png" % t for t in types]
        want = net.predict([decoded(("maps/%s/panel.png" % t).encode()) for t in types])
        assert len(got) > 0 and got == want


def test_device_image_loader_lru_accounting(tmp_path, monkeypatch):
    os.makedirs(tmp_path / "d" / "t")
    sizes = {"a": 100, "b": 60, "c": 50, "big": 500}
    for name in sizes:
        (tmp_path / "d" / "t" / (name + ".png")).write_bytes(name.encode())
    decodes = []

    def decode(buf):
        name = bytes(buf).decode()
        decodes.append(name)
        return np.zeros((sizes[name], 1, 1), np.uint8)

    def entry(name):
        return {"filepath": "d/" + name + ".png"}                          # read as d/<type>/<name>.png

    def rel_loader(**kw):
        return utils_io.DeviceImageLoader(decode=decode, **kw)

    monkeypatch.chdir(tmp_path)
    if True:
        ld = rel_loader(cache_bytes=200)
        a = ld(entry("a"), "t")
        assert (ld.hits, ld.misses, ld.used) == (0, 1, 100)
        assert ld(entry("a"), "t") is a and (ld.hits, ld.misses) == (1, 1)
        ld(entry("b"), "t")
        assert ld.used == 160
        ld(entry("a"), "t")                                              # a is now the most recently used
        ld(entry("c"), "t")                                              # 210 > 200: b, the least recently used, goes
        assert ld.used == 150 and (ld.hits, ld.misses) == (2, 3)
        assert ld(entry("a"), "t") is a and ld.hits == 3
        ld(entry("b"), "t")                                              # decoded again; c goes (a was touched after it)
        assert (ld.hits, ld.misses, ld.used) == (3, 4, 160)
        ld(entry("big"), "t")                                            # larger than the bound: decoded, not kept, nothing evicted
        assert (ld.misses, ld.used) == (5, 160)
        ld(entry("big"), "t")
        assert (ld.hits, ld.misses) == (3, 6)
        assert decodes == ["a", "b", "c", "b", "big", "big"]
        # a rewritten file is another key: size and mtime are part of it
        path = tmp_path / "d" / "t" / "a.png"
        path.write_bytes(b"c")
        os.utime(path, ns=(1, 1))
        assert ld(entry("a"), "t").shape[0] == 50 and ld.misses == 7
        # the type is part of the key; cache_bytes=0 keeps nothing
        off = rel_loader(cache_bytes=0)
        off(entry("b"), "t")
        off(entry("b"), "t")
        assert (off.hits, off.misses, off.used) == (0, 2, 0)
