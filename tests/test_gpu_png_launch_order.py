"""Which entries a PNG decode launches, and in which order: png.decode_device and png.decode_device_many are handed a context that
writes down the name of every call and forwards it, and the names are compared with lists written out here from the documented
rules (the docstrings of both, include/radnet_hip.h on segments) -- never taken from the code under test.  Every case also checks
the decoded image against the NumPy statement of tests/png_cases.py, and the device-inflate cases that the device took the file
(a pass through the fallback would record another list).  Public API only.
The files: P, 100 rows of Paeth; I, Adam7 with 7 passes; S, a run-length stream whose segments spread the pass; L, one of Up rows alone
(one segment); S2, segments of both kinds; Z, level 6 with far matches; a batch of P, a 1-bit grey file and I."""
import numpy as np
import pytest

import png_cases as K

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

UNFILTER, SEGMENTS, TILES, EXPAND = "radnet_png_unfilter_u8", "radnet_png_unfilter_segments_u8", "radnet_png_unfilter_tiles_u8", "radnet_png_expand_bgr_u8"
CRC = "radnet_crc32_segments"
CHECKED = ["radnet_deflate_rle_scan_u8", "radnet_png_gather_column_u8"]      # the Adler-32 parts, the filter-type column
INFLATE_RLE = ["radnet_inflate_find_blocks", "radnet_inflate_rle_measure", "radnet_inflate_rle_emit"] + CHECKED
LZ_HEAD, LZ_RESOLVE, LZ_GATHER = ["radnet_inflate_find_blocks", "radnet_inflate_lz_measure", "radnet_inflate_lz_emit"], "radnet_inflate_lz_resolve", "radnet_inflate_lz_gather"


class Recorder:
    """A context as decode_device takes one: call() notes the entry's name and forwards to the real context."""

    def __init__(self, ctx):
        self.ctx, self.names = ctx, []

    def call(self, name, *args):
        self.names.append(name)
        return self.ctx.call(name, *args)


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


File = type("File", (), {})


def _file(data, samples, color=2, depth=8):
    f = File()
    f.data, f.want = data, K.expand(samples, color, depth)
    return f


def run_length_file(png, samples, types):
    """An RGB8 file whose rows have the filter types `types`, filtered here and deflated as a run-length stream by png.assemble."""
    h, w = samples.shape[:2]
    lines, _ = K.filter_rows(samples.reshape(h, w * 3).astype(np.uint8), 3, types)
    return _file(png.assemble(lines.tobytes(), w, h, 2), samples)


@pytest.fixture(scope="module")
def files(png):
    rs = np.random.RandomState(61)
    out = {}
    samples = K.draw(rs, 100, 40, 2, 8)
    out["P"] = _file(K.encode(samples, 2, 8, filters=4).data, samples)
    samples = K.draw(rs, 33, 33, 2, 8)
    out["I"] = _file(K.encode(samples, 2, 8, filters="adaptive", interlace=True).data, samples)
    samples = K.draw(rs, 200, 40, 2, 8)
    rows = np.arange(200)
    out["S"] = run_length_file(png, samples, np.where(rows % 20 == 0, 0, np.where(rows % 10 == 0, 1, 2)))
    out["L"] = run_length_file(png, samples, 2)
    out["S2"] = run_length_file(png, samples, np.where(np.isin(rows, (0, 30, 130)), 0, 2))
    samples = np.tile(K.draw(rs, 8, 8, 2, 8), (8, 8, 1))
    out["Z"] = _file(K.encode(samples, 2, 8, filters=0, level=6).data, samples)
    samples = K.draw(rs, 70, 45, 0, 1)
    out["G"] = _file(K.encode(samples, 0, 1, filters=2).data, samples, 0, 1)
    return out


def segment_rows(png, f):
    return png.plan_segments(png.parse(f.data))["rows"].tolist()


def decode(png, ctx, f, **kw):
    """(the recorded names, the report) of one decode_device whose image is the expected one."""
    rec, report = Recorder(ctx), {}
    got = png.decode_device(f.data, ctx=rec, report=report, **kw)
    assert np.array_equal(got.cpu().numpy(), f.want), kw
    if kw.get("inflate", "host") != "host":
        assert report["path"] == "device" and report["reason"] is None, (kw, report)
    return rec.names, report


def test_the_files_are_what_the_cases_need(png, files):
    assert len(png.parse(files["I"].data).passes) == 7
    assert segment_rows(png, files["P"]) == [100] and segment_rows(png, files["L"]) == [200] and segment_rows(png, files["G"]) == [70]
    assert segment_rows(png, files["S"]) == [60, 60, 60, 20]             # cuts every 10 rows, 64 rows at most: they spread the pass
    assert segment_rows(png, files["S2"]) == [30, 100, 70]              # one of at most 64 rows, two above; the longest is half the pass
    assert segment_rows(png, files["Z"]) == [64]                        # the whole pass in one segment: not spread
    assert max(segment_rows(png, files["I"])) <= 17


def test_the_host_path_one_pass(png, ctx, files):
    names, report = decode(png, ctx, files["P"])
    assert names == [UNFILTER, EXPAND] and report["path"] == "host" and report["reconstruction"] is None
    names, report = decode(png, ctx, files["P"], unfilter="tiles")
    assert names == [TILES, EXPAND] and report["reconstruction"] == "tiles"


def test_the_host_path_interlaced(png, ctx, files):
    names, _ = decode(png, ctx, files["I"])
    assert names == [UNFILTER, EXPAND] * 7                               # interleaved, pass by pass
    names, report = decode(png, ctx, files["I"], unfilter="tiles")
    assert names == [TILES] + [EXPAND] * 7 and report["reconstruction"] == "tiles"      # ONE call carries all passes, however short


def test_device_inflate_with_segments_that_spread_the_pass(png, ctx, files):
    names, report = decode(png, ctx, files["S"], inflate="device")
    assert names == INFLATE_RLE + [SEGMENTS, EXPAND] and report["reconstruction"] == "segments"
    names, report = decode(png, ctx, files["S"], inflate="device", crc="device")
    assert names == [CRC] + INFLATE_RLE + [SEGMENTS, EXPAND] and report["crc"] == "device" and report["reconstruction"] == "segments"


def test_device_inflate_with_one_segment_per_pass(png, ctx, files):
    names, report = decode(png, ctx, files["L"], inflate="device")
    assert names == INFLATE_RLE + [UNFILTER, EXPAND] and report["reconstruction"] == "unfilter"
    names, report = decode(png, ctx, files["L"], inflate="device", unfilter="tiles")
    assert names == INFLATE_RLE + [TILES, EXPAND] and report["reconstruction"] == "tiles"      # 200 rows > 64: no short segment


def test_device_inflate_with_segments_of_both_kinds(png, ctx, files):
    names, report = decode(png, ctx, files["S2"], inflate="device", unfilter="tiles")
    assert names == INFLATE_RLE + [SEGMENTS, TILES, EXPAND] and report["reconstruction"] == "segments+tiles"
    names, report = decode(png, ctx, files["S2"], inflate="device")      # without tiles every segment keeps the segments call
    assert names == INFLATE_RLE + [SEGMENTS, EXPAND] and report["reconstruction"] == "segments"


def test_device_inflate_of_a_stream_with_far_matches(png, ctx, files):
    names, report = decode(png, ctx, files["Z"], inflate="device-lz")
    assert report["far_units"] > 0, report
    expected = 64 * (1 + 3 * 64)
    bound = (expected - 1).bit_length()                                  # ceil(log2(bytes)) rounds at the most, in groups of 4
    resolves = min(-(-(report["rounds"] + 1) // 4), -(-bound // 4))      # up to the group that holds the first round that rewrote nothing
    assert names == LZ_HEAD + [LZ_RESOLVE] * resolves + [LZ_GATHER] + CHECKED + [UNFILTER, EXPAND], (names, report)
    assert report["reconstruction"] == "unfilter"


@pytest.mark.parametrize("unfilter", ["band", "tiles"])
def test_many_files_in_one_pass(png, ctx, files, unfilter):
    batch = [files["P"], files["G"], files["I"]]
    imgs = [png.parse(f.data) for f in batch]
    want = []
    for bpp in sorted({im.bpp for im in imgs}):                           # one table, grouped by bpp in ascending order
        rows = np.concatenate([png.plan_segments(im)["rows"] for im in imgs if im.bpp == bpp])
        if unfilter == "band":
            want.append(SEGMENTS)
        else:                                                             # the segments of at most 64 rows, then the longer ones
            want += [SEGMENTS] * bool((rows <= 64).any()) + [TILES] * bool((rows > 64).any())
    want += [EXPAND] * sum(len(im.passes) for im in imgs)                 # in file and pass order
    assert want == ([SEGMENTS, SEGMENTS] if unfilter == "band" else [TILES, SEGMENTS, TILES]) + [EXPAND] * 9
    rec = Recorder(ctx)
    got = png.decode_device_many([f.data for f in batch], ctx=rec, unfilter=unfilter)
    assert rec.names == want
    for g, f in zip(got, batch):
        assert np.array_equal(g.cpu().numpy(), f.want)
