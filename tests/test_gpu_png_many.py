"""Many PNG files decoded in one pass (png.decode_device_many over radnet_png_plan_segments and radnet_png_unfilter_segments_u8)
against the one-file decoder and against tests/png_cases.py's expansion of the source samples; the segmented reconstruction
through the C ABI on a hand-built table; DeviceImageLoader.prefetch.  Every comparison is byte equality."""
import ctypes

import numpy as np
import pytest

import png_cases as K

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


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


def palette(n, seed=1):
    return np.random.RandomState(seed).randint(0, 256, size=(n, 3)).astype(np.uint8)


def cases(png):
    """(what, samples, colour type, depth, palette, encode arguments): every colour type and depth, Adam7 and not, widths 1, 2
    and 97, each fixed filter, random per row and adaptive, and the row counts around a wave and a band."""
    B = png.UNFILTER_BAND_ROWS
    rs = np.random.RandomState(2024)
    out = []

    def add(what, h, w, color_type, depth, filters, interlace=False, kind="full"):
        pal = palette(1 << depth, depth) if color_type == 3 else None
        out.append((what, K.draw(rs, h, w, color_type, depth, kind), color_type, depth, pal, dict(filters=filters, interlace=interlace)))

    for f in range(5):                                                    # each fixed filter; bpp 3, 1, 4, 8, 2
        fmt = [(2, 8), (0, 8), (6, 8), (6, 16), (4, 8)][f]
        add("fixed filter %d" % f, 129, 97, fmt[0], fmt[1], f)
    for k, (color_type, depth) in enumerate(K.LEGAL):                     # every legal colour type / depth pair
        add("format %d/%d" % (color_type, depth), 65 + k, (1, 2, 97)[k % 3], color_type, depth,
            np.random.RandomState(k) if k % 2 else "adaptive", interlace=k % 4 >= 2)
    for rows in (1, 63, 64, 65, 129):                                     # row counts around one wave and two
        add("%d rows, random" % rows, rows, 37, 2, 8, np.random.RandomState(rows))
        add("%d rows, Paeth" % rows, rows, 2, 2, 8, 4, kind="low")
    add("band + 1 rows, Paeth", B + 1, 33, 2, 8, 4)                       # one long segment in the launch set of the short ones
    add("band + 1 rows, random", B + 1, 5, 6, 8, np.random.RandomState(9))
    add("Adam7 97 x 200", 200, 97, 2, 8, np.random.RandomState(11), interlace=True)
    add("Adam7 1 x 70", 70, 1, 0, 8, "adaptive", interlace=True)
    add("None 200 x 200", 200, 200, 2, 8, 0)
    return out


@pytest.fixture(scope="module")
def batch(png):
    """The mixed batch, decoded once: (cases, files, decode_device_many's tensors as arrays)."""
    cs = cases(png)
    files = [K.encode(s, ct, d, palette=pal, **kw).data for _, s, ct, d, pal, kw in cs]
    many = png.decode_device_many(files)
    assert len(many) == len(files)
    assert all(t.is_cuda and t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3 and t.is_contiguous() for t in many)
    return cs, files, [t.cpu().numpy() for t in many]


def test_mixed_batch_against_the_reference_expansion(batch):
    cs, _, many = batch
    assert {c[2] for c in cs} == {0, 2, 3, 4, 6} and {c[3] for c in cs} == {1, 2, 4, 8, 16}
    for (what, s, ct, d, pal, _), got in zip(cs, many):
        want = K.expand(s, ct, d, pal)
        assert got.shape == want.shape, what
        assert np.array_equal(got, want), (what, np.argwhere((got != want).any(axis=2))[:4].tolist())


def test_mixed_batch_against_the_single_decoder(png, batch):
    cs, files, many = batch
    for (what, *_), f, got in zip(cs, files, many):
        assert np.array_equal(got, png.decode_device(f).cpu().numpy()), what


def test_the_batch_has_short_and_long_segments_and_several_bpp(png, batch):
    """What the batch is meant to exercise does occur in it: both launches, more than one bpp, cuts inside passes."""
    _, files, _ = batch
    imgs = [png.parse(f) for f in files]
    tables = [png.plan_segments(im) for im in imgs]
    rows = np.concatenate([t["rows"] for t in tables])
    assert (rows <= 64).any() and (rows > png.UNFILTER_BAND_ROWS).any() and ((rows > 64) & (rows < png.UNFILTER_BAND_ROWS)).any()
    assert {im.bpp for im in imgs} == {1, 2, 3, 4, 6, 8}
    assert any(len(t) > len(im.passes) for t, im in zip(tables, imgs))


def test_batch_of_one_and_of_none(png, batch):
    _, files, many = batch
    assert png.decode_device_many([]) == []
    for k in (0, 7, len(files) - 4):
        (one,) = png.decode_device_many([files[k]])
        assert np.array_equal(one.cpu().numpy(), many[k]) and np.array_equal(one.cpu().numpy(), png.decode_device(files[k]).cpu().numpy())
    a, b = png.decode_device_many(files[3:5], workers=1)
    assert np.array_equal(a.cpu().numpy(), many[3]) and np.array_equal(b.cpu().numpy(), many[4])


def test_two_runs_give_equal_bytes(png, batch):
    _, files, many = batch
    again = png.decode_device_many(files, workers=3)
    for a, b in zip(again, many):
        assert np.array_equal(a.cpu().numpy(), b)


def test_a_corrupt_file_raises_with_its_index(png, batch):
    _, files, _ = batch
    bad = bytearray(files[2])
    bad[-13] ^= 1                                                         # the last byte of the IDAT chunk's CRC (IEND is 12 bytes)
    with pytest.raises(ValueError, match="CRC") as single:
        png.decode_device(bytes(bad))
    got = None
    with pytest.raises(ValueError, match=r"^file 2: ") as e:
        got = png.decode_device_many([files[0], files[1], bytes(bad), files[3]])
    assert got is None and str(e.value) == "file 2: " + str(single.value)


# ---- the C ABI on a hand-built table ----------------------------------------------------------------------------------------------
SENTINEL = 0xA5


def hand_built(png):
    """One buffer: sentinels, pass A (70 rows of 12 bytes, random filters), sentinels, pass B (130 rows of 21 bytes, Paeth with two
    Sub rows), sentinels -- both bpp 3 -- and a table of A's and B's segments, shuffled."""
    rs = np.random.RandomState(77)
    a, ta = K.filter_rows(rs.randint(0, 256, (70, 12)).astype(np.uint8), 3, rs.randint(0, 5, 70))
    tb = np.full(130, 4)
    tb[[20, 100]] = 1
    b, tb = K.filter_rows(rs.randint(0, 256, (130, 21)).astype(np.uint8), 3, tb)
    at_a, at_b = 7, 7 + a.size + 5
    buf = np.full(at_b + b.size + 9, SENTINEL, np.uint8)
    buf[at_a:at_a + a.size] = a.reshape(-1)
    buf[at_b:at_b + b.size] = b.reshape(-1)
    segs = []
    for at, types, rowbytes, target in ((at_a, ta, 12, 16), (at_b, tb, 21, 64)):
        cuts = [0] + [r for r in range(1, len(types)) if types[r] <= 1 and (target == 64 or r % 3 == 0)] + [len(types)]
        segs += [(at + r0 * (1 + rowbytes), r1 - r0, rowbytes) for r0, r1 in zip(cuts[:-1], cuts[1:])]
    table = np.array(segs, png.SEGMENT)[rs.permutation(len(segs))]
    assert not np.array_equal(table["offset"], np.sort(table["offset"])) and (table["rows"] > 64).any() and (table["rows"] <= 64).any()
    return buf, table, ((at_a, 70, 12), (at_b, 130, 21))


def segments_call(ctx, dev, base_len, table, table_dev, count, bpp, handle=True):
    fn = ctx.lib.radnet_png_unfilter_segments_u8
    rc = fn(ctx.h if handle else None, dev.data_ptr() if dev is not None else None, base_len, table.ctypes.data if table is not None else None,
            table_dev.data_ptr() if table_dev is not None else None, count, bpp)
    msg = ctx.lib.radnet_last_error(ctx.h)
    return rc, (msg.decode() if msg else "")


def test_segments_abi_on_a_hand_built_table(png, ctx):
    buf, table, passes = hand_built(png)
    dev, ref = torch.from_numpy(buf).cuda(), torch.from_numpy(buf).cuda()
    table_dev = torch.from_numpy(table.view(np.uint8)).cuda()
    rc, msg = segments_call(ctx, dev, buf.size, table, table_dev, len(table), 3)
    assert rc == 0, msg
    for at, rows, rowbytes in passes:
        ctx.call("radnet_png_unfilter_u8", ref.data_ptr() + at, rows, rowbytes, 3)
    got, want = dev.cpu().numpy(), ref.cpu().numpy()
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8].tolist()
    assert not np.array_equal(got, buf)
    outside = np.ones(buf.size, bool)
    for at, rows, rowbytes in passes:
        outside[at:at + rows * (1 + rowbytes)] = False
    assert outside.sum() == 7 + 5 + 9 and (got[outside] == SENTINEL).all()


def test_segments_abi_argument_errors(png, ctx):
    buf, table, _ = hand_built(png)
    dev = torch.from_numpy(buf).cuda()
    table_dev = torch.from_numpy(table.view(np.uint8)).cuda()
    n = len(table)

    def refused(what, rc, msg, mention=None):
        assert rc != 0 and msg, what
        assert mention is None or mention in msg, (what, msg)
        ctx.sync()
        assert np.array_equal(dev.cpu().numpy(), buf), what               # nothing ran, not even the segments in front of the bad one

    def with_entry(i, **fields):
        t = table.copy()
        for k, v in fields.items():
            t[k][i] = v
        return t

    last = n - 1
    for what, t in (("offset beyond the buffer", with_entry(last, offset=buf.size - 3)),
                    ("offset far beyond the buffer", with_entry(last, offset=1 << 62)),
                    ("negative offset", with_entry(last, offset=-1)),
                    ("one row too many", with_entry(int(np.argmax(table["offset"])), rows=int(table["rows"][np.argmax(table["offset"])]) + 2)),
                    ("rowbytes % bpp", with_entry(last, rowbytes=13)),
                    ("zero rowbytes", with_entry(last, rowbytes=0)),
                    ("zero rows", with_entry(last, rows=0)),
                    ("negative rows", with_entry(last, rows=-5))):
        bad = int(np.flatnonzero((t != table))[0])
        refused(what, *segments_call(ctx, dev, buf.size, t, table_dev, n, 3), mention="segment %d" % bad)
    refused("a buffer shorter than the segments", *segments_call(ctx, dev, 100, table, table_dev, n, 3), mention="segment")
    refused("bpp", *segments_call(ctx, dev, buf.size, table, table_dev, n, 5))
    refused("null buffer", *segments_call(ctx, None, buf.size, table, table_dev, n, 3))
    refused("null host table", *segments_call(ctx, dev, buf.size, None, table_dev, n, 3))
    refused("null device table", *segments_call(ctx, dev, buf.size, table, None, n, 3))
    refused("negative count", *segments_call(ctx, dev, buf.size, table, table_dev, -1, 3))
    assert segments_call(ctx, dev, buf.size, table, table_dev, n, 3, handle=False)[0] != 0
    assert segments_call(ctx, dev, buf.size, table, table_dev, 0, 3)[0] == 0
    assert segments_call(ctx, None, 0, None, None, 0, 3)[0] == 0
    ctx.sync()
    assert np.array_equal(dev.cpu().numpy(), buf)


# ---- the loader ---------------------------------------------------------------------------------------------------------------------
def test_prefetch_then_calls_hit_the_cache(png, batch, tmp_path, monkeypatch):
    import os
    from faster_rcnn import utils_io
    cs, files, many = batch
    monkeypatch.chdir(tmp_path)
    pairs, want = [], []
    for k in (0, 5, 9, len(files) - 3):
        d = {"filepath": "maps/m%d.png" % k}
        for t, j in (("rgb", k), ("topo", k + 1)):
            path = utils_io.image_path(d["filepath"], t)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "wb") as f:
                f.write(files[j])
            pairs.append((d, t))
            want.append(many[j])
    calls = []

    def decode(buf):
        calls.append(len(buf))
        return png.decode_device(buf)

    batches = []

    def decode_many(files):
        batches.append(len(files))
        return png.decode_device_many(files)

    loader = utils_io.DeviceImageLoader(cache_bytes=64 << 20, decode=decode, decode_many=decode_many)
    assert loader.prefetch(pairs) == len(pairs) == loader.prefetched and batches == [len(pairs)] and not calls
    uncached = utils_io.DeviceImageLoader(cache_bytes=0)
    for (d, t), w in zip(pairs, want):
        got = loader(d, t)
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), uncached(d, t).cpu().numpy()) and np.array_equal(got.cpu().numpy(), w)
    assert not calls and (loader.hits, loader.misses) == (len(pairs), 0)
    assert loader.prefetch(pairs) == 0 and batches == [len(pairs)]
    plain = utils_io.DeviceImageLoader(cache_bytes=64 << 20)              # the defaults: png.decode_device_many fills, the calls hit
    assert plain.prefetch(pairs[:3]) == 3
    for (d, t), w in zip(pairs[:3], want):
        assert np.array_equal(plain(d, t).cpu().numpy(), w)
    assert (plain.hits, plain.misses) == (3, 0)
