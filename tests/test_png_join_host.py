"""The host half of join="device" (no device needed): the model of tests/png_join_cases.py against b"".join and its five mutants
against the cases named for them; radnet_png_plan_join (csrc/png_join_plan.cpp), one refusal per reason with the bad entry;
parse_compressed(join="device") -- what the staging buffer holds, the stream the model gathers from it, the header and the trailer
read through the table, the ValueErrors of broken containers --; check_modes and the option on get_image, the loader and RADNet
with the decoder stubbed."""
import struct
import types
import zlib

import numpy as np
import pytest

import png_cases as K
import png_join_cases as JC
from faster_rcnn import png, utils_io
from radnet_hip import lib as L

ERR_ARG, ERR_UNSUPPORTED = -1, -3
CASES = JC.cases()
BY_NAME = {c["name"]: c for c in CASES}


def test_the_constants_the_abi_mirror_and_the_binding():
    assert L.header_constant("RADNET_PNG_JOIN_GRAIN") == JC.GRAIN == 16 and L.header_constant("RADNET_PNG_JOIN_SPAN_GRAINS") == JC.SPAN_GRAINS == 256
    assert png.JOIN_PIECE == JC.PIECE and png.JOIN_PIECE.itemsize == 24 and png.JOIN_PIECE.names == ("src", "dst", "length")
    assert png.JOIN_MODES == ("host", "device")
    for name in ("radnet_png_plan_join", "radnet_png_join_u8"):
        assert name in L.declared_symbols() and hasattr(L.load_library(), name)


def test_the_case_table_holds_what_it_is_meant_to():
    assert len({c["name"] for c in CASES}) == len(CASES)
    assert {c["out_at"] for c in CASES} == set(JC.ALIGNMENTS) == {c["file_at"] for c in CASES}
    odd = BY_NAME["odd gaps"]["table"]
    assert set(((odd["src"] - odd["dst"]) % 16).tolist()) == set(range(16)) and set(JC.LENGTHS) <= set(odd["length"].tolist())
    run = BY_NAME["empty pieces first, last and a thousand in a row"]["table"]["length"]
    assert run[0] == 0 and run[-1] == 0 and (run[4:1004] == 0).all() and run[3] > 0 and run[1004] > 0
    assert BY_NAME["empty pieces alone"]["n"] == 0 and len(BY_NAME["empty pieces alone"]["table"]) == 7 and len(BY_NAME["the empty table"]["table"]) == 0
    small = BY_NAME["three thousand small pieces"]["table"]
    assert len(small) == 3000 and small["length"].max() == 40 and small["length"].min() == 0
    assert (2 << 20) in BY_NAME["one long piece between tiny ones"]["table"]["length"]
    assert (np.diff(BY_NAME["shuffled sources"]["table"]["src"]) < 0).any()
    over = BY_NAME["overlapping sources"]["table"]
    order = np.argsort(over["src"])
    assert ((over["src"] + over["length"])[order][:-1] > over["src"][order][1:]).any()
    assert max(len(c["file"]) for c in CASES) < (2 << 20) + 4096


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_model_equals_the_plain_join(case):
    want = JC.joined(case["file"], case["table"])
    assert len(want) == case["n"]
    for out_at in (case["out_at"], 0, 15):
        assert np.array_equal(JC.model(case["file"], case["table"], case["n"], out_at), want)


@pytest.mark.parametrize("mutant", JC.MUTANTS)
def test_every_mutant_is_caught_by_its_case(mutant):
    case = BY_NAME[JC.CAUGHT_BY[mutant]]
    want = JC.joined(case["file"], case["table"])
    assert np.array_equal(JC.model(case["file"], case["table"], case["n"], case["out_at"]), want)
    assert not np.array_equal(JC.model(case["file"], case["table"], case["n"], case["out_at"], mutant=mutant), want)


# ---- the planner ------------------------------------------------------------------------------------------------------------------------
def test_the_plan_counts_grains_and_spans():
    for case in CASES:
        for at in (case["out_at"], 0, 15):
            rc, grains, spans, bad, msg = L.png_plan_join(case["table"], len(case["file"]), case["n"], at)
            assert (rc, bad, msg) == (0, -1, ""), case["name"]
            want = -(-(at + case["n"]) // 16) if case["n"] else 0
            assert (grains, spans) == (want, -(-want // 256)), case["name"]
    assert L.png_plan_join(None, 0, 0)[:3] == (0, 0, 0)
    assert L.png_plan_join(JC.table_of([0], [4096]), 4096, 4096, 0)[1:3] == (256, 1)
    assert L.png_plan_join(JC.table_of([0], [4096]), 4096, 4096, 1)[1:3] == (257, 2)


def test_the_plan_refuses_one_reason_at_a_time():
    good = JC.table_of([10, 30, 30, 5], [10, 0, 7, 3])

    def refused(table=good, file_len=40, n=20, misalign=0, count=None, bad=-1, say="png_join", rc=ERR_ARG):
        got, grains, spans, entry, msg = L.png_plan_join(table, file_len, n, misalign, count)
        assert (got, entry) == (rc, bad) and say in msg, (got, entry, msg)
        assert (grains, spans) == (-1, -1)            # the plan is written on RADNET_OK only
    assert L.png_plan_join(good, 40, 20)[0] == 0
    refused(count=-1, say="-1 pieces")
    refused(file_len=-1, say="a file of -1 bytes")
    refused(n=-1, say="an output of -1 bytes")
    refused(misalign=16, say="misalignment")
    refused(misalign=-1, say="misalignment")
    refused(table=None, count=3, say="null table")
    for row, field, value, say in ((2, "src", -1, "leaves the file"), (2, "length", -1, "leaves the file"), (2, "src", 34, "leaves the file"),
                                   (0, "src", 31, "leaves the file"), (3, "src", (1 << 63) - 1, "leaves the file"),
                                   (1, "dst", 9, "in front of it hold 10 bytes"), (3, "dst", 18, "in front of it hold 17 bytes"),
                                   (0, "dst", 1, "in front of it hold 0 bytes")):
        t = good.copy()
        t[field][row] = value
        refused(t, bad=row, say=say)
    t = good.copy()
    t["length"][2] = (1 << 63) - 1                    # src + length leaves 64 bits
    refused(t, bad=2, say="leaves the file")
    refused(n=19, bad=3, say="passes the output")      # the total is more than n: the piece that passes it
    refused(n=21, say="the pieces hold 20 bytes, the output 21")      # and less
    refused(table=JC.table_of([], []), n=1, say="the pieces hold 0 bytes")
    assert L.load_library().radnet_png_plan_join(None, 0, 0, 0, 0, None, None, None, 0) == ERR_ARG      # a null plan
    big = (1 << 63) - 1
    refused(JC.table_of([0], [big]), file_len=big, n=big, misalign=15, say="spans", rc=ERR_UNSUPPORTED)


# ---- parse_compressed(join="device") ----------------------------------------------------------------------------------------------------
def chunks_of(data):
    pos, out = 8, []
    while pos < len(data):
        length, kind = struct.unpack(">I4s", data[pos:pos + 8])
        out.append((kind, pos, pos + 8 + length))
        pos += 12 + length
    return out


def rechunked(data, sizes):
    """The file `data` with its IDAT stream cut into chunks of `sizes` front and back: sizes = (front sizes, back sizes), the rest in
    one chunk between them."""
    front, back = sizes
    z = b"".join(data[at + 8:end] for kind, at, end in chunks_of(data) if kind == b"IDAT")
    middle = len(z) - sum(front) - sum(back)
    assert middle > 0
    parts, pos = [], 0
    for size in list(front) + [middle] + list(back):
        parts.append(K.chunk(b"IDAT", z[pos:pos + size]))
        pos += size
    first = data.index(b"IDAT") - 4
    return data[:first] + b"".join(parts) + K.chunk(b"IEND")


def files():
    """(name, file bytes): chunks of 0 bytes and of 1 byte among them, a palette, a header and a trailer that straddle chunks."""
    rng = np.random.RandomState(51)
    s = K.draw(rng, 40, 50, 2, 8)
    one = K.encode(s, 2, 8, filters="adaptive").data
    out = [("rgb_one_idat", one), ("rgb_many_idat", K.encode(s, 2, 8, filters=rng, idat_sizes=[1, 0, 7, 3000, 0, 1, 16]).data)]
    pal = rng.randint(0, 256, size=(200, 3))
    out.append(("palette_zero_first", K.encode(rng.randint(0, 200, size=(33, 70, 1)), 3, 8, filters=1, palette=pal, idat_sizes=[0, 1, 1, 500]).data))
    out.append(("split_header_and_trailer", rechunked(one, ((1,), (1, 0, 2)))))
    out.append(("interlaced_16_bit", K.encode(K.draw(rng, 9, 14, 6, 16), 6, 16, filters=rng, interlace=True, idat_sizes=[7, 1, 30]).data + b"trailing bytes"))
    return out


FILES = files()


@pytest.mark.parametrize("crc", png.CRC_MODES)
@pytest.mark.parametrize("name,data", FILES, ids=[f[0] for f in FILES])
def test_parse_compressed_stages_the_file_and_the_tables(name, data, crc):
    ref = png.parse_compressed(data, crc=crc)
    assert ref.file_len is None and ref.pieces is None
    comp = png.parse_compressed(data, crc=crc, join="device")
    idat = [(at + 8, end) for kind, at, end in chunks_of(data) if kind == b"IDAT"]
    assert (comp.n, comp.header, comp.passes, comp.bpp, comp.expected) == (ref.n, ref.header, ref.passes, ref.bpp, ref.expected)
    assert np.array_equal(comp.palette, ref.palette) and comp.file_len == len(data)
    # the table: the walk's payloads, empty ones too, dst the prefix sum
    table = comp.pieces
    assert table.dtype == png.JOIN_PIECE and np.array_equal(table, png.join_pieces(idat)) and len(table) == len(idat)
    assert table["src"].tolist() == [s for s, _ in idat] and table["length"].tolist() == [e - s for s, e in idat]
    assert table["dst"].tolist() == np.concatenate([[0], np.cumsum(table["length"])[:-1]]).tolist()
    assert L.png_plan_join(table, comp.file_len, comp.n)[0] == 0
    # the staging buffer: the file, the palette, the pad, the pieces, then what crc="device" adds -- and nothing else
    count = len(idat)
    lay = png.staging_layout(len(data), 1, png.CRC_SEGMENT.itemsize if crc == "device" else 0, count if crc == "device" else 0, sums=crc == "device",
                             pieces=count)
    assert lay == png.join_layout(comp) and lay.pieces % 8 == 0 and lay.palettes == len(data) and lay.pad == len(data) + 768
    assert lay.table == lay.pieces + 24 * count and lay.total == comp.staged.numel()
    staged = comp.staged.numpy()
    assert staged[:lay.palettes].tobytes() == bytes(data) and staged[lay.palettes:lay.pad].tobytes() == comp.palette.tobytes()
    assert not staged[lay.pad:lay.pieces].any() and staged[lay.pieces:lay.table].tobytes() == table.tobytes()
    if crc == "device":
        assert np.array_equal(comp.crc_segments, ref.crc_segments) and staged[lay.table:lay.sums].tobytes() == comp.crc_segments.tobytes()
        assert lay.sums == lay.table + 24 * count and lay.result == lay.sums + 4 * count and lay.total == lay.result + 8
        assert not staged[lay.sums:].any()
    else:
        assert comp.crc_segments is None and lay.table == lay.sums == lay.result == lay.total
    # the stream the device will gather equals the one the host joins
    joined = ref.staged.numpy()[:ref.n]
    assert np.array_equal(JC.model(staged[:comp.file_len], table, comp.n, 5), joined)
    assert comp.trailer == ref.trailer == struct.unpack(">I", joined[-4:].tobytes())[0] == zlib.adler32(zlib.decompress(joined.tobytes()))


def test_every_existing_layout_is_what_it_was():
    for n, palettes, record, count, sums in ((10, 1, 0, 0, False), (13, 1, 24, 5, True), (13, 3, 16, 7, False), (0, 1, 24, 0, True)):
        pad = n + 768 * palettes
        table = (pad + 7) & ~7 if record else pad
        result = table + record * count + (4 * count if sums else 0)
        got = png.staging_layout(n, palettes, record, count, sums=sums)
        assert tuple(got) == (n, pad, table, table + record * count, result, result + (8 if sums else 0)) and type(got) is png.Staging
    assert png.crc_layout(13, 5) == (784, 904, 924, 932)


def test_the_header_and_the_trailer_are_read_through_the_table():
    data = dict(FILES)["split_header_and_trailer"]
    lengths = [end - at - 8 for kind, at, end in chunks_of(data) if kind == b"IDAT"]
    assert lengths[0] == 1 and lengths[-3:] == [1, 0, 2] and len(lengths) == 5
    comp = png.parse_compressed(data, join="device")
    source = np.frombuffer(data, np.uint8)
    z = b"".join(data[at + 8:end] for kind, at, end in chunks_of(data) if kind == b"IDAT")
    assert png.joined_bytes(source, comp.pieces, 0, 2) == z[:2] and png.joined_bytes(source, comp.pieces, comp.n - 4, comp.n) == z[-4:]
    assert comp.trailer == int.from_bytes(z[-4:], "big") == zlib.adler32(zlib.decompress(z))
    for a, b in ((0, 0), (0, 1), (1, 2), (0, comp.n), (comp.n - 3, comp.n - 2), (comp.n - 1, comp.n), (5, 40)):
        assert png.joined_bytes(source, comp.pieces, a, b) == z[a:b], (a, b)
    # a zlib header the device inflate does not take, cut behind its first byte
    first = data.index(b"IDAT") - 4
    for head in ((0x79, 0x9C), (0x78, 0x9D), (0x78, 0xBB)):
        bad = data[:first] + K.chunk(b"IDAT", bytes(head[:1])) + K.chunk(b"IDAT") + K.chunk(b"IDAT", bytes(head[1:]) + z[2:]) + K.chunk(b"IEND")
        for join in png.JOIN_MODES:
            with pytest.raises(ValueError, match="zlib header"):
                png.parse_compressed(bad, join=join)
    short = data[:first] + K.chunk(b"IDAT", z[:1]) + K.chunk(b"IEND")      # a stream of one byte
    for join in png.JOIN_MODES:
        with pytest.raises(ValueError, match="zlib header"):
            png.parse_compressed(short, join=join)


def flip(data, at, bit=0x10):
    out = bytearray(data)
    out[at] ^= bit
    return bytes(out)


def broken_containers():
    """The broken files of tests/test_crc32_host.py and tests/test_inflate_host.py, by name."""
    out = []
    data = dict(FILES)["palette_zero_first"]
    where = {kind: (at, end) for kind, at, end in chunks_of(data) if kind != b"IDAT"}
    idat = [(at, end) for kind, at, end in chunks_of(data) if kind == b"IDAT"]
    out.append(("a PLTE CRC field", flip(data, where[b"PLTE"][1] + 2)))
    out += [("an IDAT CRC field", flip(data, idat[3][1] + 1)), ("an IDAT payload byte", flip(data, idat[3][0] + 8 + 100)),
            ("an empty IDAT chunk's CRC field", flip(data, idat[0][1]))]
    rs = np.random.RandomState(3)
    for color, depth, interlace in ((2, 8, False), (3, 4, True), (6, 16, False)):
        pal = rs.randint(0, 256, (16, 3)) if color == 3 else None
        enc = K.encode(K.draw(rs, 9, 14, color, depth), color, depth, filters=rs, interlace=interlace, palette=pal, idat_sizes=[7, 1, 30])
        out.append(("a byte 20 from the end, colour type %d" % color, flip(enc.data, len(enc.data) - 20, 4)))
    enc = K.encode(K.draw(rs, 5, 5, 0, 8), 0, 8)
    at = enc.data.index(b"IDAT")
    for first, second in ((0x79, 0x9C), (0x78, 0x9D), (0x78, 0xBB)):
        payload = bytes([first, second]) + enc.data[at + 6:enc.data.index(b"IEND") - 8]
        out.append(("a zlib header %02X %02X" % (first, second), enc.data[:at - 4] + K.chunk(b"IDAT", payload) + K.chunk(b"IEND")))
    big = K.encode(K.draw(np.random.RandomState(17), 700, 700, 2, 8), 2, 8, filters=0, idat_sizes=[8192] * 150, level=1).data
    assert len(big) > 1 << 20
    out.append(("a byte in the middle of a file above 1 MiB", flip(big, len(big) // 2, 1)))
    enc = K.encode(K.draw(np.random.RandomState(5), 6, 7, 3, 8), 3, 8, palette=np.arange(30).reshape(10, 3))
    plte, at = enc.data.index(b"PLTE") - 4, enc.data.index(b"IDAT") - 4
    head, pal, z, end = enc.data[:33], enc.data[plte:at], enc.data[at:-12], enc.data[-12:]
    bad = lambda chunk: chunk[:-1] + bytes([chunk[-1] ^ 1])      # noqa: E731
    out += [("a bad CRC in chunk 2, chunk 3 truncated", head + bad(pal) + z[:-3]), ("a second IHDR after a bad-CRC PLTE", head + bad(pal) + head[8:] + z + end),
            ("no IEND after a bad-CRC IDAT", head + pal + bad(z)), ("a bad signature", b"\x88" + enc.data[1:]), ("no PLTE for colour type 3", head + z + end)]
    return out, big


BROKEN, BIG = broken_containers()


def outcome(f):
    try:
        return "parsed", f().n
    except ValueError as e:
        return "ValueError", str(e)


@pytest.mark.parametrize("name,data", BROKEN, ids=[b[0] for b in BROKEN])
def test_broken_containers_raise_what_they_raise_with_the_host_join(name, data):
    want = outcome(lambda: png.parse_compressed(data))
    assert want[0] == "ValueError", name
    assert outcome(lambda: png.parse_compressed(data, join="device")) == want
    # with the IDAT sums left to the device a broken IDAT chunk is no host error, in either mode; everything else still is
    assert outcome(lambda: png.parse_compressed(data, crc="device", join="device")) == outcome(lambda: png.parse_compressed(data, crc="device"))


def test_a_file_above_one_mebibyte_takes_the_native_sums_and_one_copy():
    ref = png.parse_compressed(BIG)
    for crc in png.CRC_MODES:
        comp = png.parse_compressed(BIG, crc=crc, join="device")
        staged = comp.staged.numpy()
        assert staged[:comp.file_len].tobytes() == BIG and len(comp.pieces) == 151
        assert np.array_equal(JC.model(staged[:comp.file_len], comp.pieces, comp.n, 9), ref.staged.numpy()[:ref.n]) and comp.trailer == ref.trailer


# ---- the option ------------------------------------------------------------------------------------------------------------------------
def test_the_modes_are_checked_before_any_device_work():
    needs_inflate = "PNG: join=\"device\" joins the IDAT stream of the uploaded file and needs inflate=\"device\" or \"device-lz\", not inflate=\"host\""
    data = FILES[0][1]
    for kw, want in ((dict(join="gpu"), "PNG: join='gpu' (\"host\" or \"device\")"), (dict(join="device"), needs_inflate),
                     (dict(inflate="host", join="device", crc="host"), needs_inflate)):
        for taker in (png.check_modes, utils_io.DeviceImageLoader, lambda **k: png.decode_device(data, **k)):
            with pytest.raises(ValueError) as e:
                taker(**kw)
            assert str(e.value) == want, kw
    with pytest.raises(ValueError, match="join='gpu'"):
        png.parse_compressed(data, join="gpu")
    for inflate in ("device", "device-lz"):
        for crc in png.CRC_MODES:
            png.check_modes(inflate, "tiles", crc, "device")
            png.check_modes(inflate, crc=crc, join="host")
    png.check_modes(join="host")
    with pytest.raises(TypeError):
        png.decode_device_many([data], join="device")      # the many-file entry inflates on the host and takes no join


def test_get_image_the_loader_and_radnet_pass_the_option_on(tmp_path, monkeypatch):
    calls = []

    def stub(buf, **kw):
        calls.append(kw)
        return np.zeros((2, 2, 3), np.uint8)
    monkeypatch.setattr(png, "decode_device", stub)
    (tmp_path / "maps" / "grey").mkdir(parents=True)
    (tmp_path / "maps" / "grey" / "scan.png").write_bytes(FILES[0][1])
    monkeypatch.chdir(tmp_path)
    path = "maps/scan.png"
    utils_io.get_image(path, ["grey"], to_host=False)
    utils_io.get_image(path, ["grey"], to_host=False, inflate="device", join="device")
    utils_io.get_image(path, ["grey"], to_host=False, inflate="device-lz", crc="device", join="device", unfilter="tiles")
    utils_io.get_image(path, ["grey"], to_host=False, inflate="device", join="host")
    assert calls == [{}, dict(inflate="device", join="device"), dict(inflate="device-lz", crc="device", join="device", unfilter="tiles"), dict(inflate="device")]
    del calls[:]
    loader = utils_io.DeviceImageLoader(inflate="device", join="device", cache_bytes=0)
    assert (loader.inflate, loader.crc, loader.unfilter, loader.join) == ("device", "host", "band", "device")
    loader(dict(filepath=path), "grey")
    plain = utils_io.DeviceImageLoader(cache_bytes=0)
    assert plain.join == "host"
    plain(dict(filepath=path), "grey")
    assert calls == [dict(inflate="device", join="device"), {}]
    # RADNet.predict_from_path hands png_join on only when it is not the default
    from faster_rcnn.RADNet import RADNet
    assert RADNet.png_join == "host"
    seen = []
    monkeypatch.setattr(utils_io, "get_image", lambda path, kinds, **kw: seen.append(kw) or "image")
    monkeypatch.setattr(RADNet, "_takes_device_images", lambda self: True)
    monkeypatch.setattr(RADNet, "predict", lambda self, images: images)
    net = object.__new__(RADNet)
    net.C = types.SimpleNamespace(use_img_type=False, img_types=["grey"])
    assert net.predict_from_path(path) == ["image"]
    net.png_inflate, net.png_join = "device", "device"
    net.predict_from_path(path)
    assert seen == [dict(random_type=False, to_host=False, inflate="host"), dict(random_type=False, to_host=False, inflate="device", join="device")]
