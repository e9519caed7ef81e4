"""The Python model of the device inflate for any stream (tests/inflate_lz_cases.py) against zlib, and its host entry against the
model -- no GPU: every eligible case gives zlib.decompress's bytes with exactly one literal root per byte; zlib refuses exactly the
cases the model refuses (but the two refusals that are this project's own); the rounds stay within the bound and within what the
prototype counted; radnet_inflate_lz_chain equals the model's chain with every refusal code; each mutant of the model is caught by a
named case; the header's constants and record are the model's."""
import ctypes
import zlib

import numpy as np
import pytest

import inflate_cases as I
import inflate_lz_cases as Z


@pytest.mark.parametrize("name", Z.ELIGIBLE)
def test_the_model_inflates_every_eligible_case(name):
    c = Z.cases()[name]
    out, reason, stats = Z.model(name)
    assert reason is None and out == c.data == zlib.decompress(c.z), (name, reason)
    assert stats["units"] >= 1 and stats["blocks"] >= stats["units"] and 0 <= stats["far_units"] <= stats["units"]
    assert stats["rounds"] <= Z.bound(c.expected), (name, stats)
    assert stats["rounds"] <= Z.ROUNDS.get(name, 10), (name, stats)
    links, buf, src, flat, rounds, final = Z.model_buffers(name, 0xA5, 0xA5A5A5A5)
    i = np.arange(c.expected)
    assert (flat <= i).all() and (flat[flat] == flat).all(), "every byte points at a root"
    assert ((src == i) == (flat == i)).all(), "the roots are the literals, before and after"
    assert final.tobytes() == c.data
    if name in I.ELIGIBLE:                                             # a run-length stream: the same bytes as the run-length path, no far match
        assert out == I.model(name)[0] and stats["far_units"] == 0
        assert max(u[7] for u in Z.model_units(name)[1]) <= 1


def test_zlib_refuses_exactly_what_the_model_refuses():
    for name, c in Z.cases().items():
        out, reason, _ = Z.model(name)
        try:
            want = zlib.decompress(c.z)
        except zlib.error as e:
            want = None
            message = str(e)
        if name in Z.OWN_REFUSALS:
            assert out is None and reason == c.reason and want is not None, name
            continue
        assert (out is None) == (want is None), (name, reason)
        assert out == want and (reason is None) == (out is not None), name
        if c.reason is not None:
            assert reason == c.reason, (name, reason)
        if name == "hand far twin":
            assert "too far back" in message
    assert {n for n, c in Z.cases().items() if Z.model(n)[0] is not None} == set(Z.ELIGIBLE)


def test_what_the_cases_are_made_to_show():
    units = Z.model("noise memlevel 1")[2]
    assert units["units"] > 50 and units["far_units"] == units["units"]
    reach = [u[7] for u in Z.model_units("noise memlevel 1")[1]]
    assert max(reach) > 5000, "units that read thousands of bytes into the units in front of them"
    assert Z.model("mix memlevel 2")[2]["blocks"] > Z.model("mix memlevel 2")[2]["units"] > 10, "stored blocks ride along"
    assert Z.model("mix fixed")[2]["candidates"] == 0
    tokens = []
    Z.decode_unit(Z.cases()["hand far"].z, 16, tokens=tokens)
    matches = [t[1:] for t in tokens if t[0] == "match"]
    assert matches == [(258, 32768), (10, 24577), (258, 2), (258, 257), (3, 1)]
    assert Z.model_units("hand far")[1][0][7] == 0 and Z.model_units("hand far twin")[1][0][7] == 1
    assert Z.model("zeros")[2]["far_units"] == 0 and Z.model("zeros")[2]["rounds"] <= 10
    assert I.model("i level 6")[1] == "chain: a unit that did not decode (not run-length)"      # and the run-length path still refuses it


def test_the_model_accepts_every_file_the_end_to_end_test_decodes():
    files = Z.png_files()
    assert len(files) == 32
    for what, data in files:
        _, idat = Z.idat_of(data)
        want = zlib.decompress(idat)
        out, reason, stats = Z.inflate(idat, len(want))
        assert reason is None and out == want, (what, reason)
        if what == "low noise, memlevel 1":
            assert stats["units"] > 50 and stats["far_units"] > 0, stats
        if what == "low noise":
            assert stats["far_units"] > 0 and I.inflate(idat, len(want))[1] == "chain: a unit that did not decode (not run-length)"


def chain_native(units, first_bit, n, expected, link_cap=None):
    from faster_rcnn import png
    from radnet_hip import lib as L
    table = np.array([tuple(u) for u in units], png.INFLATE_LZ_UNIT)
    links = np.zeros(len(units) if link_cap is None else link_cap, png.INFLATE_LINK)
    nl, nf, bad = ctypes.c_int32(-9), ctypes.c_int32(-9), ctypes.c_int32(-9)
    rc = L.load_library().radnet_inflate_lz_chain(table.ctypes.data, len(table), first_bit, n, expected, links.ctypes.data, len(links), ctypes.byref(nl),
                                                  ctypes.byref(nf), ctypes.byref(bad))
    got = [(int(l["out_offset"]), int(l["start_bit"]), int(l["out_bytes"]), int(l["prev_byte"])) for l in links[:max(nl.value, 0)]]
    return rc, bad.value, got, nf.value


def test_the_native_chain_equals_the_model():
    seen = set()
    for name, c in Z.cases().items():
        starts, units = Z.model_units(name)
        for first_bit, n, expected in ((16, len(c.z), c.expected), (17, len(c.z), c.expected), (16, len(c.z) + 1, c.expected), (16, len(c.z), c.expected + 1)):
            want = Z.chain(units, first_bit, n, expected)
            assert chain_native(units, first_bit, n, expected) == want, (name, first_bit, n, expected)
            seen.add(want[0])
    assert seen == {Z.CHAIN_OK, Z.CHAIN_NO_START, Z.CHAIN_BAD_UNIT, Z.CHAIN_LENGTH, Z.CHAIN_TRAILER, Z.CHAIN_REACH}, seen
    # the reach against the offset, unit by unit: entered at its second unit the noise stream reaches in front of the stream
    c = Z.cases()["noise memlevel 1"]
    starts, units = Z.model_units("noise memlevel 1")
    want = Z.chain(units[1:], starts[1], len(c.z), c.expected)
    assert want[0] == Z.CHAIN_REACH and want[1] == 0 and chain_native(units[1:], starts[1], len(c.z), c.expected) == want


@pytest.mark.parametrize("mutant", Z.MUTANTS)
def test_every_mutant_of_the_model_is_caught(mutant):
    c = Z.cases()[Z.CAUGHT_BY[mutant]]
    right = Z.model(c.name)
    wrong = Z.inflate(c.z, c.expected, **{mutant: True})
    assert (right[0], right[1]) == (c.data if c.reason is None else None, c.reason)
    if mutant == "no_mod":                                             # the bytes are right; the chains are as deep as the run is long
        assert wrong[0] == right[0] and wrong[2]["rounds"] > right[2]["rounds"] + 5, (wrong[2], right[2])
        links = Z.model_buffers(c.name, 0xA5, 0xA5A5A5A5)[0]
        assert not np.array_equal(Z.emit(c.z, links, c.expected, 0xA5, 0xA5A5A5A5, no_mod=True)[1], Z.model_buffers(c.name, 0xA5, 0xA5A5A5A5)[2])
    else:
        assert (wrong[0], wrong[1]) != (right[0], right[1]), mutant
    if mutant in ("reach_from_end", "reach_off_by_one"):
        assert right[1] == Z.REACH_REASON and wrong[1] == "adler", "the chain lets it pass and only the checksum sees it"


def test_the_header_states_the_models_constants():
    from faster_rcnn import png
    from radnet_hip import lib as L
    assert L.header_constant("RADNET_INFLATE_CHAIN_REACH") == Z.CHAIN_REACH == 6
    assert L.header_constant("RADNET_INFLATE_LZ_MAX_ROUNDS") >= Z.bound((1 << 31) - 1) == 31
    assert png.INFLATE_LZ_UNIT.itemsize == 40 and png.INFLATE_LZ_UNIT.names == Z.UNIT_FIELDS
    assert png.INFLATE_LZ_CHAIN == Z.CHAIN_NAMES and L.header_constant("RADNET_INFLATE_FLAG_FINAL") == Z.FINAL
    assert [Z.bound(n) for n in (0, 1, 2, 3, 4, 5, 1 << 20, (1 << 20) + 1)] == [1, 1, 1, 2, 2, 3, 20, 21]
    assert Z.DISTANCE_TABLE[:6] == [(1, 0), (2, 0), (3, 0), (4, 0), (5, 1), (7, 1)] and Z.distance_symbol(32768) == (29, 13, 8191)
