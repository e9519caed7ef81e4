"""The host half of the tiled PNG reconstruction (unfilter="tiles"): radnet_png_plan_tiles and radnet_png_tiles_on_sweep
(csrc/png_plan.cpp over csrc/png_tile_rule.h, the rule the kernel's launch code reads too) against the NumPy model of
tests/png_tiles_cases.py.  The plan's numbers; every byte a tile reads and does not own belongs to a tile of an earlier sweep; the
tiles own every byte once; the model run over the planner's sweeps in reversed and shuffled within-sweep order gives the raw rows;
three mutants of the rule that must fail these checks; refused arguments; the planner under AddressSanitizer + UBSan in a
stand-alone program.  No device needed."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import png_tiles_cases as TC
from faster_rcnn import png, utils_io
from radnet_hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
T = png.TILE_PIXELS


def planner_sweeps(rows, pixels, bpp):
    plan = png.plan_tiles(rows, pixels * bpp, bpp)
    return plan, [png.tiles_on_sweep(rows, pixels * bpp, bpp, d) for d in range(plan.sweeps)]


def test_the_constants_the_abi_mirror_and_the_binding():
    assert png.TILE_ROWS == TC.ROWS == 64 and T >= 64 and T % 32 == 0
    assert T == L.header_constant("RADNET_PNG_TILE_PIXELS")
    for name in ("radnet_png_plan_tiles", "radnet_png_tiles_on_sweep", "radnet_png_unfilter_tiles_u8"):
        assert name in L.declared_symbols()
    assert png.TilePlan._fields == ("bands", "blocks", "sweeps", "tile_rows", "tile_pixels")


@pytest.mark.parametrize("bpp", TC.BPPS)
def test_the_plan_equals_the_model(bpp):
    for rows, pixels in TC.shapes(T) + [(4000, 4000), (1, 1 << 20), (200, 2 * T + 70)]:
        if pixels * bpp > 1 << 30:
            continue
        geo = TC.geometry(rows, pixels, T)
        plan, sweeps = planner_sweeps(rows, pixels, bpp)
        assert plan == (geo.bands, geo.blocks, geo.sweeps, 64, T), (rows, pixels)
        assert sweeps == TC.tiles_by_sweep(geo), (rows, pixels)      # the same tiles on the same sweeps, bands ascending: blockIdx.x order
    assert png.plan_tiles(4000, 12000, 3).sweeps == -(-(4000 + 63) // T) + 2 * 62


def ownership(geo, sweeps):
    """(how many tiles own each pixel, the sweep of a pixel's owner) over the tiles of `sweeps`."""
    count = np.zeros((geo.rows, geo.pixels), np.int64)
    owner = np.full((geo.rows, geo.pixels), -1, np.int64)
    for d, tiles in enumerate(sweeps):
        for band, block in tiles:
            mask = TC.owned(geo, band, block)
            count += mask
            owner[mask] = d
    return count, owner


def reads_are_earlier(geo, sweeps, owner):
    """Every pixel a tile reads and does not own is owned by a tile of a strictly earlier sweep."""
    for d, tiles in enumerate(sweeps):
        for band, block in tiles:
            if (owner[TC.read_not_owned(TC.owned(geo, band, block))] >= d).any():
                return False
    return True


def test_reads_lie_in_earlier_sweeps_and_every_byte_has_one_owner():
    for rows, pixels in TC.shapes(T) + [(200, 2 * T + 70), (300, 5 * T)]:
        geo = TC.geometry(rows, pixels, T)
        _, sweeps = planner_sweeps(rows, pixels, 1)
        count, owner = ownership(geo, sweeps)
        assert (count == 1).all(), (rows, pixels)
        assert reads_are_earlier(geo, sweeps, owner), (rows, pixels)
        assert all(len(tiles) >= 1 or (geo.blocks == 1 and d % 2 == 1) for d, tiles in enumerate(sweeps))


@pytest.fixture(scope="module")
def drawn():
    """The model cases, drawn once: (rows, pixels, bpp, kind, filtered lines, raw rows)."""
    rs = np.random.RandomState(20)
    return [(rows, pixels, bpp, kind) + TC.draw_segment(rs, rows, pixels, bpp, kind) for rows, pixels, bpp, kind in TC.model_cases(T)]


@pytest.mark.parametrize("order", ["in order", "reversed", "shuffled"])
def test_the_model_over_the_planners_sweeps_gives_the_raw_rows(drawn, order):
    how = {"in order": TC.in_order, "reversed": TC.reversed_order, "shuffled": TC.shuffled_order(7)}[order]
    for rows, pixels, bpp, kind, lines, raw in drawn:
        geo = TC.geometry(rows, pixels, T)
        _, sweeps = planner_sweeps(rows, pixels, bpp)
        got = TC.run(lines, bpp, geo, sweeps, how)
        assert np.array_equal(got, raw), (rows, pixels, bpp, kind, np.argwhere(got != raw)[:4].tolist())


MUTANT_SHAPE = (130, 300)      # three bands, several blocks at any T up to 256: every mutant has something to break


def test_a_sweep_rule_of_c_plus_b_fails():
    """Skewed tiles with d = c + b: tile (b, c) reads the last row of band b - 1 inside tile (b - 1, c + 1), which is on its own sweep."""
    rows, pixels = MUTANT_SHAPE
    geo = TC.geometry(rows, pixels, T)
    sweeps = TC.tiles_by_sweep(geo, sweep_rule=lambda band, block: band + block)
    count, owner = ownership(geo, sweeps)
    assert (count == 1).all() and not reads_are_earlier(geo, sweeps, owner)
    lines, raw = TC.draw_segment(np.random.RandomState(1), rows, pixels, 1, 4)
    assert not np.array_equal(TC.run(lines, 1, geo, sweeps, TC.in_order), raw)
    assert np.array_equal(TC.run(lines, 1, geo, TC.tiles_by_sweep(geo), TC.in_order), raw)      # the control: the stated rule on the same case


def test_blocks_of_32_pixels_fail():
    """T = 32 is below the 63 pixels of skew: the row above a tile reaches into a tile of the tile's own sweep."""
    rows, pixels = MUTANT_SHAPE
    geo = TC.geometry(rows, pixels, 32)
    sweeps = TC.tiles_by_sweep(geo)
    count, owner = ownership(geo, sweeps)
    assert (count == 1).all() and not reads_are_earlier(geo, sweeps, owner)
    lines, raw = TC.draw_segment(np.random.RandomState(2), rows, pixels, 1, 4)
    assert not np.array_equal(TC.run(lines, 1, geo, sweeps, TC.in_order), raw)


def test_a_dropped_last_block_fails():
    """blocks = ceil(P / T) forgets the skew: the lower lanes' last pixels have no owner."""
    rows, pixels = MUTANT_SHAPE[0], 2 * T + 1
    geo = TC.geometry(rows, pixels, T)
    assert geo.blocks - 1 >= 1
    sweeps = TC.tiles_by_sweep(geo, blocks=geo.blocks - 1)
    count, _ = ownership(geo, sweeps)
    assert (count == 0).any() and (count <= 1).all()
    lines, raw = TC.draw_segment(np.random.RandomState(3), rows, pixels, 1, 4)
    assert not np.array_equal(TC.run(lines, 1, geo, sweeps, TC.in_order), raw)


def test_refused_arguments_of_the_planner():
    lib = L.load_library()
    plan = (ctypes.c_int32 * 5)(*[0x5A5A5A5A] * 5)
    before = list(plan)
    for args in ((0, 12, 3), (-1, 12, 3), (5, 0, 3), (5, -3, 3), (5, 12, 5), (5, 12, 0), (5, 12, 7), (5, 13, 3), (5, (1 << 30) + 8, 8)):
        assert lib.radnet_png_plan_tiles(*args, plan) == ERR_ARG, args
        assert lib.radnet_png_tiles_on_sweep(*args, 0, None, 0) == ERR_ARG, args
    assert lib.radnet_png_plan_tiles(5, 12, 3, None) == ERR_ARG and list(plan) == before
    assert lib.radnet_png_plan_tiles(5, 12, 3, plan) == 0 and list(plan) == [1, -(-(4 + 63) // T), -(-(4 + 63) // T), 64, T]
    assert lib.radnet_png_plan_tiles(5, 1 << 30, 8, plan) == 0
    rows, rowbytes, bpp = 130, 3 * (2 * T + 1), 3
    sweeps = png.plan_tiles(rows, rowbytes, bpp).sweeps
    pairs = np.full((8, 2), 0x5A5A5A5A, np.int32)
    fn = lib.radnet_png_tiles_on_sweep
    for sweep, cap, out in ((-1, 8, pairs), (sweeps, 8, pairs), (0, -1, pairs), (0, 1, None)):
        assert fn(rows, rowbytes, bpp, sweep, None if out is None else out.ctypes.data, cap) == ERR_ARG, (sweep, cap)
    assert (pairs == 0x5A5A5A5A).all()
    n = fn(rows, rowbytes, bpp, 2, None, 0)                              # the count alone
    assert n == 2 and fn(rows, rowbytes, bpp, 2, pairs.ctypes.data, 1) == 2
    assert pairs[0].tolist() == [0, 2] and (pairs[1:] == 0x5A5A5A5A).all()      # cap entries and no more
    with pytest.raises(ValueError, match="radnet_png_plan_tiles"):
        png.plan_tiles(5, 13, 3)
    with pytest.raises(ValueError, match="radnet_png_tiles_on_sweep"):
        png.tiles_on_sweep(5, 12, 3, 99)


def test_an_unknown_unfilter_raises_without_a_device(tmp_path, monkeypatch):
    for call in (lambda: png.decode_device(b"", unfilter="bogus"), lambda: png.decode_device_many([b""], unfilter="bogus"),
                 lambda: png.decode_device(b"", inflate="device", unfilter="tile"), lambda: utils_io.DeviceImageLoader(unfilter="bogus")):
        with pytest.raises(ValueError, match="unfilter="):
            call()
    monkeypatch.chdir(tmp_path)
    os.makedirs("maps/rgb")
    with open("maps/rgb/a.png", "wb") as f:
        f.write(b"not a png")
    with pytest.raises(ValueError, match="unfilter="):
        utils_io.get_image("maps/a.png", ["rgb"], unfilter="bogus")
    from faster_rcnn.RADNet import RADNet
    assert RADNet.png_unfilter == "band" and utils_io.DeviceImageLoader().unfilter == "band"


# ---- the planner under sanitizers ---------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_tile_planner_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "png_tiles_plan_sanitize")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "rock-art-radnet_amd", "csrc", "png_plan.cpp"),
           os.path.join(ROOT, "tests", "native", "png_tiles_plan_sanitize.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    # the sanitizer runtimes are linked statically: the program needs no place in the library list and the environment stays as it is
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
