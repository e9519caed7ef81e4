"""Host-side checks of the device-image predict path: radnet_resize_bicubic_window_u8 is declared with its signature and bound with
matching argument types, and the tile descriptions RADNet.predict builds for a device image (RADNet.ImageWindow, from _spans) are
the index ranges of the reference's tiler arithmetic (RADNet.py:519-540) with the shape -- hence the ratio and the target size
-- of the copied tile.  No GPU; the kernel is tested in test_gpu_resize_window.py, the path in test_gpu_predict_device_image.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from radnet_hip import lib as L

NAME = "radnet_resize_bicubic_window_u8"
PARAMS = [("radnet_ctx*", "ctx"), ("const uint8_t*", "src"), ("int32_t", "sh"), ("int32_t", "sw"), ("int32_t", "y0"), ("int32_t", "x0"),
          ("int32_t", "wh"), ("int32_t", "ww"), ("uint8_t*", "dst"), ("int32_t", "dh"), ("int32_t", "dw"), ("int32_t", "channels")]


def test_header_declares_the_window_resize_with_its_signature():
    assert NAME in L.declared_symbols()
    text = re.sub(r"/\*.*?\*/", "", open(L.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, text)
    assert m is not None
    got = []
    for p in m.group(1).split(","):
        words = p.replace("*", "* ").split()
        got.append((" ".join(words[:-1]).replace(" *", "*"), words[-1]))
    assert got == PARAMS


def test_binding_argument_types_match_the_header():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    fn = getattr(L.load_library(), NAME)
    want = [ctypes.c_int32 if t == "int32_t" else ctypes.c_void_p for t, _ in PARAMS]
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == want
    # the argument checks need no device: a null context is refused before anything else is looked at
    assert fn(None, 1, 4, 4, 0, 0, 2, 2, 1, 2, 2, 3) != 0


# ---- the tile descriptions ------------------------------------------------------------------------------------------------
def reference_tiles(h, w, tile, step):
    """The reference's tiler arithmetic (RADNet.py:519-540), restated without NumPy: window starts every `step` along each axis, the windows
    that fit, one window flush with the far edge, duplicates dropped, sorted; tiles enumerated rows outer, columns inner."""
    def axis(n):
        pairs = set()
        for s in range(0, n, step):
            if s + tile <= n:
                pairs.add((s, s + tile))
        pairs.add((max(0, n - tile), n))
        return sorted(pairs)
    return [(y0, y1, x0, x1) for (y0, y1) in axis(h) for (x0, x1) in axis(w)]


class Shape:
    """Stands in for the image: tile_windows looks at .shape alone."""
    def __init__(self, h, w):
        self.shape = (h, w, 3)


def cfg(tile, step, full, tiles=1, img_size=300):
    from faster_rcnn.config import Config
    C = Config()
    C.tile_size, C.tile_overlap, C.include_full_img, C.max_n_tiles_train, C.img_size = tile, step, full, tiles, img_size
    return C


GEOMETRIES = [(700, 900, 400, 250), (4000, 4000, 2000, 400), (400, 400, 400, 250), (233, 310, 400, 250), (401, 399, 400, 1), (1000, 650, 300, 300),
              (300, 300, 400, 250)]          # one tile, already at img_size: handed on as it is


@pytest.mark.parametrize("h,w,tile,step", GEOMETRIES)
def test_windows_are_the_reference_tiles(h, w, tile, step):
    from faster_rcnn.RADNet import ImageWindow, RADNet, tile_windows
    img = Shape(h, w)
    C = cfg(tile, step, full=True)
    work, offs = tile_windows(img, C, ready="ev")
    ref = reference_tiles(h, w, tile, step)
    assert len(work) == len(offs) == len(ref) + 1
    if (h, w, tile, step) == (4000, 4000, 2000, 400):
        assert len(ref) == 36
    host = np.zeros((h, w, 3), np.uint8)
    net = RADNet(C, None, None, None)
    for win, off, (y0, y1, x0, x1) in zip(work, offs, ref):
        assert isinstance(win, ImageWindow) and win.img is img and win.ready == "ev"
        assert (win.y0, win.y0 + win.wh, win.x0, win.x0 + win.ww) == (y0, y1, x0, x1) and off == (x0, y0)
        assert 0 <= win.y0 and win.y0 + win.wh <= h and 0 <= win.x0 and win.x0 + win.ww <= w and win.wh >= 1 and win.ww >= 1
        copied = np.copy(host[y0:y1, x0:x1, :])                        # the host path's tile
        assert win.shape == copied.shape
        assert plan(net, win) == plan(net, copied)
    full = work[-1]
    assert (full.x0, full.y0, full.ww, full.wh) == (0, 0, w, h) and offs[-1] == (0, 0) and full.covers_image()
    assert plan(net, full) == plan(net, host)
    assert [w_.covers_image() for w_ in work[:-1]] == [(y1 - y0, x1 - x0) == (h, w) for (y0, y1, x0, x1) in ref]
    # without the full-image pass, and with tiling gated off (RADNet.py:511)
    assert len(tile_windows(img, cfg(tile, step, full=False))[0]) == len(ref)
    work, offs = tile_windows(img, cfg(tile, step, full=True, tiles=0))
    assert len(work) == 1 and work[0].covers_image() and offs == [(0, 0)]
    assert tile_windows(img, cfg(tile, step, full=False, tiles=0)) == ([], [])


def plan(net, tile):
    """(ratio, new_w, new_h) format_img_size derives from tile.shape: its resize is intercepted, nothing runs."""
    import faster_rcnn.RADNet as R
    seen = []
    saved = R.resize_cubic, R.resize_cubic_window
    R.resize_cubic = lambda img, new_w, new_h, **kw: seen.append((new_w, new_h)) or "resized"
    R.resize_cubic_window = lambda img, x0, y0, ww, wh, new_w, new_h, **kw: seen.append((new_w, new_h)) or "resized"
    try:
        t = R.ImageWindow(tile.img, tile.x0, tile.y0, tile.ww, tile.wh) if isinstance(tile, R.ImageWindow) else tile
        out, ratio = net.format_img_size(t, keep_on_device=True)
    finally:
        R.resize_cubic, R.resize_cubic_window = saved
    if not seen:                                                        # handed on as it is: already at the target size
        assert out is (t.img if isinstance(t, R.ImageWindow) else t)
        h, w = tile.shape[:2]
        seen.append((w, h))
    return (ratio,) + seen[0]


def test_window_is_refused_on_the_host_resize_path():
    from faster_rcnn.RADNet import ImageWindow, RADNet
    net = RADNet(cfg(400, 250, True), None, None, None)
    with pytest.raises(TypeError):
        net.format_img_size(ImageWindow(Shape(700, 900), 0, 0, 400, 400))
