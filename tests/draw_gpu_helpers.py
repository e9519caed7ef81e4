"""What the GPU tests of the painters share (tests/test_gpu_png_write.py, test_gpu_draw_list.py, test_gpu_draw_scene.py,
test_gpu_heat.py): the noise canvas with sentinels in its pitch padding, the expected buffer from a NumPy painter, the raw call of an
entry on a copy of the buffer, and the byte comparison of the two.  A plain module like the *_cases.py ones; it needs torch and a GPU."""
import collections

import numpy as np
import torch

import draw_list_cases as D
import draw_scene_cases as S
import png_write_cases as W

SENTINEL = 0xA5
ERR_ARG = -1

# an entry over radnet_prim tables, how the tests' tuples become its rows and pool, and its NumPy painter
Front = collections.namedtuple("Front", "entry pack paint")
LIST = Front("radnet_draw_list_u8", D.pack, D.paint_list)
SCENE = Front("radnet_draw_scene_u8", S.pack, S.paint_scene)


def canvas(h, w, pad, seed=0):
    """A noise image in a buffer of h rows of 3 * w + pad bytes, sentinels in the padding."""
    buf = np.full((h, 3 * w + pad), SENTINEL, np.uint8)
    buf[:, :3 * w] = np.random.RandomState(seed).randint(0, 256, (h, 3 * w))
    return buf


def expected(paint, buf, h, w, *args):
    """The buffer after paint(image, *args) -- W.paint, D.paint_list or S.paint_scene -- on its h x w image; the padding stays."""
    want = buf.copy()
    img = want[:, :3 * w].reshape(h, w, 3).copy()
    paint(img, *args)
    want[:, :3 * w] = img.reshape(h, 3 * w)
    return want


def raw_call(ctx, entry, buf, h, w, pitch, table, before=(), after=(), count=None, handle=True, img=True, host=True, dev=True):
    """entry(context, image, h, w, pitch, *before, host table, device table, count, *after) on a copy of the host buffer `buf` (h rows
    of `pitch` bytes): (rc, message, the buffer afterwards).  `table` is a structured array; the keywords withhold a pointer or
    replace the count.  Device memory behind the pointers in `before` and `after` is the caller's to keep alive."""
    img_dev = torch.from_numpy(buf.copy()).cuda()
    table_dev = torch.from_numpy(table.view(np.uint8).copy()).cuda() if len(table) else torch.zeros(32, dtype=torch.uint8, device="cuda")
    rc = getattr(ctx.lib, entry)(ctx.h if handle else None, img_dev.data_ptr() if img else None, h, w, pitch, *before,
                                 table.ctypes.data if host and len(table) else None, table_dev.data_ptr() if dev else None,
                                 len(table) if count is None else count, *after)
    msg = ctx.lib.radnet_last_error(ctx.h)
    ctx.sync()
    return rc, (msg.decode() if msg else ""), img_dev.cpu().numpy()


def rects_call(ctx, R, buf, h, w, pitch, rects, **kw):
    """radnet_draw_rects_u8 through raw_call."""
    return raw_call(ctx, "radnet_draw_rects_u8", buf, h, w, pitch, np.array([tuple(r) for r in rects], R.RECT).reshape(-1), **kw)


def prims_call(ctx, R, entry, buf, h, w, pitch, rows, pool=b"", n_chars=None, chars_host=True, chars_dev=True, **kw):
    """radnet_draw_list_u8 or radnet_draw_scene_u8 through raw_call, with the character pool behind the table."""
    chars = np.frombuffer(bytes(pool), np.uint8).copy()
    pool_dev = torch.from_numpy(chars).cuda() if len(chars) else torch.zeros(4, dtype=torch.uint8, device="cuda")
    after = (chars.ctypes.data if chars_host and len(chars) else None, pool_dev.data_ptr() if chars_dev and len(chars) else None,
             len(chars) if n_chars is None else n_chars)
    return raw_call(ctx, entry, buf, h, w, pitch, np.array([tuple(r) for r in rows], R.PRIM).reshape(-1), after=after, **kw)


def check(ctx, R, front, font, buf, h, w, pad, prims, what):
    """The front's entry on `prims` equals its painter on the whole buffer; returns the buffer."""
    rows, pool = front.pack(prims)
    rc, msg, got = prims_call(ctx, R, front.entry, buf, h, w, 3 * w + pad, rows, pool)
    assert rc == 0, (what, msg)
    want = expected(front.paint, buf, h, w, prims, font)
    assert np.array_equal(got, want), (what, (h, w), pad, np.argwhere(got != want)[:4].tolist())
    return got
