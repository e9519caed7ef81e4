"""The pictures the reference draws with matplotlib and cv2's drawing calls, as scenes for radnet_draw_scene_u8 (RADNet.draw_scene_device):
lines, discs, rectangles and text painted in list order in ONE launch, translucent entries mixing with what lies under them.

  * the precision/recall figure of the test driver (test.py:231-256): precision_recall_scene lays it out on the host,
    precision_recall_figure paints it on the device; evaluate.evaluate_scans(pr_plot=True) writes it to viz/precision_recall.png;
  * the label sanity views of test_data.py:214-318: positive_anchor_view and ground_truth_view;
  * the score-map views of train.py:338-347 and RADNet.py:362-367 (imshow + colorbar per anchor): score_map_figure, and what they
    were looked at for, the RPN's objectness over a whole scan: objectness_view over RADNet.objectness_maps.  These go through
    radnet_heat_paint_u8 (RADNet.heat_paint_device): uint8 level maps through a colour table, nearest cells, the package's own ramp.

What differs from the reference's pictures, on purpose and unpinned: the text is the package's own dot-matrix font (no Hershey, no
TrueType, and NO ROTATED TEXT: the precision label stands horizontally above the top-left corner of the axes, where matplotlib writes it
upwards along the axis); lines are not anti-aliased and have no caps; the legend always sits in the lower left corner of the axes
(matplotlib picks the emptiest corner); discs are radnet_draw_scene_u8's, not cv2's midpoint circles; the blend rounds an integer
quotient where cv2.addWeighted rounds a float.  Colours are given as (b, g, r), the order of the package's images."""
import numpy as np

# matplotlib's default colour cycle ('tab10'), in order, as (b, g, r)
COLOUR_CYCLE = [(180, 119, 31), (14, 127, 255), (44, 160, 44), (40, 39, 214), (189, 103, 148), (75, 86, 140), (194, 119, 227), (127, 127, 127),
                (34, 189, 188), (207, 190, 23)]
# test_data.py:220-226, (light, dark) per pair; the reference gives them as (r, g, b)
COLORMAP = [((227, 206, 166), (180, 120, 31)), ((138, 223, 178), (44, 160, 51)), ((153, 154, 251), (28, 26, 227)), ((111, 191, 253), (0, 127, 255)),
            ((214, 178, 202), (154, 61, 106))]
GROUND_TRUTH_BGR = (28, 26, 227)      # test_data.py:276 paints (227, 26, 28) into an RGB copy
BLACK, WHITE = (0, 0, 0), (255, 255, 255)
LEGEND_TRANSPARENCY = 51              # matplotlib's legend.framealpha of 0.8: 255 - round(255 * 0.8)


def figure_layout(size=1200):
    """Where the parts of the size x size figure stand, in pixels: the axes box [x0, x1] x [y0, y1] (matplotlib's default subplot
    margins), the text scale, the curves' thickness and dash, the tick length."""
    n = int(size)
    if n < 120:
        raise ValueError("precision_recall_scene: a figure of %d pixels has no room for its labels" % n)
    unit = max(1, n // 600)
    return dict(size=n, x0=int(round(0.125 * n)), x1=int(round(0.9 * n)), y0=int(round(0.12 * n)), y1=int(round(0.89 * n)), scale=max(1, n // 400), thickness=unit,
                dash=(6 * unit, 4 * unit), tick=max(2, n // 200), frame=unit)


def to_pixels(values, first, count, flip=False):
    """Data in [0, 1] to the pixels first .. first + count - 1: floor(v * (count - 1) + 0.5) in float64, clamped to the axis
    (matplotlib clips at the limits); flip counts from the far end (the image's rows grow downwards)."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    k = np.clip(np.floor(np.clip(np.nan_to_num(v), 0.0, 1.0) * (count - 1) + 0.5).astype(np.int64), 0, count - 1)
    return first + (count - 1 - k if flip else k)


def polyline(xs, ys, thickness, colour, dash=None):
    """The line entries through the pixel points (xs[i], ys[i]): consecutive points on the same pixel are dropped, so no two
    consecutive entries are identical; a single point is one entry of a point."""
    pts = [(int(x), int(y)) for x, y in zip(xs, ys)]
    pts = [p for k, p in enumerate(pts) if k == 0 or p != pts[k - 1]]
    opts = ({"dash": tuple(dash)},) if dash else ()
    if len(pts) == 1:
        pts = pts * 2
    return [("line", a[0], a[1], b[0], b[1], thickness) + tuple(colour) + opts for a, b in zip(pts[:-1], pts[1:])]


def _text_width(text, scale):
    return max(0, 6 * len(text) - 1) * scale


def precision_recall_scene(curves, mAP, size=1200):
    """The primitive list (RADNet.scene_table's tuples) of the figure of test.py:231-256 on a white size x size canvas.  Host only.
    curves = {class: (ap, precision, recall, interpolated_precision, interpolated_recall)}, what evaluate.calc_class_ap returns; mAP
    and ap are fractions, printed as percentages with two decimals like the reference.  Axes from 0 to 1 with ticks and tick labels
    every 0.2, 'Recall (TP / TP + FN)' below, 'Precision (TP / TP + FP)' horizontally above the top-left corner, the title
    'mAP: {0:.2f} %' above that; per class in sorted order the measured curve solid and the interpolated one dashed in the next colour
    of COLOUR_CYCLE (wrapping), and a legend line 'key: {0:.2f} %'."""
    L = figure_layout(size)
    x0, x1, y0, y1, s, t = L["x0"], L["x1"], L["y0"], L["y1"], L["scale"], L["thickness"]
    nx, ny = x1 - x0 + 1, y1 - y0 + 1
    prims = []
    for k in range(6):                                                       # ticks and their labels at 0.0, 0.2 .. 1.0
        label = "%.1f" % (k / 5)
        px, py = int(to_pixels([k / 5], x0, nx)[0]), int(to_pixels([k / 5], y0, ny, flip=True)[0])
        prims.append(("line", px, y1, px, y1 + L["tick"], L["frame"]) + BLACK)
        prims.append(("text", px - _text_width(label, s) // 2, y1 + L["tick"] + 9 * s, label, s) + BLACK)
        prims.append(("line", x0 - L["tick"], py, x0, py, L["frame"]) + BLACK)
        prims.append(("text", x0 - L["tick"] - 2 * s - _text_width(label, s), py + 3 * s, label, s) + BLACK)
    xlabel, ylabel, title = "Recall (TP / TP + FN)", "Precision (TP / TP + FP)", "mAP: " + "{0:.2f}".format(100 * mAP) + " %"
    prims.append(("text", (x0 + x1) // 2 - _text_width(xlabel, s) // 2, y1 + L["tick"] + 22 * s, xlabel, s) + BLACK)
    prims.append(("text", x0, y0 - 3 * s, ylabel, s) + BLACK)
    prims.append(("text", (x0 + x1) // 2 - _text_width(title, s) // 2, y0 - 14 * s, title, s) + BLACK)
    keys = sorted(curves.keys())
    for k, key in enumerate(keys):
        colour = COLOUR_CYCLE[k % len(COLOUR_CYCLE)]
        ap, precision, recall, interp_precision, interp_recall = curves[key]
        if len(recall):
            prims += polyline(to_pixels(recall, x0, nx), to_pixels(precision, y0, ny, flip=True), t, colour)
        if len(interp_recall):
            prims += polyline(to_pixels(interp_recall, x0, nx), to_pixels(interp_precision, y0, ny, flip=True), t, colour, L["dash"])
    prims.append(("rect", x0, y0, x1, y1, L["frame"]) + BLACK)               # the axes box, over the curves' ends
    if keys:                                                                 # the legend: a frame, then per class a line sample and its text
        lines = [key + ": " + "{0:.2f}".format(100 * curves[key][0]) + " %" for key in keys]
        sample, row, pad = 12 * s, 11 * s, 4 * s
        lw, lh = pad + sample + 3 * s + max(_text_width(v, s) for v in lines) + pad, pad + row * len(lines) + pad - 2 * s
        lx, ly = x0 + 6 * s, y1 - 6 * s - lh
        prims.append(("rect", lx, ly, lx + lw, ly + lh, -1) + WHITE + ({"transparency": LEGEND_TRANSPARENCY},))
        prims.append(("rect", lx, ly, lx + lw, ly + lh, 1) + (204, 204, 204))
        for k, text in enumerate(lines):
            base = ly + pad + row * k + 7 * s
            prims.append(("line", lx + pad, base - 3 * s, lx + pad + sample, base - 3 * s, t) + COLOUR_CYCLE[k % len(COLOUR_CYCLE)])
            prims.append(("text", lx + pad + sample + 3 * s, base, text, s) + BLACK)
    return prims


def precision_recall_figure(curves, mAP, size=1200, ctx=None):
    """precision_recall_scene painted on the device: a white uint8 [size][size][3] cuda tensor made there and ONE
    radnet_draw_scene_u8 launch.  Returns the device image (utils_io.imwrite writes it)."""
    import torch
    from . import RADNet as R
    prims = precision_recall_scene(curves, mAP, size)
    canvas = torch.full((int(size), int(size), 3), 255, dtype=torch.uint8, device="cuda")
    return R.draw_scene_device(canvas, prims, inplace=True, ctx=ctx)


# ---- score maps: the imshow + colorbar views of train.py:338-347 and RADNet.py:362-367, and the objectness of a whole scan ------------
# (level, b, g, r): the package's own ramp from dark violet over blue and green to yellow, rising in luma so that it reads in grey
# too.  It follows the idea of matplotlib's viridis and is unpinned against it: not its table, not its 256 colours.
HEAT_ANCHORS = ((0, 84, 4, 68), (85, 140, 90, 50), (170, 100, 180, 60), (255, 40, 230, 250))


def heat_lut(anchors=HEAT_ANCHORS):
    """The 256 x 3 uint8 (b, g, r) colour table of radnet_heat_paint_u8, interpolated in integers between the (level, b, g, r)
    anchors: (c0 * (l1 - l) + c1 * (l - l0) + (l1 - l0) // 2) // (l1 - l0) for l0 <= l <= l1.  The anchors' levels rise strictly
    from 0 to 255."""
    anchors = [tuple(int(v) for v in a) for a in anchors]
    levels = [a[0] for a in anchors]
    if len(anchors) < 2 or levels[0] != 0 or levels[-1] != 255 or any(b <= a for a, b in zip(levels[:-1], levels[1:])):
        raise ValueError("heat_lut: the anchors' levels must rise strictly from 0 to 255, not %r" % (levels,))
    if any(len(a) != 4 or not all(0 <= c <= 255 for c in a[1:]) for a in anchors):
        raise ValueError("heat_lut: an anchor is (level, b, g, r) with colours in 0..255")
    lut = np.zeros((256, 3), np.uint8)
    for (l0, *c0), (l1, *c1) in zip(anchors[:-1], anchors[1:]):
        for level in range(l0, l1 + 1):
            lut[level] = [(a * (l1 - level) + b * (level - l0) + (l1 - l0) // 2) // (l1 - l0) for a, b in zip(c0, c1)]
    return lut


def to_levels(values):
    """radnet_score_levels_u8's level rule for host arrays: clamp(floor(v * 255 + 0.5), 0, 255) with the product and the sum each
    rounded to float32; NaN gives 0.  uint8, the shape of `values`."""
    v = np.asarray(values, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.floor((v * np.float32(255.0)).astype(np.float32) + np.float32(0.5))
    return np.where(t >= 0, np.minimum(t, np.float32(255.0)), np.float32(0.0)).astype(np.uint8)      # NaN compares false


def objectness_view(img, maps, transparency=102, min_level=0, grey=True, lut=None, ctx=None):
    """The RPN's objectness over a scan: a grey copy of `img` (radnet_grey3_u8; grey=False: a plain copy) with the maps of
    RADNet.objectness_maps(img) laid over their windows in ONE radnet_heat_paint_u8 launch -- where windows overlap the larger
    level shows, a cell covers its share of the window (nearest cells, no interpolation), levels below min_level leave the scan
    visible.  Returns a new device image; img (a cuda tensor, or a NumPy array, which is uploaded) stays as it was."""
    from . import RADNet as R
    if tuple(img.shape[:2]) != tuple(maps.shape):
        raise ValueError("objectness_view: maps of a %s scan over an image of %s" % (tuple(maps.shape), tuple(img.shape[:2])))
    base = R.grey3_device(img, ctx=ctx) if grey else img                  # grey3_device makes a new image, heat_paint_device a clone
    return R.heat_paint_device(base, maps.pool, maps.places, lut=lut, transparency=transparency, min_level=min_level, inplace=bool(grey), ctx=ctx)


def score_map_scene(shape, title="", size=600):
    """Where the parts of the size x size score-map figure stand, for a map of shape (mh, mw).  Host only.  Returns a dict:
    `map` and `bar`, the destination rectangles (x0, y0, w, h) of the map -- the largest one of the map's aspect ratio inside the
    axes area, centred in it -- and of the colour bar to its right, as tall as the map; `prims`, the scene list painted over
    them: the two frames, the bar's ticks and labels 0.0 .. 1.0 (1.0 at the top) and the title, centred above the map."""
    mh, mw = (int(v) for v in shape)
    n = int(size)
    if mh < 1 or mw < 1:
        raise ValueError("score_map_scene: a map of %d x %d" % (mh, mw))
    if n < 120:
        raise ValueError("score_map_scene: a figure of %d pixels has no room for its labels" % n)
    unit, s = max(1, n // 600), max(1, n // 300)
    ax0, ax1, ay0, ay1 = int(round(0.08 * n)), int(round(0.72 * n)), int(round(0.14 * n)), int(round(0.92 * n))
    aw, ah = ax1 - ax0, ay1 - ay0
    if aw * mh <= ah * mw:                                   # the width binds
        w, h = aw, max(1, (aw * mh + mw // 2) // mw)
    else:
        w, h = max(1, (ah * mw + mh // 2) // mh), ah
    x0, y0 = ax0 + (aw - w) // 2, ay0 + (ah - h) // 2
    bx0, bw = int(round(0.78 * n)), max(2, int(round(0.04 * n)))
    tick = max(2, n // 200)
    prims = [("rect", x0 - unit, y0 - unit, x0 + w - 1 + unit, y0 + h - 1 + unit, unit) + BLACK,
             ("rect", bx0 - unit, y0 - unit, bx0 + bw - 1 + unit, y0 + h - 1 + unit, unit) + BLACK]
    for k in range(6):
        label = "%.1f" % (k / 5)
        py = int(to_pixels([k / 5], y0, h, flip=True)[0])
        prims.append(("line", bx0 + bw, py, bx0 + bw + tick, py, unit) + BLACK)
        prims.append(("text", bx0 + bw + tick + 2 * s, py + 3 * s, label, s) + BLACK)
    if title:
        prims.append(("text", max(0, x0 + w // 2 - _text_width(str(title), s) // 2), max(8 * s, y0 - 4 * s - unit), str(title), s) + BLACK)
    return dict(size=n, map=(x0, y0, w, h), bar=(bx0, y0, bw, h), prims=prims)


def score_map_figure(values, title="", size=600, lut=None, ctx=None):
    """The imshow + colorbar view of one score map (train.py:338-347, RADNet.py:362-367) on the device: `values`, a [mh][mw] array
    of scores in [0, 1] (say Y1[0, :, :, i]), through to_levels; a white size x size canvas; ONE radnet_heat_paint_u8 launch that
    places the map in the axes box (aspect ratio kept, nearest cells) and a 256-level ramp beside it as the colour bar; ONE
    radnet_draw_scene_u8 launch for the frames, the ticks and the title (score_map_scene).  Returns the device image
    (utils_io.imwrite writes it).  Not matplotlib's picture: the package's own ramp and font, no interpolation, no window."""
    import torch
    from . import RADNet as R
    levels = to_levels(values.cpu().numpy() if hasattr(values, "cpu") else values)
    if levels.ndim != 2:
        raise ValueError("score_map_figure: a map has rank 2, not %d" % levels.ndim)
    mh, mw = levels.shape
    scene = score_map_scene((mh, mw), title, size)
    pool = np.concatenate([levels.reshape(-1), np.arange(255, -1, -1, dtype=np.uint8)])      # the bar: 256 rows of one level, 255 on top
    places = [scene["map"] + (mw, mh, 0), scene["bar"] + (1, 256, mh * mw)]
    canvas = torch.full((scene["size"], scene["size"], 3), 255, dtype=torch.uint8, device="cuda")
    canvas = R.heat_paint_device(canvas, pool, places, lut=lut, inplace=True, ctx=ctx)
    return R.draw_scene_device(canvas, scene["prims"], inplace=True, ctx=ctx)


def positive_anchor_scene(Y, C, n_pos):
    """test_data.py:284-308 as primitives: per positive anchor i a filled disc of radius 3 at its centre and the anchor's box with
    thickness 2, both in the light colour of COLORMAP[i % 5].  Y = [y_rpn_cls, y_rpn_regr] as the tile generator yields them
    (1, H, W, channels); the positives are where y_rpn_regr == 1, four channels per anchor, as the reference reads them."""
    regr = np.asarray(Y[1].cpu() if hasattr(Y[1], "cpu") else Y[1])[0]
    rows, cols, chans = np.where(regr == 1)
    ratios = C.anchor_box_ratios
    prims = []
    for i in range(int(n_pos)):
        colour = COLORMAP[i % len(COLORMAP)][0]
        idx = chans[i * 4] / 4
        anchor_size = C.anchor_box_scales[int(idx / len(ratios))]
        anchor_ratio = ratios[int(idx % len(ratios))]
        cx, cy = int(cols[i * 4] * C.rpn_stride), int(rows[i * 4] * C.rpn_stride)
        half_w, half_h = int(anchor_size * anchor_ratio[0] / 2), int(anchor_size * anchor_ratio[1] / 2)
        prims.append(("disc", cx, cy, 3, -1) + colour)
        prims.append(("rect", cx - half_w, cy - half_h, cx + half_w, cy + half_h, 2) + colour)
    return prims


def positive_anchor_view(img, Y, C, n_pos, ctx=None):
    """The positive-anchor view of test_data.py:284-308 on the device: a grey copy of the (b, g, r) tile `img` (a cuda tensor or a
    NumPy array, which is uploaded) by radnet_grey3_u8, then positive_anchor_scene in one scene launch.  Returns a new device image."""
    from . import RADNet as R
    grey = R.grey3_device(img, ctx=ctx)
    return R.draw_scene_device(grey, positive_anchor_scene(Y, C, n_pos), inplace=True, ctx=ctx)


def ground_truth_scene(bboxes, alpha=0.6):
    """test_data.py:271-280 as primitives: per box an outline of thickness 3 in GROUND_TRUTH_BGR with transparency
    255 - round(255 * alpha).  The reference blends an outlined copy over the whole image once per box, with weights alpha and
    1 - alpha that sum to one: off the outline that changes nothing, on it this is the same mix, up to addWeighted's float rounding."""
    if not 0.0 <= alpha <= 1.0:
        raise ValueError("ground_truth_view: alpha = %r" % (alpha,))
    tau = 255 - int(round(255 * alpha))
    return [("rect", int(b['x1']), int(b['y1']), int(b['x2']), int(b['y2']), 3) + GROUND_TRUTH_BGR + ({"transparency": tau},) for b in bboxes]


def ground_truth_view(img, bboxes, alpha=0.6, ctx=None):
    """The blended ground-truth view of test_data.py:271-280 in one scene launch; `bboxes` are dicts with x1, y1, x2, y2 in the
    pixels of `img` (a cuda tensor, or a NumPy array, which is uploaded).  Returns a new device image; img stays as it was."""
    from . import RADNet as R
    return R.draw_scene_device(img, ground_truth_scene(bboxes, alpha), ctx=ctx)
