"""The pictures the reference draws with matplotlib and cv2's drawing calls, as scenes for radnet_draw_scene_u8 (RADNet.draw_scene_device):
lines, discs, rectangles and text painted in list order in ONE launch, translucent entries mixing with what lies under them.

  * the precision/recall figure of the test driver (test.py:231-256): precision_recall_scene lays it out on the host,
    precision_recall_figure paints it on the device; evaluate.evaluate_scans(pr_plot=True) writes it to viz/precision_recall.png;
  * the label sanity views of test_data.py:214-318: positive_anchor_view and ground_truth_view.

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
