"""Detector facade with the reference's construct / predict surface (faster_rcnn/RADNet.py).

    RADNet(C, model_rpn, model_detector, preprocess_func)              RADNet.py:33-41
    .predict(images) -> [{'class','prob','x1','y1','x2','y2'}, ...]     RADNet.py:502-718
    .predict_from_path(path)                                           RADNet.py:482-500
    .draw_detections(img, dets) / .write_predictions(dets, img, dir)   predict.py:90-181 (boxes and files; no text labels)
    .predict_region_proposals(img) / .objectness_maps(img)             RADNet.py:310-480 (the RPN alone; score maps as levels)
    .format_img / .apply_spatial_pyramid_pooling / .final_nms / .get_real_coordinates
    .predict_device(images) / .final_nms_device / .scan_tail                the merge of a scan on the device (csrc/scan_tail.hip)
    load_radnet(config_path)                                           RADNet.py:721-775

The model objects are duck-typed exactly as in the reference (anything with .predict works, which is how the
golden tests drive this class with closed-form fake models); load_radnet() builds them on the HIP engine.
NMS runs in libradnet_hip.so through faster_rcnn.rpn; the tile resize runs on the device (radnet_resize_bicubic_u8, or for an
image that is already there radnet_resize_bicubic_window_u8: tile cut + resize in one launch, see ImageWindow).
"""
import pickle
import sys

import numpy as np

from . import rpn
from .utils import get_new_img_size  # noqa: F401  (re-exported like the reference's star import)


def _spans(length, tile, step):
    """Sliding-window spans along one axis (RADNet.py:519-535): starts every `step`, windows that fit, plus one
    window flush with the far edge; duplicates removed, sorted."""
    starts = np.arange(0, length, step)
    ends = starts + tile
    ok = ends <= length
    pairs = {(int(s), int(e)) for s, e in zip(starts[ok], ends[ok])}
    pairs.add((max(0, length - tile), int(length)))
    return sorted(pairs)


class ImageWindow:
    """A tile of an image that is on the device, as a DESCRIPTION: the image and the window [y0, y0 + wh) x [x0, x0 + ww) of it,
    where the host path holds np.copy(img[y0:y0+wh, x0:x0+ww, :]) (RADNet.py:545).  `.shape` is the copied tile's, so
    format_img_size derives the same ratio, new_w and new_h from it; format_img_size(..., keep_on_device=True) turns it into one
    resize_cubic_window launch.  `ready`: an event after which the image's bytes are valid (its producer's position; None: they
    already are for every stream that will read them)."""
    __slots__ = ("img", "x0", "y0", "ww", "wh", "ready")

    def __init__(self, img, x0, y0, ww, wh, ready=None):
        self.img, self.x0, self.y0, self.ww, self.wh, self.ready = img, int(x0), int(y0), int(ww), int(wh), ready

    @property
    def shape(self):
        return (self.wh, self.ww, 3)

    def covers_image(self):
        return (self.y0, self.x0) == (0, 0) and (self.wh, self.ww) == tuple(self.img.shape[:2])


def tile_windows(img, C, ready=None):
    """The work list of one image in predict (RADNet.py:511-547, 348-350) as (windows, offsets): the tiles of _spans in the
    reference's order -- rows outer, columns inner -- when C.max_n_tiles_train > 0, then the whole image when C.include_full_img.
    Only img.shape is looked at."""
    h, w = img.shape[:2]
    spans = []
    if C.max_n_tiles_train > 0:                 # the reference gates tiling on this training knob (RADNet.py:511)
        spans = [(tx0, ty0, tx1, ty1) for (ty0, ty1) in _spans(h, C.tile_size, C.tile_overlap) for (tx0, tx1) in _spans(w, C.tile_size, C.tile_overlap)]
    work = [ImageWindow(img, tx0, ty0, tx1 - tx0, ty1 - ty0, ready) for (tx0, ty0, tx1, ty1) in spans]
    offs = [(tx0, ty0) for (tx0, ty0, tx1, ty1) in spans]
    if C.include_full_img:
        work.append(ImageWindow(img, 0, 0, w, h, ready))
        offs.append((0, 0))
    return work, offs


def _is_device_image(img):
    return not isinstance(img, np.ndarray) and bool(getattr(img, "is_cuda", False))


def check_device_image(img):
    """predict takes a device image as a uint8 [H][W][3] contiguous cuda tensor; anything else is refused here, by what is wrong."""
    import torch
    if img.dtype != torch.uint8:
        raise TypeError("predict: a device image must be uint8, not %s" % (img.dtype,))
    if img.dim() != 3:
        raise ValueError("predict: a device image must have rank 3 ([H][W][3]), not rank %d" % img.dim())
    if img.shape[2] != 3:
        raise ValueError("predict: a device image must have 3 channels ([H][W][3]), not %d" % img.shape[2])
    if img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError("predict: a device image must not be empty, shape %s" % (tuple(img.shape),))
    if not img.is_contiguous():
        raise ValueError("predict: a device image must be contiguous (strides %s for shape %s)" % (img.stride(), tuple(img.shape)))
    return img


class RADNet():

    device_resident = True      # engine-backed models: keep tiles on the device between the stages (see _detect)
    device_tail = True          # ... and decode + per-class NMS + source-pixel coordinates too (see _tail_on_device)
    png_unfilter = "band"       # predict_from_path: "tiles" reconstructs the maps' adaptive-filter rows on all CUs (png.decode_device(unfilter=))
    png_join = "host"           # predict_from_path: "device" joins the maps' IDAT payloads on the device (png.decode_device(join=); needs a device png_inflate)
    png_crc = "host"            # predict_from_path: "device" sums the maps' IDAT CRC-32s on the device (png.decode_device(crc=); needs a device png_inflate)
    png_many = False            # predict_from_path: True reads the types of C.use_img_type through ONE png.decode_device_many with the four modes below
    png_inflate = "host"        # predict_from_path: "device" / "device-lz" inflate the maps' IDAT streams on the device (png.decode_device(inflate=))
    scan_tail = False           # ... and the merge of a scan's tiles: final_nms per image, NMS across images (see _scan_tail_on)

    def __init__(self, C, model_rpn, model_detector, preprocess_func):
        self.is_object_threshold = 0.5
        self.bbox_threshold = 0.7
        self.C = C
        self.model_rpn = model_rpn
        self.model_detector = model_detector
        self.preprocess_func = preprocess_func
        self.class_mapping = {v: k for k, v in C.class_mapping.items()}

    # ---- geometry helpers ------------------------------------------------------------------------------------
    def get_real_coordinates(self, ratio, x1, y1, x2, y2):
        """Back to source-image pixels: floor-division by the resize ratio, then round (RADNet.py:44-51)."""
        return tuple(int(round(v // ratio)) for v in (x1, y1, x2, y2))

    def _network_size(self, height, width):
        """(ratio, new_w, new_h) of RADNet.py:53-74 for an image of height x width: short side -> C.img_size, long side truncated."""
        side = float(self.C.img_size)
        if width <= height:
            ratio = side / width
            return ratio, int(side), int(ratio * height)
        ratio = side / height
        return ratio, int(ratio * width), int(side)

    def format_img_size(self, img, keep_on_device=False, ctx=None):
        """Short side -> C.img_size, long side truncated (RADNet.py:53-74); bicubic resize on the device.
        keep_on_device: return the resized uint8 image as a device tensor (the device-resident tile path).  An ImageWindow (a tile
        of an image that is already on the device) becomes one resize_cubic_window launch on the lane this is called from."""
        height, width = img.shape[:2]
        ratio, new_w, new_h = self._network_size(height, width)
        if isinstance(img, ImageWindow):
            if not keep_on_device:
                raise TypeError("format_img_size: an ImageWindow is resized on the device (keep_on_device=True)")
            if img.ready is not None:
                import torch
                torch.cuda.current_stream().wait_event(img.ready)      # the lane reads the image only behind its producer
            if (new_h, new_w) == (height, width) and img.covers_image():
                return img.img, ratio                                  # propose_launch copies it into the plan's panel
            return resize_cubic_window(img.img, img.x0, img.y0, img.ww, img.wh, new_w, new_h, ctx=ctx), ratio
        if keep_on_device:
            return resize_cubic(img, new_w, new_h, to_host=False, ctx=ctx), ratio
        if (new_h, new_w) != (height, width):
            img = resize_cubic(img, new_w, new_h)
        return img, ratio

    def format_img_channels(self, img):
        img = img[:, :, (2, 1, 0)].astype(np.float32)          # BGR -> RGB (RADNet.py:83-84)
        return self.preprocess_func(np.expand_dims(img, axis=0))

    def format_img(self, img):
        img, ratio = self.format_img_size(img)
        return self.format_img_channels(img), ratio

    # ---- classifier head over the proposals -----------------------------------------------------------------------
    def apply_spatial_pyramid_pooling(self, R, feature_map):
        """RADNet.py:104-154.  R (n,4) xywh in feature-map units.  The RoIs go through the detector n_rois at a
        time, the last chunk padded with copies of its first RoI; confident non-background RoIs are decoded with
        their class's deltas and scaled to resized-image pixels."""
        chunks = self._spp_chunks(R)
        # The reference's Keras detector is built for exactly n_rois RoIs, hence its 15 calls per tile.  The HIP
        # detector takes any count (every RoI is independent under TimeDistributed), so all chunks -- padding rows
        # included, they are decoded too -- go through ONE head pass: GEMM M = 14 700 instead of 15 x 980.
        k = self.C.n_rois
        if chunks and getattr(self.model_detector, "accepts_any_roi_count", False):
            pc, pr = self.model_detector.predict([feature_map, np.concatenate(chunks, axis=1)])
            outs = [(pc[:, i * k:(i + 1) * k], pr[:, i * k:(i + 1) * k]) for i in range(len(chunks))]
        else:
            outs = [tuple(self.model_detector.predict([feature_map, ROIs])) for ROIs in chunks]
        return self._spp_decode(chunks, outs)

    def _spp_chunks(self, R):
        """RoIs n_rois at a time, the last chunk padded with copies of its first RoI (RADNet.py:110-122)."""
        k = self.C.n_rois
        chunks = []
        for start in range(0, R.shape[0], k):
            chunk = R[start:start + k, :]
            if chunk.shape[0] < k:
                padded = np.zeros((k, chunk.shape[1])).astype(chunk.dtype)
                padded[:chunk.shape[0]] = chunk
                padded[chunk.shape[0]:] = chunk[0]
                chunk = padded
            chunks.append(np.expand_dims(chunk, axis=0))
        return chunks

    def _spp_decode(self, chunks, outs):
        """Confident non-background RoIs decoded with their class's deltas, in resized-image pixels (RADNet.py:124-154)."""
        C = self.C
        stride = C.rpn_stride
        std = C.classifier_regr_std
        bboxes, probs = {}, {}
        for ROIs, (P_cls, P_regr) in zip(chunks, outs):
            for ii in range(P_cls.shape[1]):
                scores = P_cls[0, ii, :]
                best = int(np.argmax(scores))
                if np.max(scores) < self.bbox_threshold or best == P_cls.shape[2] - 1:
                    continue
                name = self.class_mapping[best]
                x, y, w, h = ROIs[0, ii, :]
                try:
                    tx, ty, tw, th = P_regr[0, ii, 4 * best:4 * (best + 1)]
                    x, y, w, h = rpn.apply_regr(x, y, w, h, tx / std[0], ty / std[1], tw / std[2], th / std[3])
                except Exception:
                    pass
                bboxes.setdefault(name, []).append([stride * x, stride * y, stride * (x + w), stride * (y + h)])
                probs.setdefault(name, []).append(np.max(scores))
        return bboxes, probs

    def final_nms(self, boxes, probs, obj_avg_threshold=0.2, obj_confidence_threshold=0.8, n_obj_avg=5):
        """RADNet.py:156-240: greedy clustering around the current best box (IoU > obj_avg_threshold); each cluster
        becomes the mean of its members above obj_confidence_threshold, or of its n_obj_avg best members."""
        if len(boxes) == 0:
            return []
        x1, y1, x2, y2 = boxes[:, 0], boxes[:, 1], boxes[:, 2], boxes[:, 3]
        np.testing.assert_array_less(x1, x2)
        np.testing.assert_array_less(y1, y2)
        if boxes.dtype.kind == "i":
            boxes = boxes.astype("float")
        area = (x2 - x1) * (y2 - y1)
        order = np.argsort(probs, kind="stable")
        clusters = []
        while len(order) > 0:
            last = len(order) - 1
            top, rest = order[last], order[:last]
            iw = np.maximum(0, np.minimum(x2[top], x2[rest]) - np.maximum(x1[top], x1[rest]))
            ih = np.maximum(0, np.minimum(y2[top], y2[rest]) - np.maximum(y1[top], y1[rest]))
            inter = iw * ih
            overlap = inter / (area[top] + area[rest] - inter + 1e-6)
            members = np.concatenate((np.where(overlap > obj_avg_threshold)[0], [last]))
            mp = probs[order[members]]
            if mp.max() < obj_confidence_threshold:
                chosen = order[members][-n_obj_avg:]
            else:
                chosen = order[members][np.nonzero(mp > obj_confidence_threshold)[0]]
            clusters.append(chosen)
            order = np.delete(order, members)
        new_boxes = [np.rint(boxes[c].mean(axis=0)).astype('int') for c in clusters]
        new_probs = [probs[c].mean() for c in clusters]
        return np.array(new_boxes), np.array(new_probs)

    def final_nms_device(self, boxes, probs, obj_avg_threshold=0.2, obj_confidence_threshold=0.8, n_obj_avg=5):
        """final_nms computed by radnet_final_nms (csrc/scan_tail.hip): same arguments, same return, bit for bit, for the arrays
        predict hands it -- integer boxes [n][4] and float32 probs [n] (anything else is a TypeError: there is no device form of
        it).  One upload, one launch, one download on the calling thread's default context, like rpn.non_max_suppression_fast.
        AssertionError where final_nms asserts (a box with x1 >= x2 or y1 >= y2).  The inputs the kernel reports and does not
        take -- a cluster whose best prob EQUALS the threshold, a coordinate beyond +-2^29, a NaN prob -- go to final_nms."""
        from radnet_hip import runtime as rt
        from radnet_hip.engine import final_nms_groups
        if len(boxes) == 0:
            return []
        boxes, probs = np.asarray(boxes), np.asarray(probs)
        if boxes.dtype.kind != "i" or boxes.ndim != 2 or boxes.shape[1] != 4 or probs.dtype != np.float32 or probs.shape != (boxes.shape[0],):
            raise TypeError("final_nms_device takes integer boxes [n][4] and float32 probs [n], not %s %s and %s %s"
                            % (boxes.dtype, boxes.shape, probs.dtype, probs.shape))
        with rt.default_scope() as ctx:
            (status, nb, npr), = final_nms_groups(ctx, [(boxes, probs)], obj_avg_threshold, obj_confidence_threshold, n_obj_avg)
        if status == -1:                        # RADNET_FINAL_NMS_MALFORMED
            raise AssertionError("final_nms: box with x1 >= x2 or y1 >= y2")
        if status < 0:
            return self.final_nms(boxes, probs, obj_avg_threshold, obj_confidence_threshold, n_obj_avg)
        return nb, npr

    # ---- inference ---------------------------------------------------------------------------------------------------
    def _detect(self, img):
        """One network pass on an image or tile: {class: (boxes in source px, probs)} after the per-class NMS 0.2.
        With the engine-backed models the tile stays on the device from the resize to the classifier outputs (resize ->
        preprocess -> base -> RPN -> decode/sort/NMS -> RoI crop-resize -> classifier): PCIe carries the source tile in and
        ~40 KB of proposals and class scores out.  `device_resident = False` forces the NumPy-facing calls the reference
        makes (RADNet.py:540-560); both give the same detections (same kernels), tests compare them."""
        ctx = self._engine().ctx if isinstance(img, ImageWindow) else None      # a window is resized on the lane the network runs on
        if self._tail_on_device():
            img_dev, ratio = self.format_img_size(img, keep_on_device=True, ctx=ctx)
            h = self.model_rpn.propose_launch(img_dev, overlap_thresh=0.7)
            n = self.model_rpn.count_finish(self.model_rpn.count_launch(h))
            return self._tail_collect(self._tail_launch(h, n, ratio))
        if self.device_resident and hasattr(self.model_rpn, "propose_device"):
            img_dev, ratio = self.format_img_size(img, keep_on_device=True, ctx=ctx)
            R, F = self.model_rpn.propose_device(img_dev, overlap_thresh=0.7)
        else:
            X, ratio = self.format_img(img)
            Y1, Y2, F = self.model_rpn.predict(X)
            R = rpn.rpn_to_roi(Y1, Y2, self.C, overlap_thresh=0.7)
        return self._finish_detect(R, F, ratio)

    def _engine(self):
        return getattr(getattr(self.model_rpn, "_s", None), "eng", None)

    def _takes_device_images(self):
        """Engine-backed models with `device_resident`: a device image stays where it is and its tiles are ImageWindows.  Otherwise
        (duck-typed models, device_resident = False) predict downloads it once and takes the host path."""
        return (self.device_resident and hasattr(self.model_rpn, "propose_launch") and hasattr(self.model_rpn, "propose_device")
                and self._engine() is not None)

    def _finish_detect(self, R, F, ratio):
        R[:, 2] -= R[:, 0]
        R[:, 3] -= R[:, 1]
        return self._per_class_nms(*self.apply_spatial_pyramid_pooling(R, F), ratio)

    def _per_class_nms(self, bboxes, probs, ratio):
        """NMS 0.2 within each class, boxes back in source pixels (RADNet.py:562-575)."""
        out = {}
        for key in bboxes:
            nb, npr = rpn.non_max_suppression_fast(np.array(bboxes[key]), np.array(probs[key]), overlap_thresh=0.2)
            real = [self.get_real_coordinates(ratio, *nb[j, :]) for j in range(nb.shape[0])]
            out[key] = (real, [npr[j] for j in range(nb.shape[0])])
        return out

    # ---- the detection tail on the device (csrc/detect_tail.hip) -------------------------------------------------------
    def _tail_on_device(self):
        """With engine-backed models and `device_tail`, _spp_decode + _per_class_nms + get_real_coordinates run as one kernel
        behind the classifier pass and a tile's detections come back as one small record array: the host no longer waits for a
        classifier pass before it has enqueued the next one (_detect_all).  Same detections as the host code, which stays the
        path of `device_tail = False`, `device_resident = False` and duck-typed models (tests compare the two)."""
        return (self.device_tail and self.device_resident and hasattr(self.model_rpn, "propose_launch")
                and hasattr(self.model_rpn, "count_launch") and hasattr(self.model_detector, "detect_launch"))

    def _tail_launch(self, h, n, ratio):
        R_dev, Rn_dev, bp = h
        return self.model_detector.detect_launch(bp, R_dev, Rn_dev, n, ratio, self.C.n_rois, self.bbox_threshold, nms_thresh=0.2)

    def _tail_collect(self, handle):
        return self._det_from_records(*self.model_detector.detect_finish(handle))

    def _det_from_records(self, cls, boxes, probs):
        """A tile's records (engine.read_detections) as _per_class_nms returns them: {class: (boxes in source px, probs)}."""
        out = {}
        for c, b, p in zip(cls.tolist(), boxes.tolist(), probs):
            real, pr = out.setdefault(self.class_mapping[c], ([], []))
            real.append(tuple(b))
            pr.append(p)
        return out

    def _detect_all_tail(self, tiles, eng):
        """_detect_all with the tail on the device.  Per tile the host reads 4 bytes -- the proposal count, from the side lane,
        which finished it a classifier pass ago; it fixes the head plan's row count -- enqueues RoIs + classifier + tail for
        tile j, starts the side lane on tile j+1, and only then collects the records of tile j-1."""
        def launch(j, head_done):
            with eng.lane("side"):
                eng.after(head_done)                     # the classifier pass that last read this buffer set
                img_dev, ratio = self.format_img_size(tiles[j], keep_on_device=True, ctx=eng.ctx)
                h = self.model_rpn.propose_launch(img_dev, overlap_thresh=0.7, slot=j % 2)
                return h, ratio, self.model_rpn.count_launch(h)

        out, done, pending = [], [None, None], None
        nxt = launch(0, None)
        for j in range(len(tiles)):
            (h, ratio, counted), nxt = nxt, None
            n = self.model_rpn.count_finish(counted)     # waits for the side lane up to tile j's proposals, nothing else
            eng.after(counted[1])
            cur = self._tail_launch(h, n, ratio)         # enqueued, not waited for
            done[j % 2] = eng.mark()
            if j + 1 < len(tiles):
                nxt = launch(j + 1, done[(j + 1) % 2])
            if pending is not None:
                out.append(self._tail_collect(pending))
            pending = cur
        out.append(self._tail_collect(pending))
        return out

    def _detect_all(self, tiles):
        """_detect over a list of tiles, in order.  With the engine-backed models two tiles are in flight: while the
        classifier works on tile j (main lane), tile j+1 is uploaded, resized and run through the base network, the RPN and
        the proposal kernels on the engine's side lane, in the other buffer set.  Same kernels, same results as _detect."""
        eng = self._engine()
        if not (self.device_resident and hasattr(self.model_rpn, "propose_launch") and eng is not None and hasattr(eng, "lane") and len(tiles) > 1):
            return [self._detect(t) for t in tiles]
        if self._tail_on_device():
            return self._detect_all_tail(tiles, eng)

        def launch(j, head_done):
            with eng.lane("side"):
                eng.after(head_done)                     # the classifier pass that last read this buffer set
                img_dev, ratio = self.format_img_size(tiles[j], keep_on_device=True, ctx=eng.ctx)
                h = self.model_rpn.propose_launch(img_dev, overlap_thresh=0.7, slot=j % 2)
                return h, ratio, eng.mark()

        k = self.C.n_rois
        out, done = [], [None, None]                     # per buffer set: event after the classifier pass that read it
        nxt = launch(0, None)
        for j in range(len(tiles)):
            (h, ratio, ready), nxt = nxt, None
            eng.after(ready)
            R, F = self.model_rpn.propose_finish(h)
            R[:, 2] -= R[:, 0]
            R[:, 3] -= R[:, 1]
            chunks = self._spp_chunks(R)
            hp = self.model_detector.predict_launch([F, np.concatenate(chunks, axis=1)])      # enqueued, not waited for
            done[j % 2] = eng.mark()
            if j + 1 < len(tiles):                       # the next tile's upload .. proposals run beside this classifier pass
                nxt = launch(j + 1, done[(j + 1) % 2])
            pc, pr = self.model_detector.predict_finish(hp)
            bboxes, probs = self._spp_decode(chunks, [(pc[:, i * k:(i + 1) * k], pr[:, i * k:(i + 1) * k]) for i in range(len(chunks))])
            out.append(self._per_class_nms(bboxes, probs, ratio))
        return out

    # ---- tiles over the ranks of a data-parallel job (inference) ------------------------------------------
    def set_distributed(self, group=None, enabled=True):
        """Shard the tiles of every image round-robin over the ranks of torch.distributed's `group` (default: the world):
        each rank runs the network passes of its tiles, the per-tile detections (a few hundred boxes: KB) are exchanged with
        all_gather_object, and every rank then runs the merge tail (final_nms per image, NMS across images) on the tiles IN
        THEIR ORIGINAL ORDER -- so every rank returns exactly what a single process returns.  The reference is single-process
        (predict.py:56-122); this is its tile loop (RADNet.py:540-600) spread over GPUs, nothing else changes."""
        self._dist_group = group
        self._dist_on = bool(enabled)

    def _detect_sharded(self, work):
        import torch.distributed as dist
        if not getattr(self, "_dist_on", False) or not (dist.is_available() and dist.is_initialized()):
            return self._detect_all(work)
        group = getattr(self, "_dist_group", None)
        world, rank = dist.get_world_size(group), dist.get_rank(group)
        if world == 1:
            return self._detect_all(work)
        mine = list(range(rank, len(work), world))
        local = self._detect_all([work[j] for j in mine]) if mine else []
        # plain Python containers on the wire (class name -> ([[x1, y1, x2, y2], ...], [prob, ...]))
        payload = [(j, {k: ([[int(v) for v in b] for b in real], [float(p) for p in pr]) for k, (real, pr) in det.items()}) for j, det in zip(mine, local)]
        gathered = [None] * world
        dist.all_gather_object(gathered, payload, group=group)
        out = [None] * len(work)
        for part in gathered:
            for j, det in part:
                out[j] = {k: ([tuple(b) for b in real], [np.float32(p) for p in pr]) for k, (real, pr) in det.items()}
        assert all(o is not None for o in out)
        return out

    def _detect_device_image(self, img):
        """The tile passes of one image that is on the device: (detections per window, window offsets).  The image may have been
        produced on the caller's current stream (png.decode_device hands it over there): its position is recorded and every lane
        waits for it before its first read (ImageWindow.ready).  The passes run with the engine's main stream current -- the stream
        its main context launches on -- whatever stream the caller is on.  The caller's reference keeps the image alive until the
        last window's records are on the host, which is behind the last launch that reads it."""
        import torch
        eng = self._engine()
        ready = eng.mark()
        work, offs = tile_windows(img, self.C, ready)
        with torch.cuda.stream(eng.main_stream):
            return self._detect_sharded(work), offs

    def predict(self, images):
        """RADNet.py:502-718: tile -> RPN -> NMS -> RoI crop-resize -> classifier -> per-class NMS, box-averaging
        merge per image, then NMS 0.4 across images.  An image is a NumPy array or a uint8 [H][W][3] contiguous cuda tensor
        (png.decode_device, utils_io.get_image(..., to_host=False), utils_io.DeviceImageLoader).  With the engine-backed models a
        device image stays on the device: every tile is cut out of it and resized in one launch (ImageWindow) and nothing
        image-sized crosses PCIe; the detections are those of the host array with the same bytes.
        `scan_tail = True` (engine-backed models, see _scan_tail_on) merges the scan on the device: same list, one download."""
        C = self.C
        for img in images:
            if _is_device_image(img):
                check_device_image(img)             # every image, before any device work starts
        if self._scan_tail_on():
            return self._scan_pass(images).to_host()
        all_boxes, all_probs = {}, {}
        for img in images:
            if _is_device_image(img) and not self._takes_device_images():
                img = img.cpu().numpy()             # one download, then the host path
            if _is_device_image(img):
                dets_img, offs = self._detect_device_image(img)
            else:
                if C.max_n_tiles_train > 0:                 # the reference gates tiling on this training knob (RADNet.py:511)
                    h, w = img.shape[:2]
                    spans = [(tx0, ty0, tx1, ty1) for (ty0, ty1) in _spans(h, C.tile_size, C.tile_overlap) for (tx0, tx1) in _spans(w, C.tile_size, C.tile_overlap)]
                else:
                    spans = []
                work = [np.copy(img[ty0:ty1, tx0:tx1, :]) for (tx0, ty0, tx1, ty1) in spans] + ([img] if C.include_full_img else [])
                offs = [(tx0, ty0) for (tx0, ty0, tx1, ty1) in spans] + ([(0, 0)] if C.include_full_img else [])
                dets_img = self._detect_sharded(work)
            self._merge_image(dets_img, offs, all_boxes, all_probs)
        return self._merge_final(all_boxes, all_probs)

    def _merge_image(self, dets_img, offs, all_boxes, all_probs):
        """The merge of one image's tiles on the host (RADNet.py:577-600): the tiles' offsets, then final_nms per class, appended
        to the call's dicts."""
        boxes_img, probs_img = {}, {}
        for det, (ox, oy) in zip(dets_img, offs):
            for key, (real, pr) in det.items():
                for (rx1, ry1, rx2, ry2), p in zip(real, pr):
                    boxes_img.setdefault(key, []).append([ox + rx1, oy + ry1, ox + rx2, oy + ry2])
                    probs_img.setdefault(key, []).append(p)
        for key in boxes_img:
            nb, npr = self.final_nms(np.array(boxes_img[key]), np.array(probs_img[key]), obj_avg_threshold=0.2,
                                     obj_confidence_threshold=0.8, n_obj_avg=5)
            for j in range(nb.shape[0]):
                all_boxes.setdefault(key, []).append(list(nb[j, :]))
                all_probs.setdefault(key, []).append(npr[j])

    def _merge_final(self, all_boxes, all_probs):
        """NMS 0.4 across the images per class (RADNet.py:700-718) -> predict's list of dicts."""
        dets = []
        for key in all_boxes:
            nb, npr = rpn.non_max_suppression_fast(np.array(all_boxes[key]), np.array(all_probs[key]), overlap_thresh=0.4)
            for j in range(nb.shape[0]):
                x1, y1, x2, y2 = nb[j, :]
                dets.append({'class': key, 'prob': npr[j], 'x1': x1, 'y1': y1, 'x2': x2, 'y2': y2})
        return dets

    # ---- the merge of a scan on the device (csrc/scan_tail.hip) -------------------------------------------------------------
    def _scan_tail_on(self):
        """`scan_tail = True` with engine-backed models and the tile tail on the device (_tail_on_device): every tile's records
        stay in a slot of one device pool, ONE radnet_scan_merge behind the last tile of the last image does what _merge_image
        and _merge_final do on the host, and one small download brings the detections.  The tile loop still reads 4 bytes per
        tile (the proposal count) and never a record.  Same detections as the host merge, which stays the path of the default
        (`scan_tail = False`), of duck-typed models, `device_tail = False`, `device_resident = False` and of predict sharded over
        ranks (set_distributed): the records of other ranks arrive on the host there."""
        eng = self._engine()
        return bool(self.scan_tail and self._tail_on_device() and eng is not None and hasattr(eng, "lane") and hasattr(eng, "scan_merge")
                    and not self._sharded())

    def _sharded(self):
        if not getattr(self, "_dist_on", False):
            return False
        import torch.distributed as dist
        return dist.is_available() and dist.is_initialized() and dist.get_world_size(getattr(self, "_dist_group", None)) > 1

    def _scan_pass(self, images, own_pool=False):
        """The tile passes of `images` with every tile's records written into its slot of a device pool, then radnet_scan_merge:
        a DeviceDetections, nothing waited for but the proposal counts.  own_pool: a pool of its own, so that the result outlives
        the next call (predict_device); otherwise the pool of the last call of the same size is used again."""
        import torch
        eng, C = self._engine(), self.C
        for img in images:
            if _is_device_image(img):
                check_device_image(img)
        per_image = []
        for img in images:
            if _is_device_image(img):
                work, offs = tile_windows(img, C, eng.mark())       # the image's bytes are valid behind the caller's stream up to here
            else:
                if C.max_n_tiles_train > 0:                 # the reference gates tiling on this training knob (RADNet.py:511)
                    h, w = img.shape[:2]
                    spans = [(tx0, ty0, tx1, ty1) for (ty0, ty1) in _spans(h, C.tile_size, C.tile_overlap) for (tx0, tx1) in _spans(w, C.tile_size, C.tile_overlap)]
                else:
                    spans = []
                work = [np.copy(img[ty0:ty1, tx0:tx1, :]) for (tx0, ty0, tx1, ty1) in spans] + ([img] if C.include_full_img else [])
                offs = [(tx0, ty0) for (tx0, ty0, tx1, ty1) in spans] + ([(0, 0)] if C.include_full_img else [])
            per_image.append((work, offs))
        tiles = [t for work, _ in per_image for t in work]
        k = C.n_rois
        rows = (300 + k - 1) // k * k                       # the head's rows for propose_launch's 300 proposals at most
        with torch.cuda.stream(eng.main_stream):
            key = (len(tiles), rows)
            cached = getattr(self, "_scan_pool", None)
            if own_pool or cached is None or cached[0] != key:
                pool, slot_words = eng.scan_pool(len(tiles), rows)
                if not own_pool:
                    self._scan_pool = (key, pool, slot_words)
            else:
                _, pool, slot_words = cached
            table = eng.scan_table([(j * slot_words, ox, oy, im) for im, (_, offs) in enumerate(per_image) for j, (ox, oy) in
                                    enumerate(offs, sum(len(w) for w, _ in per_image[:im]))])
            self._scan_tiles(tiles, eng, pool, slot_words)
            out = eng.scan_merge(pool, rows, table, obj_avg_threshold=0.2, obj_confidence_threshold=0.8, n_obj_avg=5, nms_thresh=0.4, max_boxes=300)
            done = eng.mark()
        return DeviceDetections(out, done, self, pool, slot_words, [offs for _, offs in per_image])

    def _scan_tiles(self, tiles, eng, pool, slot_words):
        """_detect_all_tail's schedule with nothing collected: tile j's records go to slot j of the pool and stay there."""
        def launch(j, head_done):
            with eng.lane("side"):
                eng.after(head_done)                     # the classifier pass that last read this buffer set
                img_dev, ratio = self.format_img_size(tiles[j], keep_on_device=True, ctx=eng.ctx)
                h = self.model_rpn.propose_launch(img_dev, overlap_thresh=0.7, slot=j % 2)
                return h, ratio, self.model_rpn.count_launch(h)

        done = [None, None]
        nxt = launch(0, None) if tiles else None
        for j in range(len(tiles)):
            (h, ratio, counted), nxt = nxt, None
            n = self.model_rpn.count_finish(counted)     # waits for the side lane up to tile j's proposals, nothing else
            eng.after(counted[1])
            R_dev, Rn_dev, bp = h
            self.model_detector.detect_launch(bp, R_dev, Rn_dev, n, ratio, self.C.n_rois, self.bbox_threshold, nms_thresh=0.2,
                                              out=pool[j * slot_words:(j + 1) * slot_words])
            done[j % 2] = eng.mark()
            if j + 1 < len(tiles):
                nxt = launch(j + 1, done[(j + 1) % 2])

    def predict_device(self, images):
        """predict with the scan merged on the device (as `scan_tail = True`, whatever the attribute says), for callers that keep
        working there: a DeviceDetections -- the merged records as a device tensor, valid behind its `ready` event; to_host()
        gives predict's list.  Engine-backed models with the tile tail on the device only (TypeError otherwise; not sharded)."""
        saved = self.scan_tail
        self.scan_tail = True
        try:
            if not self._scan_tail_on():
                raise TypeError("predict_device needs the engine-backed models of load_radnet / models.build_models with device_resident and "
                                "device_tail on, and no rank sharding: there is no host form of it (predict is)")
            return self._scan_pass(images, own_pool=True)
        finally:
            self.scan_tail = saved

    def predict_from_path(self, img_path):
        """RADNet.py:482-500: one image per type of C.img_types when C.use_img_type, else the first type's, each read by
        utils_io.get_image (faster_rcnn/png.py decodes; no OpenCV), then predict.  With the engine-backed models and
        `device_resident` the decoded images stay on the device (get_image(..., to_host=False)); otherwise they are host arrays.
        `png_inflate = "device"` or `"device-lz"` is handed to get_image as inflate=: the same images, inflated on the device where
        the file allows (run-length streams, or any deflate stream).  `png_unfilter = "tiles"` is handed on as unfilter=: the same
        images, their scanlines reconstructed by tiles.  `png_crc = "device"` is handed on as crc=: the IDAT chunks' CRC-32 summed on
        the device (with `png_inflate = "host"` that is png.decode_device's ValueError).  `png_join = "device"` is handed on as join=:
        the file goes up as it is and its IDAT payloads are joined on the device (the same rule).
        `png_many = True`, when C.use_img_type gives more than one type: the types' files are read through ONE
        png.decode_device_many with the same four modes -- one upload, and with a device inflate one search, measure and emit for
        all of them -- instead of one get_image per type; the images are the same."""
        from . import png, utils_io
        C = self.C
        to_host = not self._takes_device_images()
        how = dict(inflate=self.png_inflate)
        if self.png_unfilter != "band":
            how["unfilter"] = self.png_unfilter
        if self.png_crc != "host":
            how["crc"] = self.png_crc
        if self.png_join != "host":
            how["join"] = self.png_join
        if C.use_img_type and self.png_many and len(C.img_types) > 1:
            paths = [utils_io.image_path(img_path, img_type) for img_type in C.img_types]
            files = paths if self.png_join == "device" else [np.fromfile(p, np.uint8) for p in paths]
            images = png.decode_device_many(files, inflate=self.png_inflate, unfilter=self.png_unfilter, crc=self.png_crc, join=self.png_join)
            if to_host:
                images = [img.cpu().numpy() for img in images]
        elif C.use_img_type:
            images = [utils_io.get_image(img_path, [img_type], random_type=False, to_host=to_host, **how) for img_type in C.img_types]
        else:
            images = [utils_io.get_image(img_path, C.img_types, random_type=False, to_host=to_host, **how)]
        return self.predict(images)

    # ---- the RPN alone: objectness maps and proposals over a scan (RADNet.py:310-480, train.py:338-347) ------------------------
    def _rpn_walk(self, img, what):
        """The windows of predict's walk for the two RPN-only passes: (engine, device image, windows, offsets).  Engine-backed
        models only; `img` is a NumPy array, uploaded once, or a device image (check_device_image)."""
        eng = self._engine()
        if eng is None or not hasattr(self.model_rpn, "propose_launch") or not hasattr(eng, "main_stream"):
            raise TypeError("%s needs the engine-backed models of load_radnet / models.build_models: it reads the RPN's scores on the device, and "
                            "there is no CPU fallback for duck-typed models" % what)
        if isinstance(img, np.ndarray):
            import torch
            if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
                raise ValueError("%s: a host image must be a uint8 [H][W][3] array, not %s %s" % (what, img.dtype, img.shape))
            img = torch.from_numpy(np.ascontiguousarray(img)).cuda()
        else:
            check_device_image(img)
        work, offs = tile_windows(img, self.C, eng.mark())      # the image's bytes are valid behind the caller's stream up to here
        return eng, img, work, offs

    def objectness_maps(self, img, anchors=None):
        """Where the RPN believes there is an object: per window of predict's walk (tile_windows: the tiles in the reference's
        order, then the full image when C.include_full_img) the maximum sigmoid score over the anchors `anchors` -- None: all A
        of them; or a (first, count) range -- of every feature-map cell, as a uint8 level (radnet_score_levels_u8:
        floor(s * 255 + 0.5), figures.to_levels).  Returns a ScoreMaps: every window's [fh][fw] map in one device pool, and the
        placements that lay them over the scan (figures.objectness_view, heat_paint_device).  The passes run on the engine's main
        stream, on one lane, one window after the other; nothing but the maps, a few KB each, ever needs to come down (to_host())."""
        import torch
        eng, img, work, offs = self._rpn_walk(img, "objectness_maps")
        first, count = (0, eng.A) if anchors is None else (int(anchors[0]), int(anchors[1]))
        if first < 0 or count < 1 or first + count > eng.A:
            raise ValueError("objectness_maps: the anchors [%d, %d + %d) of %d" % (first, first, count, eng.A))
        from radnet_hip.engine import RPN_LD
        with torch.cuda.stream(eng.main_stream):
            sizes = []
            for win in work:                                    # the plans know their feature maps before anything runs
                _, new_w, new_h = self._network_size(win.wh, win.ww)
                bp = eng._plan_base(1, new_h, new_w, 0)
                sizes.append((bp["fh"], bp["fw"]))
            places, total = score_map_places(work, sizes)
            pool = torch.empty(max(1, total), dtype=torch.uint8, device=img.device)
            for win, (fh, fw), place in zip(work, sizes, places):
                start = place[6]
                img_dev, _ = self.format_img_size(win, keep_on_device=True, ctx=eng.ctx)
                rp = eng.rpn_forward(self.model_rpn._s.base_from_u8(img_dev, 0))
                assert (rp["fh"], rp["fw"]) == (fh, fw)
                # enqueued on the stream the forward ran on, so it reads rp["pred"] before the next window's forward -- the same
                # plan and the same buffer whenever two windows have one size -- overwrites it
                eng.ctx.call("radnet_score_levels_u8", rp["pred"], RPN_LD, fh * fw, first, count, pool[start:start + fh * fw])
            # the buffer sets are predict's: its side lane does not wait for this stream, so the pass is over when this returns
            eng.main_stream.synchronize()
        pool.record_stream(torch.cuda.current_stream())
        return ScoreMaps(pool, places, tuple(int(v) for v in img.shape[:2]))

    def predict_region_proposals(self, img, gt_bboxes=None):
        """RADNet.py:310-480 made to run: what the RPN proposes over a scan, without the classifier.  The walk is predict's
        (tile_windows); per window the base network, the RPN and rpn_to_roi with overlap_thresh 0.7 run on the device, the valid
        proposals and their scores come down, the boxes are multiplied by C.rpn_stride, passed through
        get_real_coordinates(ratio, ...) and moved by the window's offset.  Returns
        [{'class': 'object', 'prob': np.float32, 'x1': np.int64, 'y1': .., 'x2': .., 'y2': ..}, ...] in window order, then in
        proposal order (best score first); a window with no valid box contributes nothing.  Engine-backed models only.
        Deviations from the reference, on purpose:
          * `prob` is the proposal's RPN score where the reference writes 1.0;
          * the full-image branch uses the same x1, y1, x2, y2 times stride arithmetic as the tiles, where the reference's branch
            mixes x, y, w, h without the stride and zeroes the scores of anchors 6..8;
          * `gt_bboxes` is accepted for call compatibility and unused: its only consumer upstream is get_map, which is not
            defined there (the reason the reference's own driver, test_rpn.py, cannot run), so only the list is returned;
          * no matplotlib pop-ups: figures.score_map_figure and figures.objectness_view draw the score maps, on request."""
        import torch
        eng, img, work, offs = self._rpn_walk(img, "predict_region_proposals")
        stride = self.C.rpn_stride
        dets = []
        with torch.cuda.stream(eng.main_stream):
            for win, (ox, oy) in zip(work, offs):
                img_dev, ratio = self.format_img_size(win, keep_on_device=True, ctx=eng.ctx)
                rp = eng.rpn_forward(self.model_rpn._s.base_from_u8(img_dev, 0))
                R, Rn = eng.proposals(rp, overlap_thresh=0.7)
                n = int(Rn.cpu()[0])                            # waits for this window: the next one reuses R, Rp and Rn
                if n <= 0:
                    continue
                boxes, scores = R[:n].cpu().numpy() * stride, rp["Rp"][:n].cpu().numpy()
                for (x1, y1, x2, y2), p in zip(boxes, scores):
                    rx1, ry1, rx2, ry2 = self.get_real_coordinates(ratio, x1, y1, x2, y2)
                    dets.append({'class': 'object', 'prob': np.float32(p), 'x1': np.int64(ox + rx1), 'y1': np.int64(oy + ry1),
                                 'x2': np.int64(ox + rx2), 'y2': np.int64(oy + ry2)})
            eng.main_stream.synchronize()
        return dets

    # ---- the outputs of the predict driver (predict.py:90-181) -----------------------------------------------
    PREDICTION_MAPS = (("all_predictions.png", (255, 255, 255), None),
                       ("boat_predictions.png", (28, 26, 228), ("boat",)),
                       ("human_predictions.png", (184, 126, 55), ("human",)),
                       ("other_predictions.png", (0, 127, 255), lambda name: name not in ("boat", "human")))

    def draw_detections(self, img, dets, color=(255, 255, 255), thickness=8, classes=None, inplace=False, labels=False, label_scale=3):
        """cv2.rectangle(img, (x1, y1), (x2, y2), color, thickness) for every detection of `dets` (predict's dicts) that `classes`
        selects -- None: all; a collection of class names; or a predicate on the name --, in list order, on the device: one
        radnet_draw_rects_u8 launch (include/radnet_hip.h states the pixel set: OpenCV's for thickness 1 and FILLED, square
        outer corners where OpenCV rounds them for thicker outlines).  img: a uint8 [H][W][3] (B, G, R) contiguous cuda tensor,
        or a NumPy array, which is uploaded.  Returns the device image: a clone unless inplace.
        labels=True adds the reference's `class: percent` label to every chosen detection (predict.py:107-115), all of it as ONE
        ordered radnet_draw_list_u8 launch: per detection the outline, then label = '{}: {}'.format(class, int(100 * prob)) with
        ((tw, th), baseline) = text_size(label, label_scale) and org = (x1, y1): the label box from (x1 - 5, y1 + baseline - 5) to
        (x1 + tw + 5, y1 - th - 5) as a black outline of thickness 1 and then FILLED white, and the text at org in black.  The
        glyphs and the metrics are the package's own dot-matrix font (csrc/draw_font.h), not OpenCV's Hershey fonts, which this
        build does not have: label_scale=3 gives capitals of 21 pixels against Hershey's roughly 22 at fontScale 1.  Parity with
        cv2 is unpinned for the text as it is for the outlines."""
        if classes is None:
            chosen = list(dets)
        elif callable(classes):
            chosen = [d for d in dets if classes(d['class'])]
        else:
            names = set(classes)
            chosen = [d for d in dets if d['class'] in names]
        b, g, r = (int(v) for v in color)
        if not labels:
            rects = [(int(d['x1']), int(d['y1']), int(d['x2']), int(d['y2']), int(thickness), b, g, r) for d in chosen]
            return draw_rects_device(img, rects, inplace=inplace)
        prims = []
        for d in chosen:
            x1, y1 = int(d['x1']), int(d['y1'])
            label = '{}: {}'.format(d['class'], int(100 * d['prob']))
            (tw, th), baseline = text_size(label, label_scale)
            box = (x1 - 5, y1 + baseline - 5, x1 + tw + 5, y1 - th - 5)
            prims += [("rect", x1, y1, int(d['x2']), int(d['y2']), int(thickness), b, g, r),
                      ("rect",) + box + (1, 0, 0, 0),
                      ("rect",) + box + (-1, 255, 255, 255),
                      ("text", x1, y1, label, int(label_scale), 0, 0, 0)]
        return draw_list_device(img, prims, inplace=inplace)

    LABELLED_MAPS = ("all_predictions.png", "other_predictions.png")      # predict.py:109-115 and 172-178

    def write_predictions(self, dets, img, out_dir, labels=False, label_scale=3, deflate="host", huffman="dynamic", crc="host"):
        """What predict.py:96-181 writes for the detections of one scan, into out_dir: all_predictions.png (every detection in
        (255, 255, 255)), boat_predictions.png (boats, (28, 26, 228)), human_predictions.png (humans, (184, 126, 55)),
        other_predictions.png (every other class, (0, 127, 255)) -- each `img` (the map to annotate: a device image or a NumPy
        array, uploaded once) with 8-pixel outlines from draw_detections, encoded by png.encode_device -- and predictions.json,
        the label / confidence / x1 / y1 / x2 / y2 dicts with indent=4.  labels=True draws the reference's text labels on the two
        maps that carry them there, all_predictions.png and other_predictions.png (draw_detections(labels=True): the package's
        own font at label_scale, not OpenCV's glyphs or metrics; unpinned against cv2); the boat and human maps stay outlines
        only.  The default leaves the labels out and writes the same bytes as before they existed.  deflate / huffman go to
        png.encode_device as they are (deflate="device": the four streams are compressed on the device and only the files' bytes
        come down; crc="device" with it: the IDAT chunks' CRC-32 is summed there too, the same bytes; deflate="device-lz": the
        device deflate with far matches, per map the smaller of its stream and the run-length one); the defaults are the host
        deflate and the bytes it always wrote.  Returns the five paths."""
        import json
        import os
        from . import png
        if isinstance(img, np.ndarray):
            import torch
            png.check_writable(img)
            img = torch.from_numpy(np.ascontiguousarray(img)).cuda()
        os.makedirs(out_dir, exist_ok=True)
        paths = []
        encoder = {} if (deflate, huffman) == ("host", "dynamic") else dict(deflate=deflate, huffman=huffman)
        if crc != "host":
            encoder["crc"] = crc
        for name, color, classes in self.PREDICTION_MAPS:
            if labels and name in self.LABELLED_MAPS:
                drawn = self.draw_detections(img, dets, color=color, thickness=8, classes=classes, inplace=False, labels=True, label_scale=label_scale)
            else:
                drawn = self.draw_detections(img, dets, color=color, thickness=8, classes=classes, inplace=False)
            paths.append(os.path.join(out_dir, name))
            with open(paths[-1], "wb") as f:
                f.write(png.encode_device(drawn, **encoder))
        predictions = [{'label': d['class'], 'confidence': float(d['prob']), 'x1': int(d['x1']), 'y1': int(d['y1']), 'x2': int(d['x2']),
                        'y2': int(d['y2'])} for d in dets]
        paths.append(os.path.join(out_dir, "predictions.json"))
        with open(paths[-1], "w") as outfile:
            json.dump(predictions, outfile, indent=4)
        return paths


class DeviceDetections:
    """What RADNet.predict_device returns.  records: a device int32 tensor, radnet_scan_merge's output (include/radnet_hip.h):
    [0] count, [1] status, [2..7] reserved, then `count` records (class index, x1, y1, x2, y2, prob as fp32 bits) in predict's
    order; ready: the event behind which it is valid (the engine's main stream).  len() and to_host() wait for it."""

    def __init__(self, records, ready, net, pool, slot_words, offsets):
        self.records, self.ready = records, ready
        self._net, self._pool, self._slot_words, self._offsets, self._words = net, pool, slot_words, offsets, None

    def words(self):
        """The records' words on the host: waits for `ready`, one download, kept."""
        if self._words is None:
            self.ready.synchronize()
            self._words = self.records.cpu().numpy()
        return self._words

    @property
    def status(self):
        return int(self.words()[1])

    def __len__(self):
        return int(self.words()[0]) if self.status == 0 else len(self.to_host())

    def to_host(self):
        """predict's list of dicts.  With a negative status (a tile met a malformed box, a cluster's best prob equals the
        threshold, ...) the pool comes down once and the host merge runs on it: it raises what the host path raises, or
        returns what it returns."""
        from radnet_hip.engine import read_detections, read_scan_records
        net = self._net
        status, cls, boxes, probs = read_scan_records(self.words())
        if status == 0:
            return [{'class': net.class_mapping[c], 'prob': p, 'x1': b[0], 'y1': b[1], 'x2': b[2], 'y2': b[3]}
                    for c, b, p in zip(cls.tolist(), boxes.astype(np.int64), probs)]
        pool = self._pool.cpu().numpy()
        all_boxes, all_probs, j = {}, {}, 0
        for offs in self._offsets:
            dets_img = []
            for _ in offs:
                dets_img.append(net._det_from_records(*read_detections(pool[j * self._slot_words:(j + 1) * self._slot_words])))
                j += 1
            net._merge_image(dets_img, offs, all_boxes, all_probs)
        return net._merge_final(all_boxes, all_probs)


RECT = np.dtype([(k, np.int32) for k in ("x1", "y1", "x2", "y2", "thickness", "b", "g", "r")])      # radnet_rect, 32 bytes


def _paint_device(img, inplace, ctx, paint, clone=True):
    """What the *_device painters below share.  img: a uint8 [H][W][3] contiguous cuda tensor, or a NumPy array, which is uploaded
    (and then painted in place).  On the feed stream of `ctx` (png.decode_device's rules), after the caller's stream: out = img if
    inplace, else a clone of it (clone=False: an uninitialised image of its shape), then paint(ctx, img, out), which uploads what
    its launch needs and calls it.  Returns out, handed over to the caller's stream."""
    import torch
    from . import augmentation_device as AD
    if isinstance(img, np.ndarray):
        img, inplace = torch.from_numpy(np.ascontiguousarray(img)).cuda(), True
    check_device_image(img)
    producer = torch.cuda.current_stream()
    with AD.feed_stream(ctx) as (ctx, side):
        if side is not None:
            side.wait_stream(producer)
        out = img if inplace else (img.clone() if clone else torch.empty_like(img))
        paint(ctx, img, out)
    return AD.hand_over(out, side)


def _upload(array):
    """A host table or pool as device bytes; None for an empty one."""
    import torch
    return torch.from_numpy(array.view(np.uint8).copy()).cuda() if len(array) else None


def draw_rects_device(img, rects, inplace=False, ctx=None):
    """radnet_draw_rects_u8 on a uint8 [H][W][3] contiguous cuda tensor (a NumPy array is uploaded): `rects` is a sequence of
    (x1, y1, x2, y2, thickness, b, g, r), painted in order (thickness < 0 fills).  Returns the device image, a clone unless inplace.
    The table goes up on its own, 32 bytes per rectangle; an empty list launches nothing.  ctx and the stream rules are
    png.decode_device's."""
    table = np.array([tuple(int(v) for v in r) for r in rects], RECT).reshape(-1)

    def paint(ctx, src, out):
        if len(table):
            ctx.call("radnet_draw_rects_u8", out, out.shape[0], out.shape[1], 3 * out.shape[1], table.ctypes.data, _upload(table), len(table))
    return _paint_device(img, inplace, ctx, paint)


def _draw_prims_device(entry, img, tables, inplace, ctx):
    """radnet_draw_list_u8 or radnet_draw_scene_u8 with scene_table's (table, chars)."""
    table, chars = tables

    def paint(ctx, src, out):
        if len(table):
            ctx.call(entry, out, out.shape[0], out.shape[1], 3 * out.shape[1], table.ctypes.data, _upload(table), len(table),
                     chars.ctypes.data if len(chars) else None, _upload(chars), len(chars))
    return _paint_device(img, inplace, ctx, paint)


PRIM = np.dtype([(k, np.int32) for k in ("kind", "x1", "y1", "x2", "y2", "a", "b", "bgr")])      # radnet_prim, 32 bytes
PRIM_RECT, PRIM_TEXT = 0, 1                                                                      # RADNET_PRIM_RECT, RADNET_PRIM_TEXT
FONT_CAP_ROWS, FONT_ADVANCE = 7, 6      # the metrics of csrc/draw_font.h in dots (the glyph table itself stands only there)


def text_size(text, scale=3):
    """((w, h), baseline) of a text run of radnet_draw_list_u8, the shape cv2.getTextSize returns: w = max(0, 6 * len - 1) * scale
    (the last character's gap column is not counted), h = 7 * scale (the cap rows above the baseline), baseline = scale (the
    descender row).  The metrics of the package's own font, not Hershey's."""
    n, scale = len(label_bytes(text)), int(scale)
    return (max(0, FONT_ADVANCE * n - 1) * scale, FONT_CAP_ROWS * scale), scale


def label_bytes(text):
    """The bytes a text entry draws for `text`: ASCII, every byte outside 0x20..0x7E (what the font has) replaced by b'?'."""
    return bytes(c if 0x20 <= c <= 0x7E else 0x3F for c in str(text).encode("ascii", "replace"))


def draw_list_device(img, prims, inplace=False, ctx=None):
    """radnet_draw_list_u8 on a uint8 [H][W][3] contiguous cuda tensor (a NumPy array is uploaded): `prims` is a sequence of
    ("rect", x1, y1, x2, y2, thickness, b, g, r) and ("text", x, y, string, scale, b, g, r) -- (x, y) the left end of the baseline,
    the string through label_bytes --, painted in order in one launch, the later entry on top (include/radnet_hip.h states the
    pixel sets).  Returns the device image, a clone unless inplace.  The table (32 bytes per entry) and the character pool go up
    on their own; an empty list launches nothing.  ctx and the stream rules are draw_rects_device's."""
    return _draw_prims_device("radnet_draw_list_u8", img, scene_table(prims, list_only=True), inplace, ctx)


PRIM_LINE, PRIM_DISC = 2, 3                                                                      # RADNET_PRIM_LINE, RADNET_PRIM_DISC


def scene_table(prims, list_only=False):
    """(table, chars): radnet_draw_scene_u8's table (PRIM rows) and character pool for a sequence of
    ("rect", x1, y1, x2, y2, thickness, b, g, r), ("text", x, y, string, scale, b, g, r), ("line", x1, y1, x2, y2, t, b, g, r) and
    ("disc", cx, cy, radius, t, b, g, r) -- t < 0 fills the disc --, each optionally followed by a dict with "dash": (on, off), lines
    only, and "transparency": 0..255 (0 opaque).  list_only: radnet_draw_list_u8's table, the same rows for what draw_list_device
    takes -- 'rect' and 'text', no options --, anything else refused in its name.  Host only; include/radnet_hip.h states the pixel
    sets and the mixing rule."""
    rows, pool = [], bytearray()
    for p in prims:
        opts = {}
        if not list_only and len(p) and isinstance(p[-1], dict):      # the list has no options: a dict there is one value too many
            p, opts = p[:-1], p[-1]
        where = "%s: entry %d" % ("draw_list_device" if list_only else "draw_scene_device", len(rows))
        if list_only and p[0] not in ("rect", "text"):
            raise ValueError("%s is %r, neither 'rect' nor 'text'" % (where, p[0]))
        if set(opts) - {"dash", "transparency"} or ("dash" in opts and p[0] != "line"):
            raise ValueError("%s (%r) has the options %r" % (where, p[0], sorted(opts)))
        tau = int(opts.get("transparency", 0))
        if not 0 <= tau <= 255:
            raise ValueError("%s has the transparency %d" % (where, tau))
        if p[0] == "rect":
            _, x1, y1, x2, y2, thickness, b, g, r = p
            row = (PRIM_RECT, int(x1), int(y1), int(x2), int(y2), int(thickness), 0)
        elif p[0] == "text":
            _, x, y, string, scale, b, g, r = p
            run = label_bytes(string)
            row = (PRIM_TEXT, int(x), int(y), int(scale), 0, len(pool), len(run))
            pool += run
        elif p[0] == "line":
            _, x1, y1, x2, y2, thickness, b, g, r = p
            dash = 0
            if "dash" in opts:
                on, off = (int(v) for v in opts["dash"])
                if not (1 <= on <= 0xFFFF and 1 <= off <= 0xFFFF):
                    raise ValueError("%s has the dash (%d, %d)" % (where, on, off))
                dash = on | off << 16
            row = (PRIM_LINE, int(x1), int(y1), int(x2), int(y2), int(thickness), dash)
        elif p[0] == "disc":
            _, cx, cy, radius, thickness, b, g, r = p
            row = (PRIM_DISC, int(cx), int(cy), int(radius), 0, int(thickness), 0)
        else:
            raise ValueError("%s is %r, none of 'rect', 'text', 'line' and 'disc'" % (where, p[0]))
        rows.append(row[:6] + (_int32(row[6]), _int32(_bgr(b, g, r) | tau << 24)))
    return np.array(rows, PRIM).reshape(-1), np.frombuffer(bytes(pool), np.uint8)


def _int32(v):
    """The int32 with the bits of a value below 2^32 (a dash or a colour with bit 31 set)."""
    return v - (1 << 32) if v >= 1 << 31 else v


def draw_scene_device(img, prims, inplace=False, ctx=None):
    """radnet_draw_scene_u8 on a uint8 [H][W][3] contiguous cuda tensor (a NumPy array is uploaded): `prims` as scene_table takes
    them, draw_list_device's rectangles and text plus lines and discs, any of them translucent, painted in order in ONE launch, each
    entry mixing with what the earlier ones left.  Returns the device image, a clone unless inplace.  An empty list launches nothing.
    ctx and the stream rules are draw_rects_device's."""
    return _draw_prims_device("radnet_draw_scene_u8", img, scene_table(prims), inplace, ctx)


def grey3_device(img, inplace=False, ctx=None):
    """radnet_grey3_u8 on a uint8 [H][W][3] contiguous cuda tensor (a NumPy array is uploaded): cv2.cvtColor(BGR2GRAY) and back to
    three equal channels in one launch.  Returns the device image, a new one unless inplace."""
    return _paint_device(img, inplace, ctx, lambda ctx, src, out: ctx.call(
        "radnet_grey3_u8", src, out, src.shape[0], src.shape[1], 3 * src.shape[1], 3 * src.shape[1]), clone=False)


HEAT_PLACE = np.dtype([(k, np.int32) for k in ("x0", "y0", "w", "h", "mw", "mh")] + [("offset", np.int64)])      # radnet_heat_place, 32 bytes


class ScoreMaps:
    """What RADNet.objectness_maps returns.  pool: a device uint8 tensor, the windows' level maps one after the other; places: per
    window the tuple (x0, y0, w, h, fw, fh, offset) heat_table takes -- the window's rectangle in scan pixels, its map of fh rows of
    fw levels and where that starts in the pool; shape: (H, W) of the scan."""
    __slots__ = ("pool", "places", "shape")

    def __init__(self, pool, places, shape):
        self.pool, self.places, self.shape = pool, [tuple(int(v) for v in p) for p in places], tuple(shape)

    def to_host(self):
        """The maps as a list of [fh][fw] uint8 arrays, in window order: one download of the pool."""
        flat = self.pool.cpu().numpy()
        return [flat[off:off + fh * fw].reshape(fh, fw).copy() for (_, _, _, _, fw, fh, off) in self.places]


def score_map_places(windows, sizes):
    """(places, pool length) for the windows of tile_windows and their feature maps' (fh, fw): per window the placement
    (x0, y0, ww, wh, fw, fh, offset) that lays its map over its rectangle of the scan, the maps one after the other.  Host only."""
    places, total = [], 0
    for win, (fh, fw) in zip(windows, sizes):
        places.append((win.x0, win.y0, win.ww, win.wh, int(fw), int(fh), total))
        total += int(fh) * int(fw)
    return places, total


def heat_table(places):
    """radnet_heat_paint_u8's table (HEAT_PLACE rows, 32 bytes each) for a sequence of (x0, y0, w, h, mw, mh, offset): the
    destination rectangle [x0, x0 + w) x [y0, y0 + h) in image pixels, the map's columns and rows, its first byte in the pool.
    Host only; include/radnet_hip.h states the pixel rule."""
    rows = []
    for p in places:
        if len(p) != 7:
            raise ValueError("heat_paint_device: entry %d has %d values, not (x0, y0, w, h, mw, mh, offset)" % (len(rows), len(p)))
        rows.append(tuple(int(v) for v in p))
    return np.array(rows, HEAT_PLACE).reshape(-1)


def heat_paint_device(img, pool, places, lut=None, transparency=0, min_level=0, inplace=False, ctx=None):
    """radnet_heat_paint_u8 on a uint8 [H][W][3] contiguous cuda tensor (a NumPy array is uploaded): the maps of `places`
    (heat_table's tuples) out of `pool` -- a uint8 cuda tensor, or host bytes / a NumPy array, which are uploaded -- through the colour
    table `lut` (256 x 3 uint8 (b, g, r); None: figures.heat_lut()), in ONE launch: a pixel takes the maximum level of the placements
    that hold it, nearest cells; below min_level it stays as it is, else the colour is mixed in with `transparency` 0..255 (0
    opaque).  Returns the device image, a clone unless inplace.  An empty list launches nothing.  ctx and the stream rules are
    draw_rects_device's."""
    import torch
    table = heat_table(places)
    tau, min_level = int(transparency), int(min_level)
    if not 0 <= tau <= 255:
        raise ValueError("heat_paint_device: the transparency %d" % tau)
    if not 0 <= min_level <= 255:
        raise ValueError("heat_paint_device: min_level = %d" % min_level)
    if lut is None:
        from . import figures
        lut = figures.heat_lut()
    lut = np.ascontiguousarray(lut)
    if lut.dtype != np.uint8 or lut.shape != (256, 3):
        raise ValueError("heat_paint_device: the colour table must be 256 x 3 uint8, not %s %s" % (lut.shape, lut.dtype))
    if not (isinstance(pool, torch.Tensor) and pool.is_cuda):
        host = np.frombuffer(bytes(pool), np.uint8) if isinstance(pool, (bytes, bytearray)) else np.ascontiguousarray(pool, dtype=np.uint8).reshape(-1)
        pool = torch.from_numpy(host.copy()).cuda() if len(host) else torch.zeros(1, dtype=torch.uint8, device=img.device if isinstance(img, torch.Tensor) else "cuda")[:0]
    if pool.dtype != torch.uint8 or not pool.is_contiguous():
        raise TypeError("heat_paint_device: the pool must be a contiguous uint8 tensor, not %s" % (pool.dtype,))

    def paint(ctx, src, out):
        if len(table):
            ctx.call("radnet_heat_paint_u8", out, out.shape[0], out.shape[1], 3 * out.shape[1], pool, pool.numel(), table.ctypes.data, _upload(table), len(table),
                     _upload(lut.reshape(-1)), tau, min_level)
    return _paint_device(img, inplace, ctx, paint)


def _bgr(b, g, r):
    """b | g << 8 | r << 16 of three colour values in 0..255 (radnet_prim.bgr)."""
    b, g, r = int(b), int(g), int(r)
    if not (0 <= b <= 255 and 0 <= g <= 255 and 0 <= r <= 255):
        raise ValueError("draw_list_device: the colour (%d, %d, %d)" % (b, g, r))
    return b | g << 8 | r << 16


def resize_cubic(img, new_w, new_h, to_host=True, ctx=None):
    """cv2.resize(img, (new_w, new_h), interpolation=cv2.INTER_CUBIC) on the device (uint8 HWC).  to_host=False: the
    result stays a device tensor (an image already at the target size is just uploaded)."""
    import torch
    from radnet_hip import runtime as rt
    own = ctx is None
    ctx = rt.default_context() if own else ctx                  # a lane's context: the kernel goes to that lane's stream
    side = rt.thread_stream() if own else None                  # a worker thread resizes on its own stream (BackgroundFeed)
    import contextlib
    with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
        src = torch.from_numpy(np.ascontiguousarray(img, dtype=np.uint8)).cuda()
        if not to_host and (new_h, new_w) == tuple(img.shape[:2]):
            out = src
        else:
            out = torch.empty((new_h, new_w, img.shape[2]), dtype=torch.uint8, device="cuda")
            ctx.call("radnet_resize_bicubic_u8", src, img.shape[0], img.shape[1], out, new_h, new_w, img.shape[2])
            if to_host:
                return out.cpu().numpy()
    if side is not None:
        # a device result made on the worker's stream: its consumer's stream waits, and the caching allocator is told that the
        # memory is in use there too (it was allocated under `side`; without this it could be handed out again while the
        # consumer still reads it)
        torch.cuda.current_stream().wait_stream(side)
        out.record_stream(torch.cuda.current_stream())
    return out


def resize_cubic_window(img_dev, x0, y0, ww, wh, new_w, new_h, ctx=None):
    """cv2.resize(np.copy(img[y0:y0+wh, x0:x0+ww, :]), (new_w, new_h), interpolation=cv2.INTER_CUBIC) for an image that is on the
    device, in one launch (radnet_resize_bicubic_window_u8): the taps replicate at the window's edges.  uint8 HWC contiguous cuda
    tensor in, uint8 cuda tensor out; ctx and streams as resize_cubic(..., to_host=False, ctx=...)."""
    import contextlib
    import torch
    from radnet_hip import runtime as rt
    if not (isinstance(img_dev, torch.Tensor) and img_dev.is_cuda and img_dev.dtype == torch.uint8 and img_dev.dim() == 3 and img_dev.is_contiguous()):
        raise TypeError("resize_cubic_window takes a contiguous uint8 HWC cuda tensor")
    own = ctx is None
    ctx = rt.default_context() if own else ctx                  # a lane's context: the kernel goes to that lane's stream
    side = rt.thread_stream() if own else None                  # a worker thread resizes on its own stream (BackgroundFeed)
    sh, sw, ch = (int(v) for v in img_dev.shape)
    if side is not None:
        side.wait_stream(torch.cuda.current_stream())           # the image was made on (or handed over to) the caller's stream
    with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
        out = torch.empty((int(new_h), int(new_w), ch), dtype=torch.uint8, device=img_dev.device)
        ctx.call("radnet_resize_bicubic_window_u8", img_dev, sh, sw, int(y0), int(x0), int(wh), int(ww), out, int(new_h), int(new_w), ch)
    if side is not None:                                        # as resize_cubic: the consumer's stream waits, the allocator is told
        torch.cuda.current_stream().wait_stream(side)
        out.record_stream(torch.cuda.current_stream())
    return out


def warp_affine_device(img, mat, dsize, ctx=None):
    """cv2.warpAffine(img, mat, dsize) (bilinear, constant border 0) on the device: augmentation.warp_affine_u8's arithmetic,
    bit for bit (tests/test_gpu_resize.py), about a hundred times faster than the NumPy form for a 300x300 tile.  uint8 HWC in,
    uint8 HWC (NumPy) out."""
    import contextlib
    import torch
    from radnet_hip import runtime as rt
    from .augmentation import warp_tables
    own = ctx is None
    ctx = rt.default_context() if own else ctx
    side = rt.thread_stream() if own else None                  # a worker thread warps on its own stream (BackgroundFeed)
    dw, dh = int(dsize[0]), int(dsize[1])
    adelta, bdelta, x0, y0 = warp_tables(mat, dsize)
    img = np.ascontiguousarray(img, dtype=np.uint8)
    ch = img.size // (img.shape[0] * img.shape[1])
    with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
        src = torch.from_numpy(img).cuda()
        col = torch.from_numpy(np.concatenate([adelta, bdelta]).astype(np.int32)).cuda()
        row = torch.from_numpy(np.concatenate([x0, y0]).astype(np.int32)).cuda()
        dst = torch.empty((dh, dw) + img.shape[2:], dtype=torch.uint8, device="cuda")
        ctx.call("radnet_warp_affine_u8", src, img.shape[0], img.shape[1], ch, dst, dh, dw, col, row)
        return dst.cpu().numpy()


class _ConfigUnpickler(pickle.Unpickler):
    """config.pickle holds a plain attribute bag (config.py:5-133; train.py:176-180 dumps it): only that class and builtin
    containers / scalars are admitted, so a crafted file cannot name arbitrary callables (the reference's bare
    pickle.load, RADNet.py:724, would execute them)."""
    _BUILTINS = {"dict", "list", "tuple", "set", "frozenset", "int", "float", "bool", "str", "bytes", "complex", "slice", "range"}

    def find_class(self, module, name):
        if (module, name) == ("faster_rcnn.config", "Config"):
            from .config import Config
            return Config
        if module == "builtins" and name in self._BUILTINS:
            import builtins
            return getattr(builtins, name)
        if (module, name) == ("collections", "OrderedDict"):
            import collections
            return collections.OrderedDict
        raise pickle.UnpicklingError("config pickle refers to %s.%s: only faster_rcnn.config.Config and builtin containers are loaded"
                                     % (module, name))


def load_radnet(config_path, device_index=0, precision="fp32"):
    """RADNet.py:721-775: unpickle the Config, build the RPN (3 outputs) and detector models, load C.weights_path.
    precision="bf16": the convolutions run on bf16 matrix cores with fp32 accumulation (ResNet50, inference only)."""
    if precision not in ("fp32", "bf16"):
        raise ValueError("precision must be 'fp32' or 'bf16', not %r" % (precision,))
    from . import models
    with open(config_path, 'rb') as f:
        C = _ConfigUnpickler(f).load()
    if C.network == 'resnet50':
        from .base_models import resnet50 as base_model
    elif C.network == 'vgg16':
        from .base_models import vgg16 as base_model
    else:
        print('Not a valid base model!')
        sys.exit(1)
    _, _, model_all, model_rpn, model_detector = models.build_models(C, device_index=device_index, workload="predict", precision=precision)      # loads no train-step launch-shape table
    model_all.load_weights(str(C.weights_path).replace('\\', '/'), by_name=True)
    return RADNet(C, model_rpn, model_detector, base_model.preprocess)
