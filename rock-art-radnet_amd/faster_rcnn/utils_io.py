"""Image files for the drop-in package: utils.get_image (utils.py:111-132) and the `load_image` callbacks data_feed.get_data and
data_feed.TileFeed take.  The reference decodes with cv2.imdecode(np.fromfile(path, np.uint8), cv2.IMREAD_COLOR); here the file is
read the same way and decoded by faster_rcnn/png.py (container and inflate on the host, reconstruction and expansion on the
device), which states what "the same image" means and that parity with OpenCV itself is unpinned.  PNG only: every input of the
reference is a PNG map (predict.py:59-85)."""
import collections
import os

import numpy as np

from . import png


def image_path(img_path, img_type):
    """utils.py:124-126: the type becomes path component 1 of the '/'-split path, then os.path.join -- so 'a/b.png' reads
    'a/<type>/b.png', a bare 'b.png' reads 'b.png/<type>', and for an absolute path ('' is component 0) the join drops the root."""
    parts = img_path.split('/')
    parts.insert(1, img_type)
    return os.path.join(*parts)


def get_image(img_path, types, random_type=False, rng=np.random, to_host=True):
    """utils.get_image, draw for draw: types[0], or with random_type one rng.choice(types, 1, p=probs)[0] where the first type has
    probability 0.5 (up to three types) or 0.3 and the others share the rest.  Returns the uint8 BGR HWC image as a NumPy array,
    or with to_host=False as a cuda tensor (nothing is downloaded)."""
    img_type = types[0]
    if random_type:
        first_prob = 0.3
        if len(types) <= 3:
            first_prob = 0.5
        probs = [first_prob] + [(1.0 - first_prob) / (len(types) - 1) for i in range(len(types) - 1)]
        img_type = rng.choice(types, 1, p=probs)[0]
    buf = np.fromfile(image_path(img_path, img_type), np.uint8)
    return png.imdecode_color(buf) if to_host else png.decode_device(buf)


def image_size(path):
    """(width, height) from the file's header alone (33 bytes are read, nothing is decoded)."""
    header = png.read_header(path)
    return header.width, header.height


def load_image(img_data, img_type):
    """The callback of data_feed.get_data and data_feed.TileFeed: img_data['filepath'] in the given type, as a NumPy array."""
    return get_image(img_data["filepath"], [img_type], random_type=False)


class DeviceImageLoader:
    """load_image returning uint8 HWC cuda tensors, for TileFeed(device_augment=True), with an LRU cache of decoded images keyed
    by (path, type, file size, mtime) and bounded by cache_bytes of device memory.  A feed draws up to C.max_n_tiles_train tiles
    from one image back to back and decodes the image for each (utils.py:390), so a cache of a few images removes most decodes.
    cache_bytes=0 disables it; an image larger than the bound is decoded and not kept.  hits / misses count the calls.  The cached
    tensors are handed out as they are: the feed reads them (tile gather) and never writes them.  The images can also be passed to
    RADNet.predict directly: with the engine-backed models it cuts and resizes every tile on the device (RADNet.ImageWindow)."""

    def __init__(self, cache_bytes=1 << 30, decode=None):
        self.cache_bytes = int(cache_bytes)
        self.decode = decode                       # (file bytes as uint8 array) -> image; default: png.decode_device
        self.hits = self.misses = 0
        self.used = 0
        self._lru = collections.OrderedDict()      # key -> (image, bytes), least recently used first

    @staticmethod
    def _nbytes(img):
        return int(np.prod(img.shape))             # uint8

    def __call__(self, img_data, img_type):
        path = image_path(img_data["filepath"], img_type)
        st = os.stat(path)
        key = (path, img_type, st.st_size, st.st_mtime_ns)
        hit = self._lru.get(key)
        if hit is not None:
            self._lru.move_to_end(key)
            self.hits += 1
            return hit[0]
        self.misses += 1
        buf = np.fromfile(path, np.uint8)
        img = png.decode_device(buf) if self.decode is None else self.decode(buf)
        size = self._nbytes(img)
        if size <= self.cache_bytes:
            self._lru[key] = (img, size)
            self.used += size
            while self.used > self.cache_bytes:
                _, (_, freed) = self._lru.popitem(last=False)
                self.used -= freed
        return img
