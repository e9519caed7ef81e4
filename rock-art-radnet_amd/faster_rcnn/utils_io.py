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


def get_image(img_path, types, random_type=False, rng=np.random, to_host=True, inflate="host", unfilter="band", crc="host", join="host"):
    """utils.get_image, draw for draw: types[0], or with random_type one rng.choice(types, 1, p=probs)[0] where the first type has
    probability 0.5 (up to three types) or 0.3 and the others share the rest.  Returns the uint8 BGR HWC image as a NumPy array,
    or with to_host=False as a cuda tensor (nothing is downloaded).  inflate="device" inflates the file's IDAT stream on the device
    (png.decode_device: run-length streams; anything else takes the host path as before), inflate="device-lz" does so for a stream
    with matches at any distance; another value is png.decode_device's ValueError.  unfilter="tiles" reconstructs the scanlines by
    tiles on all CUs (png.decode_device: the same image); another value than "band" or "tiles" is its ValueError too.  crc="device"
    sums the IDAT chunks' CRC-32 on the device (png.decode_device: needs a device inflate; with inflate="host" its ValueError).
    join="device" uploads the file as it is and joins its IDAT payloads on the device (png.decode_device: the same rule)."""
    img_type = types[0]
    if random_type:
        first_prob = 0.3
        if len(types) <= 3:
            first_prob = 0.5
        probs = [first_prob] + [(1.0 - first_prob) / (len(types) - 1) for i in range(len(types) - 1)]
        img_type = rng.choice(types, 1, p=probs)[0]
    buf = np.fromfile(image_path(img_path, img_type), np.uint8)
    if inflate == "host" and unfilter == "band" and crc == "host" and join == "host":
        return png.imdecode_color(buf) if to_host else png.decode_device(buf)
    tiles = {} if unfilter == "band" else dict(unfilter=unfilter)      # the default call is the one it was
    if crc != "host":
        tiles["crc"] = crc
    if join != "host":
        tiles["join"] = join
    img = png.decode_device(buf, inflate=inflate, **tiles)
    return img.cpu().numpy() if to_host else img


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
    RADNet.predict directly: with the engine-backed models it cuts and resizes every tile on the device (RADNet.ImageWindow).
    prefetch() fills the cache ahead of the calls, many files per decode (png.decode_device_many): the types of a scan, the next
    images of a feed.  The cache holds one decoder's images: with decode= set and decode_many= not, prefetch decodes through
    decode, file by file.  unfilter="tiles" is handed to the default decoders of both (png.decode_device and decode_many's
    unfilter=); a decoder of the caller's is called as it is.  inflate=, crc= and join= are handed to the default png.decode_device
    of __call__ in the same way (crc="device" and join="device" need inflate="device" or "device-lz": png.decode_device's
    ValueError, raised here).  prefetch keeps the host parse of png.decode_device_many unless prefetch_modes=True: then inflate,
    crc and join go to the default png.decode_device_many as well (its device inflate: one search, one measure, one emit for the
    batch), and with join="device" prefetch hands it the files' paths, which it reads straight into its pinned buffer.  The
    default, False, leaves prefetch as it was; a caller's own decode / decode_many is called as it is either way."""

    def __init__(self, cache_bytes=1 << 30, decode=None, decode_many=None, unfilter="band", inflate="host", crc="host", join="host", prefetch_modes=False):
        png.check_modes(inflate, unfilter, crc, join)
        self.unfilter, self.inflate, self.crc, self.join = unfilter, inflate, crc, join
        self.prefetch_modes = bool(prefetch_modes)
        self.cache_bytes = int(cache_bytes)
        self.decode = decode                       # (file bytes as uint8 array) -> image; default: png.decode_device
        # (list of file bytes) -> list of images, for prefetch; default: png.decode_device_many, or `decode` on each file if that is set
        self.decode_many = decode_many
        self.hits = self.misses = self.prefetched = 0
        self.used = 0
        self._lru = collections.OrderedDict()      # key -> (image, bytes), least recently used first

    @staticmethod
    def _nbytes(img):
        return int(np.prod(img.shape))             # uint8

    @staticmethod
    def _key(img_data, img_type):
        path = image_path(img_data["filepath"], img_type)
        st = os.stat(path)
        return path, (path, img_type, st.st_size, st.st_mtime_ns)

    def _insert(self, key, img):
        size = self._nbytes(img)
        if size <= self.cache_bytes:
            self._lru[key] = (img, size)
            self.used += size
            while self.used > self.cache_bytes:
                _, (_, freed) = self._lru.popitem(last=False)
                self.used -= freed

    def prefetch(self, pairs):
        """Decodes the (img_data, img_type) pairs that are not in the cache, many files per decode_many call, and inserts them
        under the LRU rules, so that the calls that follow are hits.  A pair that is cached already moves to the recent end, as a
        call would move it.  A batch holds at most cache_bytes of decoded images (judged by the files' headers); a file that alone
        exceeds the bound is left to __call__; pairs that together exceed cache_bytes evict the least recently used among them, as
        calls in that order would.  hits / misses do not move.  Returns the number of images decoded (also added to `prefetched`)."""
        as_paths = False
        if self.decode_many is not None:
            decode_many = self.decode_many
        elif self.decode is not None:
            decode_many = lambda files: [self.decode(f) for f in files]      # noqa: E731  (one decoder fills the cache)
        elif self.prefetch_modes and self.inflate != "host":
            as_paths = self.join == "device"      # the files are read straight into the decoder's pinned buffer
            decode_many = lambda files: png.decode_device_many(files, unfilter=self.unfilter, inflate=self.inflate, crc=self.crc, join=self.join)      # noqa: E731
        else:
            decode_many = png.decode_device_many if self.unfilter == "band" else lambda files: png.decode_device_many(files, unfilter=self.unfilter)      # noqa: E731
        todo, seen = [], set()
        for img_data, img_type in pairs:
            path, key = self._key(img_data, img_type)
            if key in self._lru:
                self._lru.move_to_end(key)
                continue
            if key in seen:
                continue
            header = png.read_header(path)
            size = header.width * header.height * 3
            if size <= self.cache_bytes:
                seen.add(key)
                todo.append((path, key, size))
        done, batch, held = 0, [], 0
        for item in todo + [None]:
            if batch and (item is None or held + item[2] > self.cache_bytes):
                files = [path if as_paths else np.fromfile(path, np.uint8) for path, _, _ in batch]
                imgs = decode_many(files)
                for (_, key, _), img in zip(batch, imgs):
                    self._insert(key, img)
                done += len(batch)
                batch, held = [], 0
            if item is not None:
                batch.append(item)
                held += item[2]
        self.prefetched += done
        return done

    def __call__(self, img_data, img_type):
        path, key = self._key(img_data, img_type)
        hit = self._lru.get(key)
        if hit is not None:
            self._lru.move_to_end(key)
            self.hits += 1
            return hit[0]
        self.misses += 1
        buf = np.fromfile(path, np.uint8)
        if self.decode is not None:
            img = self.decode(buf)
        else:
            how = {} if self.unfilter == "band" else dict(unfilter=self.unfilter)      # the default call is the one it was
            if self.inflate != "host":
                how["inflate"] = self.inflate
            if self.crc != "host":
                how["crc"] = self.crc
            if self.join != "host":
                how["join"] = self.join
            img = png.decode_device(buf, **how)
        self._insert(key, img)
        return img


def imwrite(path, img, **kw):
    """cv2.imwrite(path, img) for a PNG map: png.encode_device(img, **kw) written to `path` (a cuda tensor stays where it is; only
    the filtered stream comes down; with deflate="device" only the compressed bytes do, huffman="dynamic" or "fixed": see
    png.encode_device; crc="device" beside deflate="device" sums the IDAT chunk's CRC-32 there too; deflate="device-lz" adds far matches and never
    writes a longer file than deflate="device", report= a dict that receives which rule ran and both sizes).  Only the .png suffix is accepted; returns
    True like cv2.imwrite."""
    path = os.fspath(path)
    if os.path.splitext(path)[1].lower() != ".png":
        raise ValueError("imwrite: only PNG files are written, not %r" % (os.path.splitext(path)[1] or path,))
    data = png.encode_device(img, **kw)
    with open(path, "wb") as f:
        f.write(data)
    return True
