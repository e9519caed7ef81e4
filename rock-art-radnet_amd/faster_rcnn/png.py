"""PNG reader for the subset the job needs: the reference decodes every input map with cv2.imdecode(buf, cv2.IMREAD_COLOR)
(utils.py:127-130), and this module produces the same thing -- uint8 [H][W][3] in B, G, R order -- without OpenCV, as
faster_rcnn/keras_h5.py reads Keras weight files without h5py.

Host (this file, no device needed): signature, chunk walk (IHDR, PLTE, the concatenated IDAT data, IEND; ancillary chunks are
skipped, tRNS among them), CRC-32 of every chunk (zlib.crc32), inflate (zlib.decompressobj of the standard library), the pass
geometry (one pass, or Adam7's up to seven) and the check that every filter-type byte is at most 4.
Device (csrc/png.hip through the C ABI, include/radnet_hip.h): scanline reconstruction in place on the uploaded stream
(radnet_png_unfilter_u8) and expansion to BGR (radnet_png_expand_bgr_u8), one launch of each per pass.  The file becomes a device
image after one upload; nothing comes back unless the caller asks for a NumPy array.  There is no CPU reconstruction.
Many files at once (decode_device_many): the files inflate on host threads (zlib releases the GIL), ONE upload carries every
stream, every palette and a table of segments -- runs of scanlines that start on a row of filter type 0 or 1 and so do not read the
row above them (radnet_png_plan_segments cuts each pass on the host) -- and one radnet_png_unfilter_segments_u8 per distinct bpp
reconstructs all passes of all files, one workgroup per segment; the bytes are decode_device's.
decode_device_many(inflate="device" / "device-lz", crc=, join=) brings the device modes below to a whole batch: the compressed
streams of all files in ONE buffer behind a radnet_inflate_stream table, ONE search, measure and emit (csrc/inflate_many.hip), the
host chain per stream, the checks of all files in front of ONE download; a file the device refuses goes to the path above alone.

decode_device(inflate="device") uploads the COMPRESSED stream instead (parse_compressed) and inflates it on the device
(csrc/inflate.hip: a speculative search for dynamic block headers at every bit offset, the units measured, chained on the host and
emitted), for run-length streams; whatever the device cannot take goes to the host path above.  The default is that path, byte for byte.
decode_device(inflate="device-lz") does so for any deflate stream (csrc/inflate_lz.hip): emit writes the literals and every byte's
source position, pointer jumping flattens the sources, a gather copies each byte from its root.
decode_device(unfilter="tiles"), and decode_device_many likewise, reconstructs rows of Up / Average / Paeth type, which allow no
segment cut, on all CUs (csrc/png_tiles.hip): tiles of 64 rows by TILE_PIXELS pixels, one launch per sweep of independent tiles.
decode_device(join="device"), beside a device inflate, uploads the FILE as it is instead of the joined IDAT payloads, and
radnet_png_join_u8 (csrc/png_join.hip) gathers the zlib stream on the device in one launch, a lane per 16-byte grain of the output.

Every leg of the read side goes through the same few statements: the container's structure is _chunks (parse sums each chunk's
CRC as the walk yields it, parse_compressed takes the whole walk first); where the streams, the palettes, a table and the device's
sums stand in the ONE uploaded buffer is staging_layout; the segments of a pass are _plan_pass (plan_segments over the scanlines,
the device-inflate path over the downloaded filter-type column); which table entries go to radnet_png_unfilter_segments_u8 and
which to radnet_png_unfilter_tiles_u8 is decided by each caller and launched by _reconstruct; the expansion is _expand_passes;
the legal values of inflate / unfilter / crc are check_modes.

Formats: colour types 0, 2, 3, 4, 6 with the bit depths 1, 2, 4, 8, 16 the PNG specification allows for each; non-interlaced and
Adam7.  Output rules: grey is replicated to three channels, depths 1 / 2 / 4 scaled by 255 / 85 / 17; palette entries are looked up
(an index beyond the PLTE length gives 0); alpha channels and tRNS are dropped, not blended; 16-bit samples keep their high byte
(libpng's strip_16); no gamma, no sBIT, no background.

Writing (assemble, encode_device): the reference writes its annotated maps with cv2.imwrite (predict.py:118-181).  Device: ONE
radnet_png_filter_rows_u8 launch turns the device image into the scanline stream (a fixed filter type or the adaptive choice per
row); the stream comes down into one pinned buffer.  Host: the stream is cut into byte ranges, each range is deflated raw on a host
thread (zlib releases the GIL) and ends in a sync flush, the last one in the final block, and the pieces are concatenated behind one
zlib header and in front of one Adler-32 -- a valid zlib stream, the mirror image of decode_device_many.  8-bit colour type 2 or 0,
not interlaced; no ancillary chunks.  The file's bytes are a function of the image and the arguments, not of the thread count.
encode_device(deflate="device") keeps the stream on the device instead (csrc/deflate.hip): radnet_deflate_rle_scan_u8 counts the
symbols of a run-length tokenisation (what Z_RLE does: matches at distance 1 only) and sums the Adler-32 parts, the host builds one
Huffman code from the 286 counts (huffman_code) or takes the fixed one, radnet_deflate_rle_emit_u8 writes one deflate block per
RADNET_DEFLATE_CHUNK bytes, radnet_deflate_pack moves the blocks together, and only the compressed bytes come down
(assemble_pieces puts the container round them).  The default, deflate="host", is the path above, byte for byte.

This restates libpng's documented transforms as OpenCV requests them for IMREAD_COLOR.  Parity with cv2 itself is UNPINNED: cv2 is
not importable in this build, so no test compares against it (tests/png_cases.py holds an independent encoder and a NumPy statement
of the rules above).  A file this module refuses raises ValueError naming the cause, where cv2.imdecode returns None.
"""
import collections
import functools
import os
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
LEGAL_DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}
ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))      # x0, y0, dx, dy

Header = collections.namedtuple("Header", "width height bit_depth color_type interlace")
Pass = collections.namedtuple("Pass", "x0 y0 dx dy pass_w pass_h rowbytes stream_offset")
# palette: uint8 [256][3] in B, G, R order, zero beyond the file's PLTE; stream: the inflated scanlines of all passes as bytes;
# passes: the non-empty passes in stream order; bpp: the filter's byte distance, max(1, channels * bit_depth / 8)
Image = collections.namedtuple("Image", "header palette stream passes bpp")


def _constant(name):
    """An integer #define of include/radnet_hip.h, the header the kernels are compiled with."""
    from radnet_hip.lib import header_constant
    return header_constant(name)


# band and chunk of radnet_png_unfilter_u8 (the seams its tests straddle), read from the header the kernel is compiled with
UNFILTER_BAND_ROWS = _constant("RADNET_PNG_UNFILTER_BAND_ROWS")
UNFILTER_CHUNK_BYTES = _constant("RADNET_PNG_UNFILTER_CHUNK_BYTES")
# the tile of radnet_png_unfilter_tiles_u8 (unfilter="tiles"): rows of a band, pixels of a column block
TILE_ROWS = _constant("RADNET_PNG_TILE_ROWS")
TILE_PIXELS = _constant("RADNET_PNG_TILE_PIXELS")
UNFILTER_MODES = ("band", "tiles")
TilePlan = collections.namedtuple("TilePlan", "bands blocks sweeps tile_rows tile_pixels")      # radnet_png_tile_plan


def plan_tiles(rows, rowbytes, bpp):
    """radnet_png_plan_tiles (host only, no device): TilePlan(bands, blocks, sweeps, tile_rows, tile_pixels) of one segment of `rows`
    scanlines of `rowbytes` bytes; sweeps is the number of launches radnet_png_unfilter_tiles_u8 makes for it.  ValueError for
    arguments the planner refuses."""
    import ctypes
    from radnet_hip import lib as L
    out = (ctypes.c_int32 * 5)()
    rc = L.load_library().radnet_png_plan_tiles(int(rows), int(rowbytes), int(bpp), out)
    if rc != 0:
        raise ValueError("PNG: radnet_png_plan_tiles refuses %d rows of %d bytes at %d bytes per pixel (%d)" % (rows, rowbytes, bpp, rc))
    return TilePlan(*out)


def tiles_on_sweep(rows, rowbytes, bpp, sweep):
    """radnet_png_tiles_on_sweep: the (band, block) pairs of a sweep in blockIdx.x order, as a list of tuples."""
    from radnet_hip import lib as L
    fn = L.load_library().radnet_png_tiles_on_sweep
    n = fn(int(rows), int(rowbytes), int(bpp), int(sweep), None, 0)
    if n < 0:
        raise ValueError("PNG: radnet_png_tiles_on_sweep refuses sweep %d of %d rows of %d bytes at %d bytes per pixel (%d)" % (sweep, rows, rowbytes, bpp, n))
    pairs = np.zeros((n, 2), np.int32)
    assert fn(int(rows), int(rowbytes), int(bpp), int(sweep), pairs.ctypes.data, n) == n
    return [tuple(p) for p in pairs.tolist()]


def _chunks(view):
    """The chunk walk behind IHDR, the one statement of the container's structure: (type, payload start, payload end) of every chunk
    from byte 33 of the file's bytes up to IEND; the type stands in the 4 bytes in front of the payload, the CRC in the 4 behind it.
    Raises ValueError for a truncated chunk header or chunk, a second IHDR, a PLTE size and a file that ends without IEND.  A chunk
    is yielded once it is whole, and what is wrong inside it is raised when the walk moves on: a consumer that sums the CRC in its
    loop body (parse) reports a mismatch in front of that, and in front of any fault of a later chunk; one that takes the whole walk
    first (parse_compressed) reports the structure first."""
    pos = 33
    while pos < len(view):
        if pos + 12 > len(view):
            raise ValueError("PNG: truncated file (chunk header at byte %d)" % pos)
        length, kind = struct.unpack(">I4s", view[pos:pos + 8])
        end = pos + 8 + length
        if length > 0x7fffffff or end + 4 > len(view):
            raise ValueError("PNG: truncated file (%r chunk of %d bytes at byte %d)" % (kind, length, pos))
        yield kind, pos + 8, end
        if kind == b"IHDR":
            raise ValueError("PNG: a second IHDR chunk")
        if kind == b"PLTE" and (length % 3 or not 3 <= length <= 768):
            raise ValueError("PNG: PLTE chunk of %d bytes" % length)
        if kind == b"IEND":
            return
        pos = end + 4
    raise ValueError("PNG: truncated file (no IEND chunk)")


def _crc_ok(view, start, end):
    """Whether the CRC field behind the payload [start, end) is the sum of the chunk's type and payload, which stand side by side."""
    return zlib.crc32(view[start - 4:end]) == int.from_bytes(view[end:end + 4], "big")


def _crc_mismatch(kind, start):
    return ValueError("PNG: CRC mismatch in the %r chunk at byte %d" % (kind, start - 8))


def _palette(header, plte):
    """The uint8 [256][3] palette in B, G, R order of a PLTE payload (None: the file has none), zero beyond its entries."""
    if header.color_type == 3 and plte is None:
        raise ValueError("PNG: palette (PLTE) missing for colour type 3")
    palette = np.zeros((256, 3), np.uint8)
    if plte is not None:
        rgb = np.frombuffer(plte, np.uint8).reshape(-1, 3)
        palette[:rgb.shape[0]] = rgb[:, ::-1]
    return palette


def _header(data):
    if data[:8] != SIGNATURE:
        raise ValueError("PNG: bad signature")
    if len(data) < 33 or data[8:16] != b"\x00\x00\x00\rIHDR":
        raise ValueError("PNG: IHDR missing or not the first chunk")
    if not _crc_ok(data, 16, 29):
        raise _crc_mismatch(b"IHDR", 16)
    width, height, depth, color, compression, filt, interlace = struct.unpack(">IIBBBBB", data[16:29])
    if width == 0 or height == 0 or width > 0x7fffffff or height > 0x7fffffff:
        raise ValueError("PNG: illegal size %d x %d" % (width, height))
    if color not in LEGAL_DEPTHS or depth not in LEGAL_DEPTHS[color]:
        raise ValueError("PNG: illegal colour type / bit depth pair %d / %d" % (color, depth))
    if compression != 0 or filt != 0 or interlace not in (0, 1):
        raise ValueError("PNG: unknown compression / filter / interlace method %d / %d / %d" % (compression, filt, interlace))
    return Header(width, height, depth, color, interlace)


def read_header(data_or_path):
    """(width, height, bit_depth, color_type, interlace) from the first 33 bytes of a file (a path) or of its bytes."""
    if isinstance(data_or_path, (str, os.PathLike)):
        with open(data_or_path, "rb") as f:
            head = f.read(33)
    else:
        head = bytes(memoryview(data_or_path)[:33])
    return _header(head)


def pass_geometry(header):
    """The non-empty passes of an image, in stream order: Pass(x0, y0, dx, dy, pass_w, pass_h, rowbytes, stream_offset)."""
    bits = CHANNELS[header.color_type] * header.bit_depth
    grid = ADAM7 if header.interlace else ((0, 0, 1, 1),)
    passes, offset = [], 0
    for x0, y0, dx, dy in grid:
        pw, ph = -(-(header.width - x0) // dx), -(-(header.height - y0) // dy)
        if pw <= 0 or ph <= 0:
            continue                                   # an empty pass occupies no bytes in the stream
        rowbytes = (pw * bits + 7) // 8
        passes.append(Pass(x0, y0, dx, dy, pw, ph, rowbytes, offset))
        offset += ph * (1 + rowbytes)
    return passes, offset


def parse(data):
    """Container and zlib: Image(header, palette, stream, passes, bpp).  Raises ValueError naming the cause for a bad signature, a
    CRC mismatch, a missing / misplaced IHDR, an illegal colour type / depth pair, a type-3 file without PLTE, a truncated or
    over-long inflated stream and a filter-type byte above 4.  Data after IEND is ignored."""
    data = bytes(data)
    header = _header(data)
    view, idat, plte = memoryview(data), [], None
    for kind, start, end in _chunks(view):
        if not _crc_ok(view, start, end):
            raise _crc_mismatch(kind, start)
        if kind == b"PLTE":
            plte = view[start:end]
        elif kind == b"IDAT":
            idat.append(view[start:end])
    palette = _palette(header, plte)
    passes, expected = pass_geometry(header)
    inflater = zlib.decompressobj()
    try:
        stream = inflater.decompress(b"".join(idat), expected + 1)
    except zlib.error as e:
        raise ValueError("PNG: the IDAT stream does not inflate (%s)" % e) from e
    if len(stream) < expected:
        raise ValueError("PNG: truncated inflated stream (%d of %d bytes)" % (len(stream), expected))
    if len(stream) > expected:
        raise ValueError("PNG: over-long inflated stream (more than the %d bytes of the image)" % expected)
    column = np.frombuffer(stream, np.uint8)
    for p in passes:
        worst = int(column[p.stream_offset:p.stream_offset + p.pass_h * (1 + p.rowbytes):1 + p.rowbytes].max())
        if worst > 4:
            raise ValueError("PNG: filter type %d (above 4) in the pass at (%d, %d)" % (worst, p.x0, p.y0))
    return Image(header, palette, stream, passes, max(1, CHANNELS[header.color_type] * header.bit_depth // 8))


INFLATE_UNIT = np.dtype([(k, np.uint32) for k in ("start_bit", "end_bit", "out_bytes", "symbols", "blocks", "status", "flags", "last_byte")])      # radnet_inflate_unit
INFLATE_LINK = np.dtype([("out_offset", np.int64), ("start_bit", np.uint32), ("out_bytes", np.uint32), ("prev_byte", np.uint32), ("reserved", np.uint32)])
INFLATE_STATUS = ("ok", "bad header", "bad code", "not run-length", "stored length mismatch", "ran past the stream", "unit too long")
INFLATE_CHAIN = ("ok", "an end bit that is no measured start", "a unit that did not decode", "a match with nothing in front of it",
                 "the inflated length differs", "the final block does not end 4 bytes before the stream's end")
INFLATE_LZ_UNIT = np.dtype([(k, np.uint32) for k in ("start_bit", "end_bit", "out_bytes", "symbols", "blocks", "status", "flags", "reach", "far_matches",
                                                     "reserved")])      # radnet_inflate_lz_unit
INFLATE_LZ_CHAIN = INFLATE_CHAIN + ("a match that reaches in front of the stream",)      # RADNET_INFLATE_CHAIN_REACH; LEAD_MATCH is never met
# container, geometry and the compressed IDAT stream of a file: staged is a pinned uint8 tensor that holds the n bytes of the zlib
# stream and, behind them, the 768 bytes of the palette; expected is the length of the inflated stream the geometry asks for
# crc_segments (parse_compressed(crc="device") alone, else None): the radnet_crc32_segment table of the IDAT chunks over the joined stream
# trailer: the Adler-32 the zlib stream ends in, as an integer
# file_len, pieces (parse_compressed(join="device") alone, else None): staged then holds the WHOLE FILE, file_len bytes, in front of
# the palette, and the radnet_png_piece table of its IDAT payloads behind it (join_layout); the n bytes of the stream exist on the
# device only, once radnet_png_join_u8 has gathered them
Compressed = collections.namedtuple("Compressed", "header palette passes bpp expected staged n crc_segments file_len pieces trailer",
                                    defaults=(None, None, None, None))
CRC_SEGMENT = np.dtype([("offset", np.int64), ("length", np.int64), ("init", np.uint32), ("expect", np.uint32)])      # radnet_crc32_segment, 24 bytes
INFLATE_MODES = ("host", "device", "device-lz")
CRC_MODES = ("host", "device")
JOIN_MODES = ("host", "device")
JOIN_PIECE = np.dtype([("src", np.int64), ("dst", np.int64), ("length", np.int64)])      # radnet_png_piece, 24 bytes
Staging = collections.namedtuple("Staging", "palettes pad table sums result total")      # staging_layout
JoinStaging = collections.namedtuple("JoinStaging", "palettes pad pieces table sums result total")      # staging_layout(pieces=)


def _check_crc(crc):
    if crc not in CRC_MODES:
        raise ValueError("PNG: crc=%r (\"host\" or \"device\")" % (crc,))


def _check_join(join):
    if join not in JOIN_MODES:
        raise ValueError("PNG: join=%r (\"host\" or \"device\")" % (join,))


def check_modes(inflate="host", unfilter="band", crc="host", join="host"):
    """The legal values of the modes of decode_device, and of whoever hands them on to it (decode_device_many,
    utils_io.DeviceImageLoader), stated once: ValueError for an inflate, unfilter, crc or join that is none of them, and for
    crc="device" or join="device" without a device inflate."""
    if inflate not in INFLATE_MODES:
        raise ValueError("PNG: inflate=%r (\"host\", \"device\" or \"device-lz\")" % (inflate,))
    if unfilter not in UNFILTER_MODES:
        raise ValueError("PNG: unfilter=%r (\"band\" or \"tiles\")" % (unfilter,))
    _check_crc(crc)
    if crc == "device" and inflate == "host":
        raise ValueError("PNG: crc=\"device\" sums the uploaded IDAT stream and needs inflate=\"device\" or \"device-lz\", not inflate=\"host\"")
    _check_join(join)
    if join == "device" and inflate == "host":
        raise ValueError("PNG: join=\"device\" joins the IDAT stream of the uploaded file and needs inflate=\"device\" or \"device-lz\", not inflate=\"host\"")


def staging_layout(n, palettes=1, record=0, count=0, sums=False, pieces=None):
    """Where everything stands in the ONE pinned buffer a decode uploads, as Staging(palettes, pad, table, sums, result, total) byte
    offsets: the n bytes of the stream(s), `palettes` palettes of 768 bytes, the pad up to the next multiple of 8, a table of
    `count` records of `record` bytes (SEGMENT or CRC_SEGMENT) and, with sums, the `count` sums and the 2 result words the device
    writes into the uploaded copy (radnet_crc32_segments).  Without a table (record 0) nothing is padded and nothing follows the
    palettes.
    pieces (join="device": n is then the length of the whole FILE, which stands where the stream stands otherwise): a table of that
    many JOIN_PIECE records stands behind the pad, 8-byte aligned, in front of the other table, which follows it without a gap;
    the result is JoinStaging(palettes, pad, pieces, table, sums, result, total)."""
    pad = n + 768 * palettes
    if pieces is None:
        table = (pad + 7) & ~7 if record else pad
    else:
        at = (pad + 7) & ~7
        table = at + JOIN_PIECE.itemsize * pieces      # a multiple of 8 again
    result = table + record * count + (4 * count if sums else 0)
    rest = (table, table + record * count, result, result + (8 if sums else 0))
    return Staging(n, pad, *rest) if pieces is None else JoinStaging(n, pad, at, *rest)


def _stage_table(host, at, table):
    """`table` into the staging buffer `host` (uint8) at the layout `at`, the pad in front of it and the room behind it zeroed."""
    host[at.pad:at.table] = 0
    host[at.table:at.sums] = table.view(np.uint8)
    host[at.sums:at.total] = 0


def crc_layout(n, count):
    """Where parse_compressed(crc="device") puts what radnet_crc32_segments needs behind the n stream bytes and the 768 palette bytes
    of the staging buffer: (table_at, sums_at, result_at, total bytes) -- the table of `count` segments 8-byte aligned, then the
    count sums and the 2 result words the device writes into the uploaded copy."""
    at = staging_layout(n, 1, CRC_SEGMENT.itemsize, count, sums=True)
    return at.table, at.sums, at.result, at.total


def join_pieces(idat):
    """The JOIN_PIECE table (radnet_png_piece) of the chunk walk's IDAT payloads, a list of (start, end) file offsets: src = start,
    length = end - start, dst = the sum of the lengths in front -- zero-length chunks keep their entries."""
    table = np.zeros(len(idat), JOIN_PIECE)
    if len(idat):
        bounds = np.asarray(idat, np.int64).reshape(-1, 2)
        table["src"], table["length"] = bounds[:, 0], bounds[:, 1] - bounds[:, 0]
        table["dst"] = np.cumsum(table["length"]) - table["length"]
    return table


def joined_bytes(source, pieces, a, b):
    """Bytes [a, b) of the joined stream, gathered from the file's bytes `source` (uint8 array) through the JOIN_PIECE table `pieces`
    without joining anything else: the zlib header and the Adler-32 trailer, either of which may straddle chunks."""
    out = bytearray()
    k = int(np.searchsorted(pieces["dst"], a, side="right")) - 1      # the last piece with dst <= a
    while a < b and 0 <= k < len(pieces):
        src, dst, length = (int(v) for v in pieces[k])
        take = min(b, dst + length) - a
        if take > 0:
            out += source[src + a - dst:src + a - dst + take].tobytes()
            a += take
        k += 1
    return bytes(out)


def join_layout(comp):
    """The staging_layout of a Compressed record, whichever modes parse_compressed ran in."""
    record, count, sums = (0, 0, False) if comp.crc_segments is None else (CRC_SEGMENT.itemsize, len(comp.crc_segments), True)
    if comp.pieces is None:
        return staging_layout(comp.n, 1, record, count, sums=sums)
    return staging_layout(comp.file_len, 1, record, count, sums=sums, pieces=len(comp.pieces))


def parse_compressed(data, crc="host", join="host"):
    """The container walk of parse() WITHOUT the inflate: Compressed(header, palette, passes, bpp, expected, staged, n).  The IDAT
    payloads are joined directly into the pinned staging buffer (the palette rides behind them, as in decode_device); the chunk
    CRCs are summed on up to 8 host threads (fixed, like MANY_DEFAULT_WORKERS: one thread's zlib.crc32 over a 35 MB map would be
    the new floor).  Checks what parse() checks of the container, and the zlib header: CM 8, a window of at most 32 KiB, FCHECK, no
    preset dictionary.  Raises ValueError naming the cause; decode_device(inflate="device") then lets the host path speak.
    crc="device": the sums of the IDAT chunks are left to radnet_crc32_segments -- every other chunk is still summed here -- and
    the result carries crc_segments, one CRC_SEGMENT per IDAT chunk (zero-length ones too) over the JOINED stream: offset where the
    chunk's payload starts in it, its length, init = zlib.crc32(b"IDAT"), expect = the chunk's CRC field.  The staging buffer
    then holds the table behind the palette and room for the sums and the result (crc_layout).
    join="device": nothing is joined here.  The staging buffer holds the WHOLE FILE, copied in one piece, then the palette, the pad,
    the JOIN_PIECE table of the IDAT payloads (join_pieces) and, for crc="device", the CRC table, the sums and the result
    (staging_layout(pieces=), join_layout); radnet_png_join_u8 gathers the stream behind the upload.  The walk, the checks and
    their order are the same; the host's CRC sums run on the caller's bytes; the zlib header and the trailer are read through the
    table (joined_bytes); the CRC segments stay offsets into the joined stream.  The result carries file_len, pieces and, in
    both modes, trailer."""
    _check_crc(crc)
    _check_join(join)
    import torch
    view = _byte_view(data)
    on_device, join_device = crc == "device", join == "device"
    w = _walk_compressed(view, crc)
    idat, n, source = w.idat, w.n, w.source
    record, count = (CRC_SEGMENT.itemsize, len(idat)) if on_device else (0, 0)
    lay = staging_layout(len(view) if join_device else n, 1, record, count, sums=on_device, pieces=len(idat) if join_device else None)
    staged = torch.empty(lay.total, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    host = staged.numpy()
    if join_device:
        host[:len(source)] = source      # the file as it is, in one copy: the device gathers the payloads
    else:
        _join_payloads(host, 0, source, idat, 1 if w.small_file else MANY_DEFAULT_WORKERS)
    host[lay.palettes:lay.pad] = w.palette.reshape(-1)
    segments = pieces = None
    if join_device:
        pieces = join_pieces(idat)
        host[lay.pad:lay.pieces] = 0
        host[lay.pieces:lay.table] = pieces.view(np.uint8)
    if on_device:
        segments = crc_segments(view, idat)
        if join_device:      # the CRC table follows the piece table without a gap
            host[lay.table:lay.sums] = segments.view(np.uint8)
            host[lay.sums:lay.total] = 0
        else:
            _stage_table(host, lay, segments)
    return Compressed(w.header, w.palette, w.passes, w.bpp, w.expected, staged, n, segments, len(source) if join_device else None, pieces, w.trailer)


# what the container walk of parse_compressed finds before anything is staged: idat is the list of (start, end) file offsets of
# the IDAT payloads, n their total, source the file's bytes as a uint8 array, small_file whether the chunks were summed one by one
Walk = collections.namedtuple("Walk", "header palette passes bpp expected n idat trailer source small_file")


def _byte_view(data):
    return memoryview(data).cast("B") if not isinstance(data, np.ndarray) else memoryview(np.ascontiguousarray(data, np.uint8)).cast("B")


def _walk_compressed(view, crc="host"):
    """The container walk and the checks of parse_compressed, which stages what this finds (decode_device_many stages many of them
    in one buffer): the whole walk first, so the structure is judged before any sum; the palette; the chunks' CRC-32 on the host
    (crc="device": all but the IDAT chunks); the zlib header and the trailer, read through the payload table because either may
    straddle chunks.  Raises parse_compressed's ValueErrors in its order."""
    header = _header(bytes(view[:33]))
    idat, plte, jobs = [], None, []
    for kind, start, end in _chunks(view):      # the whole walk: the structure is judged before any sum
        jobs.append((kind, start - 8, end))
        if kind == b"PLTE":
            plte = view[start:end]
        elif kind == b"IDAT":
            idat.append((start, end))
    palette = _palette(header, plte)
    source = np.frombuffer(view, np.uint8)

    def crc_ok(job, workers=1):
        kind, at, end = job
        if workers == 1:
            return _crc_ok(view, at + 8, end)      # one call per chunk
        return _crc32_threads(view[at + 8:end], zlib.crc32(kind), workers=workers) == int.from_bytes(view[end:end + 4], "big")
    n = sum(e - s for s, e in idat)
    small_file = sum(e - at for _, at, e in jobs) < 1 << 20
    if crc == "device":
        jobs = [j for j in jobs if j[0] != b"IDAT"]
    if small_file:
        oks = {j: crc_ok(j) for j in jobs}
    else:
        # a chunk of 4 MiB or more is cut into ranges summed on host threads (one large IDAT: this package's writer); the others
        # (8 KiB IDAT chunks by the thousand) go to radnet_png_check_crcs in one call, which spreads them over threads of its own
        from radnet_hip import lib as L
        large = [j for j in jobs if j[2] - j[1] >= 4 << 20]
        small = [j for j in jobs if j[2] - j[1] < 4 << 20]
        oks = {j: crc_ok(j, MANY_DEFAULT_WORKERS) for j in large}
        if small:
            at, end = np.array([j[1] for j in small], np.int64), np.array([j[2] for j in small], np.int64)
            bad = L.load_library().radnet_png_check_crcs(source.ctypes.data, len(source), at.ctypes.data, end.ctypes.data, len(small), MANY_DEFAULT_WORKERS)
            if bad < 0:
                raise RuntimeError("PNG: radnet_png_check_crcs failed (%d)" % bad)
            oks.update((j, k < bad) for k, j in enumerate(small))      # chunks behind the first bad one are not looked at: it is reported
    for kind, at, end in jobs:
        if not oks[(kind, at, end)]:
            raise _crc_mismatch(kind, at + 8)
    pieces = join_pieces(idat)
    head = joined_bytes(source, pieces, 0, 2)
    if n < 2 or head[0] & 15 != 8 or head[0] >> 4 > 7 or (head[0] * 256 + head[1]) % 31 or head[1] & 32:
        raise ValueError("PNG: the IDAT stream has no zlib header the device inflate takes (deflate, a window of at most 32 KiB, FCHECK, no dictionary)")
    passes, expected = pass_geometry(header)
    tail = joined_bytes(source, pieces, max(n - 4, 0), n)
    return Walk(header, palette, passes, max(1, CHANNELS[header.color_type] * header.bit_depth // 8), expected, n, idat, int.from_bytes(tail, "big"), source,
                small_file)


def _join_payloads(host, at, source, idat, workers=1):
    """The IDAT payloads `idat` ((start, end) offsets into `source`) one behind the other into host[at ..], on `workers` threads."""
    import concurrent.futures
    starts = np.concatenate([[0], np.cumsum([e - s for s, e in idat])]).astype(np.int64).tolist()

    def join(k):
        s, e = idat[k]
        host[at + starts[k]:at + starts[k] + e - s] = source[s:e]
    if workers == 1 or len(idat) < 2:
        for k in range(len(idat)):
            join(k)
    else:
        with concurrent.futures.ThreadPoolExecutor(max_workers=workers) as pool:
            list(pool.map(lambda g: [join(k) for k in range(g, len(idat), workers)], range(min(len(idat), workers))))


def crc_segments(view, idat, base=0):
    """The CRC_SEGMENT table of the IDAT chunks `idat` ((start, end) file offsets) over the JOINED stream, which stands at `base` of
    the buffer the device sums: offset where the chunk's payload starts in it, its length, init = zlib.crc32(b"IDAT"), expect =
    the chunk's CRC field."""
    segments = np.zeros(len(idat), CRC_SEGMENT)
    lengths = np.array([e - s for s, e in idat], np.int64)
    segments["offset"] = base + np.cumsum(lengths) - lengths
    segments["length"] = lengths
    segments["init"] = zlib.crc32(b"IDAT")
    segments["expect"] = [int.from_bytes(view[e:e + 4], "big") for _, e in idat]
    return segments


def _lap(report, name):
    """With report["stages"] a dict (tools/png_inflate_timing.py): the device is drained and the wall time since the last lap is
    booked under `name`, in milliseconds.  Without it nothing happens and nothing waits."""
    stages = report.get("stages")
    if stages is not None:
        import time
        import torch
        torch.cuda.synchronize()
        now = time.perf_counter()
        stages[name] = stages.get(name, 0.0) + (now - stages.get("_t", now)) * 1e3
        stages["_t"] = now


def _launch(report, ctx, name, *args):
    """ctx.call(name, *args); with report["stages"] the launch is bracketed by two events and booked under `name`."""
    stages = report.get("stages")
    if stages is None:
        return ctx.call(name, *args)
    import torch
    _lap(report, "host_between_ms")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    ctx.call(name, *args)
    e1.record()
    e1.synchronize()
    stages[name + "_ms"] = stages.get(name + "_ms", 0.0) + e0.elapsed_time(e1)
    _lap(report, "_skip")


def _measured_units(comp, dev, ctx, report, dtype, measure):
    """The records (structured array of `dtype`) of the units behind every block candidate of `comp` and behind the stream's first
    bit, as the entry `measure` fills them, or None with report["reason"].  Two syncs: the candidates, the records."""
    import torch
    n = comp.n
    refuse = lambda why: report.update(reason=why) or None      # noqa: E731
    if n < 7:
        return refuse("a zlib stream of %d bytes" % n)
    if n >= 1 << 29:
        return refuse("a zlib stream of %d bytes (bit offsets leave 32 bits)" % n)
    z, first_bit = dev.data_ptr(), 16
    cap = n // 32 + 1024
    found = torch.zeros(cap + 1, dtype=torch.int32, device="cuda")      # the count, then the candidates
    _launch(report, ctx, "radnet_inflate_find_blocks", z, n, first_bit, found.data_ptr() + 4, cap, found)
    found_host = found.cpu().numpy().view(np.uint32)
    _lap(report, "download_candidates_ms")
    count = int(found_host[0])
    report["candidates"] = count
    if count > cap:
        return refuse("%d block candidates, more than the %d the search keeps" % (count, cap))
    starts = np.union1d(found_host[1:1 + count], np.array([first_bit], np.uint32))
    units = np.zeros(len(starts), dtype)
    units["start_bit"] = starts
    units_dev = torch.from_numpy(units.view(np.uint8)).cuda()
    _lap(report, "sort_upload_units_ms")
    _launch(report, ctx, measure, z, n, units_dev, len(units))
    units = units_dev.cpu().numpy().view(dtype)
    _lap(report, "download_units_ms")
    return units


def _chained_links(comp, report, units, chain, names):
    """The links (INFLATE_LINK) of the units the host entry `chain` walks from the stream's first bit to its final block, or None
    with report["reason"]; names: what its refusal codes are called."""
    import ctypes
    from radnet_hip import lib as L
    links = np.zeros(len(units), INFLATE_LINK)
    n_links, n_false, bad = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(-1)
    rc = getattr(L.load_library(), chain)(units.ctypes.data, len(units), 16, comp.n, comp.expected, links.ctypes.data, len(links), ctypes.byref(n_links),
                                          ctypes.byref(n_false), ctypes.byref(bad))
    if rc != 0:
        if rc < 0:
            raise RuntimeError("PNG: %s failed (%d)" % (chain, rc))
        why = "chain: " + names[rc]
        if rc == 2:
            why += " (%s)" % INFLATE_STATUS[int(units["status"][bad.value])]
        report["reason"] = why
        return None
    links = links[:n_links.value]
    by_start = dict(zip(units["start_bit"].tolist(), units["blocks"].tolist()))
    report.update(false_candidates=n_false.value, units=len(links), blocks=sum(by_start[s] for s in links["start_bit"].tolist()))
    return links


def _inflate_device(comp, dev, ctx, report):
    """The inflated scanline stream of `comp` as a cuda tensor of comp.expected bytes (dev: the uploaded staging buffer), or None with
    report["reason"] saying what the device could not take.  Three syncs: the candidates, the unit records, the Adler parts with the
    filter-type column; the column comes back as report["column"]."""
    import torch
    units = _measured_units(comp, dev, ctx, report, INFLATE_UNIT, "radnet_inflate_rle_measure")
    links = None if units is None else _chained_links(comp, report, units, "radnet_inflate_chain", INFLATE_CHAIN)
    if links is None:
        return None
    links_dev = torch.from_numpy(links.view(np.uint8)).cuda()
    stream = torch.empty(max(comp.expected, 1), dtype=torch.uint8, device="cuda")
    _lap(report, "chain_upload_links_ms")
    _launch(report, ctx, "radnet_inflate_rle_emit", dev.data_ptr(), comp.n, links_dev, len(links), stream, comp.expected)
    return _checked_stream(comp, ctx, report, stream)


def _inflate_device_lz(comp, dev, ctx, report):
    """_inflate_device for any stream (csrc/inflate_lz.hip): the units measured with their distances whole and chained, the literals
    and every byte's source position emitted, the sources flattened by pointer jumping -- radnet_inflate_lz_resolve in groups of 4
    rounds, each group's counters downloaded, up to the first round that rewrote nothing and never beyond ceil(log2(bytes)) rounds --
    and the bytes gathered from their roots.  report["rounds"]: the rounds that rewrote an entry; report["far_units"]: the chained
    units that hold a match of another distance than 1."""
    import torch
    expected = comp.expected
    if expected >= 1 << 31:
        report["reason"] = "an inflated stream of %d bytes (positions leave 31 bits)" % expected
        return None
    units = _measured_units(comp, dev, ctx, report, INFLATE_LZ_UNIT, "radnet_inflate_lz_measure")
    links = None if units is None else _chained_links(comp, report, units, "radnet_inflate_lz_chain", INFLATE_LZ_CHAIN)
    if links is None:
        return None
    far = dict(zip(units["start_bit"].tolist(), units["far_matches"].tolist()))
    report["far_units"] = sum(far[s] > 0 for s in links["start_bit"].tolist())
    links_dev = torch.from_numpy(links.view(np.uint8)).cuda()
    stream = torch.empty(max(expected, 1), dtype=torch.uint8, device="cuda")
    src = torch.empty(max(expected, 1), dtype=torch.int32, device="cuda")
    _lap(report, "chain_upload_links_ms")
    _launch(report, ctx, "radnet_inflate_lz_emit", dev.data_ptr(), comp.n, links_dev, len(links), stream, src, expected)
    # ceil(log2(max(expected, 2))) rounds.  A source lies in front of its match, so a path crosses a match once; k links are k matches of
    # 3 bytes or more, 3 k <= expected, and the ceil(log2(k)) rounds that rewrite leave one of the bound to see that nothing moves any more
    bound, ran, rounds = max(1, (max(expected, 2) - 1).bit_length()), 0, None
    while rounds is None:
        if ran >= bound:
            raise RuntimeError("PNG: the source table of %d bytes is not flat after %d rounds of radnet_inflate_lz_resolve" % (expected, bound))
        group = min(4, bound - ran)
        changed = torch.zeros(group, dtype=torch.int32, device="cuda")
        _launch(report, ctx, "radnet_inflate_lz_resolve", src, expected, group, changed)
        still = np.flatnonzero(changed.cpu().numpy() == 0)
        _lap(report, "download_changed_ms")
        if len(still):
            rounds = ran + int(still[0])
        ran += group
    report["rounds"] = rounds
    _launch(report, ctx, "radnet_inflate_lz_gather", src, stream, expected)
    return _checked_stream(comp, ctx, report, stream)


def _checked_stream(comp, ctx, report, stream):
    """`stream` (the inflated bytes on the device) once its Adler-32, summed there, equals the zlib trailer, else None with the
    reason "adler"; the filter-type column comes back as report["column"].  One sync."""
    import torch
    expected = comp.expected
    chunks = -(-expected // _constant("RADNET_DEFLATE_CHUNK"))
    rows = sum(p.pass_h for p in comp.passes)
    tail = torch.zeros(DEFLATE_SYMBOLS * 4 + chunks * 16 + rows, dtype=torch.uint8, device="cuda")      # counts (not used), Adler parts, column
    _launch(report, ctx, "radnet_deflate_rle_scan_u8", stream, expected, tail, tail.data_ptr() + DEFLATE_SYMBOLS * 4)
    offsets = np.array([p.stream_offset for p in comp.passes], np.int64)
    pass_rows = np.array([p.pass_h for p in comp.passes], np.int32)
    rowbytes = np.array([p.rowbytes for p in comp.passes], np.int32)
    _launch(report, ctx, "radnet_png_gather_column_u8", stream, expected, offsets.ctypes.data, pass_rows.ctypes.data, rowbytes.ctypes.data, len(comp.passes),
             tail.data_ptr() + DEFLATE_SYMBOLS * 4 + chunks * 16)
    tail_host = tail.cpu().numpy()
    _lap(report, "download_adler_column_ms")
    parts = tail_host[DEFLATE_SYMBOLS * 4:DEFLATE_SYMBOLS * 4 + chunks * 16].view(np.uint64)
    if adler32_of_parts(parts, expected) != comp.trailer:
        report["reason"] = "adler"
        return None
    report["column"] = tail_host[DEFLATE_SYMBOLS * 4 + chunks * 16:]
    return stream


SEGMENT = np.dtype([("offset", np.int64), ("rows", np.int32), ("rowbytes", np.int32)])      # radnet_png_segment, 16 bytes
SEGMENT_TARGET_ROWS = _constant("RADNET_PNG_SEGMENT_TARGET_ROWS")      # the planners' target_rows = 0
# the `rows <= 64` split in radnet_png_unfilter_segments_u8 (csrc/png.hip): segments of at most this many rows go out in its one-wave
# launch and the longer ones in its band-sized launch, each over the index range that holds its kind, so a table stands short-first
# and neither range holds workgroups of the other kind.  Not TILE_ROWS, the height of a tile, though both are 64 today.
SEGMENT_ONE_WAVE_ROWS = 64


def _plan_pass(entry, pointer, p, offset, target_rows=0):
    """The SEGMENT table of the pass `p` whose first scanline stands at `offset` of the buffer to reconstruct, from the planner
    `entry`: "radnet_png_plan_segments" reads the pass's scanlines at `pointer`, "radnet_png_plan_segments_column" its column of
    filter types.  ValueError when the planner refuses."""
    import ctypes
    from radnet_hip import lib as L
    target = target_rows or SEGMENT_TARGET_ROWS
    cap = min(p.pass_h, 2 * (p.pass_h // target) + 2)      # two neighbours of the greedy rule together exceed target_rows
    table = np.zeros(cap, SEGMENT)
    n = getattr(L.load_library(), entry)(pointer, offset, p.pass_h, p.rowbytes, target_rows, table.ctypes.data_as(ctypes.c_void_p), cap)
    if n < 0:
        raise ValueError("PNG: %s failed (%d) on the pass at (%d, %d)" % (entry, n, p.x0, p.y0))
    return table[:n]


def _reconstruct(call, table_host, table_dev, base, length, groups):
    """The reconstruction launches over one short-first-sorted SEGMENT table (table_host, table_dev: its address on the host and in
    the uploaded copy) whose offsets count from `base`, a device buffer of `length` bytes.  groups: (bpp, first, short, count) --
    of the `count` table entries from `first` on, which share `bpp`, the first `short` go to radnet_png_unfilter_segments_u8 and
    the others to radnet_png_unfilter_tiles_u8; an empty range launches nothing.  What `short` is, the caller decides.
    call(name, *args): ctx.call, or _launch with its report."""
    for bpp, first, short, count in groups:
        for entry, at, n in (("radnet_png_unfilter_segments_u8", first, short), ("radnet_png_unfilter_tiles_u8", first + short, count - short)):
            if n:
                call(entry, base, length, table_host + SEGMENT.itemsize * at, table_dev + SEGMENT.itemsize * at, n, bpp)


def _unfilter_passes(call, passes, base, bpp):
    """One radnet_png_unfilter_u8 per pass, in place on the stream at `base`: one workgroup walks the pass."""
    for p in passes:
        call("radnet_png_unfilter_u8", base + p.stream_offset, p.pass_h, p.rowbytes, bpp)


def _expand_passes(call, header, passes, base, palette, out):
    """One radnet_png_expand_bgr_u8 per pass: the reconstructed scanlines at `base` into their pixels of the image `out`."""
    for p in passes:
        call("radnet_png_expand_bgr_u8", base + p.stream_offset, p.pass_h, p.pass_w, p.rowbytes, header.color_type, header.bit_depth, palette, out,
             header.height, header.width, p.y0, p.x0, p.dy, p.dx)


def _report_host_path(report, inflate, unfilter, crc, join="host"):
    """What the report says of a file the host path decodes, with the keys of the active modes; reason and candidates are not
    touched: after a refusal they say why, and what the device search had found."""
    report.update(path="host", false_candidates=0, units=0, blocks=0, reconstruction=None)
    if inflate == "device-lz":
        report.update(rounds=0, far_units=0)
    if unfilter == "tiles":
        report["sweeps"] = 0
    if crc == "device":
        report["crc"] = "host"
    if join == "device":
        report["join"] = "host"


def _decode_inflated_on_device(data, ctx, report, lz=False, tiles=False, crc_device=False, join_device=False):
    """decode_device's device inflate (lz: the one for any stream): the image, or None when the host path has to take the file
    (report["reason"]).  tiles: unfilter="tiles" -- segments of at most 64 rows go to radnet_png_unfilter_segments_u8, all longer ones
    to radnet_png_unfilter_tiles_u8, whether or not the segments spread the passes.  crc_device: crc="device" -- the IDAT chunks' sums
    come from radnet_crc32_segments, and a mismatch is the reason "crc: IDAT chunk k".  join_device: join="device" -- the whole file goes
    up and radnet_png_join_u8 gathers the stream into a buffer of its own, which the CRC and the inflate entries then take; the
    launches stand on the context's stream in that order, join, CRC, search."""
    import torch
    from radnet_hip.lib import RadnetError
    from . import augmentation_device as AD
    _lap(report, "_skip")
    try:
        if join_device:
            comp = parse_compressed(data, crc="device" if crc_device else "host", join="device")
        else:
            comp = parse_compressed(data, crc="device") if crc_device else parse_compressed(data)
    except ValueError as e:
        report["reason"] = "container: %s" % e
        return None
    _lap(report, "container_crc_ms")
    with AD.feed_stream(ctx) as (ctx, side):
        dev = comp.staged.cuda(non_blocking=True)
        _lap(report, "upload_ms")
        at = join_layout(comp)
        zdev = dev                               # what holds the zlib stream at its byte 0
        if join_device:
            zdev = torch.empty(max(comp.n, 1), dtype=torch.uint8, device="cuda")
            try:
                _launch(report, ctx, "radnet_png_join_u8", dev.data_ptr(), comp.file_len, comp.staged.data_ptr() + at.pieces, dev.data_ptr() + at.pieces,
                        len(comp.pieces), zdev.data_ptr(), comp.n)
            except RadnetError as e:
                report["reason"] = "join: %s" % e
                return None
            report["join"] = "device"
        if crc_device:
            # the IDAT sums right behind the upload: the table stands behind the palette, the sums and the result go into the uploaded
            # copy, and the 8 bytes of the result are on their way down before the search starts -- its first download delivers them
            count = len(comp.crc_segments)
            table_at, sums_at, result_at = at.table, at.sums, at.result
            _launch(report, ctx, "radnet_crc32_segments", zdev.data_ptr(), comp.n, comp.staged.data_ptr() + table_at, dev.data_ptr() + table_at, count,
                    dev.data_ptr() + sums_at, dev.data_ptr() + result_at)
            verdict = torch.empty(2, dtype=torch.int32, pin_memory=True)
            verdict.copy_(dev[result_at:result_at + 8].view(torch.int32), non_blocking=True)
        stream = (_inflate_device_lz if lz else _inflate_device)(comp, zdev, ctx, report)
        if crc_device:
            if stream is None:
                torch.cuda.current_stream().synchronize()      # a refusal may come before the first download; the host path is next anyway
            first_bad, n_bad = (int(v) for v in verdict)
            if n_bad:
                report["reason"] = "crc: IDAT chunk %d" % first_bad
                return None
            report["crc"] = "device"
        if stream is None:
            return None
        column = report.pop("column")
        if int(column.max()) > 4:
            report["reason"] = "a filter type above 4"
            return None
        h = comp.header
        out = torch.empty((h.height, h.width, 3), dtype=torch.uint8, device="cuda")
        base, palette = stream.data_ptr(), dev.data_ptr() + at.palettes
        call = functools.partial(_launch, report, ctx)
        # segments when they spread a pass over the device: the longest is at most half its pass
        tables, row0, spread = [], 0, True
        for p in comp.passes:
            col = np.ascontiguousarray(column[row0:row0 + p.pass_h])
            tables.append(_plan_pass("radnet_png_plan_segments_column", col.ctypes.data, p, p.stream_offset))
            spread = spread and 2 * int(tables[-1]["rows"].max()) <= p.pass_h
            row0 += p.pass_h
        if tiles or spread:
            table = np.concatenate(tables)
            # with tiles the segments above TILE_ROWS rows leave for the tiles call; without, every segment keeps the segments call
            split = TILE_ROWS if tiles else SEGMENT_ONE_WAVE_ROWS
            table = table[np.argsort(table["rows"] > split, kind="stable")]
            short = int((table["rows"] <= split).sum()) if tiles else len(table)
            table_dev = torch.from_numpy(table.view(np.uint8)).cuda()
            _lap(report, "plan_segments_ms")
            _reconstruct(call, table.ctypes.data, table_dev.data_ptr(), base, comp.expected, [(comp.bpp, 0, short, len(table))])
            if tiles:
                report["reconstruction"] = "segments+tiles" if short else "tiles"
                report["sweeps"] = max([plan_tiles(int(t["rows"]), int(t["rowbytes"]), comp.bpp).sweeps for t in table[short:]], default=0)
            else:
                report["reconstruction"] = "segments"
        else:
            _lap(report, "plan_segments_ms")
            _unfilter_passes(call, comp.passes, base, comp.bpp)
            report["reconstruction"] = "unfilter"
        _expand_passes(call, comp.header, comp.passes, base, palette, out)
    report["path"] = "device"
    return AD.hand_over(out, side)


def decode_device(data, ctx=None, inflate="host", report=None, unfilter="band", crc="host", join="host"):
    """The decoded image as a uint8 [H][W][3] (B, G, R) cuda tensor: parse, ONE pinned upload of the inflated stream (the palette
    rides behind it), then reconstruction and expansion per pass.  ctx: a radnet context whose stream is torch's current one;
    None = the calling thread's default context, on a BackgroundFeed worker thread on that thread's own stream.
    inflate="device" (opt-in; "host" is the path above, byte for byte): the COMPRESSED IDAT stream goes up instead
    (parse_compressed) and is inflated there (csrc/inflate.hip): radnet_inflate_find_blocks tries a dynamic block header at every
    bit offset, radnet_inflate_rle_measure decodes the unit behind every candidate, radnet_inflate_chain (host) follows them from the
    first block to the last, radnet_inflate_rle_emit writes the bytes; the Adler-32 and the filter-type column come from the device
    too.  That takes run-length streams only (zlib level 1 with Z_RLE: cv2.imwrite's defaults, assemble, deflate="device").  Whatever
    the device cannot take -- matches at other distances, a unit above RADNET_INFLATE_UNIT_MAX_SYMBOLS, a corrupt stream, a broken
    container -- goes to the host path, with that path's image or exception.  A dict passed as `report` receives path ("device" or
    "host"), reason (None on the device path), candidates, false_candidates, units, blocks and reconstruction ("segments" through
    radnet_png_unfilter_segments_u8 when the longest segment is at most half its pass, else "unfilter"; None on the host path).
    inflate="device-lz" (opt-in too) takes ANY deflate stream, as other tools write them at level 6 (csrc/inflate_lz.hip): the same
    search, radnet_inflate_lz_measure with the distances whole, radnet_inflate_lz_chain, radnet_inflate_lz_emit (the literals and
    every byte's source position), radnet_inflate_lz_resolve (pointer jumping, up to the first round that rewrote nothing and at most
    ceil(log2(bytes)) rounds; more is a RuntimeError) and radnet_inflate_lz_gather; then the same checks and reconstruction.  What it
    cannot take -- a unit above the symbol cap, a corrupt stream, a match that reaches in front of the stream, a broken container --
    goes to the host path as above.  In this mode the report also carries rounds (those that rewrote an entry) and far_units (the
    chained units with a match of another distance than 1).
    unfilter="tiles" (opt-in; "band" is everything above, launch for launch): rows of adaptive filter types are reconstructed on all
    CUs by radnet_png_unfilter_tiles_u8 (csrc/png_tiles.hip: tiles of 64 rows by TILE_PIXELS pixels, one launch per sweep of
    independent tiles) instead of one workgroup per pass.  On the host-inflate path ONE such call carries all passes of the file (a
    table of one entry per pass rides behind the palette in the staging buffer); on the device-inflate paths the segments of at most
    64 rows keep radnet_png_unfilter_segments_u8 and all longer ones go to the tiles entry.  The bytes are those of "band".  In this
    mode alone the report's reconstruction is "tiles" or "segments+tiles" (segments of both kinds) and it carries sweeps, the
    launches of the tiles call: the most sweeps radnet_png_plan_tiles gives for one of its segments.
    crc="device" (opt-in; needs a device inflate, with inflate="host" it is a ValueError): the CRC-32 of the IDAT chunks, the bulk
    of the file, is summed on the uploaded stream by radnet_crc32_segments (csrc/crc32.hip) right behind the upload instead of on
    host threads in front of it; the other chunks are summed on the host as before.  The verdict comes down with the search's
    candidates.  A mismatch sends the file to the host path (reason "crc: IDAT chunk k"), which raises the default's ValueError.
    In this mode alone the report carries crc: "device" when the sums were checked there, "host" when the host path took the file.
    join="device" (opt-in; needs a device inflate, with inflate="host" it is a ValueError): the IDAT payloads are not joined on the
    host.  The file's bytes go into the pinned buffer in ONE copy and up as they are -- the palette, the table of the payloads
    (join_pieces) and, for crc="device", the CRC table ride behind them --, and ONE launch, radnet_png_join_u8 (csrc/png_join.hip),
    gathers the zlib stream into a device buffer of its own, which the CRC sums and the search then take: join, CRC, search, in
    that order on the context's stream.  The container's checks, their order and their ValueErrors are the default's.  In this
    mode alone the report carries join: "device" when the stream was joined there, "host" when the host path took the file."""
    import torch
    from . import augmentation_device as AD
    check_modes(inflate, unfilter, crc, join)
    tiles = unfilter == "tiles"
    report = {} if report is None else report
    report.update(reason=None, candidates=0)
    _report_host_path(report, inflate, unfilter, crc, join)
    if inflate != "host":
        if join == "device":
            out = _decode_inflated_on_device(data, ctx, report, lz=inflate == "device-lz", tiles=tiles, crc_device=crc == "device", join_device=True)
        else:
            out = _decode_inflated_on_device(data, ctx, report, lz=inflate == "device-lz", tiles=tiles, crc_device=crc == "device")
        if out is not None:
            return out
        _report_host_path(report, inflate, unfilter, crc, join)
        report.pop("column", None)
    img = parse(data)
    n = len(img.stream)
    with AD.feed_stream(ctx) as (ctx, side):
        at = staging_layout(n, 1, SEGMENT.itemsize, len(img.passes)) if tiles else staging_layout(n)
        staged = torch.empty(at.total, dtype=torch.uint8, pin_memory=True)
        host = staged.numpy()
        host[:n] = np.frombuffer(img.stream, np.uint8)
        host[at.palettes:at.pad] = img.palette.reshape(-1)
        if tiles:      # a table of one entry per pass rides behind the palette
            table = np.array([(p.stream_offset, p.pass_h, p.rowbytes) for p in img.passes], SEGMENT)
            _stage_table(host, at, table)
        dev = staged.cuda(non_blocking=True)
        out = torch.empty((img.header.height, img.header.width, 3), dtype=torch.uint8, device="cuda")
        base = dev.data_ptr()
        if tiles:
            # every pass goes to the tiles call, whatever its height
            _reconstruct(ctx.call, host.ctypes.data + at.table, base + at.table, base, n, [(img.bpp, 0, 0, len(table))])
            report["reconstruction"] = "tiles"
            report["sweeps"] = max(plan_tiles(p.pass_h, p.rowbytes, img.bpp).sweeps for p in img.passes)
            _expand_passes(ctx.call, img.header, img.passes, base, base + at.palettes, out)
        else:
            for p in img.passes:      # the launches interleave, pass by pass
                _unfilter_passes(ctx.call, [p], base, img.bpp)
                _expand_passes(ctx.call, img.header, [p], base, base + at.palettes, out)
    return AD.hand_over(out, side)


MANY_DEFAULT_WORKERS, MANY_MAX_WORKERS = 8, 16      # host threads of decode_device_many; fixed, not read off the machine


def _parse_indexed(item):
    index, data = item
    try:
        return parse(data)
    except ValueError as e:
        raise ValueError("file %d: %s" % (index, e)) from e


def plan_segments(img, base_offset=0, target_rows=0):
    """The segment table of one parsed image whose stream will stand at base_offset of the uploaded buffer: a structured array
    (offset int64, rows int32, rowbytes int32; radnet_png_segment) from radnet_png_plan_segments, pass after pass."""
    stream = np.frombuffer(img.stream, np.uint8)
    return np.concatenate([_plan_pass("radnet_png_plan_segments", stream.ctypes.data + p.stream_offset, p, base_offset + p.stream_offset, target_rows)
                           for p in img.passes])


def _read_file(item):
    """An item of decode_device_many as the file's bytes: a path is read as np.fromfile reads it, anything else is taken as it is."""
    return np.fromfile(item, np.uint8) if isinstance(item, (str, os.PathLike)) else item


def _decode_many_host(datas, ctx, workers, unfilter, indices=None):
    """decode_device_many with inflate="host": the files (bytes, no paths) parsed on host threads, one upload, one segment table.
    indices: what the files are called in a ValueError ("file <index>: "), default their positions."""
    import concurrent.futures
    import torch
    from . import augmentation_device as AD
    indices = range(len(datas)) if indices is None else indices
    workers = min(len(datas), MANY_DEFAULT_WORKERS) if workers is None else int(workers)
    workers = max(1, min(workers, MANY_MAX_WORKERS))
    pool = concurrent.futures.ThreadPoolExecutor(max_workers=workers)
    try:
        futures = [pool.submit(_parse_indexed, item) for item in zip(indices, datas)]
        try:
            imgs = [f.result() for f in futures]                          # the first failure, in index order, is raised here
        except BaseException:
            pool.shutdown(wait=True, cancel_futures=True)                 # files not yet started are not inflated for nothing
            raise
        starts = np.concatenate([[0], np.cumsum([len(im.stream) for im in imgs])]).astype(np.int64)
        n_streams = int(starts[-1])
        tables = list(pool.map(lambda k: plan_segments(imgs[k], int(starts[k])), range(len(imgs))))
        table, bpps = _sorted_segments(tables, [im.bpp for im in imgs])
        at = staging_layout(n_streams, len(imgs), SEGMENT.itemsize, len(table))
        staged = torch.empty(at.total, dtype=torch.uint8, pin_memory=True)
        host = staged.numpy()

        def stage(k):
            host[starts[k]:starts[k + 1]] = np.frombuffer(imgs[k].stream, np.uint8)
            host[at.palettes + 768 * k:at.palettes + 768 * (k + 1)] = imgs[k].palette.reshape(-1)
        list(pool.map(stage, range(len(imgs))))
    finally:
        pool.shutdown(wait=True)                                          # the host threads are done before any device work
    _stage_table(host, at, table)
    groups = _segment_groups(table, bpps, unfilter)
    with AD.feed_stream(ctx) as (ctx, side):
        dev = staged.cuda(non_blocking=True)
        base = dev.data_ptr()
        _reconstruct(ctx.call, host.ctypes.data + at.table, base + at.table, base, n_streams, groups)
        outs = []
        for k, im in enumerate(imgs):
            out = torch.empty((im.header.height, im.header.width, 3), dtype=torch.uint8, device="cuda")
            _expand_passes(ctx.call, im.header, im.passes, base + int(starts[k]), base + at.palettes + 768 * k, out)
            outs.append(out)
    return [AD.hand_over(out, side) for out in outs]


def _sorted_segments(tables, bpp_of):
    """ONE segment table of many files' tables: grouped by bpp, inside a group the segments of at most 64 rows first (the one-wave
    launch), then the long ones.  (table, the bpp of every entry)."""
    bpps = np.concatenate([np.full(len(t), bpp, np.int64) for t, bpp in zip(tables, bpp_of)])
    table = np.concatenate(tables)
    order = np.lexsort((table["rows"] > SEGMENT_ONE_WAVE_ROWS, bpps))
    return table[order], bpps[order]


def _segment_groups(table, bpps, unfilter):
    """The (bpp, first, short, count) groups _reconstruct takes of a table _sorted_segments made."""
    groups, first = [], 0
    for bpp, n in zip(*np.unique(bpps, return_counts=True)):
        # with tiles the long segments, which stand behind the short ones of their bpp, leave the segments call for the tiles call
        short = int((table["rows"][first:first + int(n)] <= TILE_ROWS).sum()) if unfilter == "tiles" else int(n)
        groups.append((int(bpp), first, short, int(n)))
        first += int(n)
    return groups


INFLATE_STREAM = np.dtype([("z_offset", np.int64), ("n", np.int64), ("out_offset", np.int64), ("expected", np.int64)])      # radnet_inflate_stream, 32 bytes
INFLATE_MANY_MAX_STREAMS = _constant("RADNET_INFLATE_MANY_MAX_STREAMS")
MANY_MAX_COMPRESSED, MANY_MAX_INFLATED = 1 << 29, 1 << 31      # a batch stays below both (radnet_inflate_streams_check)
MANY_GRAIN = 16      # RADNET_PNG_JOIN_GRAIN: every file and every stream of a batch begins on a 16-byte boundary of the device buffer
# where everything stands in the ONE pinned buffer of a batch: the stream table (room for one entry per file) in front, then the
# compressed bytes from `z` on (join="host": the joined streams; join="device": the files as they are), then what staging_layout
# arranges behind them: the palettes, the pad, the piece tables, the CRC table, its sums and its result
ManyStaging = collections.namedtuple("ManyStaging", "streams z palettes pad pieces table sums result total")


def many_layout(files, z_bytes, pieces=None, crc_count=0, sums=False):
    """ManyStaging of a batch of `files` files whose compressed bytes take z_bytes (every file's share rounded up to MANY_GRAIN)."""
    z = INFLATE_STREAM.itemsize * files      # a multiple of 16
    at = staging_layout(z + z_bytes, files, CRC_SEGMENT.itemsize if sums else 0, crc_count, sums=sums, pieces=pieces)
    return ManyStaging(0, z, at.palettes, at.pad, at.pieces if pieces is not None else at.table, at.table, at.sums, at.result, at.total)


def _grain(n):
    return (n + MANY_GRAIN - 1) & ~(MANY_GRAIN - 1)


def _count_idat(path):
    """How many IDAT chunks the file at `path` holds, by its chunk headers alone (a seek per chunk): the room its piece table needs
    in the pinned buffer before the file is read into it.  A broken file gives what was seen; the walk speaks later."""
    count = 0
    with open(path, "rb") as f:
        f.seek(33)
        while True:
            head = f.read(8)
            if len(head) < 8:
                return count
            length, kind = struct.unpack(">I4s", head)
            count += kind == b"IDAT"
            if kind == b"IEND":
                return count
            f.seek(length + 4, 1)


def _chain_stream(units, entry, z_offset, n, expected, out_offset, names):
    """The host chain of ONE stream of a batch: `units` is its slice of the batch's sorted records, whose bits are shifted back by
    8 * z_offset for radnet_inflate_chain / radnet_inflate_lz_chain (`entry`) and whose links are shifted forward again.
    (links, None, stats) or (None, the reason as decode_device words it, None)."""
    import ctypes
    from radnet_hip import lib as L
    if n < 7:
        return None, "a zlib stream of %d bytes" % n, None
    local = units.copy()
    shift = np.uint32(8 * z_offset)
    local["start_bit"] -= shift
    ok = local["status"] == 0
    local["end_bit"][ok] -= shift
    links = np.zeros(len(local), INFLATE_LINK)
    n_links, n_false, bad = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(-1)
    rc = getattr(L.load_library(), entry)(local.ctypes.data, len(local), 16, n, expected, links.ctypes.data, len(links), ctypes.byref(n_links),
                                          ctypes.byref(n_false), ctypes.byref(bad))
    if rc != 0:
        if rc < 0:
            raise RuntimeError("PNG: %s failed (%d)" % (entry, rc))
        why = "chain: " + names[rc]
        if rc == 2:
            why += " (%s)" % INFLATE_STATUS[int(local["status"][bad.value])]
        return None, why, None
    links = links[:n_links.value]
    chained = local[np.searchsorted(local["start_bit"], links["start_bit"])]
    stats = dict(false_candidates=n_false.value, units=len(links), blocks=int(chained["blocks"].sum()))
    if "far_matches" in (local.dtype.names or ()):
        stats["far_units"] = int((chained["far_matches"] > 0).sum())
    links["start_bit"] += shift
    links["out_offset"] += out_offset
    return links, None, stats


def _decode_batch_on_device(items, ctx, workers, unfilter, inflate, crc, join, reports, report):
    """One batch of decode_device_many's device inflate.  items: the files (bytes or paths); reports: one dict per file, filled as
    decode_device fills its report.  Returns (images, refused): images[k] is the device image of file k or None, refused the
    indices the host path has to take (reports[k]["reason"] says why); or None when the common candidate counter passed its cap."""
    import concurrent.futures
    import torch
    from radnet_hip.lib import RadnetError
    from . import augmentation_device as AD
    lz, tiles, crc_device, join_device = inflate == "device-lz", unfilter == "tiles", crc == "device", join == "device"
    count = len(items)
    is_path = [isinstance(d, (str, os.PathLike)) for d in items]
    workers = min(count, MANY_DEFAULT_WORKERS) if workers is None else max(1, min(int(workers), MANY_MAX_WORKERS))
    _lap(report, "_skip")
    walks, views = [None] * count, [None] * count

    def walk(k):
        try:
            walks[k] = _walk_compressed(views[k], crc)
        except ValueError as e:
            reports[k]["reason"] = "container: %s" % e
    with concurrent.futures.ThreadPoolExecutor(max_workers=workers) as pool:
        if join_device:
            # the files go up as they are: a path is read straight into its place in the pinned buffer, and walked there
            sizes = [os.path.getsize(d) if p else len(_byte_view(d)) for d, p in zip(items, is_path)]
            file_at = np.concatenate([[0], np.cumsum([_grain(n) for n in sizes])]).astype(np.int64)
            for k in range(count):
                if not is_path[k]:
                    views[k] = _byte_view(items[k])
            list(pool.map(walk, [k for k in range(count) if not is_path[k]]))
            piece_room = [_count_idat(items[k]) if is_path[k] else (len(walks[k].idat) if walks[k] else 0) for k in range(count)]
            at = many_layout(count, int(file_at[-1]), pieces=sum(piece_room), crc_count=sum(piece_room) if crc_device else 0, sums=crc_device)
            staged = torch.empty(at.total, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
            host = staged.numpy()

            def load(k):
                place = host[at.z + int(file_at[k]):at.z + int(file_at[k]) + sizes[k]]
                if is_path[k]:
                    with open(items[k], "rb") as f:
                        got = f.readinto(memoryview(place))
                    if got != sizes[k]:
                        reports[k]["reason"] = "container: PNG: the file changed while it was read (%d of %d bytes)" % (got, sizes[k])
                        return
                    views[k] = memoryview(place)
                    walk(k)
                    if walks[k] is not None and len(walks[k].idat) > piece_room[k]:
                        walks[k], reports[k]["reason"] = None, "container: PNG: the file changed while it was read"
                else:
                    place[:] = np.frombuffer(views[k], np.uint8)
            list(pool.map(load, range(count)))
        else:
            def read(k):
                views[k] = _byte_view(_read_file(items[k]))
                walk(k)
            list(pool.map(read, range(count)))
            z_room = [_grain(w.n) if w else 0 for w in walks]
            file_at = np.concatenate([[0], np.cumsum(z_room)]).astype(np.int64)      # here: where the joined streams stand
            idat_count = sum(len(w.idat) for w in walks if w) if crc_device else 0
            at = many_layout(count, int(file_at[-1]), crc_count=idat_count, sums=crc_device)
            staged = torch.empty(at.total, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
            host = staged.numpy()
            list(pool.map(lambda k: walks[k] and _join_payloads(host, at.z + int(file_at[k]), walks[k].source, walks[k].idat), range(count)))
    live = [k for k in range(count) if walks[k] is not None]      # the files the device is given
    refused = [k for k in range(count) if walks[k] is None]
    images = [None] * count
    if not live:
        return images, refused
    # the stream table: where each zlib stream stands in the common z (16-byte grains apart) and in the common output (back to back)
    streams = np.zeros(len(live), INFLATE_STREAM)
    z_at = np.concatenate([[0], np.cumsum([_grain(walks[k].n) for k in live])]).astype(np.int64) if join_device else file_at[live]
    out_at = np.concatenate([[0], np.cumsum([walks[k].expected for k in live])]).astype(np.int64)
    streams["z_offset"], streams["n"] = z_at[:len(live)], [walks[k].n for k in live]
    streams["out_offset"], streams["expected"] = out_at[:-1], [walks[k].expected for k in live]
    z_len = int(z_at[-1]) if join_device else int(file_at[-1])
    out_len = int(out_at[-1])
    host[at.streams:at.z] = 0
    host[at.streams:at.streams + streams.nbytes] = streams.view(np.uint8)
    host[at.pad:at.pieces] = 0
    for j, k in enumerate(live):
        host[at.palettes + 768 * k:at.palettes + 768 * (k + 1)] = walks[k].palette.reshape(-1)
    crc_tables, piece_tables, piece_at = [], [], []
    for j, k in enumerate(live):
        w = walks[k]
        if join_device:
            piece_at.append(sum(len(t) for t in piece_tables))
            piece_tables.append(join_pieces(w.idat))
        if crc_device:
            crc_tables.append(crc_segments(views[k], w.idat, int(z_at[j])))
    if join_device:
        pieces = np.concatenate(piece_tables)
        host[at.pieces:at.table] = 0
        host[at.pieces:at.pieces + pieces.nbytes] = pieces.view(np.uint8)
    if crc_device:
        crc_table = np.concatenate(crc_tables)
        crc_first = np.concatenate([[0], np.cumsum([len(t) for t in crc_tables])])      # where each file's chunks begin in the table
        host[at.table:at.total] = 0
        host[at.table:at.table + crc_table.nbytes] = crc_table.view(np.uint8)
        sums_at = at.table + crc_table.nbytes      # the sums and the result follow the entries there are
        result_at = sums_at + 4 * len(crc_table)
    _lap(report, "container_crc_ms")
    refuse = lambda k, why: (reports[k].update(reason=why), refused.append(k))      # noqa: E731
    with AD.feed_stream(ctx) as (ctx, side):
        call = functools.partial(_launch, report, ctx)
        dev = staged.cuda(non_blocking=True)
        _lap(report, "upload_ms")
        base = dev.data_ptr()
        if join_device:
            # one launch per file: a piece table tiles its output from 0 on, so each file joins into its own place of the common z
            zdev = torch.empty(max(z_len, 1), dtype=torch.uint8, device="cuda")
            zbase = zdev.data_ptr()
            for j, k in enumerate(live):
                shift = JOIN_PIECE.itemsize * piece_at[j]
                try:
                    call("radnet_png_join_u8", base + at.z + int(file_at[k]), sizes[k], staged.data_ptr() + at.pieces + shift, base + at.pieces + shift,
                         len(piece_tables[j]), zbase + int(z_at[j]), walks[k].n)
                except RadnetError as e:
                    refuse(k, "join: %s" % e)
        else:
            zdev, zbase = dev, base + at.z
        if crc_device:
            call("radnet_crc32_segments", zbase, z_len, staged.data_ptr() + at.table, base + at.table, len(crc_table), base + sums_at, base + result_at)
            verdict = torch.empty(2, dtype=torch.int32, pin_memory=True)
            verdict.copy_(dev[result_at:result_at + 8].view(torch.int32), non_blocking=True)
        head = (zbase, z_len, staged.data_ptr() + at.streams, base + at.streams, len(live))
        cap = z_len // 32 + 1024
        found = torch.zeros(cap + 1, dtype=torch.int32, device="cuda")      # the count, then the candidates
        call("radnet_inflate_find_blocks_many", *head, found.data_ptr() + 4, cap, found)
        found_host = found.cpu().numpy().view(np.uint32)
        _lap(report, "download_candidates_ms")
        n_cand = int(found_host[0])
        if n_cand > cap:
            return None      # the overflow belongs to no file: the caller decodes the batch file by file
        if crc_device:
            first_bad, n_bad = (int(v) for v in verdict)
            if n_bad:      # rare: the sums the device left say whose chunks they are
                sums = dev[sums_at:result_at].cpu().numpy().view(np.uint32)
                wrong = np.flatnonzero(sums != crc_table["expect"])
                for j in sorted(set(np.searchsorted(crc_first, wrong, side="right") - 1)):
                    refuse(live[j], "crc: IDAT chunk %d" % (int(wrong[wrong >= crc_first[j]][0]) - int(crc_first[j])))
        dtype, measure, chain, names, emit = ((INFLATE_LZ_UNIT, "radnet_inflate_lz_measure_many", "radnet_inflate_lz_chain", INFLATE_LZ_CHAIN, "radnet_inflate_lz_emit_many")
                                              if lz else (INFLATE_UNIT, "radnet_inflate_rle_measure_many", "radnet_inflate_chain", INFLATE_CHAIN, "radnet_inflate_rle_emit_many"))
        first_bits = (8 * streams["z_offset"] + 16).astype(np.uint32)
        starts = np.union1d(found_host[1:1 + n_cand], first_bits)
        units = np.zeros(len(starts), dtype)
        units["start_bit"] = starts
        units_dev = torch.from_numpy(units.view(np.uint8)).cuda()
        _lap(report, "sort_upload_units_ms")
        call(measure, *head, units_dev, len(units))
        units = units_dev.cpu().numpy().view(dtype)
        _lap(report, "download_units_ms")
        lo = np.searchsorted(starts, 8 * streams["z_offset"])
        hi = np.searchsorted(starts, 8 * (streams["z_offset"] + streams["n"]))
        cand_sorted = np.sort(found_host[1:1 + n_cand])
        all_links = []
        for j, k in enumerate(live):
            zo, n = int(streams["z_offset"][j]), int(streams["n"][j])
            reports[k]["candidates"] = int(np.searchsorted(cand_sorted, 8 * (zo + n)) - np.searchsorted(cand_sorted, 8 * zo))
            if k in refused:
                continue
            links, why, stats = _chain_stream(units[lo[j]:hi[j]], chain, zo, n, int(streams["expected"][j]), int(streams["out_offset"][j]), names)
            if links is None:
                refuse(k, why)
            else:
                reports[k].update(stats)
                all_links.append(links)
        going = [j for j, k in enumerate(live) if k not in refused]
        if not going:
            return images, sorted(refused)
        links = np.concatenate(all_links)
        links_dev = torch.from_numpy(links.view(np.uint8)).cuda()
        stream = torch.empty(max(out_len, 1), dtype=torch.uint8, device="cuda")
        _lap(report, "chain_upload_links_ms")
        if lz:
            # no link writes the sources of a refused stream's bytes: they are zeroed then, which is flat (0 is a root), so that the
            # shared rounds count the streams that go on and nothing else
            src = (torch.empty if len(going) == len(live) else torch.zeros)(max(out_len, 1), dtype=torch.int32, device="cuda")
            call(emit, *head, links_dev, len(links), stream, src, out_len)
            bound, ran, rounds = max(1, (max(out_len, 2) - 1).bit_length()), 0, None
            while rounds is None:
                if ran >= bound:
                    raise RuntimeError("PNG: the source table of %d bytes is not flat after %d rounds of radnet_inflate_lz_resolve" % (out_len, bound))
                group = min(4, bound - ran)
                changed = torch.zeros(group, dtype=torch.int32, device="cuda")
                call("radnet_inflate_lz_resolve", src, out_len, group, changed)
                still = np.flatnonzero(changed.cpu().numpy() == 0)
                _lap(report, "download_changed_ms")
                if len(still):
                    rounds = ran + int(still[0])
                ran += group
            call("radnet_inflate_lz_gather", src, stream, out_len)
        else:
            call(emit, *head, links_dev, len(links), stream, out_len)
        # the Adler-32 parts and the filter-type column of every stream that is still going, all enqueued in front of ONE download
        chunk = _constant("RADNET_DEFLATE_CHUNK")
        rooms = [DEFLATE_SYMBOLS * 4 + -(-int(streams["expected"][j]) // chunk) * 16 + sum(p.pass_h for p in walks[live[j]].passes) for j in going]
        tail_at = np.concatenate([[0], np.cumsum([(r + 7) & ~7 for r in rooms])]).astype(np.int64)
        tail = torch.zeros(int(tail_at[-1]), dtype=torch.uint8, device="cuda")
        for i, j in enumerate(going):
            w, expected, t = walks[live[j]], int(streams["expected"][j]), tail.data_ptr() + int(tail_at[i])
            sptr = stream.data_ptr() + int(streams["out_offset"][j])
            parts = t + DEFLATE_SYMBOLS * 4
            call("radnet_deflate_rle_scan_u8", sptr, expected, t, parts)
            offsets = np.array([p.stream_offset for p in w.passes], np.int64)
            pass_rows = np.array([p.pass_h for p in w.passes], np.int32)
            rowbytes = np.array([p.rowbytes for p in w.passes], np.int32)
            call("radnet_png_gather_column_u8", sptr, expected, offsets.ctypes.data, pass_rows.ctypes.data, rowbytes.ctypes.data, len(w.passes),
                 parts + -(-expected // chunk) * 16)
        tail_host = tail.cpu().numpy()
        _lap(report, "download_adler_column_ms")
        tables, taken = [], []
        for i, j in enumerate(going):
            k, expected = live[j], int(streams["expected"][j])
            w, t = walks[k], tail_host[int(tail_at[i]):int(tail_at[i]) + rooms[i]]
            n_parts = -(-expected // chunk)
            parts = t[DEFLATE_SYMBOLS * 4:DEFLATE_SYMBOLS * 4 + n_parts * 16].view(np.uint64)
            column = t[DEFLATE_SYMBOLS * 4 + n_parts * 16:]
            if adler32_of_parts(parts, expected) != w.trailer:
                refuse(k, "adler")
                continue
            if int(column.max()) > 4:
                refuse(k, "a filter type above 4")
                continue
            row0, mine = 0, []
            for p in w.passes:
                col = np.ascontiguousarray(column[row0:row0 + p.pass_h])
                mine.append(_plan_pass("radnet_png_plan_segments_column", col.ctypes.data, p, int(streams["out_offset"][j]) + p.stream_offset))
                row0 += p.pass_h
            tables.append(np.concatenate(mine))
            taken.append(j)
        if not taken:
            return images, sorted(refused)
        table, bpps = _sorted_segments(tables, [walks[live[j]].bpp for j in taken])
        table_dev = torch.from_numpy(table.view(np.uint8)).cuda()
        _lap(report, "plan_segments_ms")
        _reconstruct(call, table.ctypes.data, table_dev.data_ptr(), stream.data_ptr(), out_len, _segment_groups(table, bpps, unfilter))
        for j, mine in zip(taken, tables):
            k = live[j]
            w, r = walks[k], reports[k]
            out = torch.empty((w.header.height, w.header.width, 3), dtype=torch.uint8, device="cuda")
            _expand_passes(call, w.header, w.passes, stream.data_ptr() + int(streams["out_offset"][j]), base + at.palettes + 768 * k, out)
            images[k] = out
            r.update(path="device", reason=None, reconstruction="segments")
            if lz:
                r["rounds"] = rounds
            if tiles:
                long_ones = mine[mine["rows"] > TILE_ROWS]
                r["reconstruction"] = "segments+tiles" if len(long_ones) < len(mine) else "tiles"
                r["sweeps"] = max([plan_tiles(int(t["rows"]), int(t["rowbytes"]), w.bpp).sweeps for t in long_ones], default=0)
            if crc_device:
                r["crc"] = "device"
            if join_device:
                r["join"] = "device"
    return [im if im is None else AD.hand_over(im, side) for im in images], sorted(refused)


def _batches(items):
    """decode_device_many's batches: consecutive runs of the files whose lengths (each rounded up to 16; an upper bound of the
    compressed stream) stay below 2^29 in total, whose inflated streams stay below 2^31 and whose count stays within
    RADNET_INFLATE_MANY_MAX_STREAMS.  A file whose first 33 bytes give no geometry counts as empty: the walk refuses it."""
    runs, z, out = [[]], 0, 0
    for k, d in enumerate(items):
        try:
            size = os.path.getsize(d) if isinstance(d, (str, os.PathLike)) else len(_byte_view(d))
            expected = pass_geometry(read_header(d))[1]
        except (ValueError, OSError):
            size, expected = _grain(0), 0
        if runs[-1] and (z + _grain(size) >= MANY_MAX_COMPRESSED or out + expected >= MANY_MAX_INFLATED or len(runs[-1]) >= INFLATE_MANY_MAX_STREAMS):
            runs.append([])
            z = out = 0
        runs[-1].append(k)
        z, out = z + _grain(size), out + expected
    return runs


class HostInflateModeError(ValueError, TypeError):
    """decode_device_many asked for crc= or join= on the device beside its host inflate.  It is check_modes' ValueError, message
    included, as decode_device raises it; and it is still a TypeError, which is what the entry raised for these keywords while it
    had only the host inflate, so a caller that asked "does the many-file entry take this?" that way gets the answer it got."""


def decode_device_many(datas, ctx=None, workers=None, unfilter="band", inflate="host", crc="host", join="host", report=None):
    """decode_device for a list of files in one pass: a list of uint8 [H][W][3] (B, G, R) cuda tensors, byte for byte what
    [decode_device(d) for d in datas] returns.  The files are parsed (CRC, inflate) on `workers` host threads (default
    min(len(datas), 8), at most 16); a file that fails raises its ValueError prefixed with "file <index>: " before any device
    work.  Then ONE pinned staging buffer and ONE upload: the streams, the palettes, the segment table (8-byte aligned, short
    segments first inside each bpp); one radnet_png_unfilter_segments_u8 per distinct bpp; one radnet_png_expand_bgr_u8 per pass.
    ctx and the stream rules are decode_device's.  unfilter="tiles": inside each bpp the segments of at most 64 rows go as above and
    the longer ones to one radnet_png_unfilter_tiles_u8; the bytes are the same.  An item may be a path (str / os.PathLike): it is
    read as np.fromfile reads it.
    inflate="device" / "device-lz" (opt-in; crc="device" and join="device" need one of them, as check_modes says -- beside the host
    inflate that ValueError is a HostInflateModeError, which is also the TypeError the entry raised before it had the keywords): the result is
    byte for byte [decode_device(d, inflate=, unfilter=, crc=, join=) for d in datas], but the batch pays decode_device's host
    round trips once, not once per file.  The compressed streams go into ONE pinned buffer with ONE upload, every stream on a
    16-byte boundary, behind the radnet_inflate_stream table and in front of the palettes and the other tables (many_layout);
    with join="device" the FILES go up as they are -- a path is read with readinto straight into its place in the pinned
    buffer -- and one radnet_png_join_u8 per file gathers its stream into the common buffer.  Then ONE radnet_crc32_segments
    (crc="device"), ONE radnet_inflate_find_blocks_many, ONE measure, radnet_inflate_chain / radnet_inflate_lz_chain per stream on
    the host, ONE emit, for "device-lz" ONE shared resolve loop and gather, the Adler scan and the column gather of every file in
    front of ONE download, and the reconstruction over ONE segment table (planned from the downloaded columns) as above.
    A file the device refuses -- for decode_device's reasons: far matches under "device", a unit over the symbol cap, a chain
    refusal, Adler, a filter type above 4, a CRC mismatch, a container parse_compressed refuses -- goes, alone, to the path above
    together with the other refused ones; the rest keep the device path and the result keeps the order of `datas`.  An invalid
    file therefore raises what it raises today, "file <index>: ...", the lowest index first.  When the common candidate counter
    passes its cap (compressed bytes / 32 + 1024) the overflow belongs to no file, and the batch is decoded file by file through
    decode_device with the same modes; that is rare -- a stream needs a valid-looking dynamic header every 32 bytes.
    A list whose files reach 2^29 bytes in total (their lengths stand in for the compressed streams'), whose inflated streams reach
    2^31, or that holds more than RADNET_INFLATE_MANY_MAX_STREAMS files is cut into consecutive batches here.  "device-lz" keeps a
    source table of 4 bytes per inflated byte of a batch on the device beside the 1 byte of the stream itself.
    report (a dict): report["files"][k] carries decode_device's keys for file k (path, reason, candidates, false_candidates, units,
    blocks, reconstruction -- "segments", or with unfilter="tiles" "segments+tiles" / "tiles" -- and rounds, far_units, sweeps, crc,
    join in their modes; rounds is the batch's), report["batches"] the number of batches, report["overflow"] how many of them
    went file by file; a dict under report["stages"] receives the staged timing as in decode_device."""
    try:
        check_modes(inflate, unfilter, crc, join)
    except ValueError as e:
        if inflate == "host" and unfilter in UNFILTER_MODES and "device" in (crc, join):
            raise HostInflateModeError(str(e)) from None
        raise
    datas = list(datas)
    report = {} if report is None else report
    files = [dict(reason=None, candidates=0) for _ in datas]
    for r in files:
        _report_host_path(r, inflate, unfilter, crc, join)
    report.update(files=files, batches=0, overflow=0)
    if not datas:
        return []
    if inflate == "host":
        return _decode_many_host([_read_file(d) for d in datas], ctx, workers, unfilter)
    images, refused = [None] * len(datas), []
    for run in _batches(datas):
        report["batches"] += 1
        got = _decode_batch_on_device([datas[k] for k in run], ctx, workers, unfilter, inflate, crc, join, [files[k] for k in run], report)
        if got is None:
            report["overflow"] += 1
            for k in run:
                try:
                    images[k] = decode_device(_read_file(datas[k]), ctx, inflate=inflate, report=files[k], unfilter=unfilter, crc=crc, join=join)
                except ValueError as e:
                    raise ValueError("file %d: %s" % (k, e)) from e
            continue
        for k, im in zip(run, got[0]):
            images[k] = im
        refused += [run[i] for i in got[1]]
    if refused:
        refused = sorted(refused)
        for k in refused:
            _report_host_path(files[k], inflate, unfilter, crc, join)
        for k, im in zip(refused, _decode_many_host([_read_file(datas[k]) for k in refused], ctx, workers, unfilter, indices=refused)):
            images[k] = im
    return images


def imdecode_color(data):
    """cv2.imdecode(data, cv2.IMREAD_COLOR) for a PNG file's bytes: decode_device, downloaded to a NumPy array."""
    return decode_device(data).cpu().numpy()


# ---- writing ------------------------------------------------------------------------------------------------------------------------
FILTER_MODES = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": 5}      # `mode` of radnet_png_filter_rows_u8
STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "filtered": zlib.Z_FILTERED, "huffman": zlib.Z_HUFFMAN_ONLY, "rle": zlib.Z_RLE,
              "fixed": zlib.Z_FIXED}
IDAT_MAX = 0x7fffffff      # a chunk's length field


def _chunk_bytes(kind, payload=b""):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(payload, zlib.crc32(kind)))


def _zlib_header(level):
    """CMF / FLG for deflate with a 32 KiB window; FLEVEL as zlib derives it from the level, FCHECK so that the pair divides by 31."""
    level = 6 if level == -1 else level
    flevel = 0 if level in (0, 1) else 1 if level < 6 else 2 if level == 6 else 3
    head = (0x78 << 8) | (flevel << 6)
    return struct.pack(">H", head + (31 - head % 31) % 31)


def _deflate_piece(piece, level, strategy, last):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(piece) + c.flush(zlib.Z_FINISH if last else zlib.Z_SYNC_FLUSH)


def _workers(pieces, workers):
    workers = min(pieces, MANY_DEFAULT_WORKERS) if workers is None else int(workers)
    return max(1, min(workers, MANY_MAX_WORKERS))


def assemble(stream_bytes, width, height, color_type, level=1, strategy="rle", workers=None, chunk_bytes=1 << 20):
    """The PNG file of a filtered scanline stream (8 bits per sample, colour type 0 or 2, not interlaced): signature, IHDR, one
    IDAT, IEND.  The stream is cut into ranges of chunk_bytes bytes; each is deflated raw (zlib.compressobj(level, DEFLATED, -15, 9,
    strategy)) on one of `workers` host threads (default min(pieces, 8), at most 16) and ends in Z_SYNC_FLUSH, the last in
    Z_FINISH; the IDAT holds the zlib header, the pieces in order and zlib.adler32 of the whole stream.  No device is involved.
    The bytes depend on the arguments other than `workers`; the inflated stream depends on stream_bytes alone."""
    import concurrent.futures
    view = memoryview(stream_bytes).cast("B")
    width, height, level, chunk_bytes = int(width), int(height), int(level), int(chunk_bytes)
    if color_type not in (0, 2):
        raise ValueError("PNG: the writer takes colour type 0 or 2, not %r" % (color_type,))
    if width < 1 or height < 1 or width > 0x7fffffff or height > 0x7fffffff:
        raise ValueError("PNG: illegal size %d x %d" % (width, height))
    if len(view) != height * (1 + width * CHANNELS[color_type]):
        raise ValueError("PNG: a stream of %d bytes for %d x %d pixels of colour type %d" % (len(view), width, height, color_type))
    if not -1 <= level <= 9:
        raise ValueError("PNG: deflate level %d" % level)
    if chunk_bytes < 1:
        raise ValueError("PNG: chunk_bytes %d" % chunk_bytes)
    if isinstance(strategy, str):
        if strategy not in STRATEGIES:
            raise ValueError("PNG: unknown deflate strategy %r (one of %s)" % (strategy, ", ".join(sorted(STRATEGIES))))
        strategy = STRATEGIES[strategy]
    starts = range(0, len(view), chunk_bytes)
    jobs = [(view[s:s + chunk_bytes], level, strategy, s + chunk_bytes >= len(view)) for s in starts]
    workers = _workers(len(jobs), workers)
    if workers == 1:
        pieces = [_deflate_piece(*job) for job in jobs]
        adler = zlib.adler32(view)
    else:
        with concurrent.futures.ThreadPoolExecutor(max_workers=workers) as pool:
            check = pool.submit(zlib.adler32, view)
            pieces = list(pool.map(lambda job: _deflate_piece(*job), jobs))
            adler = check.result()
    idat = b"".join([_zlib_header(level)] + pieces + [struct.pack(">I", adler & 0xffffffff)])
    if len(idat) > IDAT_MAX:
        raise ValueError("PNG: an IDAT chunk of %d bytes (at most 2^31 - 1)" % len(idat))
    ihdr = struct.pack(">IIBBBBB", width, height, 8, color_type, 0, 0, 0)
    return b"".join([SIGNATURE, _chunk_bytes(b"IHDR", ihdr), _chunk_bytes(b"IDAT", idat), _chunk_bytes(b"IEND")])


def _filter_mode(filter):
    if isinstance(filter, str):
        if filter not in FILTER_MODES:
            raise ValueError("PNG: unknown filter %r (one of %s, or 0..4)" % (filter, ", ".join(FILTER_MODES)))
        return FILTER_MODES[filter]
    if int(filter) not in range(5):
        raise ValueError("PNG: filter type %r (0..4, or a name)" % (filter,))
    return int(filter)


def check_writable(img):
    """(height, width, channels) of an image encode_device takes: uint8, [H][W][3] or [H][W], not empty, contiguous if on the device."""
    if str(img.dtype).split(".")[-1] != "uint8":
        raise TypeError("PNG: the writer takes a uint8 image, not %s" % (img.dtype,))
    shape = tuple(int(v) for v in img.shape)
    if len(shape) not in (2, 3) or (len(shape) == 3 and shape[2] != 3):
        raise ValueError("PNG: the writer takes an image [H][W][3] (B, G, R) or [H][W], not shape %s" % (shape,))
    if shape[0] < 1 or shape[1] < 1:
        raise ValueError("PNG: the writer takes no empty image, shape %s" % (shape,))
    if not isinstance(img, np.ndarray) and not img.is_contiguous():
        raise ValueError("PNG: a device image must be contiguous (strides %s for shape %s)" % (img.stride(), shape))
    return shape[0], shape[1], 1 if len(shape) == 2 else 3


# ---- deflate on the device ---------------------------------------------------------------------------------------------------------
DEFLATE_CODE = np.dtype([("bits", np.uint16), ("length", np.uint16)])      # radnet_deflate_code, 4 bytes
DEFLATE_SYMBOLS = 286
DEFLATE_DIST_SYMBOLS = 30
HuffmanCode = collections.namedtuple("HuffmanCode", "code header header_nbits dist_nbits")      # the arguments of radnet_deflate_rle_emit_u8


def huffman_code(hist):
    """The literal/length code of an image from the 286 counts of radnet_deflate_rle_scan_u8 and the dynamic block header that
    describes it (radnet_deflate_build_code: host only, no device): HuffmanCode(code, header, header_nbits, dist_nbits) with code a
    structured array of 286 (bits, length), lengths of at most 15 bits and Kraft sum 1, header the block header's bytes (BFINAL 0,
    BTYPE 10, ...; header_nbits bits of them count) and dist_nbits = 1, the distance code of the one-symbol distance table."""
    import ctypes
    from radnet_hip import lib as L
    hist = np.ascontiguousarray(hist, np.uint32).reshape(-1)
    if hist.size != DEFLATE_SYMBOLS:
        raise ValueError("PNG: a histogram of %d counts (the literal/length alphabet has %d)" % (hist.size, DEFLATE_SYMBOLS))
    code = np.zeros(DEFLATE_SYMBOLS, DEFLATE_CODE)
    header = np.zeros(_constant("RADNET_DEFLATE_HEADER_MAX_BITS") // 8, np.uint8)
    nbits = ctypes.c_int32(0)
    rc = L.load_library().radnet_deflate_build_code(hist.ctypes.data, code.ctypes.data, header.ctypes.data, header.size, ctypes.byref(nbits))
    if rc != 0:
        raise ValueError("PNG: radnet_deflate_build_code failed (%d)" % rc)
    return HuffmanCode(code, header[:(nbits.value + 7) // 8].tobytes(), nbits.value, 1)


def fixed_code():
    """The fixed code of RFC 1951, 3.2.6 as a HuffmanCode: lengths 8 / 9 / 7 / 8, canonical; the header is BFINAL 0, BTYPE 01; a
    distance code has 5 bits."""
    code = np.zeros(DEFLATE_SYMBOLS, DEFLATE_CODE)
    s = np.arange(DEFLATE_SYMBOLS)
    code["length"] = np.where(s < 144, 8, np.where(s < 256, 9, np.where(s < 280, 7, 8)))
    code["bits"] = np.where(s < 144, 0x30 + s, np.where(s < 256, 0x190 + s - 144, np.where(s < 280, s - 256, 0xC0 + s - 280)))
    return HuffmanCode(code, b"\x02", 3, 5)


def adler32_of_parts(parts, n):
    """The Adler-32 of a stream of n bytes from radnet_deflate_rle_scan_u8's parts, per chunk of len bytes at offset s the sums
    S1 = sum(byte[i]) and S2 = sum((len - i) * byte[i]):  a = 1 + sum(S1),  b = n + sum(S2 + (n - s - len) * S1),  both mod 65521."""
    chunk = _constant("RADNET_DEFLATE_CHUNK")
    a, b = 1, int(n)
    for c, (s1, s2) in enumerate(np.asarray(parts, np.uint64).reshape(-1, 2).tolist()):
        start = c * chunk
        a += s1
        b += s2 + (n - start - min(chunk, n - start)) * s1
    return ((b % 65521) << 16) | (a % 65521)


def _gf2_times(mat, vec):
    out, i = 0, 0
    while vec:
        if vec & 1:
            out ^= mat[i]
        vec >>= 1
        i += 1
    return out


def crc32_combine(crc1, crc2, len2):
    """zlib.crc32(a + b) from crc1 = zlib.crc32(a), crc2 = zlib.crc32(b) and len2 = len(b): zlib's crc32_combine (the operator that
    appends len2 zero bytes, by repeated squaring over GF(2)), which the standard library does not export."""
    if len2 <= 0:
        return crc1
    square = lambda mat: [_gf2_times(mat, mat[n]) for n in range(32)]      # noqa: E731
    odd = [0xedb88320] + [1 << n for n in range(31)]      # the operator for one zero bit
    even = square(odd)                                     # two
    odd = square(even)                                     # four
    while True:
        even = square(odd)
        if len2 & 1:
            crc1 = _gf2_times(even, crc1)
        len2 >>= 1
        if not len2:
            break
        odd = square(even)
        if len2 & 1:
            crc1 = _gf2_times(odd, crc1)
        len2 >>= 1
        if not len2:
            break
    return crc1 ^ crc2


def crc32_device(t, value=0, ctx=None):
    """zlib.crc32(bytes of t, value) of a contiguous uint8 cuda tensor, summed where it stands: radnet_crc32_segments with one
    segment (csrc/crc32.hip), one small upload (the table) and one small download (the sum).  ctx as for decode_device."""
    import torch
    from . import augmentation_device as AD
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()):
        raise TypeError("PNG: crc32_device takes a contiguous uint8 cuda tensor")
    if not 0 <= int(value) <= 0xffffffff:
        raise ValueError("PNG: a running CRC-32 of %d" % int(value))
    n = int(t.numel())
    table = np.zeros(1, CRC_SEGMENT)
    table[0] = (0, n, int(value), 0)
    producer = torch.cuda.current_stream()
    with AD.feed_stream(ctx) as (ctx, side):
        if side is not None:
            side.wait_stream(producer)
            t.record_stream(side)
        work = torch.zeros(CRC_SEGMENT.itemsize + 16, dtype=torch.uint8, device="cuda")      # the table, the sum, the result
        work[:CRC_SEGMENT.itemsize].copy_(torch.from_numpy(table.view(np.uint8)))
        at = work.data_ptr() + CRC_SEGMENT.itemsize
        ctx.call("radnet_crc32_segments", t.data_ptr() if n else None, n, table.ctypes.data, work, 1, at, at + 4)
        return int(work[CRC_SEGMENT.itemsize:CRC_SEGMENT.itemsize + 4].cpu().numpy().view(np.uint32)[0])


def _crc32_threads(view, crc, workers=MANY_DEFAULT_WORKERS, least=1 << 20):
    """zlib.crc32(view, crc) with the buffer cut into at most `workers` ranges of at least `least` bytes, each summed on a host thread
    (zlib releases the GIL) and the sums joined by crc32_combine."""
    import concurrent.futures
    n = len(view)
    ranges = max(1, min(workers, n // least))
    if ranges == 1:
        return zlib.crc32(view, crc)
    step = -(-n // ranges)
    with concurrent.futures.ThreadPoolExecutor(max_workers=ranges) as pool:
        sums = list(pool.map(lambda s: zlib.crc32(view[s:s + step]), range(0, n, step)))
    for k, part in enumerate(sums):
        crc = crc32_combine(crc, part, min(step, n - k * step))
    return crc


def assemble_pieces(packed, adler, width, height, color_type, idat_crc=None):
    """The PNG file round a deflate stream made elsewhere (8 bits per sample, colour type 0 or 2, not interlaced): signature, IHDR,
    one IDAT holding the zlib header 78 01, `packed` (raw deflate blocks, the last one final) and the Adler-32 `adler` of what they
    inflate to, IEND.  Nothing is inflated or checked here but the sizes.  `packed` is read twice and copied once: the chunk's
    CRC-32 is summed over ranges of it on up to 8 host threads, then the file is joined.  idat_crc: the running value behind
    `packed`, zlib.crc32(b"IDAT" + the zlib header + packed), summed elsewhere (deflate_device(crc="device")); then only the 4 Adler
    bytes are added here and `packed` is read once.  The caller answers for it: a wrong value gives a file with a wrong CRC."""
    width, height, adler = int(width), int(height), int(adler)
    if color_type not in (0, 2):
        raise ValueError("PNG: the writer takes colour type 0 or 2, not %r" % (color_type,))
    if width < 1 or height < 1 or width > 0x7fffffff or height > 0x7fffffff:
        raise ValueError("PNG: illegal size %d x %d" % (width, height))
    if not 0 <= adler <= 0xffffffff:
        raise ValueError("PNG: an Adler-32 of %d" % adler)
    view = memoryview(packed).cast("B")
    if len(view) + 6 > IDAT_MAX:
        raise ValueError("PNG: an IDAT chunk of %d bytes (at most 2^31 - 1)" % (len(view) + 6))
    head, tail = b"IDAT" + _zlib_header(1), struct.pack(">I", adler)
    if idat_crc is not None and not 0 <= int(idat_crc) <= 0xffffffff:
        raise ValueError("PNG: a running CRC-32 of %d" % int(idat_crc))
    crc = zlib.crc32(tail, _crc32_threads(view, zlib.crc32(head)) if idat_crc is None else int(idat_crc))
    ihdr = struct.pack(">IIBBBBB", width, height, 8, color_type, 0, 0, 0)
    return b"".join([SIGNATURE, _chunk_bytes(b"IHDR", ihdr), struct.pack(">I", len(view) + 6), head, view, tail, struct.pack(">I", crc), _chunk_bytes(b"IEND")])


def deflate_device(dev, ctx, huffman="dynamic", crc="host"):
    """(packed, adler): the raw deflate blocks (bytes-like, in a pinned buffer) and the Adler-32 of the uint8 cuda tensor `dev` of n
    bytes, on the radnet context ctx whose stream is current: scan, ONE small download (286 counts, the Adler parts), the code
    (huffman_code, or fixed_code for huffman="fixed"), emit, pack, the 8 bytes of the total, ONE download of exactly that many.
    crc="device": (packed, adler, idat_crc) -- the packed bytes are summed where they stand (radnet_crc32_segments, one segment)
    and idat_crc, what assemble_pieces takes, is zlib.crc32(b"IDAT" + the zlib header + packed); its 4 bytes come down in the
    download of the packed bytes."""
    import torch
    _check_crc(crc)
    n = int(dev.numel())
    chunk = _constant("RADNET_DEFLATE_CHUNK")
    chunks = -(-n // chunk)
    scan = torch.zeros(DEFLATE_SYMBOLS * 4 + chunks * 16, dtype=torch.uint8, device="cuda")      # 1144 bytes: the parts stand 8-aligned
    ctx.call("radnet_deflate_rle_scan_u8", dev, n, scan, scan.data_ptr() + DEFLATE_SYMBOLS * 4)
    scan_host = torch.empty(scan.numel(), dtype=torch.uint8, pin_memory=True)
    scan_host.copy_(scan, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    hist = scan_host.numpy()[:DEFLATE_SYMBOLS * 4].view(np.uint32)
    adler = adler32_of_parts(scan_host.numpy()[DEFLATE_SYMBOLS * 4:].view(np.uint64), n)
    hc = fixed_code() if huffman == "fixed" else huffman_code(hist)
    return _emit_rle(dev, ctx, hc, hist, adler, crc)


def _emit_rle(dev, ctx, hc, hist, adler, crc):
    """deflate_device behind its scan: the run-length pieces of `dev` with the code hc built from the counts hist."""
    from radnet_hip import lib as L
    n = int(dev.numel())
    chunks = -(-n // _constant("RADNET_DEFLATE_CHUNK"))
    piece_cap = int(L.load_library().radnet_deflate_piece_cap(hc.code.ctypes.data, hc.header_nbits, hc.dist_nbits))
    if piece_cap < 0:
        raise ValueError("PNG: radnet_deflate_piece_cap failed (%d)" % piece_cap)
    header = np.frombuffer(hc.header, np.uint8)
    emit = lambda pieces, sizes: ctx.call("radnet_deflate_rle_emit_u8", dev, n, hc.code.ctypes.data, header.ctypes.data, hc.header_nbits,      # noqa: E731
                                          hc.dist_nbits, pieces, piece_cap, sizes)
    # the bits of all tokens follow from the counts (a match: at most 5 extra bits and the distance code); per piece the header,
    # the flush and the padding come on top
    counts = hist.astype(np.int64)
    token_bits = int((counts * hc.code["length"].astype(np.int64)).sum()) + int(counts[257:].sum()) * (5 + hc.dist_nbits)
    out_cap = (token_bits + 7) // 8 + chunks * ((hc.header_nbits + 7) // 8 + 16)
    return _emit_pack_download(ctx, emit, chunks, piece_cap, out_cap, adler, crc)


def huffman_codes_lz(hist_ll, hist_d):
    """The two codes of an image from the counts of radnet_deflate_lz_scan_u8 and the dynamic block header that describes them
    (radnet_deflate_build_codes_lz: host only, no device): (code_ll [286], code_d [30], header bytes, header_nbits)."""
    import ctypes
    from radnet_hip import lib as L
    hist_ll = np.ascontiguousarray(hist_ll, np.uint32).reshape(-1)
    hist_d = np.ascontiguousarray(hist_d, np.uint32).reshape(-1)
    if hist_ll.size != DEFLATE_SYMBOLS or hist_d.size != DEFLATE_DIST_SYMBOLS:
        raise ValueError("PNG: histograms of %d and %d counts (the alphabets have %d and %d)" % (hist_ll.size, hist_d.size, DEFLATE_SYMBOLS, DEFLATE_DIST_SYMBOLS))
    code_ll, code_d = np.zeros(DEFLATE_SYMBOLS, DEFLATE_CODE), np.zeros(DEFLATE_DIST_SYMBOLS, DEFLATE_CODE)
    header = np.zeros(_constant("RADNET_DEFLATE_HEADER_MAX_BITS") // 8, np.uint8)
    nbits = ctypes.c_int32(0)
    rc = L.load_library().radnet_deflate_build_codes_lz(hist_ll.ctypes.data, hist_d.ctypes.data, code_ll.ctypes.data, code_d.ctypes.data, header.ctypes.data,
                                                        header.size, ctypes.byref(nbits))
    if rc != 0:
        raise ValueError("PNG: radnet_deflate_build_codes_lz failed (%d)" % rc)
    return code_ll, code_d, header[:(nbits.value + 7) // 8].tobytes(), nbits.value


def stream_bits(hist_ll, code_ll, header_nbits, chunks, hist_d=None, code_d=None, dist_nbits=0):
    """radnet_deflate_stream_bits: the bits of all headers, tokens and end-of-blocks of `chunks` pieces with these counts and codes;
    without hist_d and code_d the run-length rule, every match followed by dist_nbits bits."""
    from radnet_hip import lib as L
    hist_ll = np.ascontiguousarray(hist_ll, np.uint32)
    hist_d = None if hist_d is None else np.ascontiguousarray(hist_d, np.uint32)
    bits = int(L.load_library().radnet_deflate_stream_bits(hist_ll.ctypes.data, None if hist_d is None else hist_d.ctypes.data, code_ll.ctypes.data,
                                                           None if code_d is None else code_d.ctypes.data, dist_nbits, header_nbits, chunks))
    if bits < 0:
        raise ValueError("PNG: radnet_deflate_stream_bits failed (%d)" % bits)
    return bits


def deflate_device_lz(dev, ctx, near=1, crc="host", report=None):
    """deflate_device with far matches (csrc/deflate_lz.hip, THE LZ TOKEN RULE of include/radnet_hip.h), priced against the
    run-length rule before anything is emitted: both scans run -- radnet_deflate_rle_scan_u8 and radnet_deflate_lz_scan_u8 with
    `near`, the pixel stride --, ONE small download brings both sets of counts and the Adler parts, both codes are built and
    radnet_deflate_stream_bits gives both sizes.  The LZ stream is emitted when bits_lz + 7 * chunks < bits_rle (a piece pads up to
    7 bits more under one rule than under the other, so the file is then never the longer one); otherwise, ties included, the
    run-length stream is, and the bytes are deflate_device's.  Returns what deflate_device returns.  A dict passed as `report`
    receives rule ("lz" or "rle"), bits_lz, bits_rle, matches (the LZ rule's) and far_matches (those at a distance other than 1 and
    `near`: the distance counts cannot tell more, and tell this only for near <= 4).  The token table takes 4 bytes per stream byte
    on the device (about 190 MB for a 4000x4000 RGB map) and is allocated before the rules are priced, so also when run-length wins."""
    import torch
    _check_crc(crc)
    from radnet_hip import lib as L
    n = int(dev.numel())
    chunks = -(-n // _constant("RADNET_DEFLATE_CHUNK"))
    ll, dd = DEFLATE_SYMBOLS * 4, DEFLATE_DIST_SYMBOLS * 4
    at_lz, at_d, at_parts = ll, 2 * ll, (2 * ll + dd + 7) & ~7      # the run-length counts, the LZ counts, the distance counts, the parts
    scan = torch.zeros(at_parts + chunks * 16, dtype=torch.uint8, device="cuda")
    tokens = torch.empty(n, dtype=torch.int32, device="cuda")
    base = scan.data_ptr()
    ctx.call("radnet_deflate_rle_scan_u8", dev, n, scan, base + at_parts)      # both scans write the same Adler parts, to the same place
    ctx.call("radnet_deflate_lz_scan_u8", dev, n, int(near), tokens, base + at_lz, base + at_d, base + at_parts)
    scan_host = torch.empty(scan.numel(), dtype=torch.uint8, pin_memory=True)
    scan_host.copy_(scan, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    host = scan_host.numpy()
    hist_rle, hist_ll, hist_d = host[:ll].view(np.uint32), host[at_lz:at_lz + ll].view(np.uint32), host[at_d:at_d + dd].view(np.uint32)
    adler = adler32_of_parts(host[at_parts:].view(np.uint64), n)
    hc = huffman_code(hist_rle)
    code_ll, code_d, header_bytes, header_nbits = huffman_codes_lz(hist_ll, hist_d)
    bits_rle = stream_bits(hist_rle, hc.code, hc.header_nbits, chunks, dist_nbits=hc.dist_nbits)
    bits_lz = stream_bits(hist_ll, code_ll, header_nbits, chunks, hist_d, code_d)
    rule = "lz" if bits_lz + 7 * chunks < bits_rle else "rle"
    if report is not None:
        near_symbols = {0} | ({near - 1} if near <= 4 else set())
        report.update(rule=rule, bits_lz=bits_lz, bits_rle=bits_rle, matches=int(hist_ll[257:].sum()),
                      far_matches=int(sum(int(c) for s, c in enumerate(hist_d) if s not in near_symbols)))
    if rule == "rle":
        return _emit_rle(dev, ctx, hc, hist_rle, adler, crc)
    piece_cap = int(L.load_library().radnet_deflate_lz_piece_cap(code_ll.ctypes.data, code_d.ctypes.data, header_nbits))
    if piece_cap < 0:
        raise ValueError("PNG: radnet_deflate_lz_piece_cap failed (%d)" % piece_cap)
    header = np.frombuffer(header_bytes, np.uint8)
    emit = lambda pieces, sizes: ctx.call("radnet_deflate_lz_emit_u8", dev, n, tokens, code_ll.ctypes.data, code_d.ctypes.data, header.ctypes.data,      # noqa: E731
                                          header_nbits, pieces, piece_cap, sizes)
    out_cap = (bits_lz + 7) // 8 + chunks * 16     # exact but for each piece's flush and padding
    return _emit_pack_download(ctx, emit, chunks, piece_cap, out_cap, adler, crc)


def _emit_pack_download(ctx, emit, chunks, piece_cap, out_cap, adler, crc):
    """The second half of deflate_device and deflate_device_lz: emit(pieces, sizes) writes `chunks` pieces of at most piece_cap bytes,
    radnet_deflate_pack moves them together (out_cap: what they cannot pass), the 8 bytes of the total and then exactly that many
    bytes come down; crc="device" sums them first.  Returns what deflate_device returns."""
    import torch
    pieces = torch.empty(chunks * piece_cap, dtype=torch.uint8, device="cuda")
    sizes = torch.empty(chunks, dtype=torch.int32, device="cuda")
    emit(pieces, sizes)
    room = 8 + CRC_SEGMENT.itemsize + 12 if crc == "device" else 0      # behind the packed bytes: padding, one segment, its sum, the result
    out = torch.empty(out_cap + room, dtype=torch.uint8, device="cuda")
    total = torch.empty(1, dtype=torch.int64, device="cuda")
    ctx.call("radnet_deflate_pack", pieces, piece_cap, sizes, chunks, out, out_cap, total)
    total_host = torch.empty(1, dtype=torch.int64, pin_memory=True)
    total_host.copy_(total, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    size = int(total_host[0])
    if size > out_cap:
        raise RuntimeError("PNG: the deflate pieces hold %d bytes, more than the %d their counts allow" % (size, out_cap))
    if crc != "device":
        packed = torch.empty(size, dtype=torch.uint8, pin_memory=True)
        packed.copy_(out[:size], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return packed.numpy(), adler
    # the chunk's sum, as far as the packed bytes: one segment over out[:size] that starts from the sum of the type and the zlib header.
    # The table goes up, and the sum comes down, in the buffer of the packed bytes: no launch and no wait but radnet_crc32_segments's own
    table_at = (size + 7) & ~7
    sum_at = table_at + CRC_SEGMENT.itemsize
    table = torch.zeros(CRC_SEGMENT.itemsize, dtype=torch.uint8, pin_memory=True)
    table.numpy().view(CRC_SEGMENT)[0] = (0, size, zlib.crc32(b"IDAT" + _zlib_header(1)), 0)
    out[table_at:sum_at].copy_(table, non_blocking=True)
    ctx.call("radnet_crc32_segments", out, size, table.data_ptr(), out.data_ptr() + table_at, 1, out.data_ptr() + sum_at, out.data_ptr() + sum_at + 4)
    packed = torch.empty(sum_at + 4, dtype=torch.uint8, pin_memory=True)
    packed.copy_(out[:sum_at + 4], non_blocking=True)
    torch.cuda.current_stream().synchronize()
    return packed.numpy()[:size], adler, int(packed.numpy()[sum_at:sum_at + 4].view(np.uint32)[0])


HOST_DEFLATE_DEFAULTS = dict(level=1, strategy="rle", workers=None, chunk_bytes=1 << 20)


def encode_device(img, filter="adaptive", level=1, strategy="rle", workers=None, chunk_bytes=1 << 20, ctx=None, deflate="host", huffman="dynamic", crc="host",
                  report=None):
    """The PNG file (bytes) of a contiguous uint8 cuda tensor [H][W][3] (B, G, R; written as 8-bit RGB) or [H][W] (8-bit grey); a
    NumPy array is uploaded first -- there is no CPU filter path, as there is no CPU reconstruction.  filter: "adaptive" (per row
    the type with the smallest sum of |signed residual|, the lowest on a tie), a fixed type 0..4 or its name.  One
    radnet_png_filter_rows_u8 launch, one download of the stream into a pinned buffer, then assemble() with level / strategy
    (OpenCV's imwrite defaults: 1, Z_RLE) / workers / chunk_bytes.  ctx and the stream rules are decode_device's; a worker thread's
    own stream waits for the stream that is current at the call, where the image is taken to be ready.
    deflate="device": the stream stays on the device and is deflated there (deflate_device: run-length tokens, one Huffman code per
    image for huffman="dynamic", RFC 1951's fixed code for huffman="fixed"); only the compressed bytes come down and
    assemble_pieces wraps them.  The file inflates to the same stream as the host path's but its bytes differ.  level, strategy,
    workers and chunk_bytes belong to the host deflate: any of them off its default together with deflate="device" is a ValueError.
    crc="device" (opt-in; needs deflate="device", with deflate="host" it is a ValueError): the IDAT chunk's CRC-32 is summed over the
    packed bytes on the device (csrc/crc32.hip) and comes down with them; the host adds the 4 Adler bytes.  The file's bytes are
    those of crc="host".
    deflate="device-lz" (opt-in): deflate="device" with far matches (deflate_device_lz; `near` is the pixel stride, 3 or 1): the LZ
    stream and the run-length stream are priced from their counts and the smaller one is emitted, so the file is never longer than
    deflate="device"'s and equals it byte for byte when run-length wins.  One dynamic code pair per image: huffman="fixed" is a
    ValueError beside it, as the host deflate's keywords are; crc="device" is accepted.  A dict passed as `report` receives rule
    ("lz" or "rle"), bits_lz, bits_rle, matches and far_matches in this mode and is left alone in the others."""
    import torch
    from . import augmentation_device as AD
    mode = _filter_mode(filter)
    if deflate not in ("host", "device", "device-lz"):
        raise ValueError("PNG: deflate=%r (\"host\", \"device\" or \"device-lz\")" % (deflate,))
    if huffman not in ("dynamic", "fixed"):
        raise ValueError("PNG: huffman=%r (\"dynamic\" or \"fixed\")" % (huffman,))
    _check_crc(crc)
    if crc == "device" and deflate == "host":
        raise ValueError("PNG: crc=\"device\" sums the bytes deflate=\"device\" leaves on the device and cannot be set with deflate=\"host\"")
    if deflate != "host":
        given = dict(level=level, strategy=strategy, workers=workers, chunk_bytes=chunk_bytes)
        off = sorted(k for k, v in given.items() if v != HOST_DEFLATE_DEFAULTS[k])
        if off:
            raise ValueError("PNG: %s belong%s to the host deflate and cannot be set with deflate=\"%s\"" % (", ".join(off), "s" if len(off) == 1 else "", deflate))
    if deflate == "device-lz" and huffman == "fixed":
        raise ValueError("PNG: deflate=\"device-lz\" builds its two codes from the image and cannot be set with huffman=\"fixed\"")
    h, w, channels = check_writable(img)
    if isinstance(img, np.ndarray):
        img = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    elif not img.is_cuda:
        raise TypeError("PNG: the writer takes a cuda tensor or a NumPy array, not a tensor on %s" % (img.device,))
    n = h * (1 + w * channels)
    producer = torch.cuda.current_stream()
    with AD.feed_stream(ctx) as (ctx, side):
        if side is not None:
            side.wait_stream(producer)
            img.record_stream(side)
        dev = torch.empty(n, dtype=torch.uint8, device="cuda")
        ctx.call("radnet_png_filter_rows_u8", img, h, w, channels, w * channels, mode, dev)
        if deflate == "device-lz":
            packed, adler, *idat_crc = deflate_device_lz(dev, ctx, near=channels, crc=crc, report=report)
            return assemble_pieces(packed, adler, w, h, 2 if channels == 3 else 0, idat_crc=idat_crc[0] if idat_crc else None)
        if deflate == "device":
            if crc == "device":
                packed, adler, idat_crc = deflate_device(dev, ctx, huffman, crc="device")
                return assemble_pieces(packed, adler, w, h, 2 if channels == 3 else 0, idat_crc=idat_crc)
            packed, adler = deflate_device(dev, ctx, huffman)
            return assemble_pieces(packed, adler, w, h, 2 if channels == 3 else 0)
        staged = torch.empty(n, dtype=torch.uint8, pin_memory=True)
        staged.copy_(dev, non_blocking=True)
        torch.cuda.current_stream().synchronize()
    return assemble(staged.numpy(), w, h, 2 if channels == 3 else 0, level, strategy, workers, chunk_bytes)
