"""PNG encode on the device (``pano_png_filter``, ``pano_deflate``, csrc/png_enc.hip).

A PNG cannot be Pillow's bytes: zlib's match search is serial.  The contract is that the file
decodes to exactly the image's pixels, that the same image gives the same bytes on every run, and
that the file is about as small as Pillow's (DESIGN 5h has the measured sizes).

``filter_device`` makes the filtered scanlines, ``deflate_device`` codes any device byte buffer
as a zlib stream, ``container`` wraps such a stream as an 8-bit RGB PNG, ``encode_device`` does
the three in a row, and ``write`` routes an image to the device or, when ``encodable`` says no
(other channel counts, other dtypes), to Pillow.
"""
import ctypes as C
import zlib

import numpy as np

from . import _lib

CHUNK = _lib.DEFLATE_CHUNK  # input bytes per deflate block
MAX_SIDE = (1 << 31) - 1    # what a PNG's IHDR holds
MAX_DEFLATE = _lib.DEFLATE_MAX_BYTES - 1    # pano_deflate's limit
MAX_IDAT = (1 << 31) - 1    # a chunk's length field
SIGNATURE = b"\x89PNG\r\n\x1a\n"
PNG_EXTENSIONS = (".png",)


def _on_device(x, dev):
    import torch
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x))
    return x if x.device == dev else x.to(dev)


def encodable(img):
    """Whether ``encode_device`` covers the image (else Pillow does): uint8, [h][w][3], sides
    1 .. 2^31 - 1, scanlines within ``pano_deflate``'s limit."""
    shape = tuple(img.shape)
    return (_lib.is_rgb_u8(img)
            and 1 <= shape[0] <= MAX_SIDE and 1 <= shape[1] <= MAX_SIDE
            and shape[0] * (1 + 3 * shape[1]) <= MAX_DEFLATE)


def filter_device(img, order="bgr", eng=None):
    """The filtered PNG scanlines of a uint8 [h][w][3] image (a device tensor, or a host array
    that is uploaded): a uint8 device tensor [h][1 + 3 w], per row the filter's number and the
    filtered bytes in RGB order.  ``order`` is the channel order of ``img``.  Any row pitch works
    as long as the pixels of a row are contiguous (a crop view of a mosaic needs no copy).
    Queued on the engine's stream.  Raises ValueError for what ``encodable`` rejects."""
    import torch
    if order not in ("bgr", "rgb"):
        raise ValueError(f"order {order!r}: 'bgr' or 'rgb'")
    if not encodable(img):
        raise ValueError(f"{tuple(img.shape)} {img.dtype}: not a case the device encodes")
    eng = _lib._engine(eng)
    img = _lib.rgb_on_device(img, eng)
    h, w = int(img.shape[0]), int(img.shape[1])
    out = torch.empty((h, 1 + 3 * w), dtype=torch.uint8, device=img.device)
    eng.call("pano_png_filter", img, h, w, img.stride(0), _lib.PNG_BGR if order == "bgr" else 0,
             out)
    return out


def deflate_device(data, eng=None):
    """The zlib stream (RFC 1950) of a byte buffer (a uint8 device tensor, or host bytes / a
    host array that are uploaded): the header ``78 01``, the raw deflate stream of
    ``pano_deflate`` (one dynamic-Huffman block per ``CHUNK`` bytes, matches at distance 1 only),
    the Adler-32 big-endian.  ``zlib.decompress`` returns the buffer.  The call waits on the
    stream twice and downloads the stream; not capturable."""
    import torch
    eng = _lib._engine(eng)
    dev = torch.device(eng.device)
    if isinstance(data, (bytes, bytearray, memoryview)):
        data = np.frombuffer(bytes(data), np.uint8).copy()
    data = _on_device(data, dev)
    if data.dtype != torch.uint8:
        raise ValueError(f"{data.dtype}: a byte buffer is uint8")
    data = data.contiguous().view(-1)
    n = int(data.numel())
    if n > MAX_DEFLATE:
        raise ValueError(f"{n} bytes: pano_deflate takes at most {MAX_DEFLATE}")
    work_bytes = int(eng.lib.pano_deflate_work_bytes(n))
    work = torch.empty(work_bytes, dtype=torch.uint8, device=dev)
    stream, nbytes, adler = C.c_void_p(), C.c_int64(), C.c_uint32()
    eng.call("pano_deflate", data if n else None, n, work, work_bytes, C.byref(stream),
             C.byref(nbytes), C.byref(adler))
    return b"\x78\x01" + C.string_at(stream.value, nbytes.value) + adler.value.to_bytes(4, "big")


def code_lengths_device(freq, max_bits, eng=None):
    """``pano_deflate_lengths``: the optimal code lengths of at most ``max_bits`` bits for the
    symbol frequencies ``freq`` (up to 288 of them, their sum below 2^32), as a uint8 array."""
    import torch
    eng = _lib._engine(eng)
    dev = torch.device(eng.device)
    f = np.ascontiguousarray(freq, dtype=np.int64)
    if f.ndim != 1 or f.min(initial=0) < 0 or int(f.sum()) >= 1 << 32:
        raise ValueError("frequencies: one row of non-negative counts, their sum below 2^32")
    fd = torch.from_numpy(f.astype(np.uint32).view(np.int32)).to(dev)
    out = torch.zeros(len(f), dtype=torch.uint8, device=dev)
    eng.call("pano_deflate_lengths", fd, len(f), int(max_bits), out)
    return out.cpu().numpy()


def _chunk(kind, body):
    return len(body).to_bytes(4, "big") + kind + body + zlib.crc32(kind + body).to_bytes(4, "big")


def container(zstream, width, height, idat_bytes=MAX_IDAT):
    """The PNG file around a zlib stream of filtered scanlines: the signature, ``IHDR`` (8-bit,
    colour type 2, no interlace), the stream cut into ``IDAT`` chunks of at most ``idat_bytes``
    bytes, ``IEND``."""
    if not 1 <= idat_bytes <= MAX_IDAT:
        raise ValueError(f"idat_bytes {idat_bytes}: 1 .. {MAX_IDAT}")
    if not (1 <= width <= MAX_SIDE and 1 <= height <= MAX_SIDE):
        raise ValueError(f"{width} x {height}: sides are 1 .. {MAX_SIDE}")
    view = memoryview(zstream)
    out = [SIGNATURE, _chunk(b"IHDR", width.to_bytes(4, "big") + height.to_bytes(4, "big")
                             + bytes([8, 2, 0, 0, 0]))]
    for at in range(0, max(len(view), 1), idat_bytes):
        out.append(_chunk(b"IDAT", bytes(view[at:at + idat_bytes])))
    out.append(_chunk(b"IEND", b""))
    return b"".join(out)


def encode_device(img, order="bgr", eng=None, idat_bytes=MAX_IDAT):
    """The PNG file of a uint8 [h][w][3] image (device tensor or host array, ``order`` "bgr" or
    "rgb"; a crop view needs no copy): ``Image.open`` returns exactly its pixels, the same image
    gives the same bytes on every run.  Raises ValueError for what ``encodable`` rejects."""
    eng = _lib._engine(eng)
    lines = filter_device(img, order, eng)
    h, w = int(img.shape[0]), int(img.shape[1])
    return container(deflate_device(lines, eng), w, h, idat_bytes)


def write(path, img, order="bgr", eng=None):
    """Save a uint8 [h][w][3] image as PNG: on the device when ``encodable``, else through
    Pillow as before.  Returns "device" or "pillow"."""
    if encodable(img):
        data = encode_device(img, order, eng)
        with open(path, "wb") as fid:
            fid.write(data)
        return "device"
    from PIL import Image as PilImage
    a = img.cpu().numpy() if hasattr(img, "cpu") else np.asarray(img)
    if order == "bgr" and a.ndim == 3 and a.shape[2] >= 3:
        a = np.concatenate([a[..., 2::-1], a[..., 3:]], axis=2)
    PilImage.fromarray(np.ascontiguousarray(a)).save(path, "PNG")
    return "pillow"
