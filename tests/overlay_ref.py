"""The references of the overlay tests: visualize.py's blend as Pillow computes it, the same as the float32 formula the kernel
states, PNG decoding by Pillow and by libsamrs_io, and the PNG row filters restated in numpy."""
import ctypes
import io

import numpy as np
from PIL import Image


def overlay_ref(image: np.ndarray, seg: np.ndarray, lut: np.ndarray, alpha: float) -> np.ndarray:
    """visualize.py: Image.blend(image, seg_color, alpha) with seg_color = lut[seg]; uint8 [H, W, 3]."""
    image, colour = np.ascontiguousarray(image, dtype=np.uint8), np.ascontiguousarray(lut[seg], dtype=np.uint8)
    return np.asarray(Image.blend(Image.fromarray(image), Image.fromarray(colour), alpha))


def blend_f32(a: np.ndarray, b: np.ndarray, alpha: float) -> np.ndarray:
    """(uint8)(a + alpha * (b - a)) in float32: the product rounded, the sum rounded, the result truncated."""
    d = (b.astype(np.int32) - a.astype(np.int32)).astype(np.float32)
    prod = np.float32(alpha) * d
    assert prod.dtype == np.float32
    return (a.astype(np.float32) + prod).astype(np.uint8)


def decode_pillow(data: bytes) -> np.ndarray:
    """Pillow checks every chunk's CRC, the zlib stream and its Adler-32."""
    im = Image.open(io.BytesIO(data))
    assert im.format == "PNG" and im.mode == "RGB"
    return np.asarray(im)


def decode_native(data: bytes) -> np.ndarray:
    from samrs_amd import tile_io
    lib = tile_io.load_library()
    buf = np.frombuffer(data, dtype=np.uint8)
    h, w = int.from_bytes(data[20:24], "big"), int.from_bytes(data[16:20], "big")
    dst = np.empty((h, w, 3), np.uint8)
    hh, ww = ctypes.c_int(0), ctypes.c_int(0)
    rc = lib.samrs_io_png_decode_rgb(buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), buf.size,
                                     dst.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), dst.size, ctypes.byref(hh), ctypes.byref(ww))
    assert rc == 0 and (hh.value, ww.value) == (h, w), (rc, hh.value, ww.value)
    return dst


def filter_rows(img: np.ndarray) -> np.ndarray:
    """The five PNG filters of every row of uint8 [H, W, 3]: uint8 [5, H, 3 W] (bytes per pixel 3; outside the image = 0)."""
    h, w, _ = img.shape
    x = img.reshape(h, 3 * w).astype(np.int32)
    a = np.zeros_like(x); a[:, 3:] = x[:, :-3]
    b = np.zeros_like(x); b[1:] = x[:-1]
    c = np.zeros_like(x); c[1:, 3:] = x[:-1, :-3]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]).astype(np.uint8)


def adaptive_filters(img: np.ndarray) -> np.ndarray:
    """Per row the filter with the least sum of |filtered byte as int8|, the lowest number on a tie: int [H]."""
    f = filter_rows(img).astype(np.int64)
    cost = np.where(f < 128, f, 256 - f).sum(axis=2)          # [5, H]
    return np.argmin(cost, axis=0)                            # argmin returns the first minimum


def filter_bytes_of(data: bytes) -> np.ndarray:
    """The filter byte of every row of a one-IDAT truecolour 8-bit PNG."""
    import zlib
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[12:16] == b"IHDR" and data[37:41] == b"IDAT"
    w, h = int.from_bytes(data[16:20], "big"), int.from_bytes(data[20:24], "big")
    n = int.from_bytes(data[33:37], "big")
    raw = zlib.decompress(data[41:41 + n])
    assert len(raw) == h * (3 * w + 1)
    return np.frombuffer(raw, np.uint8).reshape(h, 3 * w + 1)[:, 0].astype(np.int64)
