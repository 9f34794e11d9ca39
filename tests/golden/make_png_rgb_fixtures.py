"""Generate tests/golden/png_rgb_fixtures.npz: small 8-bit PNG files (grey, RGB, grey + alpha,
RGBA) and the RGB pixels PIL (libpng-equivalent, the stand-in for the reference's
cv2.imread(color_path) + cvtColor(BGR2RGB), capture_stream.py:402) makes of them with
.convert("RGB"): grey replicated, alpha dropped.  Run: python tests/golden/make_png_rgb_fixtures.py

The files cover what a colour PNG writer can emit: PIL's own encoder (adaptive row filters) at
compress levels 0 / 1 / 6 / 9, and the encoder below with every row filter forced (None, Sub, Up,
Average, Paeth, a per-row mix) for each of the four colour types at 70 x 37 (two 64-row bands of
the unfilter, a width that is no multiple of its 8-step chunk), stored / fixed-Huffman /
Huffman-only / RLE deflate blocks, IDAT split into 1-byte and 7-byte chunks, tRNS + tEXt before
the data, and odd sizes (1 x 1, 1 x 37, 29 x 3, 130 x 5).  Data only: key png_<i> (u8 file bytes),
img_<i> (u8 [H, W, 3] expected), name_<i>.
"""
from __future__ import annotations

import io
import os
import struct
import zlib

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
SIG = b"\x89PNG\r\n\x1a\n"
COLOUR_TYPE = {1: 0, 3: 2, 2: 4, 4: 6}        # samples per pixel -> IHDR colour type
MODE = {1: "L", 3: "RGB", 2: "LA", 4: "RGBA"}


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def encode_u8(img, filters=None, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, idat_size=8192, extra_chunks=()):
    """an 8-bit PNG of img u8 [H, W, C] (C = 1 grey, 2 grey + alpha, 3 RGB, 4 RGBA) with the given
    row filter types (a list, one per row, or an int; None = 0) and zlib settings"""
    H, W, C = img.shape
    out = bytearray()
    prev = np.zeros(W * C, np.int64)
    for r in range(H):
        x = img[r].reshape(-1).astype(np.int64)
        ft = filters if isinstance(filters, int) else (int(filters[r]) if filters is not None else 0)
        a = np.concatenate([np.zeros(C, np.int64), x[:-C]])
        c = np.concatenate([np.zeros(C, np.int64), prev[:-C]])
        f = [x, x - a, x - prev, x - ((a + prev) >> 1), x - paeth(a, prev, c)][ft]
        out.append(ft)
        out += (f & 255).astype(np.uint8).tobytes()
        prev = x
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    z = co.compress(bytes(out)) + co.flush()

    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xffffffff)

    png = SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, COLOUR_TYPE[C], 0, 0, 0))
    for t, d in extra_chunks:
        png += chunk(t, d)
    step = max(1, idat_size)
    for i in range(0, len(z), step):
        png += chunk(b"IDAT", z[i:i + step])
    return png + chunk(b"IEND", b"")


def colour_like(H, W, C, seed):
    """a frame-like image: gradients, a flat box, sensor noise, saturated corners; the alpha
    channel (the last of C = 2 / 4) a ramp with holes"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    ch = []
    for k in range(C):
        v = 40.0 * k + 2.0 * x + (1.0 + k) * y + rng.normal(0, 3, (H, W))
        v[H // 4:H // 2, W // 3:2 * W // 3] = 200 - 30 * k
        ch.append(v)
    img = np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8)
    img[:max(1, H // 8), :max(1, W // 6)] = 255
    img[-max(1, H // 9):, -max(1, W // 5):] = 0
    if C in (2, 4):
        img[..., -1] = np.where(rng.random((H, W)) < 0.1, 0, (x * 255) // max(1, W - 1))
    return img


def pil_png(img, **kw):
    b = io.BytesIO()
    Image.fromarray(img).save(b, format="PNG", **kw)
    return b.getvalue()


def cases():
    out = []
    rng = np.random.default_rng(1)
    mix = list(rng.integers(0, 5, 70))
    for C in (1, 3, 2, 4):
        base = colour_like(70, 37, C, C)
        for ft in range(5):
            out.append((f"{MODE[C]}_filter{ft}", encode_u8(base, filters=ft)))
        out.append((f"{MODE[C]}_filter_mix", encode_u8(base, filters=mix)))
    rgb = colour_like(70, 37, 3, 7)
    out.append(("stored", encode_u8(rgb, filters=mix, level=0)))
    out.append(("fixed", encode_u8(rgb, filters=mix, strategy=zlib.Z_FIXED)))
    out.append(("huffman_only", encode_u8(rgb, filters=mix, strategy=zlib.Z_HUFFMAN_ONLY)))
    out.append(("rle", encode_u8(rgb, filters=mix, strategy=zlib.Z_RLE)))
    out.append(("idat1", encode_u8(rgb, filters=mix, idat_size=1)))
    out.append(("idat7_level9", encode_u8(colour_like(70, 37, 4, 8), filters=mix, level=9, idat_size=7)))
    out.append(("trns_text", encode_u8(rgb, filters=mix, extra_chunks=[(b"tEXt", b"Software\x00test"),
                                                                        (b"tRNS", bytes(6))])))
    pil = colour_like(48, 64, 3, 9)
    for lvl in (0, 1, 6, 9):
        out.append((f"pil_level{lvl}", pil_png(pil, compress_level=lvl)))
    out.append(("one_pixel", encode_u8(np.array([[[7, 130, 255]]], np.uint8), filters=4)))
    out.append(("row37", encode_u8(colour_like(1, 37, 4, 2), filters=1)))
    out.append(("col3", encode_u8(colour_like(29, 3, 3, 3), filters=list(rng.integers(0, 5, 29)))))
    out.append(("rows130", encode_u8(colour_like(130, 5, 2, 4), filters=list(rng.integers(0, 5, 130)))))
    return out


def main():
    arrs = {}
    for i, (name, png) in enumerate(cases()):
        im = Image.open(io.BytesIO(png))
        assert im.mode in MODE.values(), (name, im.mode)
        arrs[f"png_{i}"] = np.frombuffer(png, np.uint8)
        arrs[f"img_{i}"] = np.asarray(im.convert("RGB"))
        arrs[f"name_{i}"] = np.array(name)
    path = os.path.join(HERE, "png_rgb_fixtures.npz")
    np.savez_compressed(path, **arrs)
    print(path, len(arrs) // 3, "files", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
