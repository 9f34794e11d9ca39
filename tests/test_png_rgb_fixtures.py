"""The colour PNG fixtures (tests/golden/png_rgb_fixtures.npz, made by
tests/golden/make_png_rgb_fixtures.py) pinned on the CPU: every file reopens in PIL (the
libpng-equivalent decoder standing in for the reference's cv2.imread(color_path) +
cvtColor(BGR2RGB), capture_stream.py:402) to its stored RGB pixels, and the oracle's unfilter
(oracle/png.py) over the zlib-inflated IDAT stream gives the same samples, grey replicated and
alpha dropped."""
import io
import os
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

from oracle import png as P

FIX = os.path.join(os.path.dirname(__file__), "golden", "png_rgb_fixtures.npz")
BPP = {0: 1, 2: 3, 4: 2, 6: 4}      # IHDR colour type -> bytes per pixel at bit depth 8


def fixtures():
    z = np.load(FIX)
    n = sum(1 for k in z.files if k.startswith("png_"))
    return [(str(z[f"name_{i}"]), z[f"png_{i}"].tobytes(), z[f"img_{i}"]) for i in range(n)]


def test_fixture_set_covers_the_cases():
    fx = fixtures()
    names = {n for n, _, _ in fx}
    for mode in ("L", "RGB", "LA", "RGBA"):
        for ft in ("filter0", "filter1", "filter2", "filter3", "filter4", "filter_mix"):
            assert f"{mode}_{ft}" in names
    for n in ("stored", "fixed", "huffman_only", "rle", "idat1", "idat7_level9", "trns_text", "pil_level0",
              "pil_level1", "pil_level6", "pil_level9"):
        assert n in names
    shapes = {i.shape for _, _, i in fx}
    assert {(70, 37, 3), (48, 64, 3), (1, 1, 3), (1, 37, 3), (29, 3, 3), (130, 5, 3)} <= shapes
    assert os.path.getsize(FIX) < 512 * 1024
    assert all(i.dtype == np.uint8 for _, _, i in fx)


@pytest.mark.parametrize("name,png,img", fixtures(), ids=lambda v: v if isinstance(v, str) else "")
def test_fixture_reopens_in_pil_and_oracle_unfilter_agrees(name, png, img):
    np.testing.assert_array_equal(np.asarray(Image.open(io.BytesIO(png)).convert("RGB")), img, err_msg=name)
    ch = list(P.chunks(png))
    assert png[:8] == P.SIG and ch[0][0] == b"IHDR"
    W, H, depth, ctype, _, _, interlace = struct.unpack(">IIBBBBB", ch[0][1])
    assert depth == 8 and interlace == 0 and (H, W) == img.shape[:2]
    bpp = BPP[ctype]
    raw = zlib.decompress(b"".join(d for t, d in ch if t == b"IDAT"))
    assert len(raw) == H * (bpp * W + 1)
    px = P.unfilter(raw, H, W, bpp).reshape(H, W, bpp)
    want = px[..., :3] if bpp >= 3 else np.repeat(px[..., :1], 3, axis=2)
    np.testing.assert_array_equal(want, img, err_msg=name)
