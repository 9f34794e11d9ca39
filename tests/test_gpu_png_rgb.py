"""GPU colour-PNG decode (bf_png_decode_rgb, bf_png.hip) bit-exact against PIL (the
libpng-equivalent decoder standing in for the reference's cv2.imread(color_path) +
cvtColor(BGR2RGB), capture_stream.py:402 CA-1M): the committed fixtures (the four 8-bit colour
types with every row filter, stored / fixed / dynamic blocks, split IDATs, tRNS, 1-pixel, 1-row
and 3-band images), a mixed-type batch, CA-1M-sized 768 x 1024 frames, a batch with refused and
corrupt files (each flagged with its own status bit, the good files still exact), the 16-bit
entry point's refusal of 8-bit files, and DecodedFrameStream reading rgb/*.png (and a directory
that mixes JPEG and PNG colour files) with color_decode="gpu"."""
import importlib.util
import io
import os
import struct
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import png as P

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FIX = os.path.join(GOLDEN, "png_rgb_fixtures.npz")


def _generator():
    """the fixture generator's 8-bit encoder (forced row filters, zlib strategy, IDAT split)"""
    spec = importlib.util.spec_from_file_location("make_png_rgb_fixtures",
                                                  os.path.join(GOLDEN, "make_png_rgb_fixtures.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from boxfusion_amd import _lib
    _lib.lib()
    return _lib


def fixtures():
    z = np.load(FIX)
    n = sum(1 for k in z.files if k.startswith("png_"))
    return [(str(z[f"name_{i}"]), z[f"png_{i}"].tobytes(), z[f"img_{i}"]) for i in range(n)]


def decode(L, blobs, H, W, check=True):
    from boxfusion_amd.capture_stream import upload_files
    files, offs, offs_h = upload_files(blobs, "cuda")
    out, st = L.png_decode_rgb(files, offs, H, W, offsets_host=offs_h, check=check)
    torch.cuda.synchronize()
    return out.cpu().numpy(), st.cpu().numpy()


def pil_rgb(png):
    return np.asarray(Image.open(io.BytesIO(png)).convert("RGB"))


@pytest.mark.parametrize("name,png,img", fixtures(), ids=lambda v: v if isinstance(v, str) else "")
def test_fixture_bit_exact(L, name, png, img):
    H, W = img.shape[:2]
    got, st = decode(L, [png], H, W)
    assert st.tolist() == [0]
    assert got.shape == (1, H, W, 3) and got.dtype == np.uint8
    np.testing.assert_array_equal(got[0], img, err_msg=name)


def test_mixed_colour_types_one_launch(L):
    """every 70 x 37 fixture in one launch: grey, RGB, grey + alpha and RGBA files side by side"""
    fx = [(n, p, i) for n, p, i in fixtures() if i.shape == (70, 37, 3)]
    assert len(fx) >= 31
    kinds = {struct.unpack(">IIBBBBB", next(P.chunks(p))[1])[3] for _, p, _ in fx}
    assert kinds == {0, 2, 4, 6}
    got, st = decode(L, [p for _, p, _ in fx], 70, 37)
    assert not st.any()
    for k, (n, _, img) in enumerate(fx):
        np.testing.assert_array_equal(got[k], img, err_msg=n)


def test_full_size_ca1m_frames(L):
    """four 768 x 1024 RGB frames in one launch: PIL's encoder (adaptive filters) at compress levels
    1 / 6 / 9 and one file with Paeth forced on every row"""
    from boxfusion_amd.synthetic import frame_rgbd
    imgs = [frame_rgbd(f * 7, 768, 1024)[0] for f in range(4)]
    blobs = [G.pil_png(imgs[k], compress_level=lvl) for k, lvl in enumerate((1, 6, 9))]
    blobs.append(G.encode_u8(imgs[3], filters=4))
    got, st = decode(L, blobs, 768, 1024)
    assert not st.any()
    for k, (png, img) in enumerate(zip(blobs, imgs)):
        np.testing.assert_array_equal(got[k], img, err_msg=f"file {k}")
        np.testing.assert_array_equal(got[k], pil_rgb(png))


def _chunk(t, d):
    return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xffffffff)


def _with_payload(png, mutate):
    """rebuild a PNG with its concatenated IDAT payload mutated (one IDAT chunk)"""
    ch = list(P.chunks(png))
    z = mutate(bytearray(b"".join(d for t, d in ch if t == b"IDAT")))
    out, done = P.SIG, False
    for t, d in ch:
        if t == b"IDAT":
            if not done:
                out += _chunk(t, bytes(z))
                done = True
        else:
            out += _chunk(t, d)
    return out


def _with_ihdr(png, **kw):
    """the same file with IHDR fields replaced (depth / ctype / interlace)"""
    ch = list(P.chunks(png))
    f = dict(zip(("W", "H", "depth", "ctype", "comp", "filt", "interlace"), struct.unpack(">IIBBBBB", ch[0][1])))
    f.update(kw)
    out = P.SIG + _chunk(b"IHDR", struct.pack(">IIBBBBB", *f.values()))
    for t, d in ch[1:]:
        out += _chunk(t, d)
    return out


def _refusal_cases():
    H, W = 48, 64
    img = G.colour_like(H, W, 3, 11)
    good = G.encode_u8(img, filters=4)

    def bad_filter(z):
        raw = bytearray(zlib.decompress(bytes(z)))
        raw[5 * (3 * W + 1)] = 7
        return bytearray(zlib.compress(bytes(raw)))

    def bad_adler(z):
        z[-1] ^= 0x5a
        return z

    rng = np.random.default_rng(3)
    g16 = io.BytesIO()
    Image.fromarray(rng.integers(0, 65536, (H, W)).astype(np.uint16)).save(g16, format="PNG")
    pal = io.BytesIO()
    Image.fromarray(img).convert("P").save(pal, format="PNG")
    # 16 bits per sample RGB: 6 bytes per pixel, filter None on every row
    raw16 = b"".join(b"\x00" + rng.integers(0, 256, 6 * W, dtype=np.uint8).tobytes() for _ in range(H))
    rgb16 = (P.SIG + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 16, 2, 0, 0, 0)) +
             _chunk(b"IDAT", zlib.compress(raw16)) + _chunk(b"IEND", b""))
    assert Image.open(g16).mode in ("I;16", "I;16B", "I") and Image.open(pal).mode == "P"
    assert Image.open(io.BytesIO(rgb16)).size == (W, H)
    return img, [("good", good, 0),
                 ("grey16", g16.getvalue(), 4),
                 ("palette", pal.getvalue(), 4),
                 ("rgb16", rgb16, 4),
                 ("interlaced", _with_ihdr(good, interlace=1), 4),      # refused at IHDR, before the Adam7 data
                 ("size", G.encode_u8(img[:40], filters=1), 128),
                 ("filter", _with_payload(good, bad_filter), 64),
                 ("adler", _with_payload(good, bad_adler), 32),
                 ("truncated", good[:len(good) // 2], 8),
                 ("good2", G.encode_u8(np.concatenate([img, img[..., :1]], -1), filters=3, strategy=zlib.Z_FIXED), 0)]


def test_refused_and_corrupt_files_flagged_good_files_exact(L):
    img, cases = _refusal_cases()
    got, st = decode(L, [c[1] for c in cases], 48, 64, check=False)
    for k, (name, _, bit) in enumerate(cases):
        if bit == 0:
            assert st[k] == 0, name
            np.testing.assert_array_equal(got[k], img, err_msg=name)
        else:
            assert st[k] & bit, (name, st[k])
    with pytest.raises(L.HipError, match="did not decode"):
        decode(L, [cases[0][1], cases[1][1]], 48, 64, check=True)


def test_u16_entry_still_refuses_eight_bit_rgb(L):
    from boxfusion_amd.capture_stream import upload_files
    png = G.encode_u8(G.colour_like(48, 64, 3, 11), filters=4)
    files, offs, offs_h = upload_files([png], "cuda")
    _, st = L.png_decode_u16(files, offs, 48, 64, offsets_host=offs_h, check=False)
    assert int(st.cpu()[0]) & 4


def test_argument_checks(L):
    from boxfusion_amd.capture_stream import upload_files
    png = G.encode_u8(G.colour_like(48, 64, 3, 11), filters=4)
    files, offs, offs_h = upload_files([png], "cuda")
    with pytest.raises(L.HipError, match="offsets run past"):
        L.png_decode_rgb(files[:100], offs, 48, 64, offsets_host=offs_h)
    with pytest.raises(L.HipError, match=r"offsets \[F\+1\]"):
        L.png_decode_rgb(files, offs, 48, 64, offsets_host=offs_h[:1])
    with pytest.raises(L.HipError):                    # W > 4096
        L.png_decode_rgb(files, offs, 1, 4097, offsets_host=offs_h)
    assert L.png_rgb_workspace_bytes(1, 48, 64, len(png)) > L.png_workspace_bytes(1, 48, 64, len(png))
    # the C entry point: an empty batch is OK, a short workspace is BF_ERR_CAPACITY (and launches nothing)
    import ctypes
    wb = L.png_rgb_workspace_bytes(1, 48, 64, len(png))
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    out = torch.zeros((1, 48, 64, 3), dtype=torch.uint8, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")

    def call(F, work_bytes):
        return L.lib().bf_png_decode_rgb(
            ctypes.c_void_p(files.data_ptr()), ctypes.c_void_p(offs.data_ptr()), ctypes.c_int(F), ctypes.c_int(48),
            ctypes.c_int(64), ctypes.c_longlong(len(png) if F else 0), ctypes.c_longlong(len(png) if F else 0),
            ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(work.data_ptr()), ctypes.c_size_t(work_bytes),
            ctypes.c_void_p(st.data_ptr()), None)
    assert call(0, wb) == 0
    assert call(1, wb - 1) == -3
    torch.cuda.synchronize()
    assert not out.any()


UP = np.eye(4, dtype=np.float32)
UP[1:3, :3] = [[0, 0, 1], [0, -1, 0]]           # camera y down the world z: the upright roll


def _write_frames(tmp_path, kinds):
    from boxfusion_amd.synthetic import frame_rgbd
    (tmp_path / "rgb").mkdir()
    (tmp_path / "depth").mkdir()
    cps, dps = [], []
    for f, kind in enumerate(kinds):
        rgb, d = frame_rgbd(f, 480, 640)
        cp, dp = tmp_path / "rgb" / f"{f}.{kind}", tmp_path / "depth" / f"{f}.png"
        if kind == "png":
            Image.fromarray(rgb).save(cp)
        else:
            Image.fromarray(rgb).save(cp, quality=90)
        Image.fromarray(np.clip(d * 1000.0, 0, 65535).astype(np.uint16)).save(dp)
        cps.append(str(cp))
        dps.append(str(dp))
    return cps, dps


def test_decoded_frame_stream_png_colour_gpu_equals_host(L, tmp_path):
    """a CA-1M style directory (rgb/*.png + depth/*.png): color_decode="gpu" (bf_png_decode_rgb)
    gives the same samples as the host PIL decode, bit for bit"""
    from boxfusion_amd.capture_stream import DecodedFrameStream
    from boxfusion_amd.synthetic import SCANNET_K
    cps, dps = _write_frames(tmp_path, ["png"] * 5)
    poses = [UP] * 5
    host = list(DecodedFrameStream(cps, dps, poses, SCANNET_K, 1000.0, device="cuda", batch=3, color_decode="host"))
    gpu = list(DecodedFrameStream(cps, dps, poses, SCANNET_K, 1000.0, device="cuda", batch=3, color_decode="gpu"))
    assert len(host) == len(gpu) == 5
    for a, b in zip(host, gpu):
        torch.testing.assert_close(a["wide"]["image"].cpu(), b["wide"]["image"].cpu(), rtol=0, atol=0)
        torch.testing.assert_close(a["wide"]["depth"].cpu(), b["wide"]["depth"].cpu(), rtol=0, atol=0)


def test_decoded_frame_stream_mixed_jpeg_and_png(L, tmp_path):
    """one directory with .jpg and .png colour files, three per batch: each file goes to its own
    decoder and the frames come back in order -- the PNG frames equal the host decode, the JPEG
    frames equal decode_color_jpegs on the same bytes; a file that is neither raises"""
    from boxfusion_amd.capture_stream import (ROT_K, DecodedFrameStream, decode_color_jpegs, decode_depth_pngs)
    from boxfusion_amd.sensor import get_orientation
    from boxfusion_amd.synthetic import SCANNET_K
    kinds = ["jpg", "png", "png", "jpg", "png"]
    cps, dps = _write_frames(tmp_path, kinds)
    poses = [UP] * 5
    host = list(DecodedFrameStream(cps, dps, poses, SCANNET_K, 1000.0, device="cuda", batch=3, color_decode="host"))
    gpu = list(DecodedFrameStream(cps, dps, poses, SCANNET_K, 1000.0, device="cuda", batch=3, color_decode="gpu"))
    assert len(gpu) == 5
    for i, (a, b) in enumerate(zip(host, gpu)):
        assert b["meta"]["timestamp"] == i
        torch.testing.assert_close(a["wide"]["depth"].cpu(), b["wide"]["depth"].cpu(), rtol=0, atol=0)
        if kinds[i] == "png":
            want = a["wide"]["image"]
        else:
            with open(cps[i], "rb") as fh, open(dps[i], "rb") as dh:
                col = decode_color_jpegs([fh.read()], 480, 640, "cuda")
                dep = decode_depth_pngs([dh.read()], 480, 640, "cuda")
            want, _ = L.ingest_rgbd(col[0], dep[0].view(torch.int16), 1000.0, ROT_K[get_orientation(UP)], src_bgr=False)
        torch.testing.assert_close(want.cpu(), b["wide"]["image"].cpu(), rtol=0, atol=0)
    other = tmp_path / "rgb" / "5.bmp"
    other.write_bytes(b"BM" + bytes(64))
    with pytest.raises(ValueError, match="5.bmp"):
        list(DecodedFrameStream([str(other)], dps[:1], poses[:1], SCANNET_K, 1000.0, device="cuda",
                                color_decode="gpu"))
