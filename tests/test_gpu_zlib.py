"""GPU decode of bare zlib streams of u16 samples (bf_zlib_decode_u16 / _depth, the depth frames of
a ScanNet .sens container) bit-exact against np.frombuffer(zlib.decompress(s), '<u2'): every
encoder setting that changes the block kinds, four kinds of content, outputs whose per-stream base
is not 16-byte aligned (inside sentinels), ScanNet's 480 x 640, streams at odd byte offsets, the
fused depth scaling, bad streams flagged next to good ones, and the host-side offset checks."""
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BAD_CHUNK, BAD_ZLIB, BAD_ADLER, SIZE = 8, 16, 32, 128
H0, W0 = 48, 64


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from boxfusion_amd import _lib
    _lib.lib()
    return _lib


def ref(stream, H, W):
    return np.frombuffer(zlib.decompress(stream), "<u2").reshape(H, W)


def deflate(img, level=6, wbits=15, strategy=zlib.Z_DEFAULT_STRATEGY, full_flush=False):
    raw = np.ascontiguousarray(img, "<u2").tobytes()
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    if full_flush:          # an empty stored block in the middle, new tables after it
        h = len(raw) // 2 + 1
        return co.compress(raw[:h]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(raw[h:]) + co.flush()
    return co.compress(raw) + co.flush()


ENCODINGS = [dict(level=1), dict(level=6), dict(level=9), dict(level=0), dict(strategy=zlib.Z_FIXED),
             dict(strategy=zlib.Z_HUFFMAN_ONLY), dict(strategy=zlib.Z_RLE), dict(wbits=9), dict(wbits=9, level=9),
             dict(wbits=15, level=1, strategy=zlib.Z_FIXED), dict(full_flush=True), dict(full_flush=True, level=0)]


def depth_mm(f, H, W):
    from boxfusion_amd.synthetic import frame_rgbd
    return np.clip(frame_rgbd(f * 7, H, W)[1] * 1000.0, 0, 65535).astype(np.uint16)


def contents(H, W):
    return {"depth": depth_mm(1, H, W),
            "zeros": np.zeros((H, W), np.uint16),
            "noise": np.random.default_rng(5).integers(0, 65536, (H, W)).astype(np.uint16),
            "ramp": (np.arange(H * W) % 65536).astype(np.uint16).reshape(H, W)}


def u16_numpy(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def decode(L, blobs, H, W, check=True, **kw):
    from boxfusion_amd.capture_stream import upload_files
    streams, offs, offs_h = upload_files(blobs, "cuda")
    out, st = L.zlib_decode_u16(streams, offs, H, W, offsets_host=offs_h, check=check, **kw)
    torch.cuda.synchronize()
    got = out.cpu().numpy() if out.dtype == torch.float32 else u16_numpy(out)
    return got, st.cpu().numpy()


@pytest.mark.parametrize("kind", ["depth", "zeros", "noise", "ramp"])
def test_encodings_bit_exact(L, kind):
    """every encoding of one image in one launch (one wave per stream)"""
    img = contents(H0, W0)[kind]
    blobs = [deflate(img, **e) for e in ENCODINGS]
    got, st = decode(L, blobs, H0, W0)
    assert st.tolist() == [0] * len(blobs)
    for k, (e, b) in enumerate(zip(ENCODINGS, blobs)):
        np.testing.assert_array_equal(got[k], ref(b, H0, W0), err_msg=f"{kind} {e}")
        np.testing.assert_array_equal(got[k], img)


def _in_sentinels(F, H, W, dtype, lead):
    """out [F,H,W] `lead` elements into a sentinel-filled buffer -> (buffer, out view, sentinel)"""
    n, tail = F * H * W, 37
    if dtype == torch.float32:
        big = torch.full((lead + n + tail,), -7.5, dtype=torch.float32, device="cuda")
        sentinel = np.float32(-7.5)
    else:
        host = np.full(lead + n + tail, 0xABCD, np.uint16)
        big = torch.from_numpy(host.view(np.int16)).to("cuda").view(torch.uint16)
        sentinel = np.uint16(0xABCD)
    return big, big[lead:lead + n].view(F, H, W), sentinel


@pytest.mark.parametrize("H,W,F", [(5, 3, 3), (1, 1, 2), (3, 8, 3)])
@pytest.mark.parametrize("scale", [None, 1000.0])
def test_unaligned_outputs_stay_inside(L, H, W, F, scale):
    """2 H W % 16 != 0 (30, 2 and 48 + a 2- / 4-byte aligned base): each stream's samples land at
    their own unaligned base and nothing around `out` is written"""
    rng = np.random.default_rng(H * 100 + W)
    imgs = [rng.integers(0, 65536, (H, W)).astype(np.uint16) for _ in range(F)]
    blobs = [deflate(im, level=(0, 6, 9)[k % 3]) for k, im in enumerate(imgs)]
    dt = torch.uint16 if scale is None else torch.float32
    for lead in (3, 8, 9):
        big, out, sentinel = _in_sentinels(F, H, W, dt, lead)
        got, st = decode(L, blobs, H, W, out=out, depth_scale=scale)
        assert st.tolist() == [0] * F
        want = np.stack([ref(b, H, W) for b in blobs])
        if scale is not None:
            want = want.astype(np.float32) / np.float32(scale)
        np.testing.assert_array_equal(got, want)
        host = big.cpu().numpy() if scale is not None else u16_numpy(big)
        n = F * H * W
        np.testing.assert_array_equal(host[lead:lead + n].reshape(F, H, W), want)
        assert (host[:lead] == sentinel).all() and (host[lead + n:] == sentinel).all(), (lead, host[:lead], host[lead + n:])


def test_scannet_size_one_launch(L):
    """480 x 640 (614,400 bytes per stream: many flushes, the window wraps past 32 KiB)"""
    H, W = 480, 640
    imgs = [depth_mm(f, H, W) for f in range(3)]
    imgs.append((imgs[2] // 50) * 50)              # quantised: long repeat runs
    encs = [dict(level=6), dict(level=0), dict(level=9, strategy=zlib.Z_RLE), dict(level=1, wbits=15, full_flush=True)]
    blobs = [deflate(im, **e) for im, e in zip(imgs, encs)]
    got, st = decode(L, blobs, H, W)
    assert st.tolist() == [0, 0, 0, 0]
    for k, b in enumerate(blobs):
        np.testing.assert_array_equal(got[k], ref(b, H, W), err_msg=str(encs[k]))
        np.testing.assert_array_equal(got[k], imgs[k])


def test_streams_at_odd_offsets(L):
    c = contents(H0, W0)
    good = [deflate(c["depth"], level=6), deflate(c["noise"], level=0), deflate(c["ramp"], level=9),
            deflate(c["zeros"], level=1)]
    blobs = [good[0], b"\x78", good[1], b"\x78\x9c\x03", good[2], b"\x00", good[3]]
    starts = np.cumsum([0] + [len(b) for b in blobs])[:-1]
    assert any(int(starts[k]) % 2 for k in (2, 4, 6)) and any(int(starts[k]) % 4 for k in (2, 4, 6))
    got, st = decode(L, blobs, H0, W0, check=False)
    for k in (1, 3, 5):
        assert st[k] & BAD_CHUNK, (k, st[k])
    for k, g in zip((0, 2, 4, 6), good):
        assert st[k] == 0, (k, st[k])
        np.testing.assert_array_equal(got[k], ref(g, H0, W0), err_msg=f"stream {k} at byte {starts[k]}")


def test_depth_scale_and_out_in_place(L):
    from boxfusion_amd.capture_stream import upload_files
    imgs = [depth_mm(f, H0, W0) for f in range(3)]
    blobs = [deflate(im) for im in imgs]
    want16 = np.stack([ref(b, H0, W0) for b in blobs])
    for scale in (1000.0, 6553.5):
        got, st = decode(L, blobs, H0, W0, depth_scale=scale)
        assert got.dtype == np.float32 and not st.any()
        np.testing.assert_array_equal(got, want16.astype(np.float32) / np.float32(scale))
    streams, offs, offs_h = upload_files(blobs, "cuda")
    out = torch.zeros((3, H0, W0), dtype=torch.float32, device="cuda")
    ret, _ = L.zlib_decode_u16(streams, offs, H0, W0, out=out, offsets_host=offs_h, depth_scale=1000.0)
    assert ret.data_ptr() == out.data_ptr()
    np.testing.assert_array_equal(out.cpu().numpy(), want16.astype(np.float32) / np.float32(1000.0))
    out16 = torch.zeros((3, H0, W0), dtype=torch.int16, device="cuda").view(torch.uint16)
    ret, _ = L.zlib_decode_u16(streams, offs, H0, W0, out=out16)              # offsets read back from the device
    assert ret.data_ptr() == out16.data_ptr()
    np.testing.assert_array_equal(u16_numpy(out16), want16)


def _fix_check(z):
    """FCHECK so that CMF * 256 + FLG is a multiple of 31 again"""
    z[1] &= 0xe0
    z[1] += (31 - ((z[0] << 8) | z[1]) % 31) % 31
    return z


def test_bad_streams_flagged_good_streams_exact(L):
    img = depth_mm(2, H0, W0)
    raw = img.tobytes()
    good = zlib.compress(raw, 6)
    assert len(raw) == 2 * H0 * W0

    adler = bytearray(good)
    adler[-1] ^= 0x5a
    fdict = bytearray(good)
    fdict[1] |= 0x20
    fdict = _fix_check(fdict)
    assert fdict[1] & 0x20 and ((fdict[0] << 8) | fdict[1]) % 31 == 0
    cm = bytearray(good)
    cm[0] = (cm[0] & 0xf0) | 9
    cm = _fix_check(cm)
    assert cm[0] & 15 == 9 and ((cm[0] << 8) | cm[1]) % 31 == 0
    block = bytearray(zlib.compress(raw, 0))        # stored blocks: break LEN / NLEN
    block[5] ^= 0xff
    short = zlib.compress(raw[:-10], 6)
    extra = bytes(range(32))
    long_ = zlib.compress(raw + extra, 6)
    long_stored = zlib.compress(raw + extra, 0)
    other = deflate((img // 3).astype(np.uint16), level=9)
    cases = [("good", good, 0), ("adler", bytes(adler), BAD_ADLER), ("fdict", bytes(fdict), BAD_ZLIB),
             ("cm", bytes(cm), BAD_ZLIB), ("block", bytes(block), BAD_ZLIB), ("short", short, SIZE),
             ("long", long_, SIZE), ("after_long", other, 0), ("long_stored", long_stored, SIZE),
             ("after_long_stored", good, 0), ("three_bytes", good[:3], BAD_CHUNK),
             ("last", deflate(img, strategy=zlib.Z_FIXED), 0)]
    blobs = [c[1] for c in cases]
    big, out, sentinel = _in_sentinels(len(cases), H0, W0, torch.uint16, 8)
    got, st = decode(L, blobs, H0, W0, check=False, out=out)
    for k, (name, b, bit) in enumerate(cases):
        if bit == 0:
            assert st[k] == 0, (name, st[k])
            np.testing.assert_array_equal(got[k], ref(b, H0, W0), err_msg=name)
        else:
            assert st[k] & bit, (name, st[k])
    host = u16_numpy(big)
    assert (host[:8] == sentinel).all() and (host[8 + got.size:] == sentinel).all()
    with pytest.raises(L.HipError, match="did not decode"):
        decode(L, blobs, H0, W0, check=True)
    with pytest.raises(L.HipError, match="stream 1: Adler-32 mismatch"):
        decode(L, blobs[:2], H0, W0, check=True)


def test_host_offset_checks(L):
    blob = deflate(depth_mm(0, H0, W0))
    streams = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).to("cuda")
    n = len(blob)
    for offs, why in (([0, n + 1], "run past"), ([0, n, n - 4], "decrease"), ([4, 2, n], "decrease")):
        o = torch.tensor(offs, dtype=torch.int64)
        with pytest.raises(L.HipError, match=why):
            L.zlib_decode_u16(streams, o.to("cuda"), H0, W0, offsets_host=o)
    o = torch.tensor([0, n], dtype=torch.int64)
    with pytest.raises(L.HipError, match="out"):
        L.zlib_decode_u16(streams, o.to("cuda"), H0, W0, offsets_host=o,
                          out=torch.zeros((2, H0, W0), dtype=torch.int16, device="cuda").view(torch.uint16))


def test_no_streams(L):
    streams = torch.zeros(1, dtype=torch.uint8, device="cuda")
    offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    for scale, dt in ((None, torch.uint16), (1000.0, torch.float32)):
        out, st = L.zlib_decode_u16(streams, offs, H0, W0, depth_scale=scale)
        assert tuple(out.shape) == (0, H0, W0) and out.dtype == dt
        assert st.numel() == 0 and st.dtype == torch.int32
    from boxfusion_amd.capture_stream import decode_depth_zlib
    assert tuple(decode_depth_zlib([], H0, W0).shape) == (0, H0, W0)


def test_decode_depth_zlib_helper(L):
    from boxfusion_amd.capture_stream import decode_depth_zlib
    imgs = [depth_mm(f, H0, W0) for f in range(2)]
    out = decode_depth_zlib([memoryview(deflate(im)) for im in imgs], H0, W0)
    assert out.dtype == torch.uint16
    np.testing.assert_array_equal(u16_numpy(out), np.stack(imgs))
    with pytest.raises(L.HipError, match="did not decode"):
        decode_depth_zlib([deflate(imgs[0]), deflate(imgs[1][:-1])], H0, W0)
