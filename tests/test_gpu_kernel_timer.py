"""_lib.KernelTimer: what bench.py's roofline objects rest on.  Every timed wrapper, at the smallest
shape it accepts, appends exactly one record while a timer entered on this thread is active; the
record's tags, FLOPs and bytes equal the literals below (worked out from the formulas in
KernelTimer's docstring and the wrappers' own comments), and the timed call returns what the same
call returns outside the timer, bit for bit."""
import threading

import numpy as np
import pytest
import torch

from oracle import oracle as OR
from tests.test_gpu_fusion import CAP, HipBackend, _hexagon_views, _t, nms_cfg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from boxfusion_amd import _lib
    return _lib


def _randn(*shape, seed=0, dtype=torch.float32):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(*shape, device="cuda", generator=g).to(dtype)


def _one_record(L, call, tags, flops, nbytes):
    """call() outside the timer, then inside: one record with these tags / FLOPs / bytes; returns
    (untimed result, timed result)"""
    want = call()
    with L.KernelTimer() as t:
        got = call()
    assert len(t.records) == 1
    rt, rf, rb = t.records[0][:3]
    assert rt == tags
    assert (rf, rb) == (flops, nbytes)
    assert t.summary()["launches"] == 1 and t.summary(lambda tg: tg["kind"] != tags["kind"])["launches"] == 0
    return want, got


# 128 x 128 x 64: 2*M*N*K = 2097152 FLOPs; A + W = 2 * (128*64 + 128*64) = 32768 bytes
GEMM_CASES = {
    # + bf16 out 128*128*2
    "bf16": (dict(), dict(out_bf16=True, resid=False), 32768.0 + 32768.0),
    # + f32 out 128*128*4 + the f32 residual read 128*128*4
    "f32_resid": (dict(out_dtype=torch.float32, resid=(128, 128)), dict(out_bf16=False, resid=True),
                  32768.0 + 65536.0 + 65536.0),
    # + f32 out + a 16-row residual table 16*128*4
    "f32_resid_mod": (dict(out_dtype=torch.float32, resid=(16, 128), resid_mod=16), dict(out_bf16=False, resid=True),
                      32768.0 + 65536.0 + 8192.0),
}


@pytest.mark.parametrize("case", sorted(GEMM_CASES))
def test_gemm_record(L, case):
    kw, tg, nbytes = GEMM_CASES[case]
    kw = dict(kw)
    if "resid" in kw:
        kw["resid"] = _randn(*kw["resid"], seed=3)
    a, w, bias = _randn(128, 64, seed=1, dtype=torch.bfloat16), _randn(128, 64, seed=2, dtype=torch.bfloat16), _randn(128, seed=4)
    tags = dict(kind="gemm", act=1, M=128, N=128, K=64, large=False, **tg)     # N < 512: the 128x128 kernel
    want, got = _one_record(L, lambda: L.gemm(a, w, bias, "gelu", **kw), tags, 2097152.0, nbytes)
    assert got.dtype == kw.get("out_dtype", torch.bfloat16) and torch.equal(got, want)


def test_gemm_fp8_record(L):
    a, w = (_randn(128, 128, seed=5) * 3).to(L.FP8), (_randn(128, 128, seed=6) * 0.5).to(L.FP8)
    bias = _randn(128, seed=7)
    tags = dict(kind="gemm_fp8", act=0, out="torch.bfloat16", resid=False, M=128, N=128, K=128)
    # 2 * 128^3 FLOPs; bytes A + W at one byte (2 * 16384) + bf16 out 16384 * 2
    want, got = _one_record(L, lambda: L.gemm_fp8(a, w, 0.37, bias), tags, 4194304.0, 65536.0)
    assert got.dtype == torch.bfloat16 and torch.equal(got, want)


@pytest.mark.parametrize("fp8out", [False, True])
def test_attention_record(L, fp8out):
    B, H, S, D = 1, 1, 64, 64
    q, k, v = (_randn(B * S, H * D, seed=s, dtype=torch.bfloat16) for s in (8, 9, 10))
    tags = dict(kind="attn", D=64, sq=64, sk=64, batch=1, heads=1)
    if fp8out:
        def call():
            o = torch.zeros(B * S, H * D, device="cuda", dtype=torch.uint8).view(L.FP8)
            return L.attention_fp8out(q, k, v, o, B, H, S, S, D, D ** -0.5, 448.0 / 3.0)
        # bytes per (batch, head): D * (2 sq bf16 Q + 4 sk bf16 K, V + sq fp8 O) = 64 * 448
        want, got = _one_record(L, call, dict(tags, fp8out=True), 1048576.0, 28672.0)
    else:
        def call():
            o = torch.zeros(B * S, H * D, device="cuda", dtype=torch.bfloat16)
            return L.attention(q, k, v, o, B, H, S, S, D, D ** -0.5)
        # 4 * Sq * Sk * D FLOPs; bytes 2 * D * (2 sq + 2 sk) = 2 * 64 * 256
        want, got = _one_record(L, call, tags, 1048576.0, 32768.0)
    assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)) and got.view(torch.uint8).any()


def _boxes(n, seed):
    rng = np.random.default_rng(seed)
    b = np.concatenate([rng.normal(0, 0.05, (n, 3)), rng.uniform(0.4, 0.6, (n, 3))], 1).astype(np.float32)
    return _t(OR.box_corners(b, np.repeat(np.eye(3, dtype=np.float32)[None], n, 0)))


def test_obb_iou_record(L):
    corners = _boxes(4, 11)
    # work = the 4 * 3 / 2 box pairs; bytes 96 * n corners + 8 * n^2 f64 IoUs
    want, got = _one_record(L, lambda: L.obb_iou_matrix(corners), dict(kind="obb_iou", n=4), 6.0, 512.0)
    assert torch.equal(got, want) and float(got[0, 1]) > 0


def test_nms_scan_record(L):
    n = 3
    corners = _boxes(n, 12)
    iou = L.obb_iou_matrix(corners)
    scores = _t(np.array([0.9, 0.8, 0.7], np.float32))
    poses = _t(np.repeat(np.eye(4, dtype=np.float32)[None], n, 0))
    items, lens = OR.pack_lists([[i] for i in range(n)], CAP)

    def call():
        it, ln, vn = _t(items, torch.int32), _t(lens, torch.int32), _t(np.zeros(n, np.float32))     # updated in place
        keep, succ, ev, cnt = L.nms_scan(iou, corners, scores, torch.arange(n, dtype=torch.int32, device="cuda"),
                                         poses, it, ln, vn, nms_cfg(L))
        c = cnt.tolist()
        assert c[3] == 0
        return keep[:c[0]], succ[:c[1]], ev[:c[2]], cnt, it, ln, vn

    want, got = _one_record(L, call, dict(kind="nms_scan", n=3), 3.0, 72.0)      # n boxes; 8 n^2 bytes of IoUs
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert 0 < len(got[0]) < n          # overlapping boxes: something was suppressed


@pytest.mark.parametrize("packed_out", [False, True])
def test_fusion_fit_record(L, packed_out):
    vb, vr, vs, vp, vt = (_t(x) for x in _hexagon_views())
    be = HipBackend(L)
    off, cnt = _t(np.array([0], np.int32), torch.int32), _t(np.array([3], np.int32), torch.int32)

    def call():
        return L.fusion_fit(off, cnt, vb, vr, vs, vp, vt, be.pst, be.fcfg, max_views=3, packed_out=packed_out)

    want = call()
    with L.KernelTimer() as t:
        got = call()
    assert len(t.records) == 1
    tags, work, nbytes = t.records[0][:3]
    assert tags == dict(kind="fusion_fit", jobs=1) and nbytes == 0.0
    # work = views * particles * iterations of the job, read from the launch's own iteration count
    iters = int(got[1][1] if packed_out else got[2][0])
    assert iters > 0
    s = t.summary()
    assert s["launches"] == 1 and s["flops"] == float(iters * 3 * be.fcfg.pst_size) and s["bytes"] == 0.0
    assert callable(work) and work() == s["flops"]
    for a, b in zip(got, want):
        assert (a is None and b is None) or torch.equal(a, b)


@pytest.mark.parametrize("backproject", [False, True])
def test_depth_preprocess_record(L, backproject):
    depth = _randn(1, 32, 32, seed=13).abs() + 0.5
    args = ()
    if backproject:
        K = torch.tensor([[[30.0, 0, 16], [0, 30.0, 16], [0, 0, 1]]], device="cuda")
        args = (K, torch.eye(4, device="cuda")[None].contiguous())
    # no FLOPs; bytes 8 per pixel (depth read + standardised map written), + 13 per pixel (xyz, valid)
    want, got = _one_record(L, lambda: L.depth_preprocess(depth, *args),
                            dict(kind="depth", backproject=backproject, b=1, h=32, w=32), 0.0,
                            21504.0 if backproject else 8192.0)
    assert len(got) == (4 if backproject else 2)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    # depth_standardize is the same launch without K / RT
    w2, g2 = _one_record(L, lambda: L.depth_standardize(depth), dict(kind="depth", backproject=False, b=1, h=32, w=32),
                         0.0, 8192.0)
    assert torch.equal(g2[0], want[0]) and torch.equal(g2[1], want[1]) and torch.equal(w2[0], g2[0])


def test_only_the_entering_thread_while_active(L):
    corners = _boxes(4, 11)
    want = L.obb_iou_matrix(corners)
    got = []
    with L.KernelTimer() as t:
        th = threading.Thread(target=lambda: got.append(L.obb_iou_matrix(corners)))
        th.start()
        th.join()
        assert t.records == []                      # another thread's launch
        L.obb_iou_matrix(corners)
        assert len(t.records) == 1
    assert torch.equal(got[0], want)
    assert torch.equal(L.obb_iou_matrix(corners), want)
    assert len(t.records) == 1 and not t.active and L._TIMER is None       # after __exit__


def test_depth_preprocess_under_capture_needs_ws_with_timer(L):
    depth = _randn(1, 32, 32, seed=13).abs() + 0.5
    L.depth_preprocess(depth)
    torch.cuda.synchronize()
    with L.KernelTimer() as t:
        with pytest.raises(L.HipError, match="caller-owned ws"):
            with torch.cuda.graph(torch.cuda.CUDAGraph()):
                L.depth_preprocess(depth)
    assert t.records == []
    torch.cuda.synchronize()
    out, params = L.depth_preprocess(depth)         # and the eager path is as before
    assert torch.isfinite(out).all() and torch.isfinite(params).all()
