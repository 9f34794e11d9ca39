"""The persistent GEMMs' tile walk at the smallest shapes that reach each of its K-tile bodies.

k_gemm256q walks tile by tile with the first K-tile, the K-tiles inside the tile (a straight-line
loop), the one that starts staging the next tile and the last K-tile as separate bodies; with
3 K-tiles the inner loop never runs, with 5 it runs twice.  1 and 2 K-tiles fall to k_gemm256p,
whose lookahead then crosses one or two tile boundaries.  Every case is compared with the fp32
torch definition at the tolerance tests/test_gpu_gemm_sweep.py uses for that output type; the
reference of a shape is computed once and shared by its cases.

Which kernel a call reaches.  The persistent kernels store 16-byte row chunks, so they take a bf16
output only where N is a multiple of 8 and an f32 output where it is a multiple of 4; `kernel=-1`
does not override that.  N = 4, 252 and 516 therefore reach them with the f32 outputs only (their
bf16 outputs run the 128 x 128 k_gemm), and N = 8, 248 and 520 with every output type.
`expect_bf16` / `expect_fp8` state the kernel and tile height each call of this file is meant to
reach; the tests that speak of a kernel assert it through them, and test_kernel_choice runs every
case of the file once more in a child process under BF_GEMM_LOG=1 and holds the library's own
record of its choices against them, so no case can fall to another kernel unnoticed.

A workgroup without a tile cannot be built through the ABI (the persistent grid never exceeds the
tile count), so the uneven walks here are the ones it can produce: one workgroup walking 6 tiles,
a grid where half the workgroups walk 2 tiles and half 1, and one tile per workgroup.
"""
import functools
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MS = (1, 255, 257, 513)
NS = (4, 252, 516, 8, 248, 520)     # % 8 == 4: f32 outputs only on the persistent kernels; % 8 == 0: all
NS_FP8 = (8, 248, 520)              # the fp8 entry point takes N % 8 == 0 only
KS, KS_FP8 = (64, 128, 192, 320), (128, 256, 384, 640)      # 1, 2, 3, 5 K-tiles
HEIGHTS = (160, 192, 224, 256)
ACTS = {None: 0, "gelu": 1, "relu": 2}
Q, P, G = "k_gemm256q", "k_gemm256p", "k_gemm"

EXPECTED = None      # the child process of test_kernel_choice collects the expected log lines here


def rel_err(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def tol_bf16(K, out_bf16):
    return 8e-3 if out_bf16 else 2e-5 * math.sqrt(K / 64) + 1e-5


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from boxfusion_amd import _lib
    yield _lib


def expect_bf16(L, M, N, K, act, dt, resid, row_map, plan):
    """(kernel, tile rows) bf_gemm_bf16 is to run for a contiguous problem under a `kernel=-1` plan"""
    bf16 = dt == torch.bfloat16
    if N % (8 if bf16 else 4):
        return G, 128
    rows = plan.get("tile_rows") or L.gemm_tile_rows(M, N, K, dict(plan))
    variant = plan.get("variant", 5)
    # k_gemm256q: >= 3 K-tiles, no row map, plain / GELU bf16 outputs and plain / residual f32 ones
    fit = K // 64 >= 3 and not row_map and (act is None or (act == "gelu" and bf16 and not resid))
    if fit and (variant == 6 or (variant == 5 and (bf16 or resid or rows < 256))):
        return Q, rows
    return P, 256


def expect_fp8(L, M, N, K, dt, resid, plan):
    """(kernel, tile rows) of bf_gemm_fp8: k_gemm256q from 3 K-tiles on for the bf16 outputs, and
    for the fp8 outputs under variant 6; the heights are the latency model's"""
    variant = plan.get("variant", 5)
    if K // 128 >= 3 and not resid and (dt == torch.bfloat16 or (dt == L.FP8 and variant == 6)):
        return Q, plan.get("tile_rows") or L.gemm_tile_rows(M, N, K, dict(objective=1))
    return P, 256


def _gemm(L, a, w, b, act, out, plan, resid=None, row_map=None):
    M, (N, K) = a.shape[0], w.shape
    kern, rows = expect_bf16(L, M, N, K, act, out.dtype, resid is not None, row_map is not None, plan)
    if EXPECTED is not None:
        EXPECTED.add(f"bf_gemm M={M} N={N} K={K} act={ACTS[act]} resid={int(resid is not None)} resid_mod=0 "
                     f"row_map={int(row_map is not None)} out={'bf16' if out.dtype == torch.bfloat16 else 'f32'}"
                     f" -> {kern} rows={rows}")
    L.gemm(a, w, b, act=act, resid=resid, out=out, row_map=row_map, plan=dict(plan))
    return kern


def _gemm_fp8(L, a8, w8, sc, b, act, out, plan, resid=None, out_qscale=1.0):
    (M, K), N = a8.shape, w8.shape[0]
    kern, rows = expect_fp8(L, M, N, K, out.dtype, resid is not None, plan)
    if EXPECTED is not None:
        kind = {torch.float32: "f32", torch.bfloat16: "bf16", L.FP8: "fp8"}[out.dtype]
        EXPECTED.add(f"bf_gemm_fp8 M={M} N={N} K={K} act={ACTS[act]} resid={int(resid is not None)} out={kind}"
                     f" -> {kern} rows={rows}")
    L.gemm_fp8(a8, w8, sc, bias=b, act=act, resid=resid, out=out, out_qscale=out_qscale, plan=dict(plan))
    return kern


@functools.lru_cache(maxsize=None)
def _problem(M, N, K):
    """operands, residual, row map and the fp32 pre-activation product of one shape (read-only)"""
    g = torch.Generator(device="cuda").manual_seed(M * 31 + N * 7 + K)
    a = torch.randn(M, K, device="cuda", generator=g).bfloat16()
    w = (torch.randn(N, K, device="cuda", generator=g) / math.sqrt(K)).bfloat16()
    b = torch.randn(N, device="cuda", generator=g)
    r = torch.randn(M + 5, N, device="cuda", generator=g)
    rm = torch.randperm(M + 5, device="cuda", generator=g)[:M].int()
    y = a.float() @ w.float().T + b
    return a, w, b, r, rm, y


def _check_all_epilogues(L, M, N, K, plan):
    """every output type and epilogue of bf_gemm_bf16 on one shape under `plan`; returns the outputs
    and the kernel each was meant to run on"""
    a, w, b, r, rm, y = _problem(M, N, K)
    outs, kern = {}, {}
    for act, ref in ((None, y), ("gelu", F.gelu(y)), ("relu", F.relu(y))):
        for dt in (torch.bfloat16, torch.float32):
            out = torch.full((M, N), float("nan"), device="cuda", dtype=dt)
            kern[(act, dt)] = _gemm(L, a, w, b, act, out, plan)
            assert torch.isfinite(out).all(), ("unwritten outputs", M, N, K, act, dt, plan)
            assert rel_err(out, ref) < tol_bf16(K, dt == torch.bfloat16), (M, N, K, act, dt, plan)
            outs[(act, dt)] = out
    # f32 with a separate residual, and in place
    out = torch.full((M, N), float("nan"), device="cuda")
    kern["resid"] = _gemm(L, a, w, b, None, out, plan, resid=r[:M])
    assert rel_err(out, y + r[:M]) < tol_bf16(K, False), (M, N, K, "resid", plan)
    outs["resid"] = out
    out = r[:M].clone()
    kern["inplace"] = _gemm(L, a, w, b, None, out, plan, resid=out)
    assert rel_err(out, y + r[:M]) < tol_bf16(K, False), (M, N, K, "inplace", plan)
    outs["inplace"] = out
    # row map (scattered output rows, residual read at the mapped row); the rows outside stay
    out = torch.zeros(M + 5, N, device="cuda")
    kern["row_map"] = _gemm(L, a, w, b, None, out, plan, resid=r, row_map=rm)
    assert rel_err(out[rm.long()], y + r[rm.long()]) < tol_bf16(K, False), (M, N, K, "row_map", plan)
    mask = torch.ones(M + 5, dtype=torch.bool, device="cuda")
    mask[rm.long()] = False
    assert not out[mask].any(), "rows outside the map were written"
    return outs, kern


# the forms k_gemm256q serves (the bench's: qkv, fc1 + GELU, proj / fc2 + residual), and all of them
Q_FORMS_F32 = ((None, torch.float32), "resid", "inplace")
Q_FORMS = ((None, torch.bfloat16), ("gelu", torch.bfloat16)) + Q_FORMS_F32


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M", MS)
def test_kstep_paths_bf16(L, M, K):
    """1, 2, 3 and 5 K-tiles x ragged M x ragged N, every epilogue, under `kernel=-1` (these shapes
    are far below the size the shape rule sends to the persistent kernels).  Where N is a multiple
    of 8 every output runs on them, and from 3 K-tiles on the bf16 and the residual forms run
    k_gemm256q; at the other N only the f32 outputs do."""
    for N in NS:
        _, kern = _check_all_epilogues(L, M, N, K, dict(kernel=-1))
        on_persistent = [k for k, v in kern.items() if v != G]
        if N % 8 == 0:
            assert len(on_persistent) == len(kern), kern
        else:
            assert all(isinstance(k, str) or k[1] == torch.float32 for k in on_persistent), kern
            assert len(on_persistent) == 6, kern
        if K >= 192:
            forms = ("resid", "inplace") + (((None, torch.bfloat16), ("gelu", torch.bfloat16)) if N % 8 == 0 else ())
            assert all(kern[k] == Q for k in forms), kern


@pytest.mark.parametrize("K", [192, 320])
@pytest.mark.parametrize("N", [516, 520])
def test_kstep_tile_heights(L, N, K):
    """tile heights 160 / 192 / 224 / 256 on k_gemm256q (variant 6; at N = 516 the f32 forms only):
    each against torch, and (as the kernel tests hold it for k_gemm256q) bit-equal to one another,
    since the K-order MFMA chain of an output does not depend on the height"""
    M = 513
    base = None
    for bm in HEIGHTS:
        outs, kern = _check_all_epilogues(L, M, N, K, dict(kernel=-1, tile_rows=bm, variant=6))
        assert all(kern[k] == Q for k in (Q_FORMS if N % 8 == 0 else Q_FORMS_F32)), kern
        if base is None:
            base = outs
        else:
            for k in outs:
                assert torch.equal(outs[k], base[k]), ("tile height changed a value", bm, k)


@pytest.mark.parametrize("cu_budget", [2, 8, 16])
@pytest.mark.parametrize("K", [192, 320])
def test_kstep_uneven_walks(L, K, cu_budget):
    """513 x 520 at 160-row tiles is 4 x 3 = 12 tiles: 6 per workgroup on a budget of 2 CUs (the
    walk crosses 5 tile boundaries), 2 or 1 on 8, exactly 1 on 16; every form k_gemm256q serves
    runs on it.  The budget sizes the grid only, so the values equal those of the full chip bit
    for bit."""
    M, N = 513, 520
    pl = dict(kernel=-1, tile_rows=160, variant=6)
    assert L.gemm_grid(M, N, K, dict(pl, cu_budget=cu_budget)) == {2: 2, 8: 8, 16: 12}[cu_budget]
    full, _ = _check_all_epilogues(L, M, N, K, pl)
    outs, kern = _check_all_epilogues(L, M, N, K, dict(pl, cu_budget=cu_budget))
    assert all(kern[k] == Q for k in Q_FORMS), kern
    for k in outs:
        assert torch.equal(outs[k], full[k]), ("the CU budget changed a value", cu_budget, k)


@pytest.mark.parametrize("K", [192, 320])
def test_kstep_kernels_agree(L, K):
    """k_gemm256q (variant 6) against k_gemm256p (variant 1) on the no-activation f32 forms, at
    the bound the kernel tests hold between the two (their accumulators are laid out differently:
    close, not bit-equal)"""
    M, N = 513, 516
    q, kq = _check_all_epilogues(L, M, N, K, dict(kernel=-1, variant=6))
    p, kp = _check_all_epilogues(L, M, N, K, dict(kernel=-1, variant=1))
    for k in Q_FORMS_F32:
        assert (kq[k], kp[k]) == (Q, P), (k, kq[k], kp[k])
        assert rel_err(q[k], p[k]) < 1e-6, k


@functools.lru_cache(maxsize=None)
def _problem_fp8(M, N, K):
    from boxfusion_amd import _lib as L
    g = torch.Generator(device="cuda").manual_seed(M * 13 + N + K)
    a8 = (torch.randn(M, K, device="cuda", generator=g) * 0.5).to(L.FP8)
    w8 = (torch.randn(N, K, device="cuda", generator=g) * 0.5).to(L.FP8)
    b = torch.randn(N, device="cuda", generator=g)
    r = torch.randn(M, N, device="cuda", generator=g)
    sc = 1.0 / math.sqrt(K)
    y = (a8.float() @ w8.float().T) * sc + b
    return a8, w8, b, r, sc, y


@pytest.mark.parametrize("K", KS_FP8)
@pytest.mark.parametrize("M", MS)
def test_kstep_paths_fp8(L, M, K):
    """fp8 operands (128-element K-tiles), ragged M x ragged N at the model's height and at each
    forced one: 1 and 2 K-tiles (k_gemm256p) and 3 and 5 (k_gemm256q for the bf16 outputs, and for
    the fp8 outputs under variant 6), f32 / f32 + residual / bf16 / fp8 outputs, with and without
    GELU"""
    oqs = 4.0
    for N in NS_FP8:
        a8, w8, b, r, sc, y = _problem_fp8(M, N, K)
        for bm in (0,) + HEIGHTS:
            pl = dict(kernel=-1, tile_rows=bm)
            out = torch.full((M, N), float("nan"), device="cuda")
            _gemm_fp8(L, a8, w8, sc, b, None, out, pl)
            assert rel_err(out, y) < 1e-4, (M, N, K, bm)
            out = r.clone()
            _gemm_fp8(L, a8, w8, sc, b, None, out, pl, resid=out)
            assert rel_err(out, y + r) < 1e-4, (M, N, K, bm)
            for variant in (5, 6):
                pv = dict(pl, variant=variant)
                for act, ref in ((None, y), ("gelu", F.gelu(y))):
                    out = torch.full((M, N), float("nan"), device="cuda", dtype=torch.bfloat16)
                    kern = _gemm_fp8(L, a8, w8, sc, b, act, out, pv)
                    assert kern == (Q if K >= 384 else P)
                    assert torch.isfinite(out).all()
                    assert rel_err(out, ref) < 8e-3, (M, N, K, bm, act, variant)
                    out = torch.zeros(M, N, device="cuda", dtype=L.FP8)
                    kern = _gemm_fp8(L, a8, w8, sc, b, act, out, pv, out_qscale=oqs)
                    assert kern == (Q if K >= 384 and variant == 6 else P)
                    assert rel_err(out.float() / oqs, ref.clamp(-448.0 / oqs, 448.0 / oqs)) < 6e-2, \
                        (M, N, K, bm, act, variant)   # e4m3


def _all_cases(L):
    """every case of this file, in the parametrisation's terms"""
    for M in MS:
        for K in KS:
            test_kstep_paths_bf16(L, M, K)
        for K in KS_FP8:
            test_kstep_paths_fp8(L, M, K)
    for K in (192, 320):
        for N in (516, 520):
            test_kstep_tile_heights(L, N, K)
        for cu_budget in (2, 8, 16):
            test_kstep_uneven_walks(L, K, cu_budget)
        test_kstep_kernels_agree(L, K)


def test_kernel_choice():
    """The library's record of the kernel and tile height it chose (BF_GEMM_LOG=1: one line per
    distinct shape, epilogue and choice, read once per process, hence the child) for every call of
    this file equals what expect_bf16 / expect_fp8 state: no call runs on another kernel or height,
    and every choice the file means to reach is reached."""
    env = dict(os.environ, PYTHONPATH=ROOT, BF_GEMM_LOG="1")
    r = subprocess.run([sys.executable, "-u", os.path.abspath(__file__)], cwd=ROOT, env=env, timeout=110,
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    expected = {ln for ln in r.stdout.splitlines() if ln.startswith("bf_gemm")}
    logged = {ln for ln in r.stderr.splitlines() if ln.startswith("bf_gemm")}
    assert logged == expected, (sorted(logged - expected)[:10], sorted(expected - logged)[:10])
    # and the walk's bodies are among them: 3 and 5 K-tiles on k_gemm256q at every height, for the
    # bench's three forms and the fp8-operand ones
    for K in (192, 320):
        for bm in HEIGHTS:
            for key in ("act=0 resid=0 resid_mod=0 row_map=0 out=bf16", "act=1 resid=0 resid_mod=0 row_map=0 out=bf16",
                        "act=0 resid=1 resid_mod=0 row_map=0 out=f32"):
                assert f"bf_gemm M=513 N=520 K={K} {key} -> {Q} rows={bm}" in logged
            for key in ("act=0 resid=0 out=bf16", "act=1 resid=0 out=bf16", "act=0 resid=0 out=fp8", "act=1 resid=0 out=fp8"):
                assert f"bf_gemm_fp8 M=513 N=520 K={2 * K} {key} -> {Q} rows={bm}" in logged


if __name__ == "__main__":
    from boxfusion_amd import _lib
    EXPECTED = set()
    _all_cases(_lib)
    torch.cuda.synchronize()
    print("\n".join(sorted(EXPECTED)), flush=True)
