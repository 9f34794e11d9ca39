"""CU-time of the persistent GEMM by tile height, and what a second stream makes of the CUs a
256-row grid leaves free.

Part 1: the six path shapes at 160 / 192 / 224 / 256 rows, alone: time (HIP events, median of 3
rounds of 10), grid (bf_gemm_grid_plan) and CU-time = grid x time.
Part 2: two streams, each looping one CLIP ViT-H layer's GEMM sequence (qkv, proj + residual,
fc1 + GELU, fc2 + residual) on its own buffers, bf_gemm_plan.objective 0 (throughput) and 1
(latency) interleaved in one process; wall time per layer pair.  `lockstep`: both streams run the
same GEMM at the same time; `skewed`: the second stream starts at fc1, so a residual GEMM meets a
qkv / fc1 GEMM.  One stream alone beside it (the single-stream cost).
usage: gemm_height_cutime.py [--layers N] [--rounds R]"""
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from boxfusion_amd import _lib  # noqa: E402

SHAPES = [  # name, M, N, K, act, out_bf16, resid
    ("clip_qkv", 32896, 3840, 1280, None, True, False),
    ("clip_proj", 32896, 1280, 1280, None, False, True),
    ("clip_fc1", 32896, 5120, 1280, "gelu", True, False),
    ("clip_fc2", 32896, 1280, 5120, None, False, True),
    ("cutr_resid768", 12800, 768, 3072, None, False, True),
    ("cutr_w_qkv", 36864, 2304, 768, None, True, False),
]
HEIGHTS = [160, 192, 224, 256]


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def bench(fn, iters=10):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def operands(M, N, K, ob, use_resid, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randn(M, K, device="cuda", generator=g).bfloat16()
    w = (torch.randn(N, K, device="cuda", generator=g) / math.sqrt(K)).bfloat16()
    bias = torch.randn(N, device="cuda", generator=g)
    out = (torch.randn(M, N, device="cuda", generator=g) if use_resid
           else torch.empty((M, N), device="cuda", dtype=torch.bfloat16 if ob else torch.float32))
    return a, w, bias, out


def part1(rounds):
    print("== part 1: one GEMM alone, by tile height (f32 residual GEMMs in place, k_gemm256q) ==", flush=True)
    for name, M, N, K, act, ob, use_resid in SHAPES:
        a, w, bias, out = operands(M, N, K, ob, use_resid, 1)
        times = {h: [] for h in HEIGHTS}
        for _ in range(rounds):
            for h in HEIGHTS:
                pl = dict(tile_rows=h)
                times[h].append(bench(lambda: _lib.gemm(a, w, bias, act=act, resid=out if use_resid else None,
                                                        out=out, plan=pl)))
        pick = {o: _lib.gemm_tile_rows(M, N, K, plan=dict(objective=o)) for o in (0, 1)}
        print(f"{name:14s} M={M} N={N} K={K}  objective 0 -> {pick[0]} rows, objective 1 -> {pick[1]} rows", flush=True)
        for h in HEIGHTS:
            us = sorted(times[h])[len(times[h]) // 2]
            grid = _lib.gemm_grid(M, N, K, plan=dict(tile_rows=h))
            tiles = -(-M // h) * -(-N // 256)
            print(f"    {h} rows: {tiles:5d} tiles -> {grid:3d} workgroups  {us:7.1f} us  "
                  f"{grid * us / 1e3:7.1f}k CU.us", flush=True)


class Layer:
    """one CLIP ViT-H layer's GEMMs on buffers of its own (the attention / LayerNorm between them
    left out: only the GEMMs' sharing of the CUs is measured)"""

    def __init__(self, seed, M=32896, W=1280):
        g = torch.Generator(device="cuda").manual_seed(seed)
        rn = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
        self.h = rn(M, W).bfloat16()
        self.x = rn(M, W)
        self.qkv = torch.empty((M, 3 * W), device="cuda", dtype=torch.bfloat16)
        self.mid = torch.empty((M, 4 * W), device="cuda", dtype=torch.bfloat16)
        self.w = [(rn(n, k) / math.sqrt(k)).bfloat16() for n, k in
                  ((3 * W, W), (W, W), (4 * W, W), (W, 4 * W))]
        self.b = [rn(n) * 0.01 for n in (3 * W, W, 4 * W, W)]

    def gemm(self, i, pl):
        w, b = self.w[i], self.b[i]
        if i == 0:
            _lib.gemm(self.h, w, b, out=self.qkv, plan=pl)
        elif i == 1:
            _lib.gemm(self.h, w, b, resid=self.x, out=self.x, plan=pl)
        elif i == 2:
            _lib.gemm(self.h, w, b, act="gelu", out=self.mid, plan=pl)
        else:
            _lib.gemm(self.mid, w, b, resid=self.x, out=self.x, plan=pl)


def corun(layers, streams, objective, n_layers, skew):
    """launch n_layers x 4 GEMMs on each stream, interleaved GEMM by GEMM; wall us per layer (pair)"""
    pl = dict(objective=objective)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for step in range(4 * n_layers):
        for k, (ly, st) in enumerate(zip(layers, streams)):
            with torch.cuda.stream(st):
                ly.gemm((step + (2 * k if skew else 0)) % 4, pl)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / n_layers


def part2(n_layers, rounds):
    print(f"== part 2: CLIP layer GEMM sequence, {n_layers} layers per timing, wall us per layer (pair) ==", flush=True)
    layers = [Layer(11), Layer(12)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    modes = [("one stream", 1, False), ("two streams lockstep", 2, False), ("two streams skewed", 2, True)]
    res = {(m[0], o): [] for m in modes for o in (0, 1)}
    for o in (0, 1):                                           # warm-up (attributes, clocks)
        corun(layers, streams, o, 2, False)
    for _ in range(rounds):
        for name, ns, skew in modes:
            for o in (0, 1):
                res[(name, o)].append(corun(layers[:ns], streams[:ns], o, n_layers, skew))
    for name, ns, skew in modes:
        med = {}
        for o in (0, 1):
            v = sorted(res[(name, o)])
            med[o] = v[len(v) // 2]
            print(f"{name:22s} objective {o}: median {med[o]:8.1f} us  (min {v[0]:8.1f}, max {v[-1]:8.1f})", flush=True)
        print(f"{name:22s} objective 0 / objective 1 = {med[0] / med[1]:.4f}", flush=True)
    for ly in layers:
        assert torch.isfinite(ly.qkv.float()).all()


if __name__ == "__main__":
    torch.cuda.init()
    print(torch.cuda.get_device_name(0), flush=True)
    if "--no-part1" not in sys.argv:
        part1(arg("--rounds1", 3))
    part2(arg("--layers", 16), arg("--rounds", 7))
