"""Hash the outputs of a grid of GEMM calls, one line per call: to compare two builds of the library
bit for bit (a kernel restructure that must not move a value).

usage: BF_LIB_PATH=/path/to/libboxfusion_hip.so python scripts/gemm_hash.py > a.txt    (per build)
       diff a.txt b.txt

The grid: bf16 and fp8 operands, the model's tile height and each forced one, every output type
and epilogue, ragged M and N, 3 / 5 / 20 K-tiles, CU budgets of 2 / 200 / all, variants 1 / 5 / 6.
"""
import hashlib
import itertools
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from boxfusion_amd import _lib as L  # noqa: E402

MS, NS = (1, 255, 513, 1300), (8, 252, 520, 1288)
PLANS = [dict(kernel=-1, tile_rows=bm, variant=v, cu_budget=cu)
         for bm, v, cu in itertools.product((0, 160, 192, 224, 256), (1, 5, 6), (0, 2, 200))
         if cu == 0 or (bm in (0, 160) and v != 1)]


def sha(t):
    return hashlib.sha1(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:16]


def main():
    n = 0
    for M, N, nk in itertools.product(MS, NS, (3, 5, 20)):
        g = torch.Generator(device="cuda").manual_seed(M * 31 + N * 7 + nk)
        K = 64 * nk
        a = torch.randn(M, K, device="cuda", generator=g).bfloat16()
        w = (torch.randn(N, K, device="cuda", generator=g) / math.sqrt(K)).bfloat16()
        b = torch.randn(N, device="cuda", generator=g)
        r = torch.randn(M, N, device="cuda", generator=g)
        a8 = (torch.randn(M, 2 * K, device="cuda", generator=g) * 0.5).to(L.FP8)
        w8 = (torch.randn(N, 2 * K, device="cuda", generator=g) * 0.5).to(L.FP8)
        for pl in PLANS:
            tag = f"M={M} N={N} nk={nk} rows={pl['tile_rows']} variant={pl['variant']} cus={pl['cu_budget']}"
            for act, dt in itertools.product((None, "gelu", "relu"), (torch.bfloat16, torch.float32)):
                if dt == torch.bfloat16 and N % 8:
                    continue
                out = torch.zeros(M, N, device="cuda", dtype=dt)
                L.gemm(a, w, b, act=act, out=out, plan=dict(pl))
                print(f"bf16 {tag} act={act} out={dt} {sha(out)}")
                n += 1
            out = torch.zeros(M, N, device="cuda")
            L.gemm(a, w, b, resid=r, out=out, plan=dict(pl))
            print(f"bf16 {tag} resid {sha(out)}")
            out = r.clone()
            L.gemm(a, w, b, resid=out, out=out, plan=dict(pl))
            print(f"bf16 {tag} inplace {sha(out)}")
            n += 2
            if N % 8:
                continue
            sc = 1.0 / math.sqrt(2 * K)
            for act, dt in itertools.product((None, "gelu"), (torch.float32, torch.bfloat16, L.FP8)):
                if act and dt == torch.float32:
                    continue
                out = torch.zeros(M, N, device="cuda", dtype=dt)
                L.gemm_fp8(a8, w8, sc, bias=b, act=act, out=out, out_qscale=4.0 if dt == L.FP8 else 1.0, plan=dict(pl))
                print(f"fp8 {tag} act={act} out={dt} {sha(out)}")
                n += 1
            out = r.clone()
            L.gemm_fp8(a8, w8, sc, bias=b, resid=out, out=out, plan=dict(pl))
            print(f"fp8 {tag} inplace {sha(out)}")
            n += 1
    print(f"{n} calls", file=sys.stderr)


if __name__ == "__main__":
    main()
