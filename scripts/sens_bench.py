"""Depth decode throughput for ScanNet .sens containers: the GPU decode of bare zlib streams
(bf_zlib_decode_u16) in launches of 64 and of 1024 streams of 480 x 640 synthetic depth compressed
at zlib level 6, against zlib.decompress on host threads, and bf_png_decode_u16 on the same images
written as PNG by PIL (level 6) -- the same inflate plus the chunk walk and the unfilter.  One
warm-up launch (checked against the host decode), then the median of `reps` timed launches.
usage: python scripts/sens_bench.py [reps] [host_threads]"""
import io
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

H, W = 480, 640


def depth_images(n_distinct=16):
    from boxfusion_amd.synthetic import frame_rgbd
    return [np.clip(frame_rgbd(f * 5, H, W)[1].astype(np.float64) * 1000.0, 0, 65535).astype(np.uint16)
            for f in range(n_distinct)]


def host_rate(blobs, threads, seconds=3.0):
    def dec(b):
        return np.frombuffer(zlib.decompress(b), "<u2").reshape(H, W)
    n = 0
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        while time.perf_counter() - t0 < seconds:
            batch = blobs * max(1, threads // len(blobs) + 1)
            list(ex.map(dec, batch))
            n += len(batch)
    return n / (time.perf_counter() - t0)


def gpu_rate(decode, workspace_bytes, blobs, want_last, reps):
    from boxfusion_amd.capture_stream import upload_files
    F = len(blobs)
    data, offs, offs_h = upload_files(blobs, "cuda")
    out = torch.empty((F, H, W), dtype=torch.int16, device="cuda").view(torch.uint16)
    work = torch.empty(workspace_bytes(F, H, W, int(offs_h[-1])), dtype=torch.uint8, device="cuda")
    decode(data, offs, H, W, out=out, offsets_host=offs_h, work=work)          # warm-up, checked
    assert np.array_equal(out[F - 1].view(torch.int16).cpu().numpy().view(np.uint16), want_last)
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        decode(data, offs, H, W, out=out, offsets_host=offs_h, work=work, check=False)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ms = float(np.median(ts))
    return ms, min(ts), max(ts), F / ms * 1e3


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    threads = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    from boxfusion_amd import _lib
    _lib.lib()
    imgs = depth_images()
    zs = [zlib.compress(im.tobytes(), 6) for im in imgs]
    pngs = []
    for im in imgs:
        b = io.BytesIO()
        Image.fromarray(im).save(b, format="PNG", compress_level=6)
        pngs.append(b.getvalue())
    print(f"{len(imgs)} distinct {W} x {H} depth maps: zlib level 6 mean {np.mean([len(z) for z in zs]) / 1e3:.0f} KB, "
          f"PNG (PIL, level 6) mean {np.mean([len(p) for p in pngs]) / 1e3:.0f} KB", flush=True)
    for F in (64, 1024):
        for name, pool, decode, wsb in (("bf_zlib_decode_u16", zs, _lib.zlib_decode_u16, _lib.zlib_workspace_bytes),
                                        ("bf_png_decode_u16", pngs, _lib.png_decode_u16, _lib.png_workspace_bytes)):
            blobs = [pool[i % len(pool)] for i in range(F)]
            ms, lo, hi, rate = gpu_rate(decode, wsb, blobs, imgs[(F - 1) % len(imgs)], reps)
            print(f"{name} {F} per launch: {ms:.2f} ms (median of {reps}; min {lo:.2f}, max {hi:.2f}) -> "
                  f"{rate:.0f} streams/s", flush=True)
    print(f"host zlib.decompress, {threads} threads: {host_rate(zs, threads):.0f} streams/s", flush=True)


if __name__ == "__main__":
    main()
