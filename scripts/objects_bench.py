"""Times of bf_label_points on a synthetic room (a measurement aid, no threshold):

  room         about 2 M points on the walls, floor and ceiling of a 6 x 5 x 2.8 m room and on the faces of the
               boxes standing in it, one point per occupied 1 cm voxel, sorted by voxel key (x, then y, then z)
               as SceneCloud.points() hands them over; against 16 and 128 boxes with a random yaw
  kernel       _lib.label_points as the product calls it (outputs allocated and initialised in the call), and
               bf_label_points_ex alone on outputs made beforehand, each with the per-wave cull off and on, on
               the sorted points and on the same points shuffled; with BF_OBJ_STAT_PAIR_TESTS
  torch        the same labelling as chunked torch broadcast ops on the same device: per chunk of 65536 points
               the [chunk, B, 3] offsets, the three dot products, the comparison, an argmin over the masked
               volumes, and scatter-reduced counts and extents; its labels are compared with the kernel's

Device times are the median of REPS runs between device events after a warm-up, with their min and max.
--scale shrinks the room's point count for a rehearsal.  One JSON line at the end."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from boxfusion_amd import _lib, scene_objects  # noqa: E402

REPS = 9
ROOM_LO, ROOM_HI = np.array([-3.0, -2.5, 0.0]), np.array([3.0, 2.5, 2.8])
VOXEL = 0.01
TORCH_CHUNK = 65536


def device_ms(fn):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return dict(ms=round(float(np.median(out)), 4), min=round(float(min(out)), 4), max=round(float(max(out)), 4))


def box_corners(rng, n):
    """n boxes standing on the floor with a random yaw: corners f64 [n,8,3]"""
    half = rng.uniform([0.15, 0.15, 0.15], [0.9, 0.6, 0.6], size=(n, 3))
    centre = np.concatenate([rng.uniform(ROOM_LO[:2] + 0.9, ROOM_HI[:2] - 0.9, size=(n, 2)), half[:, 2:3]], 1)
    yaw = rng.uniform(0, 2 * np.pi, n)
    R = np.zeros((n, 3, 3))
    R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1], R[:, 2, 2] = np.cos(yaw), -np.sin(yaw), np.sin(yaw), np.cos(yaw), 1.0
    signs = np.array([[sx, sy, sz] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)], np.float64)
    return centre[:, None] + np.einsum("sk,bk,bjk->bsj", signs, half, R), centre, R, half


def room_points(rng, boxes, target):
    """points on the room's six faces and on the boxes' faces, one per occupied voxel, sorted by voxel key"""
    _, centre, R, half = boxes
    size = ROOM_HI - ROOM_LO
    parts = []
    area = 2.0 * sum(np.prod(np.delete(size, axis)) for axis in range(3))
    for axis in range(3):
        for side in (ROOM_LO, ROOM_HI):                           # 2.5 samples per wanted point: most voxels get one
            p = rng.uniform(ROOM_LO, ROOM_HI, size=(int(2.5 * target * np.prod(np.delete(size, axis)) / area), 3))
            p[:, axis] = side[axis] + rng.normal(0, 0.003, len(p))
            parts.append(p)
    per_box = int(target * 0.5 / len(centre))
    for c, r, h in zip(centre, R, half):
        q = rng.uniform(-1, 1, size=(per_box, 3)) * h
        ax = rng.integers(0, 3, per_box)
        q[np.arange(per_box), ax] = np.sign(q[np.arange(per_box), ax]) * h[ax] * 0.98
        parts.append(c + q @ r.T)
    p = np.concatenate(parts)
    idx = np.floor(p / VOXEL).astype(np.int64) + (1 << 20)
    key = (idx[:, 0] << 42) | (idx[:, 1] << 21) | idx[:, 2]
    key, first = np.unique(key, return_index=True)                # sorted by key, one point per voxel
    return p[first].astype(np.float32)


def torch_label(xyz, rows, margin=0.0):
    """the rule of include/boxfusion_objects.h as broadcast ops: (labels int32 [n], counts int64 [B,2],
    extents f32 [B,3,2])"""
    n, B = xyz.shape[0], rows.shape[0]
    c, A, lim, vol = rows[:, 0:3], rows[:, 3:12].reshape(B, 3, 3), rows[:, 12:15] + margin, rows[:, 15]
    labels = torch.empty(n, dtype=torch.int32, device=xyz.device)
    support = torch.zeros(B, dtype=torch.int64, device=xyz.device)
    owned = torch.zeros(B, dtype=torch.int64, device=xyz.device)
    lo = torch.full((B, 3), float("inf"), device=xyz.device)
    hi = torch.full((B, 3), float("-inf"), device=xyz.device)
    inf = torch.tensor(float("inf"), device=xyz.device)
    for a in range(0, n, TORCH_CHUNK):
        p = xyz[a:a + TORCH_CHUNK]
        d = p[:, None, :] - c[None]                               # [m,B,3]
        t = (d[:, :, None, 0] * A[None, :, :, 0] + d[:, :, None, 1] * A[None, :, :, 1]) + d[:, :, None, 2] * A[None, :, :, 2]
        inside = (t.abs() <= lim[None]).all(-1) & torch.isfinite(p).all(-1)[:, None]
        support += inside.sum(0)
        best = torch.where(inside, vol[None], inf).argmin(1)
        hit = inside.any(1)
        labels[a:a + TORCH_CHUNK] = torch.where(hit, best, torch.full_like(best, -1)).to(torch.int32)
        own = best[hit]
        owned += torch.bincount(own, minlength=B)
        tb = t[hit, own]                                          # [k,3]
        lo.scatter_reduce_(0, own[:, None].expand(-1, 3), tb, "amin")
        hi.scatter_reduce_(0, own[:, None].expand(-1, 3), tb, "amax")
    return labels, torch.stack([support, owned], 1), torch.stack([lo, hi], -1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the point count by this factor (rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("objects_bench: needs a HIP device")
    lib = _lib.lib()
    dev = torch.device("cuda")
    out = dict(device=torch.cuda.get_device_name(0), reps=REPS, chunk=_lib.OBJ_CHUNK)
    for n_boxes in (16, 128):
        rng = np.random.default_rng(n_boxes)
        boxes = box_corners(rng, n_boxes)
        host = room_points(rng, boxes, int(1.6e6 * args.scale))
        rows, degenerate = scene_objects.box_rows(boxes[0])
        assert not degenerate.any()
        rows = torch.from_numpy(rows).to(dev)
        row = dict(points=len(host), boxes=n_boxes)
        for order, pts in (("sorted", host), ("shuffled", host[rng.permutation(len(host))])):
            xyz = torch.from_numpy(pts).to(dev)
            res = {}
            for cull in (False, True):
                name = f"{order}_cull_{'on' if cull else 'off'}"
                row[name] = device_ms(lambda: _lib.label_points(xyz, rows, 0.0, cull=cull))
                labels, counts, extents, stats = _lib.label_points(xyz, rows, 0.0, cull=cull)
                row[name].update(pair_tests=int(stats[_lib.OBJ_STATS.index("pair_tests")].item()))
                args_ = (_lib._ptr(xyz), len(pts), _lib._ptr(rows), n_boxes, 0.0, _lib._ptr(labels), _lib._ptr(counts),
                         _lib._ptr(extents), _lib._ptr(stats), int(cull), _lib._stream())
                row[name].update(kernel_only=device_ms(lambda: lib.bf_label_points_ex(*args_)))
                res[cull] = _lib.label_points(xyz, rows, 0.0, cull=cull)
                print(n_boxes, name, row[name], flush=True)
            same = all(bool((a == b).all()) for a, b in zip(res[False][:3], res[True][:3]))
            row[f"{order}_cull_same_bits"] = same
            if order == "sorted":
                row["torch"] = device_ms(lambda: torch_label(xyz, rows))
                tl, tc, _ = torch_label(xyz, rows)
                row["torch"].update(label_mismatches=int((tl != res[True][0]).sum().item()),
                                    count_mismatches=int((tc != res[True][1]).sum().item()),
                                    labelled=int((res[True][0] >= 0).sum().item()))
                print(n_boxes, "torch", row["torch"], flush=True)
        out[f"boxes_{n_boxes}"] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
