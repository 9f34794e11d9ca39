"""Times of the three evaluation kernels against numpy / scipy on the host (a measurement aid, no
threshold):

  bf_gt_frustum     N = 2000 boxes x M = 5000 poses, against the reference's loop over the poses
                    (data_process/filter_gt_boxes.py:36-62 restated in numpy, one np.dot per pose)
  bf_nn_min_dist2   Q = 16000 queries x P = 4 M points, against scipy's cKDTree (build + query with
                    16 workers; the reference builds its KDTree per call as well)
  bf_obb_iou_exact  a 500 x 500 matrix of boxes scattered through a room, against qhull
                    (HalfspaceIntersection + ConvexHull) on the pairs whose centres' midpoint lies
                    inside both boxes, the ones qhull can be handed without a search for an interior
                    point; qhull's time per pair is what the comparison rests on

Device times are the median of REPS runs between device events after a warm-up; host times are one
run each.  --scale shrinks every size for a rehearsal.  One JSON line at the end."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from scipy.spatial import ConvexHull, HalfspaceIntersection, cKDTree
from scipy.spatial.transform import Rotation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from boxfusion_amd import _lib  # noqa: E402

REPS = 7
WORKERS = 16
SIGNS = np.array([[sx, sy, sz] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)], np.float64)


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
    return float(np.median(out)), float(min(out)), float(max(out))


def host_s(fn):
    t = time.perf_counter()
    r = fn()
    return time.perf_counter() - t, r


def random_boxes(rng, n, room, lo, hi):
    c = rng.uniform(0, 1, (n, 3)) * room
    h = rng.uniform(lo, hi, (n, 3)) / 2
    R = Rotation.random(n, random_state=rng).as_matrix()
    return np.concatenate([c, (R * h[:, None, :]).transpose(0, 2, 1).reshape(n, 9)], 1)


def corners_of(boxes):
    return boxes[:, None, :3] + np.einsum("sk,nkj->nsj", SIGNS, boxes[:, 3:].reshape(-1, 3, 3))


def bench_frustum(rng, N, M, dev):
    K = np.array([[500.0, 0, 320], [0, 500.0, 240], [0, 0, 1]])
    W, H, near, far = 640, 480, 0.1, 100.0
    corners = corners_of(random_boxes(rng, N, np.array([10.0, 10.0, 3.0]), 0.2, 1.5))
    # a hand-held walk through the room: positions along a loop, the camera turning as it goes
    t = np.linspace(0, 1, M)
    poses = np.tile(np.eye(4), (M, 1, 1))
    poses[:, :3, :3] = Rotation.from_euler("yx", np.stack([2 * np.pi * 3 * t, 0.3 * np.sin(20 * t)], 1)).as_matrix()
    poses[:, :3, 3] = np.stack([5 + 3 * np.cos(2 * np.pi * t), 5 + 3 * np.sin(2 * np.pi * t), 1.5 + 0 * t], 1)
    poses[M // 3] = -np.inf

    def host():
        seen = np.zeros((N, 8), bool)
        hom = np.concatenate([corners, np.ones((N, 8, 1))], -1)
        with np.errstate(all="ignore"):
            for i in range(M):
                cam = np.dot(hom, np.linalg.inv(poses[i]).T)
                x, y, z = cam[..., 0], cam[..., 1], cam[..., 2]
                ok = (z > near) & (z < far)
                u = (K[0, 0] * x / z + K[0, 2]).astype(int)
                v = (K[1, 1] * y / z + K[1, 2]).astype(int)
                seen |= ok & (u >= 0) & (u < W) & (v >= 0) & (v < H)
        return seen
    host_t, want = host_s(host)
    with np.errstate(all="ignore"):
        pinv = torch.from_numpy(np.linalg.inv(poses)).to(dev)
    c = torch.from_numpy(corners).to(dev)
    run = lambda: _lib.gt_frustum_seen(c, pinv, 500.0, 500.0, 320.0, 240.0, W, H, near, far)  # noqa: E731
    ms = device_ms(run)
    got = run().cpu().numpy().astype(bool)
    return dict(N=N, M=M, device_ms=round(ms[0], 3), device_ms_min_max=[round(ms[1], 3), round(ms[2], 3)],
                host_s=round(host_t, 3), corners_differing=int((got != want).sum()),
                corners_seen=int(want.sum()), boxes_kept=int((want.sum(1) >= 6).sum()))


def bench_nn(rng, Q, P, dev):
    pts = rng.uniform(0, 10, (P, 3)) * [1, 1, 0.3]
    q = rng.uniform(0, 10, (Q, 3)) * [1, 1, 0.3]
    build_t, tree = host_s(lambda: cKDTree(pts))
    query_t, (want, _) = host_s(lambda: tree.query(q, k=1, workers=WORKERS))
    dq, dp = torch.from_numpy(q).to(dev), torch.from_numpy(pts).to(dev)
    ms = device_ms(lambda: _lib.nn_min_dist2(dq, dp))
    got = np.sqrt(_lib.nn_min_dist2(dq, dp).cpu().numpy())
    pair_rate = Q * P / (ms[0] * 1e-3)
    return dict(Q=Q, P=P, device_ms=round(ms[0], 3), device_ms_min_max=[round(ms[1], 3), round(ms[2], 3)],
                kdtree_build_s=round(build_t, 3), kdtree_query_s=round(query_t, 3),
                worst_rel_diff=float(np.max(np.abs(got - want) / want)),
                device_pairs_per_s=float(f"{pair_rate:.4g}"), device_f64_flops_per_s=float(f"{8 * pair_rate:.4g}"))


def planes(box):
    c, A = box[:3], box[3:].reshape(3, 3)
    out = []
    for a in A:
        ln = np.linalg.norm(a)
        n = a / ln
        out += [np.r_[n, -(n @ c + ln)], np.r_[-n, -(-n @ c + ln)]]
    return np.array(out)


def bench_iou(rng, n, dev, max_qhull=2000):
    a = random_boxes(rng, n, np.array([10.0, 10.0, 3.0]), 0.3, 2.0)
    b = random_boxes(rng, n, np.array([10.0, 10.0, 3.0]), 0.3, 2.0)
    da, db = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    ms = device_ms(lambda: _lib.obb_iou_exact(da, db))
    iou = _lib.obb_iou_exact(da, db).cpu().numpy()
    pa = np.stack([planes(x) for x in a])
    pb = np.stack([planes(x) for x in b])
    cand = np.argwhere(iou > 0)
    todo = []
    for i, j in cand:
        mid = np.r_[(a[i, :3] + b[j, :3]) / 2, 1.0]
        if (pa[i] @ mid < 0).all() and (pb[j] @ mid < 0).all():
            todo.append((i, j, mid[:3]))
        if len(todo) == max_qhull:
            break

    def qhull():
        out = []
        for i, j, mid in todo:
            v = ConvexHull(HalfspaceIntersection(np.concatenate([pa[i], pb[j]]), mid).intersections).volume
            va, vb = (8 * np.prod(np.linalg.norm(x[3:].reshape(3, 3), axis=1)) for x in (a[i], b[j]))
            out.append(v / (va + vb - v))
        return np.array(out)
    q_t, want = host_s(qhull)
    got = np.array([iou[i, j] for i, j, _ in todo])
    return dict(P=n, G=n, device_ms=round(ms[0], 3), device_ms_min_max=[round(ms[1], 3), round(ms[2], 3)],
                overlapping_pairs=int(len(cand)), qhull_pairs=len(todo), qhull_s=round(q_t, 3),
                qhull_us_per_pair=round(q_t / max(len(todo), 1) * 1e6, 1),
                worst_iou_diff=float(np.abs(got - want).max()) if len(todo) else None)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scale", type=float, default=1.0, help="shrink every size by this factor (rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench: needs a HIP device")
    _lib.lib()
    dev = torch.device("cuda")
    s = args.scale
    rng = np.random.default_rng(0)
    out = dict(device=torch.cuda.get_device_name(0), host_threads=WORKERS, reps=REPS)
    out["frustum"] = bench_frustum(rng, max(int(2000 * s), 1), max(int(5000 * s), 1), dev)
    print("frustum", out["frustum"], flush=True)
    out["nn"] = bench_nn(rng, max(int(16000 * s), 1), max(int(4_000_000 * s), 1), dev)
    print("nn", out["nn"], flush=True)
    out["iou"] = bench_iou(rng, max(int(500 * s), 2), dev)
    print("iou", out["iou"], flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
