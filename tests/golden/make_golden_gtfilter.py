"""Golden fixture for the ground-truth box filter: runs the REFERENCE's frustum_culling_bbox_level and
check_bbox_proximity (data_process/filter_gt_boxes.py:24-68, :75-93) on a small designed scene.

The reference file is a script with hard-coded paths and `import open3d`, so it cannot be imported.
This generator reads it at run time with `ast`, takes only those two function definitions and
executes them with numpy and scipy.spatial.KDTree.  Only the output is committed, and it holds
arrays only:  python tests/golden/make_golden_gtfilter.py  ->  tests/golden/gt_filter.npz

The per-corner mask is local to the reference function, which returns only the per-box decision
(>= 6 corners).  It is read out through the function itself: a box made of eight copies of one corner
is visible exactly when that corner is.

Every case is there on purpose (the `kind` array names them): boxes fully in view, behind every
camera, beyond `far`, with a corner at u or v in (-1, 0), with exactly 5 and exactly 6 seen corners,
seen only across frames of two different views, one all -inf pose, and exactly 3 and exactly 4 near
corners.  Every decision has a margin above 1e-6, asserted below, so a correct restatement must
reproduce the masks with nothing left out.
"""
import ast
import os

import numpy as np
from scipy.spatial import KDTree
from scipy.spatial.transform import Rotation

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("BOXFUSION_REFERENCE", "/root/reference")
W, H = 64, 48
NEAR, FAR, THRESH = 0.1, 100.0, 0.1
MARGIN = 1e-6
SIGNS = np.array([[sx, sy, sz] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)], np.float64)


def reference_functions():
    src = open(os.path.join(REF, "data_process", "filter_gt_boxes.py")).read()
    want = ("frustum_culling_bbox_level", "check_bbox_proximity")
    defs = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name in want]
    assert sorted(d.name for d in defs) == sorted(want)
    ns = {"np": np, "KDTree": KDTree}
    exec(compile(ast.Module(body=defs, type_ignores=[]), "filter_gt_boxes.py", "exec"), ns)
    return ns["frustum_culling_bbox_level"], ns["check_bbox_proximity"]


def cuboid(centre, half, rot):
    return np.asarray(centre) + (SIGNS * np.asarray(half)) @ np.asarray(rot).T


def pose(rotvec, t):
    P = np.eye(4)
    P[:3, :3] = Rotation.from_rotvec(rotvec).as_matrix()
    P[:3, 3] = t
    return P


def make_poses(rng):
    """view A looks along +z from near the origin, view B along +x; pose 5 is a lost-tracking pose"""
    poses = [pose([0, 0, 0], [0, 0, 0])]
    for _ in range(4):
        poses.append(pose(rng.uniform(-0.08, 0.08, 3), rng.uniform(-0.2, 0.2, 3)))
    poses.append(np.full((4, 4), -np.inf))
    for _ in range(6):
        r = Rotation.from_rotvec(rng.uniform(-0.08, 0.08, 3)) * Rotation.from_rotvec([0, np.pi / 2, 0])
        poses.append(pose(r.as_rotvec(), rng.uniform(-0.2, 0.2, 3)))
    return np.stack(poses)


def main():
    frustum, proximity = reference_functions()
    rng = np.random.default_rng(20)
    K = np.array([[50.0, 0, 32.0], [0, 50.0, 24.0], [0, 0, 1.0]])
    poses = make_poses(rng)
    M = len(poses)
    depth_maps = np.zeros((M, H, W), np.uint16)
    view_of = np.array([0] * 5 + [-1] + [1] * 6)

    def seen_by(corners, which):
        """[N,8] per-corner visibility over the poses `which`, through the reference function"""
        flat = corners.reshape(-1, 1, 3).repeat(8, 1)
        with np.errstate(all="ignore"):
            return frustum(flat, K, poses[which], depth_maps[which], NEAR, FAR).reshape(-1, 8)

    def per_frame(corners):
        return np.stack([seen_by(corners, [m]) for m in range(M)])       # [M,N,8]

    def random_box(centre, lo=0.4, hi=1.2):
        return cuboid(centre, rng.uniform(lo, hi, 3) / 2, Rotation.random(random_state=rng).as_matrix())

    boxes, kind = [], []

    def search(name, count, draw, accept):
        got = 0
        for _ in range(20000):
            b = draw()
            pf = per_frame(b[None])[:, 0]                                # [M,8]
            if accept(pf):
                boxes.append(b)
                kind.append(name)
                got += 1
                if got == count:
                    return
        raise AssertionError(f"no {name} box found")

    total = lambda pf: int(pf.any(0).sum())                               # noqa: E731
    best_frame = lambda pf: int(pf.sum(1).max())                          # noqa: E731
    search("in_view", 6, lambda: random_box([rng.uniform(-1, 1), rng.uniform(-0.7, 0.7), rng.uniform(4, 7)]),
           lambda pf: total(pf) == 8)
    search("behind", 4, lambda: random_box([rng.uniform(-4, -2), rng.uniform(-1, 1), rng.uniform(-6, -2)]),
           lambda pf: total(pf) == 0)
    search("beyond_far", 4, lambda: random_box([rng.uniform(-8, 8), rng.uniform(-6, 6), rng.uniform(104, 130)], 1, 3),
           lambda pf: total(pf) == 0)
    # a corner whose u (then v) falls in (-1, 0) in one frame and that no other frame sees
    finite = [m for m in range(M) if np.isfinite(poses[m]).all()]
    trunc_frame = {}
    for name, axis in (("u_trunc", 0), ("v_trunc", 1)):
        for _ in range(5000):
            m0 = int(rng.choice(finite))
            z = rng.uniform(3.5, 5.0)
            a = np.array([0.0, 0.0, z])
            a[axis] = (-rng.uniform(0.2, 0.8) - K[axis, 2]) / K[axis, axis] * z
            a[1 - axis] = rng.uniform(-0.3, 0.3)
            half = rng.uniform(0.3, 0.6, 3)
            b = cuboid(a + half, half, np.eye(3))                        # corner 0 is `a`, in camera m0's frame
            b = b @ poses[m0][:3, :3].T + poses[m0][:3, 3]
            pf = per_frame(b[None])[:, 0]
            if pf[m0, 0] and pf[:, 0].sum() == 1:
                boxes.append(b)
                kind.append(name)
                trunc_frame[name] = m0
                break
        else:
            raise AssertionError(name)
    edge = lambda: random_box([rng.choice([-1, 1]) * rng.uniform(2.2, 3.6), rng.uniform(-1, 1), rng.uniform(3, 5)],  # noqa: E731
                              0.6, 1.6)
    search("seen_5", 4, edge, lambda pf: total(pf) == 5)
    search("seen_6", 4, edge, lambda pf: total(pf) == 6)

    def between():
        ang = np.deg2rad(rng.uniform(35, 55))
        r = rng.uniform(3, 6)
        return random_box([r * np.sin(ang), rng.uniform(-0.5, 0.5), r * np.cos(ang)], 1.5, 3.5)

    def two_views(pf):
        a, b = pf[view_of == 0].any(0), pf[view_of == 1].any(0)
        return (a | b).sum() >= 6 and a.sum() < 6 and b.sum() < 6 and best_frame(pf) < 6
    search("two_views", 4, between, two_views)
    search("any", 12, lambda: random_box(rng.uniform(-6, 8, 3), 0.4, 2.0), lambda pf: True)
    corners = np.stack(boxes)
    kind = np.array(kind)
    N = len(corners)

    # ---- the frustum decisions and their margins -------------------------------------------------------
    with np.errstate(all="ignore"):
        frustum_mask = frustum(corners, K, poses, depth_maps, NEAR, FAR)
    seen = seen_by(corners, np.arange(M))
    assert np.array_equal(seen.sum(1) >= 6, frustum_mask)
    assert np.array_equal(seen, per_frame(corners).any(0))
    hom = np.concatenate([corners, np.ones((N, 8, 1))], -1)
    for m in range(M):
        if not np.isfinite(poses[m]).all():
            with np.errstate(all="ignore"):
                assert not seen_by(corners, [m]).any()
            continue
        cam = np.dot(hom, np.linalg.inv(poses[m]).T)
        x, y, z = cam[..., 0], cam[..., 1], cam[..., 2]
        assert (np.abs(z - NEAR) > MARGIN).all() and (np.abs(FAR - z) > MARGIN).all()
        ok = (z > NEAR) & (z < FAR)
        u, v = (K[0, 0] * x / z + K[0, 2])[ok], (K[1, 1] * y / z + K[1, 2])[ok]
        assert (np.abs(u) < 2.0 ** 31).all() and (np.abs(v) < 2.0 ** 31).all()
        for val, size in ((u, W), (v, H)):
            assert (np.abs(val + 1) > MARGIN).all() and (np.abs(val - size) > MARGIN).all()
    # the cases are what they are named
    pf = per_frame(corners)
    tot = seen.sum(1)
    assert (tot[kind == "in_view"] == 8).all() and (tot[kind == "seen_5"] == 5).all()
    assert (tot[kind == "seen_6"] == 6).all() and (tot[kind == "behind"] == 0).all()
    assert (pf.sum(2).max(0)[kind == "two_views"] < 6).all() and frustum_mask[kind == "two_views"].all()
    for name, axis in (("u_trunc", 0), ("v_trunc", 1)):
        c = np.linalg.inv(poses[trunc_frame[name]]) @ np.append(corners[kind == name][0, 0], 1.0)
        val = K[axis, axis] * c[axis] / c[2] + K[axis, 2]
        assert -1 + MARGIN < val < -MARGIN and seen[kind == name][0, 0]

    # ---- scene points: a background away from every corner, then points planted next to chosen corners ----
    flat = corners.reshape(-1, 3)
    bg = rng.uniform(-8, 10, (6000, 3))
    bg = bg[KDTree(flat).query(bg)[0] > 3 * THRESH]
    near_count = rng.integers(0, 9, N)
    visible = np.where(frustum_mask)[0]
    near_count[visible[:10]] = [3, 3, 4, 4, 0, 8, 5, 2, 4, 3]
    hidden = np.where(~frustum_mask)[0]
    near_count[hidden[:4]] = [8, 4, 3, 0]
    planted = []
    for i in range(N):
        for j in rng.permutation(8)[:near_count[i]]:
            for _ in range(int(rng.integers(1, 4))):
                d = rng.normal(size=3)
                planted.append(corners[i, j] + d / np.linalg.norm(d) * rng.uniform(0.02, 0.08))
    points = np.concatenate([bg[:3000 - len(planted)], np.array(planted)])
    points = points[rng.permutation(len(points))]
    dists = KDTree(points).query(flat, k=1)[0].reshape(N, 8)
    assert (np.abs(dists - THRESH) > MARGIN).all()
    prox_all = proximity(corners, points, THRESH)
    assert np.array_equal(prox_all, (dists < THRESH).sum(1) >= 4)
    cnt = (dists < THRESH).sum(1)
    assert {3, 4} <= set(cnt[frustum_mask].tolist())
    prox_visible = proximity(corners[frustum_mask], points, THRESH)
    assert np.array_equal(prox_visible, prox_all[frustum_mask])
    filtered = corners[frustum_mask][prox_visible]

    np.savez_compressed(os.path.join(HERE, "gt_filter.npz"), corners=corners, kind=kind, K=K, poses=poses,
                        image_hw=np.array([H, W]), near=NEAR, far=FAR, threshold=THRESH, points=points,
                        seen=seen, frustum_mask=frustum_mask, dists=dists, proximity_all=prox_all,
                        proximity_visible=prox_visible, filtered=filtered)
    print(f"gt_filter.npz: {N} boxes, {M} poses, {len(points)} points; frustum keeps {int(frustum_mask.sum())}, "
          f"proximity keeps {len(filtered)}; seen-corner counts {np.bincount(tot, minlength=9).tolist()}, "
          f"near-corner counts of the kept {np.bincount(cnt[frustum_mask], minlength=9).tolist()}")


if __name__ == "__main__":
    main()
