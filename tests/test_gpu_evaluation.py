"""Evaluation on the GPU: bf_gt_frustum and bf_nn_min_dist2 against the reference's
data_process/filter_gt_boxes.py (through tests/golden/gt_filter.npz, which the reference's own two
functions produced) and scipy's cKDTree; bf_obb_iou_exact against closed forms and qhull; then
filter_gt_boxes, score and the command line on top of them.

The IoU bound of 1e-9 absolute is derived, not measured: the tolerance band of the coplanar rule
moves a face by at most 1e-12 x the half-diagonal, which changes the volume by at most that times the
surface area, and for aspect ratios up to 100:1 that is below 1e-9 of the box volume.  Each family
prints the largest error it actually shows (run with -s to see it)."""
import json
import os
import pickle

import numpy as np
import pytest
import torch
from scipy.spatial import ConvexHull, HalfspaceIntersection, cKDTree
from scipy.spatial.transform import Rotation

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gt_filter.npz")
FR_CHUNK, FR_GROUPS = 64, 32        # poses per LDS pass of bf_gt_frustum, pose chunks walked side by side
NN_CHUNK, NN_GROUPS = 1024, 256     # the same of bf_nn_min_dist2 and its points
IOU_TOL = 1e-9


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from boxfusion_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def G():
    return dict(np.load(GOLDEN))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(DEV)


# ---- frustum --------------------------------------------------------------------------------------
def frustum_seen(L, G, corners, poses):
    K = G["K"]
    with np.errstate(all="ignore"):
        pose_inv = np.linalg.inv(poses)
    H, W = G["image_hw"]
    return L.gt_frustum_seen(dev(corners), dev(pose_inv), K[0, 0], K[1, 1], K[0, 2], K[1, 2], int(W), int(H),
                             float(G["near"]), float(G["far"])).cpu().numpy().astype(bool)


def test_frustum_matches_reference(L, G):
    seen = frustum_seen(L, G, G["corners"], G["poses"])
    assert np.array_equal(seen, G["seen"])
    assert np.array_equal(seen.sum(1) >= 6, G["frustum_mask"])
    # the cases the fixture was built for are all there
    tot = G["seen"].sum(1)
    assert {0, 5, 6, 8} <= set(tot.tolist()) and not np.isfinite(G["poses"]).all()


def blind_poses(G, count):
    """`count` finite poses that see none of the boxes (the real ones moved 500 m along y), with a
    lost-tracking pose among them"""
    base = G["poses"][np.isfinite(G["poses"]).all((1, 2))]
    out = np.tile(base, (count // len(base) + 1, 1, 1))[:count].copy()
    out[:, 1, 3] += 500.0
    out[count // 2] = -np.inf
    return out


@pytest.mark.parametrize("lead", [3 * FR_CHUNK, 3 * FR_CHUNK - 6, (FR_GROUPS + 2) * FR_CHUNK + 5])
def test_frustum_many_pose_chunks(L, G, lead):
    """the informative poses come last (in the tail chunk, across a chunk boundary, and in a block's
    second chunk), after poses that see nothing, so no early exit can hide a chunk"""
    poses = np.concatenate([blind_poses(G, lead), G["poses"]])
    assert np.array_equal(frustum_seen(L, G, G["corners"], poses), G["seen"])
    assert not frustum_seen(L, G, G["corners"], poses[:lead]).any()


def test_frustum_single_box(L, G):
    for i in (0, 17, len(G["corners"]) - 1):
        assert np.array_equal(frustum_seen(L, G, G["corners"][i:i + 1], G["poses"]), G["seen"][i:i + 1])


def test_frustum_public(L, G):
    from boxfusion_amd import evaluation as E
    mask, seen = E.frustum_visible(G["corners"], G["K"], G["poses"], G["image_hw"], float(G["near"]), float(G["far"]))
    assert np.array_equal(mask, G["frustum_mask"]) and np.array_equal(seen, G["seen"])
    mask, seen = E.frustum_visible(G["corners"][:0], G["K"], G["poses"], G["image_hw"])
    assert mask.shape == (0,) and seen.shape == (0, 8)


# ---- nearest distance --------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, NN_CHUNK + 17, 3 * NN_CHUNK, (NN_GROUPS + 1) * NN_CHUNK + 5])
def test_nn_matches_kdtree(L, P):
    rng = np.random.default_rng(P)
    q = rng.uniform(-3, 3, (296, 3))
    pts = rng.uniform(-3, 3, (P, 3))
    d2 = L.nn_min_dist2(dev(q), dev(pts))
    again = L.nn_min_dist2(dev(q), dev(pts))
    assert torch.equal(d2.view(torch.int64), again.view(torch.int64))
    want = cKDTree(pts).query(q, k=1)[0]
    np.testing.assert_allclose(np.sqrt(d2.cpu().numpy()), want, rtol=1e-14, atol=0)


def test_nn_no_points(L):
    d2 = L.nn_min_dist2(dev(np.zeros((5, 3))), dev(np.zeros((0, 3))))
    assert torch.isinf(d2).all()


def test_proximity_matches_reference(L, G):
    from boxfusion_amd import evaluation as E
    mask, dist = E.proximity_mask(G["corners"], G["points"], float(G["threshold"]))
    assert np.array_equal(mask, G["proximity_all"])
    np.testing.assert_allclose(dist, G["dists"], rtol=1e-14, atol=0)
    near = (G["dists"] < G["threshold"]).sum(1)[G["frustum_mask"]]
    assert {3, 4} <= set(near.tolist())


# ---- exact IoU: helpers and oracles ------------------------------------------------------------------
def box12(c, h, R=None):
    R = np.eye(3) if R is None else R
    return np.concatenate([np.asarray(c, np.float64), (R * np.asarray(h, np.float64)).T.reshape(-1)])


def planes(box):
    c, A = box[:3], box[3:].reshape(3, 3)
    out = []
    for a in A:
        ln = np.linalg.norm(a)
        n = a / ln
        out += [np.r_[n, -(n @ c + ln)], np.r_[-n, -(-n @ c + ln)]]      # n.x + off <= 0
    return np.array(out)


def volume(box):
    return 8.0 * np.prod(np.linalg.norm(box[3:].reshape(3, 3), axis=1))


def strictly_inside(box, p):
    return bool((planes(box) @ np.r_[p, 1.0] < 0).all())


def qhull_iou(a, b, interior):
    v = ConvexHull(HalfspaceIntersection(np.concatenate([planes(a), planes(b)]), np.asarray(interior)).intersections).volume
    return v / (volume(a) + volume(b) - v), v


def run_iou(L, a, b, with_inter=True):
    out = L.obb_iou_exact(dev(np.reshape(a, (-1, 12))), dev(np.reshape(b, (-1, 12))), with_inter=with_inter)
    return tuple(o.cpu().numpy() for o in out) if with_inter else out.cpu().numpy()


def pairwise(L, A, B):
    """the diagonal of the IoU / intersection matrices of two equally long box lists"""
    iou, inter = run_iou(L, np.stack(A), np.stack(B))
    return np.diagonal(iou).copy(), np.diagonal(inter).copy(), iou, inter


def rotated_pairs(n, offset, seed0):
    rng = np.random.default_rng(seed0)
    A, B = [], []
    for t in range(n):
        c1 = rng.uniform(-1, 1, 3)
        c2 = c1 + rng.uniform(-offset, offset, 3)
        A.append(box12(c1, rng.uniform(0.2, 1, 3), Rotation.random(random_state=seed0 + t).as_matrix()))
        B.append(box12(c2, rng.uniform(0.2, 1, 3), Rotation.random(random_state=seed0 + 5000 + t).as_matrix()))
    return A, B


def check_invariants(L, A, B, iou, inter):
    """every pair: 0 <= inter <= min(VA, VB), and iou(A, B) == iou(B, A) within 1e-12.  The kernel
    bounds inter by its own rounding of the two volumes; volume() here rounds three norms and three
    products on its own, so the two sides may differ by a few units in the last place: 8 are allowed"""
    va, vb = np.array([volume(x) for x in A]), np.array([volume(x) for x in B])
    lim = np.minimum(va[:, None], vb[None, :]) * (1 + 8 * np.finfo(np.float64).eps)
    assert (inter >= 0).all() and (inter <= lim).all()
    back, _ = run_iou(L, np.stack(B), np.stack(A))
    assert np.abs(iou - back.T).max() <= 1e-12


# ---- exact IoU: the closed-form family -----------------------------------------------------------------
def aabb_iou(a, b):
    ca, ha, cb, hb = a[:3], np.abs(a[3:].reshape(3, 3)).sum(0), b[:3], np.abs(b[3:].reshape(3, 3)).sum(0)
    ext = np.minimum(ca + ha, cb + hb) - np.maximum(ca - ha, cb - hb)
    v = float(np.prod(ext)) if (ext > 0).all() else 0.0
    return v / (8 * np.prod(ha) + 8 * np.prod(hb) - v), v


def test_iou_axis_aligned_closed_form(L):
    rng = np.random.default_rng(3)
    A, B, exact_zero = [], [], []

    def add(a, b, zero=False):
        A.append(a)
        B.append(b)
        exact_zero.append(zero)
    for _ in range(5):                                                   # identical
        b = box12(rng.uniform(-5, 5, 3), rng.uniform(0.1, 2, 3))
        add(b, b.copy())
    for _ in range(5):                                                   # nested
        c, h = rng.uniform(-5, 5, 3), rng.uniform(0.5, 2, 3)
        add(box12(c, h), box12(c + rng.uniform(-0.1, 0.1, 3), h * rng.uniform(0.2, 0.6, 3)))
    for ax in range(3):                                                  # face to face: exactly 0
        off = np.zeros(3)
        off[ax] = 1.0
        add(box12(np.zeros(3), [0.5] * 3), box12(off, [0.5] * 3), zero=True)
        add(box12(np.zeros(3), [0.25, 0.5, 0.75]), box12(-1.5 * off, [1.25, 1.0, 0.75]), zero=True)
    for _ in range(5):                                                   # disjoint
        c = rng.uniform(-5, 5, 3)
        add(box12(c, rng.uniform(0.1, 1, 3)), box12(c + rng.choice([-1, 1], 3) * rng.uniform(2.5, 6, 3),
                                                    rng.uniform(0.1, 1, 3)), zero=True)
    for d in (0, 1e-15, -1e-15, 1e-13, -1e-13, 1e-9, -1e-9):             # a shared floor plane, then nearly
        add(box12([0, 0, 0.5], [1, 1, 0.5]), box12([0.5, 0, 0.25 + d], [1, 1, 0.25]))
        add(box12([0.5, 0, 0.25 + d], [1, 1, 0.25]), box12([0, 0, 0.5], [1, 1, 0.5]))
        add(box12([0.3, 0.5 + d, -2], [0.2, 0.5, 0.4]), box12([0.3, 0.75, -2.1], [0.7, 0.75, 1.0]))  # a side plane
    for _ in range(100):                                                 # general position
        c = rng.uniform(-1, 1, 3)
        add(box12(c, rng.uniform(0.2, 1, 3)), box12(c + rng.uniform(-0.5, 0.5, 3), rng.uniform(0.2, 1, 3)))
    got, got_v, iou, inter = pairwise(L, A, B)
    want = np.array([aabb_iou(a, b) for a, b in zip(A, B)])
    err = np.abs(got - want[:, 0])
    print(f"\nclosed-form family: {len(A)} pairs, largest IoU error {err.max():.3e}, "
          f"largest volume error {np.abs(got_v - want[:, 1]).max():.3e}")
    zero = np.array(exact_zero)
    assert (got[zero] == 0).all() and (got_v[zero] == 0).all()
    assert err.max() <= IOU_TOL
    check_invariants(L, A, B, iou, inter)


# ---- exact IoU: the rotated family ----------------------------------------------------------------------
def test_iou_rotated_vs_qhull(L):
    A, B = rotated_pairs(300, 0.3, 0)
    got, _, iou, inter = pairwise(L, A, B)
    want = np.array([qhull_iou(a, b, (a[:3] + b[:3]) / 2)[0] for a, b in zip(A, B)])   # none may be skipped
    err = np.abs(got - want)
    print(f"\nrotated family: 300 pairs, largest IoU error {err.max():.3e}")
    assert err.max() <= IOU_TOL
    check_invariants(L, A, B, iou, inter)


def test_iou_rotated_wide_vs_qhull(L):
    A, B = rotated_pairs(400, 0.8, 10000)
    got, _, iou, inter = pairwise(L, A, B)
    errs = []
    for a, b, g in zip(A, B, got):
        mid = (a[:3] + b[:3]) / 2
        if strictly_inside(a, mid) and strictly_inside(b, mid):          # what qhull's interior point needs
            errs.append(abs(g - qhull_iou(a, b, mid)[0]))
    print(f"\nwide rotated family: {len(errs)} of 400 pairs compared, largest IoU error {max(errs):.3e}")
    assert len(errs) >= 200 and max(errs) <= IOU_TOL
    check_invariants(L, A, B, iou, inter)


def test_iou_identical_rotated(L):
    rng = np.random.default_rng(11)
    A = [box12(rng.uniform(-5, 5, 3), rng.uniform(0.05, 2, 3), Rotation.random(random_state=t).as_matrix())
         for t in range(200)]
    got, got_v, _, _ = pairwise(L, A, [a.copy() for a in A])
    print(f"\nidentical rotated boxes: largest |IoU - 1| {np.abs(got - 1).max():.3e}")
    assert np.abs(got - 1).max() <= 1e-12


def test_iou_yaw_only_shared_floor_and_ceiling(L):
    rng = np.random.default_rng(12)
    A, B, mids = [], [], []
    for _ in range(100):
        c0 = rng.uniform(-3, 3, 3)
        R0 = Rotation.from_euler("z", rng.uniform(0, 3)).as_matrix()
        R1 = Rotation.from_euler("z", rng.uniform(0, 3)).as_matrix()
        A.append(box12(c0, [0.5, 0.4, 0.3], R0))
        B.append(box12(c0 + np.array([0.1, 0.05, 0]), [0.45, 0.35, 0.3], R1))
        mids.append(c0 + np.array([0.05, 0.02, 0]))
    got, _, iou, inter = pairwise(L, A, B)
    want = np.array([qhull_iou(a, b, m)[0] for a, b, m in zip(A, B, mids)])
    err = np.abs(got - want)
    print(f"\nyaw-only pairs on shared floor and ceiling planes: largest IoU error {err.max():.3e}")
    assert err.max() <= IOU_TOL
    check_invariants(L, A, B, iou, inter)


def test_iou_matrix_shapes(L):
    """1x1, 3x5 (the remainder of a wave's four pairs), 37x29 (several blocks) and 0x4: an entry
    depends on its pair alone, so the small matrices are corners of the large one, bit for bit"""
    A, B = rotated_pairs(37, 0.5, 20000)
    B = B[:29]
    iou, inter = run_iou(L, np.stack(A), np.stack(B))
    assert iou.shape == (37, 29)
    for p, g in ((1, 1), (3, 5)):
        i2, v2 = run_iou(L, np.stack(A[:p]), np.stack(B[:g]))
        assert np.array_equal(i2, iou[:p, :g]) and np.array_equal(v2, inter[:p, :g])
    only = run_iou(L, np.stack(A), np.stack(B), with_inter=False)           # inter == NULL
    assert np.array_equal(only, iou)
    # rows and columns are where they belong: pair (i, i) overlaps by construction, and single pairs agree
    assert (np.diagonal(iou) > 0).sum() >= 20
    for i, j in ((36, 28), (5, 17), (20, 3)):
        one, _ = run_iou(L, A[i], B[j])
        assert one[0, 0] == iou[i, j]
    check_invariants(L, A, B, iou, inter)
    e_iou, e_inter = run_iou(L, np.zeros((0, 12)), np.stack(B[:4]))
    assert e_iou.shape == (0, 4) and e_inter.shape == (0, 4)
    assert run_iou(L, np.stack(A[:4]), np.zeros((0, 12)), with_inter=False).shape == (4, 0)


def test_iou_empty_box_is_zero(L):
    a = box12([0, 0, 0], [1, 1, 1])
    flat = box12([0, 0, 0], [1, 1, 0.0])
    iou, inter = run_iou(L, np.stack([a, flat]), np.stack([flat, a]))
    assert iou[0, 0] == 0 and iou[1, 0] == 0 and iou[1, 1] == 0 and (inter[[0, 1, 1], [0, 0, 1]] == 0).all()
    assert abs(iou[0, 1] - 1) <= 1e-12


# ---- score, filter, command line ------------------------------------------------------------------------
SIGNS = np.array([[sx, sy, sz] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)], np.float64)


def corners_of(box):
    return box[:3] + SIGNS @ box[3:].reshape(3, 3)


def synthetic_scene():
    """12 ground-truth boxes 10 m apart; 9 predictions shifted along an own axis to IoU 0.6, 2 to IoU
    0.3 (a shift by the fraction s of the box's length gives (1 - s) / (1 + s)), 3 far away"""
    rng = np.random.default_rng(5)
    gt = [box12([10.0 * (i % 4), 10.0 * (i // 4), rng.uniform(-1, 1)], rng.uniform(0.3, 1.5, 3),
                Rotation.random(random_state=100 + i).as_matrix()) for i in range(12)]
    pred = []
    for i in range(11):
        target = 0.6 if i < 9 else 0.3
        s = (1 - target) / (1 + target)
        b = gt[i].copy()
        b[:3] += 2 * s * b[3 + 3 * (i % 3):6 + 3 * (i % 3)]
        pred.append(b)
    for i in range(3):
        pred.append(box12([100.0 + 5 * i, -50, 0], [0.5, 0.6, 0.7], Rotation.random(random_state=i).as_matrix()))
    order = rng.permutation(len(pred))
    pred_c = np.stack([corners_of(pred[i])[rng.permutation(8)] for i in order])
    gt_c = np.stack([corners_of(g)[rng.permutation(8)] for g in gt])
    return pred_c, gt_c


def check_scene_score(res):
    assert res["n_pred"] == 14 and res["n_gt"] == 12 and len(res["matches"]) == 11
    for t, tp in ((0.25, 11), (0.5, 9)):
        r = res["at"][t]
        p, q = tp / 14, tp / 12
        assert r["tp"] == tp
        assert abs(r["precision"] - p) <= 1e-12 and abs(r["recall"] - q) <= 1e-12
        assert abs(r["f1"] - 2 * p * q / (p + q)) <= 1e-12
    v = np.sort([m[2] for m in res["matches"]])
    assert np.abs(v[:2] - 0.3).max() <= IOU_TOL and np.abs(v[2:] - 0.6).max() <= IOU_TOL
    assert abs(res["mean_iou"] - (9 * 0.6 + 2 * 0.3) / 11) <= IOU_TOL


def test_score_synthetic_scene(L):
    from boxfusion_amd import evaluation as E
    pred_c, gt_c = synthetic_scene()
    iou = E.iou_matrix(pred_c, gt_c)
    assert iou.is_cuda and iou.dtype == torch.float64 and tuple(iou.shape) == (14, 12)
    check_scene_score(E.score(pred_c, gt_c))


def test_filter_gt_boxes_end_to_end(L, G):
    from boxfusion_amd import evaluation as E
    args = (G["corners"], G["K"], G["poses"], G["image_hw"])
    kw = dict(near=float(G["near"]), far=float(G["far"]), dist_threshold=float(G["threshold"]))
    for points in (G["points"], torch.from_numpy(G["points"]).to(DEV)):
        kept, mask = E.filter_gt_boxes(*args, points, **kw)
        assert np.array_equal(mask, G["frustum_mask"])
        assert np.array_equal(kept, G["filtered"])
    assert 0 < len(G["filtered"]) < G["frustum_mask"].sum() < len(G["corners"])


def write_ply_f64(path, pts):
    with open(path, "wb") as fh:
        fh.write(("ply\nformat binary_little_endian 1.0\n" f"element vertex {len(pts)}\n"
                  "property double x\nproperty double y\nproperty double z\nend_header\n").encode("ascii"))
        fh.write(np.ascontiguousarray(pts, "<f8").tobytes())


def test_cli_filter_and_score(L, G, tmp_path, capsys):
    from PIL import Image
    from boxfusion_amd import evaluation as E
    seq = tmp_path / "seq"
    (seq / "depth").mkdir(parents=True)
    H, W = (int(v) for v in G["image_hw"])
    Image.fromarray(np.zeros((H, W), np.uint16)).save(seq / "depth" / "0.png")
    with open(seq / "instances.json", "w") as fh:
        json.dump([{"id": i, "corners": c.tolist()} for i, c in enumerate(G["corners"])], fh)
    np.savetxt(seq / "K_depth.txt", G["K"])
    np.save(seq / "all_poses.npy", G["poses"])
    write_ply_f64(seq / "mesh.ply", G["points"])
    assert E.main(["filter", str(seq)]) == 0                             # the defaults are the fixture's settings
    out = capsys.readouterr().out
    assert f"({len(G['corners'])}, 8, 3)" in out and f"({len(G['filtered'])}, 8, 3)" in out
    assert np.array_equal(np.load(seq / "after_filter_boxes.npy"), G["filtered"])

    pred_c, gt_c = synthetic_scene()
    with open(tmp_path / "scene_boxes.pkl", "wb") as fh:
        pickle.dump([[(0, c.astype(np.float32), 1.0) for c in pred_c]], fh)
    np.save(tmp_path / "gt.npy", gt_c.astype(np.float32))
    assert E.main(["score", str(tmp_path / "scene_boxes.pkl"), str(tmp_path / "gt.npy"), "--json",
                   str(tmp_path / "score.json")]) == 0
    res = json.load(open(tmp_path / "score.json"))
    assert res["n_pred"] == 14 and res["n_gt"] == 12
    # f32 corners, as the pipeline writes them: the counts are exact, the IoUs near
    assert res["at"]["0.25"]["tp"] == 11 and res["at"]["0.5"]["tp"] == 9
    assert abs(res["at"]["0.5"]["precision"] - 9 / 14) <= 1e-12
    assert "precision" in capsys.readouterr().out
