"""The host side of boxfusion_amd.evaluation: boxes_from_corners, match / score bookkeeping, the PLY
and box-list readers and the command line's argument errors (no GPU)."""
import os
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

from boxfusion_amd import evaluation as E
from boxfusion_amd import results as RS
from boxfusion_amd.visualize import points_to_ply

SIGNS = np.array([[sx, sy, sz] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)], np.float64)


def cuboid(c, h, R):
    return np.asarray(c) + (SIGNS * np.asarray(h)) @ np.asarray(R).T


def rebuilt(box):
    return box[:3] + SIGNS @ box[3:].reshape(3, 3)


def same_point_set(a, b, tol):
    d = np.linalg.norm(a[:, None] - b[None], axis=-1)
    return d.min(1).max() <= tol and d.min(0).max() <= tol


# ---- boxes_from_corners --------------------------------------------------------------------------------
def test_boxes_from_corners_rotated_any_vertex_order():
    rng = np.random.default_rng(0)
    for t in range(20):
        c, h = rng.uniform(-5, 5, 3), np.sort(rng.uniform(0.1, 2.0, 3))[::-1] * [1.0, 0.8, 0.6]
        R = Rotation.random(random_state=t).as_matrix()
        corners = cuboid(c, h, R)
        perms = np.stack([corners[rng.permutation(8)] for _ in range(50)])
        boxes = E.boxes_from_corners(perms)
        assert boxes.shape == (50, 12) and boxes.dtype == np.float64
        np.testing.assert_allclose(boxes[:, :3], np.broadcast_to(c, (50, 3)), rtol=0, atol=1e-12)
        # distinct extents: the canonical form is one and the same row for every vertex order
        np.testing.assert_allclose(boxes, np.broadcast_to(boxes[0], (50, 12)), rtol=0, atol=1e-12)
        np.testing.assert_allclose(np.linalg.norm(boxes[0, 3:].reshape(3, 3), axis=1), h, rtol=0, atol=1e-12)
        for b in boxes[::7]:
            assert same_point_set(rebuilt(b), corners, 1e-12)
            A = b[3:].reshape(3, 3)
            assert np.abs(A @ A.T - np.diag(np.diag(A @ A.T))).max() <= 1e-12      # orthogonal axes


def test_boxes_from_corners_cube_and_device_order():
    """a cube has no longest axis to go by: the corner set is still reproduced; and the pipeline's own
    corner order (GeneralInstance3DBoxes.corners) is one of the orders"""
    rng = np.random.default_rng(1)
    R = Rotation.random(random_state=3).as_matrix()
    corners = cuboid([1, 2, 3], [0.5, 0.5, 0.5], R)
    for _ in range(50):
        b = E.boxes_from_corners(corners[rng.permutation(8)][None])[0]
        assert same_point_set(rebuilt(b), corners, 1e-12)
    sx = np.array([-1, 1, 1, -1, -1, 1, 1, -1.0])
    sy = np.array([-1, -1, 1, 1, -1, -1, 1, 1.0])
    sz = np.array([-1, -1, -1, -1, 1, 1, 1, 1.0])
    dev_order = np.array([0.3, -1, 2]) + (np.stack([sx, sy, sz], 1) * [0.7, 0.2, 0.4]) @ R.T
    b = E.boxes_from_corners(dev_order.astype(np.float32)[None])[0]
    assert same_point_set(rebuilt(b), dev_order, 1e-6)
    assert E.boxes_from_corners(np.zeros((0, 8, 3))).shape == (0, 12)


def test_boxes_from_corners_rejects_non_cuboids():
    corners = cuboid([0, 0, 0], [1, 0.5, 0.25], np.eye(3))
    sheared = corners.copy()
    sheared[:, 0] += 0.2 * sheared[:, 2]                                  # a sheared hexahedron
    with pytest.raises(ValueError, match="not a cuboid"):
        E.boxes_from_corners(sheared[None])
    with pytest.raises(ValueError, match="box 1"):
        E.boxes_from_corners(np.stack([corners, sheared]))
    moved = corners.copy()
    moved[5] += [0.0, 0.01, 0.0]                                         # one corner off by 0.4 % of the diagonal
    with pytest.raises(ValueError):
        E.boxes_from_corners(moved[None])
    moved[5] = corners[5] + [0.0, 1e-4, 0.0]                             # within 1e-3 of the diagonal: accepted
    E.boxes_from_corners(moved[None])
    with pytest.raises(ValueError):
        E.boxes_from_corners(np.zeros((2, 7, 3)))


# ---- match / score --------------------------------------------------------------------------------------
def test_match_greedy_descending():
    iou = np.array([[0.9, 0.8, 0.0],
                    [0.85, 0.1, 0.0],
                    [0.0, 0.0, 0.3]])
    p, g, v = E.match(iou)
    # 0.9 first; it bars 0.85 and 0.8; then 0.3, then 0.1
    assert p.tolist() == [0, 2, 1] and g.tolist() == [0, 2, 1] and v.tolist() == [0.9, 0.3, 0.1]
    p, g, v = E.match(torch.from_numpy(iou))
    assert p.tolist() == [0, 2, 1] and p.dtype == np.int64 and v.dtype == np.float64


def test_match_ties():
    # equal IoUs: the lower pred index first, then the lower gt index
    iou = np.array([[0.5, 0.5],
                    [0.5, 0.5]])
    p, g, _ = E.match(iou)
    assert list(zip(p.tolist(), g.tolist())) == [(0, 0), (1, 1)]
    iou = np.array([[0.0, 0.7, 0.7],
                    [0.7, 0.7, 0.0],
                    [0.7, 0.0, 0.2]])
    p, g, v = E.match(iou)
    assert list(zip(p.tolist(), g.tolist())) == [(0, 1), (1, 0), (2, 2)] and v.tolist() == [0.7, 0.7, 0.2]
    # pairs that do not overlap are never matched
    p, g, v = E.match(np.zeros((3, 2)))
    assert len(p) == len(g) == len(v) == 0
    with pytest.raises(ValueError):
        E.match(np.zeros(4))


def test_score_from_iou_counts():
    iou = np.array([[0.6, 0.0, 0.0, 0.0],
                    [0.0, 0.3, 0.0, 0.0],
                    [0.0, 0.0, 0.2, 0.0]])
    res = E.score_from_iou(iou, thresholds=(0.25, 0.5))
    assert res["n_pred"] == 3 and res["n_gt"] == 4
    assert res["matches"] == [(0, 0, 0.6), (1, 1, 0.3), (2, 2, 0.2)]
    assert abs(res["mean_iou"] - (0.6 + 0.3 + 0.2) / 3) < 1e-15
    a, b = res["at"][0.25], res["at"][0.5]
    assert a["tp"] == 2 and a["precision"] == 2 / 3 and a["recall"] == 2 / 4
    assert abs(a["f1"] - 2 * (2 / 3) * 0.5 / (2 / 3 + 0.5)) < 1e-15
    assert b["tp"] == 1 and b["precision"] == 1 / 3 and b["recall"] == 1 / 4
    # a threshold is met at equality
    assert E.score_from_iou(np.array([[0.5]]), thresholds=(0.5,))["at"][0.5]["tp"] == 1


def test_score_empty_sides():
    box = cuboid([0, 0, 0], [1, 1, 1], np.eye(3))[None]
    none = np.zeros((0, 8, 3))
    for pred, gt in ((none, box), (box, none), (none, none)):
        res = E.score(pred, gt)                                           # nothing to compare: no device needed
        assert res["n_pred"] == len(pred) and res["n_gt"] == len(gt)
        assert res["matches"] == [] and res["mean_iou"] == 0.0
        for t in (0.25, 0.5):
            assert res["at"][t] == {"tp": 0, "precision": 0.0, "recall": 0.0, "f1": 0.0}


class _Inst:
    """what results.global_save_list reads of an Instances3D"""

    def __init__(self, corners):
        self.pred_boxes_3d = SimpleNamespace(corners=torch.from_numpy(corners))
        self.categories = None

    def __len__(self):
        return self.pred_boxes_3d.corners.shape[0]


# ---- files -------------------------------------------------------------------------------------------------
def test_read_ply_round_trips_points_to_ply(tmp_path):
    rng = np.random.default_rng(2)
    xyz = rng.uniform(-5, 5, (257, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (257, 3), dtype=np.uint8)
    path = str(tmp_path / "cloud.ply")
    points_to_ply(xyz, rgb, path)
    got = E.read_ply_points(path)
    assert got.dtype == np.float64 and np.array_equal(got, xyz.astype(np.float64))
    points_to_ply(xyz[:0], rgb[:0], path)
    assert E.read_ply_points(path).shape == (0, 3)


def test_read_ply_ascii_double_and_extra_properties(tmp_path):
    rng = np.random.default_rng(3)
    pts = rng.uniform(-5, 5, (11, 3))
    path = tmp_path / "mesh.ply"
    with open(path, "w") as fh:
        fh.write("ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 11\nproperty uchar red\n"
                 "property double x\nproperty double y\nproperty double z\nelement face 1\n"
                 "property list uchar int vertex_indices\nend_header\n")
        for p in pts:
            fh.write("7 " + " ".join(repr(float(v)) for v in p) + "\n")
        fh.write("3 0 1 2\n")
    assert np.array_equal(E.read_ply_points(str(path)), pts)
    # binary doubles between other properties
    dt = np.dtype([("nx", "<f4"), ("z", "<f8"), ("x", "<f8"), ("flag", "u1"), ("y", "<f8")])
    v = np.zeros(11, dt)
    v["x"], v["y"], v["z"] = pts.T
    with open(path, "wb") as fh:
        fh.write(b"ply\nformat binary_little_endian 1.0\nelement vertex 11\nproperty float nx\nproperty double z\n"
                 b"property double x\nproperty uchar flag\nproperty double y\nend_header\n" + v.tobytes())
    assert np.array_equal(E.read_ply_points(str(path)), pts)
    with open(path, "wb") as fh:
        fh.write(b"ply\nformat binary_big_endian 1.0\nelement vertex 0\nproperty float x\nend_header\n")
    with pytest.raises(ValueError, match="not supported"):
        E.read_ply_points(str(path))
    with open(path, "wb") as fh:
        fh.write(b"ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\n"
                 b"property float z\nend_header\n" + bytes(40))
    with pytest.raises(ValueError, match="truncated"):
        E.read_ply_points(str(path))


def test_load_boxes_pkl_reads_global_save_list(tmp_path):
    rng = np.random.default_rng(4)
    corners = np.stack([cuboid(rng.uniform(-2, 2, 3), rng.uniform(0.4, 1, 3), np.eye(3)) for _ in range(5)])
    corners = corners.astype(np.float32)
    inst = _Inst(corners)
    path = str(tmp_path / "seq_boxes.pkl")
    RS.save_box(RS.global_save_list(inst, ["chair"], "scannet"), path)
    got = E.load_boxes_pkl(path)
    assert got.dtype == np.float64 and np.array_equal(got, corners.astype(np.float64))
    with open(path, "wb") as fh:
        pickle.dump({"boxes": 1}, fh)
    with pytest.raises(ValueError):
        E.load_boxes_pkl(path)


def test_png_size(tmp_path):
    from PIL import Image
    Image.fromarray(np.zeros((48, 64), np.uint16)).save(tmp_path / "0.png")
    assert E.png_size(str(tmp_path / "0.png")) == (48, 64)
    (tmp_path / "bad.png").write_bytes(b"not a png at all, but long enough")
    with pytest.raises(ValueError):
        E.png_size(str(tmp_path / "bad.png"))


# ---- command line ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv", [[], ["filter"], ["score", "only_one.pkl"], ["rank", "a", "b"],
                                  ["filter", "seq", "--dist", "near"]])
def test_cli_usage_errors(argv, capsys):
    with pytest.raises(SystemExit) as e:
        E.main(argv)
    assert e.value.code == 2
    assert "usage" in capsys.readouterr().err


def test_cli_missing_inputs(tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        E.main(["filter", str(tmp_path / "nowhere")])
    assert e.value.code == 2 and "not a directory" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:                                  # an empty sequence directory
        E.main(["filter", str(tmp_path)])
    assert e.value.code == 2 and "mesh.ply is missing" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        E.main(["score", str(tmp_path / "a_boxes.pkl"), str(tmp_path / "gt.npy")])
    assert e.value.code == 2 and "a_boxes.pkl is missing" in capsys.readouterr().err
    (tmp_path / "a_boxes.pkl").write_bytes(b"")
    np.save(tmp_path / "gt.npy", np.zeros((0, 8, 3)))
    with pytest.raises(SystemExit) as e:
        E.main(["score", str(tmp_path / "a_boxes.pkl"), str(tmp_path / "gt.npy"), "--iou", "1.5"])
    assert e.value.code == 2 and "--iou" in capsys.readouterr().err


def test_cli_score_without_overlap_needs_no_device(tmp_path, capsys):
    """an empty ground-truth file is scored on the host: every count is zero"""
    box = cuboid([0, 0, 0], [1, 1, 1], np.eye(3)).astype(np.float32)
    with open(tmp_path / "a_boxes.pkl", "wb") as fh:
        pickle.dump([[(0, box, 1.0)]], fh)
    np.save(tmp_path / "gt.npy", np.zeros((0, 8, 3)))
    assert E.main(["score", str(tmp_path / "a_boxes.pkl"), str(tmp_path / "gt.npy")]) == 0
    out = capsys.readouterr().out
    assert "pred 1  gt 0" in out and "precision 0.0000" in out
    assert os.path.exists(tmp_path / "a_boxes.pkl")
