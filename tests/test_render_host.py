"""The renderer off the GPU: the numpy restatement of its passes (tests/render_util.py) against cases
worked by hand, the camera helpers of boxfusion_amd.render, and the two command lines' arguments."""
import numpy as np
import pytest

from tests import render_util as RU
from tests.sens_util import upright_pose

F = np.float32
H, W = 48, 64
INTR = (F(50.0), F(52.0), F(30.25), F(20.75))          # fx fy cx cy
IDENTITY = RU.camera_rows(np.eye(4)[None])


def _one(xyz, rgb, r=0, near=0.05, far=20.0, layer=1, keys=None):
    keys = RU.new_keys(1, H, W) if keys is None else keys
    RU.draw_points(keys, np.array(xyz, F), np.array(rgb, np.uint8), IDENTITY, INTR, near, far, r, layer)
    return keys


def test_key_round_trip():
    rng = np.random.default_rng(0)
    z = rng.uniform(0.01, 50.0, 200).astype(F)
    rgb = rng.integers(0, 256, (200, 3), dtype=np.uint8)
    for layer in (0, 1):
        key = RU.pack_key(layer, z, rgb)
        assert key.dtype == np.uint64 and (key != RU.EMPTY).all() and (key & np.uint64(0xFF) == 0xFF).all()
        lay, z2, rgb2 = RU.unpack_key(key)
        assert (lay == layer).all() and np.array_equal(z2.view(np.uint32), z.view(np.uint32)) and np.array_equal(rgb2, rgb)
    # the layout, bit by bit: layer 63, bits(1.0f) = 0x3F800000 at 62..32, R G B, 0xFF
    assert int(RU.pack_key(1, F(1.0), [1, 2, 3])) == (1 << 63) | (0x3F800000 << 32) | 0x010203FF
    assert int(RU.pack_key(0, F(1.0), [1, 2, 3])) == (0x3F800000 << 32) | 0x010203FF
    # keys order like (layer, depth, colour)
    assert RU.pack_key(0, F(9.0), [255] * 3) < RU.pack_key(1, F(0.1), [0] * 3)
    assert RU.pack_key(1, F(1.0), [255] * 3) < RU.pack_key(1, F(1.0000001), [0] * 3)


def test_principal_ray_lands_on_the_principal_pixel():
    keys = _one([[0.0, 0.0, 2.5]], [[10, 20, 30]])
    rgb, depth = RU.resolve(keys, (7, 8, 9))
    iy, ix = 21, 30                                    # floor(20.75 + 0.5), floor(30.25 + 0.5)
    assert (keys != RU.EMPTY).sum() == 1 and keys[0, iy, ix] == RU.pack_key(1, F(2.5), [10, 20, 30])
    assert depth[0, iy, ix] == F(2.5) and rgb[0, iy, ix].tolist() == [10, 20, 30]
    assert depth.sum() == F(2.5) and rgb[0, 0, 0].tolist() == [7, 8, 9]
    # u = 50 * 0.1 / 2 + 30.25 = 32.75 -> 33; v = 52 * -0.2 / 2 + 20.75 = 15.55 -> 16; radius 1: nine pixels
    keys = _one([[0.1, -0.2, 2.0]], [[1, 1, 1]], r=1)
    ys, xs = np.nonzero(keys[0] != RU.EMPTY)
    assert sorted(set(ys)) == [15, 16, 17] and sorted(set(xs)) == [32, 33, 34] and len(ys) == 9


def test_nearer_point_wins_and_ties_go_to_the_smaller_colour():
    for order in ([0, 1], [1, 0]):
        pts = np.array([[0.0, 0.0, 3.0], [0.0, 0.0, 2.0]], F)[order]
        col = np.array([[200, 0, 0], [0, 200, 0]], np.uint8)[order]
        rgb, depth = RU.resolve(_one(pts, col))
        assert depth[0, 21, 30] == F(2.0) and rgb[0, 21, 30].tolist() == [0, 200, 0]
        col = np.array([[9, 0, 1], [8, 255, 255]], np.uint8)[order]
        rgb, depth = RU.resolve(_one([[0.0, 0.0, 2.0]] * 2, col))
        assert rgb[0, 21, 30].tolist() == [8, 255, 255]
    # the overlay layer wins over a nearer scene point
    keys = _one([[0.0, 0.0, 1.0]], [[1, 2, 3]])
    rgb, depth = RU.resolve(_one([[0.0, 0.0, 4.0]], [[4, 5, 6]], layer=0, keys=keys))
    assert depth[0, 21, 30] == F(4.0) and rgb[0, 21, 30].tolist() == [4, 5, 6]


def test_rejection_rules_and_the_image_border():
    d = RU.draw_points(RU.new_keys(1, H, W), np.array([[0, 0, -1.0], [0, 0, 0.05], [0, 0, 20.0], [np.nan, 0, 1],
                                                       [0, np.inf, 1], [9.0, 0, 1.0], [0, 0, 1.0]], F),
                       np.zeros((7, 3), np.uint8), IDENTITY, INTR, 0.05, 20.0, 0, 1)
    assert d == dict(pairs=7, nonfinite=2, near=2, far=1, outside=1)
    # u = -1.0 with radius 0 passes the window test (-(r+1) <= u) and rounds to pixel -1: nothing drawn
    x = (F(-1.0) - INTR[2]) / INTR[0]
    assert (_one([[x, 0.0, 1.0]], [[1, 1, 1]]) != RU.EMPTY).sum() == 0
    keys = _one([[x, 0.0, 1.0]], [[1, 1, 1]], r=1)                 # radius 1 reaches column 0
    assert sorted(set(np.nonzero(keys[0] != RU.EMPTY)[1])) == [0]


def test_edge_near_clip_and_sample_cap():
    intr = INTR
    # an edge along the optical axis direction from behind the camera to in front of it: the behind end
    # moves onto the near plane
    s, fate = RU.edge_samples((F(0.1), F(0.0), F(-1.0)), (F(0.1), F(0.0), F(3.0)), intr, H, W, 0.05)
    assert fate == "near_clipped" and s[2].max() <= F(3.0) and s[2].min() >= F(0.05)
    # an edge 1 mm in front of the near plane that spans +-1000 m sideways: millions of pixels before the
    # clip, at most max(W, H) + 1 samples after it
    s, fate = RU.edge_samples((F(-1000.0), F(0.0), F(0.051)), (F(1000.0), F(0.0), F(0.051)), intr, H, W, 0.05)
    assert fate == "drawn" and 2 <= len(s[0]) <= max(W, H) + 1
    assert RU.edge_samples((F(0), F(0), F(-2.0)), (F(1), F(0), F(0.01)), intr, H, W, 0.05) == (None, "behind")
    assert RU.edge_samples((F(50), F(0), F(1.0)), (F(60), F(1), F(1.0)), intr, H, W, 0.05) == (None, "offscreen")
    # a horizontal edge at depth 2 from u = 10.25 to u = 40.25: n = 30, every sample at Z = 2 on row 21
    keys = RU.new_keys(1, H, W)
    a, b = ((F(10.25) - intr[2]) / intr[0] * F(2.0), F(0.0), F(2.0)), ((F(40.25) - intr[2]) / intr[0] * F(2.0), F(0.0), F(2.0))
    s, _ = RU.edge_samples(a, b, intr, H, W, 0.05)
    assert len(s[0]) == 31
    RU.splat(keys[0], np.zeros((H, W), np.int64), *s[:2], 0, RU.pack_key(1, s[2], np.zeros((31, 3), np.uint8)))
    ys, xs = np.nonzero(keys[0] != RU.EMPTY)
    assert set(ys) == {21} and xs.min() == 10 and xs.max() == 40 and len(xs) == 31


def test_resolve_backgrounds():
    keys = _one([[0.0, 0.0, 2.0]], [[1, 2, 3]])
    img = np.random.default_rng(1).integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    rgb, depth = RU.resolve(keys, img)
    want = img.copy()
    want[0, 21, 30] = [1, 2, 3]
    assert np.array_equal(rgb, want) and (depth != 0).sum() == 1


# ---- cameras -------------------------------------------------------------------------------------------
BOXES = [((-1.0, -2.0, 0.0), (3.0, 2.5, 2.4)), ((0.0, 0.0, 0.0), (0.2, 0.1, 0.3)), ((-8.0, 1.0, -1.0), (9.0, 2.0, 6.0))]


def _project(pose, K, pts):
    inv = np.linalg.inv(np.asarray(pose, np.float64))
    c = np.asarray(pts, np.float64) @ inv[:3, :3].T + inv[:3, 3]
    return np.stack([K[0, 0] * c[:, 0] / c[:, 2] + K[0, 2], K[1, 1] * c[:, 1] / c[:, 2] + K[1, 2]], 1), c[:, 2]


@pytest.mark.parametrize("lo,hi", BOXES)
@pytest.mark.parametrize("size", [(480, 640), (37, 53)])
def test_orbit_and_topdown_cameras(lo, hi, size):
    from boxfusion_amd import render as R
    from boxfusion_amd.synthetic import SCANNET_K
    h, w = size
    K = SCANNET_K.astype(np.float64) * (w / 640.0)
    K[2, 2] = 1.0
    lo, hi = np.array(lo), np.array(hi)
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    poses = list(R.orbit_poses(lo, hi, 5, elevation_deg=35.0, K3=K, H=h, W=w)) + [R.topdown_pose(lo, hi, K, h, w)]
    assert len(poses) == 6
    for i, P in enumerate(poses):
        assert P.shape == (4, 4) and P.dtype == np.float32 and P[3].tolist() == [0, 0, 0, 1]
        rot = P[:3, :3].astype(np.float64)
        np.testing.assert_allclose(rot @ rot.T, np.eye(3), atol=1e-6)
        assert abs(np.linalg.det(rot) - 1.0) < 1e-6
        uv, z = _project(P, K, [(lo + hi) / 2])
        assert abs(uv[0, 0] - (w - 1) / 2) <= 1.0 and abs(uv[0, 1] - (h - 1) / 2) <= 1.0 and z[0] > 0
        uv, z = _project(P, K, corners)
        assert (z > 0).all() and (uv[:, 0] >= -0.5).all() and (uv[:, 0] <= w - 0.5).all()
        assert (uv[:, 1] >= -0.5).all() and (uv[:, 1] <= h - 0.5).all()
        if i < 5:       # camera y points down the world's z, and the camera is above the centre
            assert rot[2, 1] < 0 and P[2, 3] > (lo[2] + hi[2]) / 2
    top = poses[-1][:3, :3]
    np.testing.assert_array_equal(top, np.diag([1.0, -1.0, -1.0]).astype(np.float32))
    # the helpers' convention is the synthetic scenes' and sens_util's: camera y down the world z
    assert upright_pose()[2, 1] < 0
    assert R.orbit_poses(lo, hi, 0).shape == (0, 4, 4)


def test_camera_rows_is_the_restatement_s():
    from boxfusion_amd import render as R
    import torch
    poses = np.stack([upright_pose((0.1, 0.2, 1.3)), np.eye(4, dtype=np.float32)])
    np.testing.assert_array_equal(R.camera_rows(poses), RU.camera_rows(poses))
    np.testing.assert_array_equal(R.camera_rows(torch.from_numpy(poses)), RU.camera_rows(poses))
    assert R.camera_rows(poses[0]).shape == (1, 12)
    with pytest.raises(ValueError):
        R.camera_rows(np.eye(3))


def test_box_colors_are_the_ply_writer_s():
    from boxfusion_amd import render as R
    from boxfusion_amd.visualize import random_color_v2
    c = R.box_colors(5)
    assert c.dtype == np.uint8 and c.shape == (5, 3)
    np.testing.assert_array_equal(c[3], np.rint(random_color_v2(3 / 5) * 255.0).astype(np.uint8))


# ---- command lines -------------------------------------------------------------------------------------
def test_render_cli_arguments(tmp_path):
    from boxfusion_amd import render as R
    p = R.parser()
    a = p.parse_args(["cloud.ply", "out"])
    assert (a.cloud, a.out_dir, a.boxes, a.views, a.size, a.radius) == ("cloud.ply", "out", None, 8, [480, 640], 1)
    a = p.parse_args(["c.ply", "o", "--boxes", "s_boxes.pkl", "--views", "3", "--size", "37", "53", "--radius", "0"])
    assert (a.boxes, a.views, a.size, a.radius) == ("s_boxes.pkl", 3, [37, 53], 0)
    R.check_render_arguments(p, a)
    for bad in (["--radius", "5"], ["--views", "-1"], ["--size", "0", "10"]):
        with pytest.raises(SystemExit):
            R.check_render_arguments(p, p.parse_args(["c.ply", "o"] + bad))
    with pytest.raises(SystemExit):
        p.parse_args(["c.ply"])


def test_sens_render_cli_arguments():
    from boxfusion_amd import sens as S
    p = S.parser()
    a = p.parse_args(["render", "scene.sens", "out"])
    assert (a.cmd, a.sens, a.out, a.boxes, a.views, a.size, a.radius) == ("render", "scene.sens", "out", None, 8, [480, 640], 1)
    assert (a.voxel, a.start, a.stop, a.step, a.max_depth) == (0.02, 0, None, 1, 10.0)
    a = p.parse_args(["render", "s.sens", "o", "--voxel", "0.05", "--start", "2", "--stop", "9", "--step", "3",
                      "--max-depth", "4", "--views", "2", "--size", "48", "64", "--radius", "2", "--boxes", "b.pkl"])
    assert (a.voxel, a.start, a.stop, a.step, a.max_depth, a.views, a.size, a.radius, a.boxes) == \
        (0.05, 2, 9, 3, 4.0, 2, [48, 64], 2, "b.pkl")
    c = p.parse_args(["cloud", "s.sens", "o.ply"])                 # the cloud subcommand keeps its options
    assert (c.voxel, c.start, c.stop, c.step, c.max_depth) == (0.02, 0, None, 1, 10.0) and not hasattr(c, "views")
    with pytest.raises(SystemExit):
        S.main(["render", "s.sens", "o", "--radius", "9"])


def test_boxes_argument_reads_the_global_box_list(tmp_path):
    from boxfusion_amd import render as R
    from boxfusion_amd.results import save_box
    rng = np.random.default_rng(0)
    boxes = rng.normal(size=(3, 8, 3))
    save_box([[(0, b, 1.0) for b in boxes]], str(tmp_path / "s_boxes.pkl"))
    got = R.load_boxes_argument(str(tmp_path / "s_boxes.pkl"))
    assert got.dtype == np.float32 and np.array_equal(got, boxes.astype(np.float32))
    assert R.load_boxes_argument(None) is None
