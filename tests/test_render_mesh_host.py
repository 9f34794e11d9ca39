"""The triangle pass's numpy restatement (tests/tri_util.py) has the properties the renderer promises
(DESIGN.md §4 "Renderer", *Triangles*), shown on the CPU so that the bit-for-bit GPU comparison
(tests/test_gpu_render_mesh.py) cannot hide behind it: every pixel inside a closed outline is covered
exactly once, also when vertices and edges pass exactly through pixel centres, and a wall fused from depth
frames renders back into its cameras within half a voxel of the depth that went in."""
import numpy as np
import pytest

from tests import render_util as RU
from tests import tri_util as T

F = np.float32


def outline_mask(xyz, ny, nx, intr, H, W, closed=False):
    """the pixel centres strictly inside the grid's border, from the snapped border vertices alone"""
    border = T.grid_outline(ny, nx)
    *_, xs, ys = T.snap(T.IDENTITY_ROWS[0], xyz[border], intr)
    return T.strictly_inside(xs, ys, H, W, closed)


def draw(xyz, rgb, faces, rows, intr, H, W, **kw):
    keys = RU.new_keys(len(rows), H, W)
    args = dict(near=0.05, far=20.0, cull=0, shade=0, layer=1)
    args.update(kw)
    count, fates = T.draw_triangles(keys, xyz, rgb, faces, rows, intr, **args)
    return keys, count, fates


def test_strictly_inside_by_hand():
    """a 4 x 3 px square with corners on pixel centres: the two inner centres, not the eight on the outline"""
    m = T.strictly_inside([256, 4 * 256, 4 * 256, 256], [256, 256, 3 * 256, 3 * 256], 5, 6)
    want = np.zeros((5, 6), bool)
    want[2, 2:4] = True
    np.testing.assert_array_equal(m, want)


@pytest.mark.parametrize("size", [(48, 64), (37, 53)])
def test_exactly_once(size):
    H, W = size
    intr = (0.8 * W, 0.78 * W, W / 2 - 0.3, H / 2 + 0.2)
    xyz, rgb, faces = T.jittered_grid(H, W, intr)
    assert len(faces) == 330
    inside = outline_mask(xyz, 12, 16, intr, H, W)
    assert inside.mean() > 0.6
    keys, count, fates = draw(xyz, rgb, faces, T.IDENTITY_ROWS, intr, H, W)
    assert fates["drawn"] == 330
    assert (count[0][inside] == 1).all() and count.max() == 1
    assert (count[0][~outline_mask(xyz, 12, 16, intr, H, W, closed=True)] == 0).all()
    # any order of the faces and of each face's vertices: the same coverage (which vertex comes first decides
    # the order of the f64 sums, so depth and colour may move by a rounding)
    rng = np.random.default_rng(0)
    shuffled = faces[rng.permutation(len(faces))]
    shuffled = np.stack([f[rng.permutation(3)] for f in shuffled])
    assert (shuffled != faces).any()
    keys2, count2, _ = draw(xyz, rgb, shuffled, T.IDENTITY_ROWS, intr, H, W)
    np.testing.assert_array_equal(count2, count)
    np.testing.assert_array_equal(keys2 == RU.EMPTY, keys == RU.EMPTY)
    # with cull the flipped faces are gone
    _, count3, fates3 = draw(xyz, rgb, shuffled, T.IDENTITY_ROWS, intr, H, W, cull=1)
    assert 0 < fates3["culled"] < 330 and count3.max() == 1 and (count3[0][inside] == 0).any()


def test_ties():
    H, W = 37, 53
    xyz, rgb, faces = T.tie_grid()
    *_, u, v, xs, ys = T.snap(T.IDENTITY_ROWS[0], xyz, T.TIE_INTR)
    assert (xs % 256 == 0).all() and (ys % 256 == 0).all()                     # every vertex on a pixel centre
    inside = outline_mask(xyz, 8, 10, T.TIE_INTR, H, W)
    keys, count, fates = draw(xyz, rgb, faces, T.IDENTITY_ROWS, T.TIE_INTR, H, W)
    assert fates["drawn"] == len(faces) and fates["ties"] >= 20
    assert (count[0][inside] == 1).all() and count.max() == 1
    # the outline: its top and left edges belong to the mesh, its bottom and right edges do not
    x0, x1, y0, y1 = xs.min() // 256, xs.max() // 256, ys.min() // 256, ys.max() // 256
    assert (count[0, y0, x0:x1] == 1).all() and (count[0, y0:y1, x0] == 1).all()
    assert (count[0, y1, x0:x1 + 1] == 0).all() and (count[0, y0:y1 + 1, x1] == 0).all()


def test_uniform_colour_is_exact_and_shade_darkens():
    H, W = 37, 53
    xyz, _, faces = T.tie_grid()
    rgb = np.tile(np.array([[201, 7, 255]], np.uint8), (len(xyz), 1))
    keys, count, _ = draw(xyz, rgb, faces, T.IDENTITY_ROWS, T.TIE_INTR, H, W)
    got, depth = RU.resolve(keys)
    assert (got[count > 0] == [201, 7, 255]).all() and (depth[count > 0] == 1).all()
    shaded, _, _ = draw(xyz, rgb, faces, T.IDENTITY_ROWS, T.TIE_INTR, H, W, shade=1)
    s, _ = RU.resolve(shaded)
    on = count > 0
    assert (s[on] <= got[on]).all() and (s[on][:, 2] >= 0.3 * 255 - 1).all() and (s[on] < got[on]).any()
    # mid-grey without colours
    grey, _, _ = draw(xyz, None, faces, T.IDENTITY_ROWS, T.TIE_INTR, H, W)
    assert (RU.resolve(grey)[0][on] == T.GREY).all()


@pytest.mark.parametrize("case", T.WALL_CASES)
def test_fused_wall(case):
    voxel, H, W, focal = case
    w = T.wall_scene(*case)
    xyz, rgb, faces = w["mesh"]
    K = w["K"]
    keys, count, fates = draw(xyz, rgb, faces, RU.camera_rows(w["poses"]), (K[0, 0], K[1, 1], K[0, 2], K[1, 2]), H, W, shade=1)
    _, depth = RU.resolve(keys)
    inn = T.inner(H, W)
    worst = 0.0
    for i in range(3):
        assert (count[i][inn] == 1).all()
        worst = max(worst, float(np.abs(depth[i] - w["depths"][i])[inn].max()) / voxel)
    print(f"fused wall {case}: worst depth error {worst:.3f} voxel")
    assert worst <= 0.5
    # the faces show their front to the cameras that observed them: nothing is culled from there but slivers
    _, culled, fc = draw(xyz, rgb, faces, RU.camera_rows(w["poses"]), (K[0, 0], K[1, 1], K[0, 2], K[1, 2]), H, W, cull=1)
    assert fc["culled"] <= 0.001 * fc["pairs"] and (culled[:, inn] == 1).mean() > 0.999


def test_drop_rules_by_hand():
    """one triangle per rule, identity camera"""
    intr, H, W = T.TIE_INTR, 37, 53
    tri = np.array([[0, 0, 1], [0, 0.25, 1], [0.25, 0, 1]], F)                 # u 20..28, v 14..22, area2 < 0: the front
    one = lambda xyz, faces=((0, 1, 2),), **kw: draw(np.asarray(xyz, F), None, np.array(faces), T.IDENTITY_ROWS, intr, H, W, **kw)
    keys, count, f = one(tri, cull=1)
    assert f["drawn"] == 1 and count.sum() == 36                               # (8 + 7 + ... + 1): the hypotenuse's centres are not its
    assert one(tri[[0, 2, 1]], cull=1)[2]["culled"] == 1 and one(tri[[0, 2, 1]])[1].sum() == 36
    assert one(tri, faces=((0, 1, 3),))[2]["bounds"] == 1 and one(tri, faces=((-1, 1, 2),))[2]["bounds"] == 1
    for bad in (np.nan, np.inf):
        t = tri.copy()
        t[1, 0] = bad
        assert one(t)[2]["range"] == 1
    near = tri.copy()
    near[2, 2] = 0.04
    assert one(near)[2]["range"] == 1 and one(tri, far=1.0)[2]["range"] == 1
    wide = tri.copy()
    wide[1, 0] = 2.0 ** 17                                                     # u = 2^22 + 20
    assert one(wide)[2]["bounds"] == 1
    assert one(tri[[0, 1, 1]])[2]["culled"] == 1                               # zero area
    assert one(tri * F(1e-4) + F([0, 0, 1]) * F(1 - 1e-4))[2]["culled"] == 1   # snaps to zero area


def test_pipeline_hands_the_mesh_to_finish_only_when_given_both():
    """Pipeline.run(snapshots=..., mesh=...) calls finish(cloud, boxes, mesh=mesh); without a mesh the call is the
    one it always was (stand-ins for both stages: no model, no device)"""
    import torch
    from boxfusion_amd.pipeline import Pipeline

    class Detect:
        B, Kd3 = 1, np.eye(3, dtype=F)

        def preprocess_frames(self, depth, poses):
            return None

        def __call__(self, rgb, depth, poses):
            return [None]

    class Fusion:
        all_pred_box = None

        def keyframe(self, i, pose, pred):
            pass

        def finish(self, i, pose, flag):
            pass

    class Snapshots:
        def __init__(self):
            self.shots, self.finished = [], []

        def snapshot(self, count, pose, rgb, boxes):
            self.shots.append(count)

        def finish(self, *args, **kwargs):
            self.finished.append((args, kwargs))

    class Volume:
        frames = 0

        def integrate(self, depth, K, poses, rgb):
            self.frames += len(poses)

    def frames(ids):
        return torch.zeros((len(ids), 4, 6, 3), dtype=torch.uint8), torch.ones((len(ids), 4, 6)), np.stack([np.eye(4, dtype=F)] * len(ids))

    snaps, vol = Snapshots(), Volume()
    Pipeline(Detect(), Fusion(), 2).run(frames, 4, snapshots=snaps)
    Pipeline(Detect(), Fusion(), 2).run(frames, 4, snapshots=snaps, mesh=vol)
    Pipeline(Detect(), Fusion(), 2).run(frames, 4, mesh=vol)
    assert snaps.finished == [((None, None), {}), ((None, None), {"mesh": vol})]
    assert snaps.shots == [0, 2, 3, 0, 2, 3] and vol.frames == 4
