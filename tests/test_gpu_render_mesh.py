"""The renderer's triangle pass on the GPU (bf_render_triangles through boxfusion_amd.render) against its
numpy restatement (tests/tri_util.py), bit for bit: np.testing.assert_array_equal on the keys and on the
resolved rgb and depth bits.

As in test_gpu_render.py, before a comparison the restatement's own output must show that the picture is
not vacuous: at least 20 % of the pixels covered, at least 5 % of the (triangle, view) pairs dropped by
every rule the case claims, a pixel offered two or more triangles.  tests/test_render_mesh_host.py shows on
the CPU that the restatement covers closed surfaces exactly once and renders a fused wall back into its
cameras; here the same scenes run on the device."""
import ctypes

import numpy as np
import pytest
import torch
from PIL import Image

from tests import render_util as RU
from tests import sens_util as U
from tests import tri_util as T

pytestmark = pytest.mark.gpu

DEV = "cuda"
F = np.float32
SIZES = [(48, 64), (37, 53)]
NEAR, FAR = 0.5, 6.0


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from boxfusion_amd import _lib
    _lib.lib()
    return _lib


# ---- the cameras of test_gpu_render.py -----------------------------------------------------------------
def pinhole(H, W):
    return np.array([[0.8 * W, 0, W / 2 - 0.3], [0, 0.78 * W, H / 2 + 0.2], [0, 0, 1]], np.float32)


def intr_of(K):
    return (K[0, 0], K[1, 1], K[0, 2], K[1, 2])


def cameras(V):
    base = U.upright_pose((0.3, -0.2, 1.1)).astype(np.float64)
    out = [base]
    for a, t in ((0.25, (0.4, 0.0, -0.3)), (-0.3, (-0.5, 0.1, 0.2)))[:V - 1]:
        M = np.eye(4)
        M[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        M[:3, 3] = t
        out.append(base @ M)
    return np.stack(out).astype(np.float32)


def to_world(pc):
    P = cameras(1)[0].astype(np.float64)
    return (np.asarray(pc, np.float64) @ P[:3, :3].T + P[:3, 3]).astype(np.float32)


# ---- scenes --------------------------------------------------------------------------------------------
N_BAD_INDEX = 120


def soup(m=2000, seed=21):
    """m triangles around camera 0: centres in the box of test_gpu_render.random_points (a quarter behind the
    camera or nearer than NEAR, a fifth beyond FAR), sizes log-uniform from 2 mm (sub-pixel) to 6 m (wider
    than the view), 5 % of the vertices NaN / inf, 4 % of the triangles with a vertex a thousand kilometres
    to the side (the 2^22 px guard band), 6 % of the faces with an index of -1 or n, 3 % degenerate"""
    rng = np.random.default_rng(seed)
    centre = rng.uniform([-3, -2.5, -2], [3, 2.5, 8], (m, 3))
    size = np.exp(rng.uniform(np.log(0.002), np.log(6.0), m))
    pc = centre[:, None, :] + rng.uniform(-0.5, 0.5, (m, 3, 3)) * size[:, None, None]
    aside = rng.choice(m, m // 25, replace=False)
    pc[aside, 0] = np.stack([rng.choice([-1e6, 1e6], len(aside)), rng.uniform(-1, 1, len(aside)), rng.uniform(1, 5, len(aside))], 1)
    xyz = to_world(pc.reshape(-1, 3))
    n = len(xyz)
    bad = rng.choice(n, n // 20, replace=False)
    xyz[bad, rng.integers(0, 3, len(bad))] = rng.choice([np.nan, np.inf, -np.inf], len(bad))
    faces = np.arange(n, dtype=np.int32).reshape(m, 3).copy()
    wrong = rng.choice(m, N_BAD_INDEX * m // 2000, replace=False)
    faces[wrong, rng.integers(0, 3, len(wrong))] = rng.choice([-1, n], len(wrong))
    flat = rng.choice(m, 3 * m // 100, replace=False)
    faces[flat, 1] = faces[flat, 0]
    return xyz, rng.integers(0, 256, (n, 3), dtype=np.uint8), faces


def visible_triangles(m, seed):
    """m triangles a few pixels to half the image across, all inside every rule"""
    rng = np.random.default_rng(seed)
    centre = rng.uniform([-0.6, -0.4, 1.0], [0.6, 0.4, 3.0], (m, 3))
    pc = centre[:, None, :] + rng.uniform(-0.5, 0.5, (m, 3, 3)) * rng.uniform(0.02, 0.6, (m, 1, 1))
    return to_world(pc.reshape(-1, 3)), rng.integers(0, 256, (3 * m, 3), dtype=np.uint8), np.arange(3 * m, dtype=np.int32).reshape(m, 3)


def mesh_call(xyz, rgb, faces, near=NEAR, far=FAR, cull=False, shade=True, overlay=False, coop=None):
    return ("mesh", dict(xyz=xyz, rgb=rgb, faces=np.asarray(faces), near=near, far=far, cull=cull, shade=shade, overlay=overlay,
                         coop=coop))


def points_call(xyz, rgb, r=0, near=0.05, far=20.0, overlay=False):
    return ("points", dict(xyz=xyz, rgb=rgb, r=r, near=near, far=far, overlay=overlay))


def boxes_call(corners, colors, hw=0, xray=False, near=0.05):
    return ("boxes", dict(corners=np.asarray(corners, np.float32), colors=np.asarray(colors, np.uint8), hw=hw, xray=xray, near=near))


def box(centre, dims):
    """corners [8,3], axis-aligned, in the project's v0..v7 order"""
    sx = np.array([-1, 1, 1, -1, -1, 1, 1, -1.0])
    sy = np.array([-1, -1, 1, 1, -1, -1, 1, 1.0])
    sz = np.array([-1, -1, -1, -1, 1, 1, 1, 1.0])
    return np.stack([sx, sy, sz], 1) * (np.asarray(dims, np.float64) / 2) + np.asarray(centre, np.float64)


# ---- both sides ----------------------------------------------------------------------------------------
def reference(H, W, K, poses, calls, start=None):
    """the calls through the restatements; start: a reference to continue from (it is copied)"""
    rows, intr, V = RU.camera_rows(poses), intr_of(K), len(poses)
    if start is None:
        ref = dict(keys=RU.new_keys(V, H, W), count=np.zeros((V, H, W), np.int64), fates={}, tri_count=np.zeros((V, H, W), np.int64))
    else:
        ref = dict(keys=start["keys"].copy(), count=start["count"].copy(), fates=dict(start["fates"]),
                   tri_count=start["tri_count"].copy())
    for kind, kw in calls:
        if kind == "mesh":
            own = np.zeros((V, H, W), np.int64)
            T.draw_triangles(ref["keys"], kw["xyz"], kw["rgb"], kw["faces"], rows, intr, kw["near"], kw["far"], int(kw["cull"]),
                             int(kw["shade"]), 0 if kw["overlay"] else 1, count=own, fates=ref["fates"])
            ref["count"] += own
            ref["tri_count"] += own
        elif kind == "points":
            RU.draw_points(ref["keys"], kw["xyz"], kw["rgb"], rows, intr, kw["near"], kw["far"], kw["r"], 0 if kw["overlay"] else 1,
                           count=ref["count"])
        else:
            RU.draw_edges(ref["keys"], kw["corners"], kw["colors"], rows, intr, kw["near"], kw["hw"], 0 if kw["xray"] else 1,
                          count=ref["count"])
    return ref


def gpu_draw(H, W, K, poses, calls, stats=None):
    from boxfusion_amd.render import Renderer
    ren = Renderer(H, W, K, views=len(poses), device=DEV)
    for kind, kw in calls:
        if kind == "mesh":
            ren.draw_mesh(kw["xyz"], kw["faces"], kw["rgb"], poses, shade=kw["shade"], cull=kw["cull"], near=kw["near"], far=kw["far"],
                          overlay=kw["overlay"], stats=stats, coop_pixels=kw["coop"])
        elif kind == "points":
            ren.draw_points(kw["xyz"], kw["rgb"], poses, radius=kw["r"], near=kw["near"], far=kw["far"], overlay=kw["overlay"])
        else:
            ren.draw_boxes(kw["corners"], kw["colors"], poses, half_width=kw["hw"], xray=kw["xray"], near=kw["near"])
    return ren


def gpu_keys(ren):
    return ren.keys.cpu().numpy().view(np.uint64)


def compare(ren, ref, background=(3, 2, 1)):
    np.testing.assert_array_equal(gpu_keys(ren), ref["keys"])
    rgb, depth = ren.resolve(background)
    want_rgb, want_depth = RU.resolve(ref["keys"], background)
    np.testing.assert_array_equal(rgb.cpu().numpy(), want_rgb)
    np.testing.assert_array_equal(depth.cpu().numpy().view(np.int32), want_depth.view(np.int32))
    return rgb, depth


def check_stats(stats, ref):
    """the kernel's counters against the restatement's: equal, but for the atomics issued, which the early-out
    only bounds: every pixel that shows a triangle took at least one, no covered pixel more than one"""
    got = [int(a) for a in stats.cpu()]
    want = T.stats_of(ref["fates"], ref["tri_count"])
    assert got[:5] == want, (got, want)
    assert sum(want[:4]) == ref["fates"]["pairs"]
    assert got[5] <= got[4]


_SOUP = {}


def soup_reference(H, W, V, cull, shade):
    """the 2000-triangle soup every soup picture starts from (computed once per case, never changed)"""
    key = (H, W, V, cull, shade)
    if key not in _SOUP:
        call = mesh_call(*soup(), cull=cull, shade=shade)
        ref = reference(H, W, pinhole(H, W), cameras(V), [call])
        f, pairs = ref["fates"], ref["fates"]["pairs"]
        assert pairs == 2000 * V
        for rule in ("range", "bounds") + (("culled",) if cull else ()):
            assert f[rule] >= 0.05 * pairs, (rule, f)
        assert f["bounds"] > N_BAD_INDEX * V                                  # the guard band took some too
        assert f["drawn"] >= 0.1 * pairs
        assert (ref["keys"] != RU.EMPTY).mean() >= 0.2 and ref["tri_count"].max() >= 2
        _SOUP[key] = (call, ref)
    return _SOUP[key]


# ---- the soup ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cull,shade", [(False, True), (True, False)])
@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 2000])
def test_triangle_soup(L, size, V, m, cull, shade):
    """m = 2000: the soup alone; smaller m: m visible triangles drawn by a second call over it (m = 0: a valid
    call that launches nothing)"""
    H, W = size
    call, ref = soup_reference(H, W, V, cull, shade)
    calls = [call]
    if m != 2000:
        calls.append(mesh_call(*visible_triangles(m, 200 + m), near=0.05, far=20.0, cull=cull, shade=shade))
        ref = reference(H, W, pinhole(H, W), cameras(V), calls[1:], start=ref)
    stats = torch.zeros(6, dtype=torch.int64, device=DEV)
    ren = gpu_draw(H, W, pinhole(H, W), cameras(V), calls, stats=stats)
    compare(ren, ref)
    check_stats(stats, ref)


@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("size", SIZES)
def test_one_image_every_route(L, size, V):
    """the cooperative route for every triangle, the default split, the own-lane route for every triangle,
    another order of the faces and two launches: one image"""
    H, W = size
    call, ref = soup_reference(H, W, V, False, True)
    xyz, rgb, faces = soup()
    K, poses = pinhole(H, W), cameras(V)
    with np.errstate(all="ignore"):
        big = T.setup(RU.camera_rows(poses)[0], xyz, faces.astype(np.int64), F(NEAR), F(FAR), intr_of(K), 0)
    assert (big["fate"] == 0).sum() > 100                                       # both routes have work at the default
    perm = np.random.default_rng(1).permutation(len(faces))
    routes = dict(coop=[mesh_call(xyz, rgb, faces, coop=0)], default=[call], own=[mesh_call(xyz, rgb, faces, coop=2 ** 30)],
                  tiny_threshold=[mesh_call(xyz, rgb, faces, coop=9)], permuted=[mesh_call(xyz, rgb, faces[perm])],
                  halves=[mesh_call(xyz, rgb, faces[:777]), mesh_call(xyz, rgb, faces[777:], coop=0)])
    for name, calls in routes.items():
        np.testing.assert_array_equal(gpu_keys(gpu_draw(H, W, K, poses, calls)), ref["keys"], err_msg=name)


def test_block_assignment(L):
    """a launch of fewer blocks than the chip has CUs deals consecutive triangles to different waves, a larger one
    keeps them together: 32 views of 8 blocks are the larger kind, and each is the one-view picture"""
    H, W = SIZES[1]
    call, ref = soup_reference(H, W, 1, False, True)
    ren = gpu_draw(H, W, pinhole(H, W), np.repeat(cameras(1), 32, 0), [call])
    keys = gpu_keys(ren)
    for v in range(32):
        np.testing.assert_array_equal(keys[v], ref["keys"][0])


# ---- closed surfaces -----------------------------------------------------------------------------------
@pytest.mark.parametrize("coop", [0, None, 2 ** 30])
@pytest.mark.parametrize("size", SIZES)
def test_exactly_once_grid(L, size, coop):
    H, W = size
    K = pinhole(H, W)
    xyz, rgb, faces = T.jittered_grid(H, W, intr_of(K))
    pose = np.eye(4, dtype=np.float32)[None]
    calls = [mesh_call(xyz, rgb, faces, near=0.05, far=20.0, coop=coop)]
    ref = reference(H, W, K, pose, calls)
    assert ref["fates"]["drawn"] == 330 and ref["tri_count"].max() == 1 and (ref["tri_count"] == 1).mean() > 0.6
    stats = torch.zeros(6, dtype=torch.int64, device=DEV)
    ren = gpu_draw(H, W, K, pose, calls, stats=stats)
    compare(ren, ref)
    check_stats(stats, ref)
    # every pixel is offered at most one triangle, so nothing is early-outed: one pixel, one atomic
    assert int(stats[4]) == int(stats[5]) == int((gpu_keys(ren) != RU.EMPTY).sum())


@pytest.mark.parametrize("coop", [0, None, 2 ** 30])
def test_ties_grid(L, coop):
    H, W = 37, 53
    K = np.array([[32, 0, T.TIE_INTR[2]], [0, 32, T.TIE_INTR[3]], [0, 0, 1]], np.float32)
    xyz, rgb, faces = T.tie_grid()
    pose = np.eye(4, dtype=np.float32)[None]
    calls = [mesh_call(xyz, rgb, faces, near=0.05, far=20.0, coop=coop)]
    ref = reference(H, W, K, pose, calls)
    assert ref["fates"]["ties"] >= 20 and ref["tri_count"].max() == 1
    stats = torch.zeros(6, dtype=torch.int64, device=DEV)
    ren = gpu_draw(H, W, K, pose, calls, stats=stats)
    compare(ren, ref)
    check_stats(stats, ref)
    assert int(stats[4]) == int((gpu_keys(ren) != RU.EMPTY).sum())


# ---- the fused wall ------------------------------------------------------------------------------------
WALL = T.WALL_CASES[0]


def behind_the_wall():
    return T.MR.look_at((0.0, 0.0, -2.7), (0.0, 0.01, -1.2), up=(0.0, 1.0, 0.0))[None]


def test_cull_and_shade(L):
    voxel, H, W, focal = WALL
    w = T.wall_scene(*WALL)
    xyz, rgb, faces = w["mesh"]
    K, poses = w["K"], w["poses"]
    kw = dict(near=0.05, far=20.0)
    front = reference(H, W, K, poses, [mesh_call(xyz, rgb, faces, cull=False, **kw)])
    culled = reference(H, W, K, poses, [mesh_call(xyz, rgb, faces, cull=True, **kw)])
    inn = T.inner(H, W)
    assert (front["tri_count"][:, inn] == 1).all()
    np.testing.assert_array_equal(culled["keys"], front["keys"])               # seen from the observing side: nothing to cull
    compare(gpu_draw(H, W, K, poses, [mesh_call(xyz, rgb, faces, cull=True, **kw)]), culled)
    compare(gpu_draw(H, W, K, poses, [mesh_call(xyz, rgb, faces, cull=False, **kw)]), front)
    # from behind: covered without cull, empty with it, every pair counted as culled
    back = behind_the_wall()
    ref_back = reference(H, W, K, back, [mesh_call(xyz, rgb, faces, cull=False, **kw)])
    assert (ref_back["keys"] != RU.EMPTY).mean() > 0.5 and ref_back["fates"]["drawn"] + ref_back["fates"]["culled"] == len(faces)
    compare(gpu_draw(H, W, K, back, [mesh_call(xyz, rgb, faces, cull=False, **kw)]), ref_back)
    stats = torch.zeros(6, dtype=torch.int64, device=DEV)
    ren = gpu_draw(H, W, K, back, [mesh_call(xyz, rgb, faces, cull=True, **kw)], stats=stats)
    assert (gpu_keys(ren) == RU.EMPTY).all()
    assert [int(a) for a in stats.cpu()] == [0, 0, 0, len(faces), 0, 0]
    # one colour, no shading: exactly that colour; shaded: the restatement's bits, darker and not flat
    one = np.tile(np.array([[201, 7, 255]], np.uint8), (len(xyz), 1))
    flat_ref = reference(H, W, K, poses, [mesh_call(xyz, one, faces, shade=False, **kw)])
    rgb_flat, _ = compare(gpu_draw(H, W, K, poses, [mesh_call(xyz, one, faces, shade=False, **kw)]), flat_ref)
    on = torch.from_numpy(flat_ref["keys"] != RU.EMPTY)
    assert (rgb_flat.cpu()[on] == torch.tensor([201, 7, 255], dtype=torch.uint8)).all()
    lit_ref = reference(H, W, K, poses, [mesh_call(xyz, one, faces, shade=True, **kw)])
    rgb_lit, _ = compare(gpu_draw(H, W, K, poses, [mesh_call(xyz, one, faces, shade=True, **kw)]), lit_ref)
    lit = rgb_lit.cpu()[on]
    assert (lit[:, 2] < 255).any() and (lit[:, 2] >= 76).all() and len(torch.unique(lit[:, 2])) > 3
    # no colours: mid-grey
    from boxfusion_amd.render import Renderer
    ren = Renderer(H, W, K, views=3, device=DEV)
    ren.draw_mesh(torch.from_numpy(xyz).to(DEV), torch.from_numpy(faces).to(DEV).long(), None, poses, shade=False)
    grey_ref = reference(H, W, K, poses, [mesh_call(xyz, None, faces, shade=False, **kw)])
    rgb_grey, _ = compare(ren, grey_ref)
    assert (rgb_grey.cpu()[on] == 128).all()


def test_mixed_picture(L):
    """mesh + points + box edges + an x-ray box in two call orders; a box behind the wall is hidden by the mesh
    and shows through the same wall drawn as points"""
    voxel, H, W, focal = WALL
    w = T.wall_scene(*WALL)
    xyz, rgb, faces = w["mesh"]
    K, poses = w["K"], w["poses"]
    hidden_box = boxes_call(box((0.0, 0.0, -1.9), (0.6, 0.5, 0.4))[None], [[255, 0, 0]], hw=0)
    xray_box = boxes_call(box((0.2, 0.1, -2.0), (0.5, 0.5, 0.5))[None], [[0, 255, 0]], hw=1, xray=True)
    rng = np.random.default_rng(6)                                             # a cloud between the cameras and the wall
    front_pts = points_call(rng.uniform([-0.5, -0.4, -1.0], [0.5, 0.4, -0.3], (300, 3)).astype(F),
                            rng.integers(0, 256, (300, 3), dtype=np.uint8), r=1)
    mesh = mesh_call(xyz, rgb, faces, near=0.05, far=20.0)
    calls = [mesh, front_pts, hidden_box, xray_box]
    ref = reference(H, W, K, poses, calls)
    inn = T.inner(H, W)
    red = lambda keys: (RU.unpack_key(keys)[2] == [255, 0, 0]).all(-1) & (keys != RU.EMPTY)
    box_only = reference(H, W, K, poses, [hidden_box])
    assert (red(box_only["keys"]) & inn).sum() > 60                           # the box is in view
    assert not (red(ref["keys"]) & inn).any()                                  # and the mesh hides all of it
    as_points = reference(H, W, K, poses, [points_call(xyz, rgb, r=0), hidden_box])
    assert (red(as_points["keys"]) & inn).sum() > 20                           # the point-drawn wall does not
    assert ((RU.unpack_key(ref["keys"])[0] == 0) & (ref["keys"] != RU.EMPTY)).sum() > 30     # the x-ray box is on top
    assert ref["count"].max() >= 2
    compare(gpu_draw(H, W, K, poses, calls), ref)
    compare(gpu_draw(H, W, K, poses, calls[::-1]), ref)
    compare(gpu_draw(H, W, K, poses, [points_call(xyz, rgb, r=0), hidden_box]), as_points)


@pytest.fixture(scope="module")
def wall_volume(L):
    """a TsdfVolume that fused the wall's three frames on the device"""
    from boxfusion_amd.scene_mesh import TsdfVolume
    voxel, H, W, focal = WALL
    w = T.wall_scene(*WALL)
    vol = TsdfVolume(voxel=voxel, trunc_voxels=4, capacity=1 << 12, max_depth=10.0, device=DEV)
    vol.integrate(torch.from_numpy(np.stack(w["depths"])).to(DEV), w["K"], w["poses"])
    return vol


def test_end_to_end(L, wall_volume):
    """depth frames -> TsdfVolume -> render_scene(mesh=...) into the cameras they came from: every inner pixel
    covered, the depth within half a voxel of the input"""
    from boxfusion_amd import render as R
    voxel, H, W, focal = WALL
    w = T.wall_scene(*WALL)
    rgb, depth = R.render_scene(None, None, w["poses"], w["K"], H, W, mesh=wall_volume, near=0.05, far=20.0)
    v, c, f = wall_volume.mesh()
    triple_rgb, triple_depth = R.render_scene(None, None, w["poses"], w["K"], H, W, mesh=(v, c, f), near=0.05, far=20.0)
    assert torch.equal(rgb, triple_rgb) and torch.equal(depth, triple_depth)
    stats = torch.zeros(6, dtype=torch.int64, device=DEV)
    ren = R.Renderer(H, W, w["K"], views=3, device=DEV)
    ren.draw_mesh(v, f, c, w["poses"], stats=stats)
    ref = reference(H, W, w["K"], w["poses"], [mesh_call(v.cpu().numpy(), c.cpu().numpy(), f.cpu().numpy(), near=0.05, far=20.0)])
    compare(ren, ref)
    inn = T.inner(H, W)
    depth = depth.cpu().numpy()
    worst = 0.0
    for i in range(3):
        assert (ref["tri_count"][i][inn] == 1).all() and (depth[i][inn] > 0).all()
        worst = max(worst, float(np.abs(depth[i] - w["depths"][i])[inn].max()) / voxel)
    print(f"end to end: worst depth error {worst:.3f} voxel")
    assert worst <= 0.5


def _read_png(path, H, W):
    im = np.array(Image.open(path))
    assert im.shape == (H, W, 3) and im.dtype == np.uint8
    return im


def test_snapshot_writer_mesh_views(L, wall_volume, tmp_path):
    from boxfusion_amd import render as R
    H, W = SIZES[0]
    sw = R.SnapshotWriter(tmp_path / "o", pinhole(H, W), H, W, cloud_views=2)
    paths = sw.finish(None, None, mesh=wall_volume)
    assert [p.split("/")[-1] for p in paths] == ["mesh_0.png", "mesh_1.png", "mesh_top.png"] and sw.written == paths
    shown = [(_read_png(p, H, W).any(-1)).mean() for p in paths]
    assert max(shown) > 0.1 and shown[2] > 0.1, shown                         # the wall from above (its front), and from the side
    assert R.SnapshotWriter(tmp_path / "n", pinhole(H, W), H, W, cloud_views=0).finish(None, None, mesh=wall_volume) == []
    assert R.SnapshotWriter(tmp_path / "m", pinhole(H, W), H, W, cloud_views=2).finish(None, None) == []


def _tiny_sens(tmp_path):
    """four frames of a smooth wall about 2 m in front of a camera that looks along the world's +y"""
    from boxfusion_amd.synthetic import frame_rgbd
    HC, WC, HD, WD, n = 96, 128, 48, 64, 4
    colors = [U.jpeg_bytes(frame_rgbd(i * 3, HC, WC)[0], quality=90) for i in range(n)]
    v, u = np.mgrid[:HD, :WD]
    depths = [((2.0 + 0.3 * np.sin(u / 20.0 + 0.1 * i) * np.cos(v / 15.0)) * 1000.0).astype(np.uint16) for i in range(n)]
    poses = [U.upright_pose((0.05 * i, 0.1, 1.2)) for i in range(n)]
    Kd = np.eye(4, dtype=np.float32)
    Kd[:2, :3] = [[57.8, 0, 31.5], [0, 57.8, 23.5]]
    path = tmp_path / "scene.sens"
    U.write_sens(path, colors, depths, poses, (HC, WC), intrinsic_depth=Kd)
    return path


def test_command_lines(L, wall_volume, tmp_path, capsys):
    from boxfusion_amd import render as R
    from boxfusion_amd import sens as S
    ply = tmp_path / "wall.ply"
    nv, nf = wall_volume.save_ply(str(ply))
    size = ["--views", "2", "--size", "37", "53"]
    names = ["overview_0.png", "overview_1.png", "overview_top.png"]
    assert R.main([str(ply), str(tmp_path / "mesh")] + size) == 0
    assert f"{nv} vertices, {nf} faces -> 3 views" in capsys.readouterr().out
    assert R.main([str(ply), str(tmp_path / "points"), "--as-points", "--radius", "0"] + size) == 0
    assert f"{nv} points -> 3 views" in capsys.readouterr().out
    assert R.main([str(ply), str(tmp_path / "plain"), "--no-cull", "--no-shade"] + size) == 0
    pics = {d: [_read_png(tmp_path / d / n, 37, 53) for n in names] for d in ("mesh", "points", "plain")}
    assert sorted(p.name for p in (tmp_path / "mesh").iterdir()) == names
    top = {d: pics[d][2] for d in pics}
    assert top["mesh"].any(-1).mean() > 0.1 and top["points"].any(-1).mean() > 0.02
    assert not np.array_equal(top["mesh"], top["points"])
    assert not np.array_equal(top["mesh"], top["plain"])                       # the shading
    assert all(pics["plain"][k].any(-1).mean() >= pics["mesh"][k].any(-1).mean() for k in range(3))   # culling only removes
    # a .sens container: the TSDF's surface instead of the cloud
    path = _tiny_sens(tmp_path)
    args = ["--voxel", "0.05", "--max-depth", "4", "--views", "4", "--size", "37", "53"]
    names = [f"overview_{k}.png" for k in range(4)] + ["overview_top.png"]
    assert S.main(["render", str(path), str(tmp_path / "sm"), "--mesh", "--capacity", "4096"] + args) == 0
    assert "5 views in" in capsys.readouterr().out
    assert S.main(["render", str(path), str(tmp_path / "sc")] + args) == 0
    shown = [_read_png(tmp_path / "sm" / n, 37, 53).any(-1).mean() for n in names]
    # culled: the orbit camera on the side the wall was seen from (-y, the fourth) shows it, the one behind it does not
    assert shown[3] > 0.1 and shown[1] < 0.02, shown
    assert not np.array_equal(_read_png(tmp_path / "sm" / names[3], 37, 53), _read_png(tmp_path / "sc" / names[3], 37, 53))


# ---- arguments -----------------------------------------------------------------------------------------
def test_argument_bounds(L):
    """BF_ERR_ARG for every bound of bf_render_triangles, through the C entry point itself"""
    H, W = SIZES[0]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    xyz, rgb, faces = visible_triangles(4, 0)
    dev = dict(vertices=t(xyz), rgb=t(rgb), faces=t(faces), cams=t(RU.camera_rows(cameras(1))),
               keys=torch.full((1, H, W), -1, dtype=torch.int64, device=DEV))
    K = pinhole(H, W)

    def call(**over):
        a = dict(vertices=dev["vertices"].data_ptr(), rgb=dev["rgb"].data_ptr(), n=12, faces=dev["faces"].data_ptr(), m=4,
                 cams=dev["cams"].data_ptr(), V=1, fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], H=H, W=W, near=0.05, far=20.0,
                 cull=0, shade=1, layer=1, coop=64, keys=dev["keys"].data_ptr(), stats=None)
        a.update(over)
        p, f, i, q = ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_longlong
        rc = L.lib().bf_render_triangles(p(a["vertices"]), p(a["rgb"]), q(a["n"]), p(a["faces"]), q(a["m"]), p(a["cams"]), i(a["V"]),
                                         f(a["fx"]), f(a["fy"]), f(a["cx"]), f(a["cy"]), i(a["H"]), i(a["W"]), f(a["near"]),
                                         f(a["far"]), i(a["cull"]), i(a["shade"]), i(a["layer"]), i(a["coop"]), p(a["keys"]),
                                         p(a["stats"]), L._stream())
        torch.cuda.synchronize()
        return rc

    bad = [dict(vertices=None), dict(rgb=None), dict(faces=None), dict(cams=None), dict(keys=None), dict(n=-1), dict(m=-1),
           dict(cull=2), dict(cull=-1), dict(shade=2), dict(shade=-1), dict(layer=2), dict(layer=-1), dict(coop=-1),
           dict(V=0), dict(V=65536), dict(H=0), dict(W=16385), dict(fx=0.0), dict(fy=float("inf")), dict(cx=float("nan")),
           dict(near=0.0), dict(far=0.05), dict(far=float("nan"))]
    for over in bad:
        assert call(**over) == -1, over
    assert (dev["keys"] == -1).all()                                            # nothing above drew anything
    # empty inputs are valid calls that launch nothing, whatever the pointers
    assert call(m=0, faces=None) == 0 and call(n=0, vertices=None, rgb=None) == 0
    assert (dev["keys"] == -1).all()
    assert call() == 0 and (dev["keys"] != -1).any()
    # the binding and the Renderer refuse what they can see
    from boxfusion_amd.render import Renderer
    ren = Renderer(H, W, K, views=1, device=DEV)
    with pytest.raises(L.HipError):
        L.render_triangles(ren.keys, dev["vertices"], dev["rgb"], dev["faces"], dev["cams"], ren.intr, 0.05, 20.0, 0, 1, 1,
                           coop_pixels=-1)
    with pytest.raises(L.HipError):
        L.render_triangles(ren.keys, dev["vertices"], dev["rgb"], dev["faces"].long(), dev["cams"], ren.intr, 0.05, 20.0, 0, 1, 1)
    with pytest.raises(L.HipError):
        L.render_triangles(ren.keys, dev["vertices"], dev["rgb"], dev["faces"], dev["cams"], ren.intr, 0.05, 20.0, 0, 1, 1,
                           stats=torch.zeros(5, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        ren.draw_mesh(xyz, faces[:, :2], rgb, cameras(1))
    with pytest.raises(ValueError):
        ren.draw_mesh(xyz, faces, rgb[:5], cameras(1))
    with pytest.raises(ValueError):
        ren.draw_mesh(xyz, faces, rgb, cameras(3))
    ren.draw_mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), None, cameras(1))
    ren.draw_mesh(xyz, np.zeros((0, 3), np.int64), rgb, cameras(1))
    assert (ren.keys == -1).all()
