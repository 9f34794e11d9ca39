"""The renderer on the GPU (bf_render.hip through boxfusion_amd.render) against its numpy restatement
(tests/render_util.py), bit for bit: rgb with torch.equal and depth viewed as int32.

Every picture is a list of draw calls applied to both sides.  Before a comparison the restatement's own
output must show that the picture is not vacuous (check_caps): at least 20 % of the pixels covered, at
least 5 % of the candidates dropped by every rejection rule the case claims, and a pixel with two or
more candidates where collisions are claimed.  Scenes and seeds were chosen on the CPU so that the
restatement alone satisfies these."""
import numpy as np
import pytest
import torch
from PIL import Image

from tests import render_util as RU
from tests import sens_util as U

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


# ---- cameras and scenes --------------------------------------------------------------------------------
def pinhole(H, W):
    return np.array([[0.8 * W, 0, W / 2 - 0.3], [0, 0.78 * W, H / 2 + 0.2], [0, 0, 1]], np.float32)


def cameras(V):
    """camera -> world [V,4,4]: sens_util's upright camera, then the same yawed and shifted"""
    base = U.upright_pose((0.3, -0.2, 1.1)).astype(np.float64)
    out = [base]
    for a, t in ((0.25, (0.4, 0.0, -0.3)), (-0.3, (-0.5, 0.1, 0.2)))[:V - 1]:
        M = np.eye(4)
        M[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        M[:3, 3] = t
        out.append(base @ M)
    return np.stack(out).astype(np.float32)


def to_world(pc):
    """camera-0 coordinates -> world f32 (the rounding is part of the scene, not of the test)"""
    P = cameras(1)[0].astype(np.float64)
    return (np.asarray(pc, np.float64) @ P[:3, :3].T + P[:3, 3]).astype(np.float32)


def random_points(n, seed):
    """a box that straddles the camera: a quarter behind it or nearer than NEAR, a fifth beyond FAR,
    about half of the rest beside the image, and 6 % NaN / inf"""
    rng = np.random.default_rng(seed)
    xyz = to_world(rng.uniform([-3, -2.5, -2], [3, 2.5, 8], (n, 3)))
    bad = rng.choice(n, (6 * n + 99) // 100, replace=False) if n else np.zeros(0, np.int64)
    xyz[bad, rng.integers(0, 3, len(bad))] = rng.choice([np.nan, np.inf, -np.inf], len(bad))
    return xyz, rng.integers(0, 256, (n, 3), dtype=np.uint8)


def visible_points(n, seed):
    rng = np.random.default_rng(seed)
    return to_world(rng.uniform([-0.8, -0.6, 1.0], [0.8, 0.6, 3.0], (n, 3))), rng.integers(0, 256, (n, 3), dtype=np.uint8)


def points_call(xyz, rgb, r=0, near=NEAR, far=FAR, overlay=False):
    return ("points", dict(xyz=xyz, rgb=rgb, r=r, near=near, far=far, overlay=overlay))


def boxes_call(corners, colors, hw=0, xray=False, mask=None, near=NEAR):
    return ("boxes", dict(corners=np.asarray(corners, np.float32), colors=np.asarray(colors, np.uint8), hw=hw, xray=xray,
                          mask=mask, near=near))


def box(centre, dims, yaw=0.0, pitch=0.0):
    """corners [8,3] in camera-0 coordinates, in the project's v0..v7 order (sign table of
    GeneralInstance3DBoxes.corners), turned about the camera's y (yaw) and x (pitch) axes"""
    sx = np.array([-1, 1, 1, -1, -1, 1, 1, -1.0])
    sy = np.array([-1, -1, 1, 1, -1, -1, 1, 1.0])
    sz = np.array([-1, -1, -1, -1, 1, 1, 1, 1.0])
    c = np.stack([sx, sy, sz], 1) * (np.asarray(dims, np.float64) / 2)
    cy, sy_, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    Ry = np.array([[cy, 0, sy_], [0, 1, 0], [-sy_, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    return c @ (Ry @ Rx).T + np.asarray(centre, np.float64)


# ---- both sides ----------------------------------------------------------------------------------------
def reference(H, W, V, calls):
    K, rows = pinhole(H, W), RU.camera_rows(cameras(V))
    intr = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    keys, count, drops, fates = RU.new_keys(V, H, W), np.zeros((V, H, W), np.int64), {}, {}
    for kind, kw in calls:
        if kind == "points":
            RU.draw_points(keys, kw["xyz"], kw["rgb"], rows, intr, kw["near"], kw["far"], kw["r"], 0 if kw["overlay"] else 1,
                           count=count, drops=drops)
        else:
            RU.draw_edges(keys, kw["corners"], kw["colors"], rows, intr, kw["near"], kw["hw"], 0 if kw["xray"] else 1,
                          mask=kw["mask"], count=count, fates=fates)
    return dict(keys=keys, count=count, drops=drops, fates=fates)


def check_caps(ref, point_rules=(), edge_rules=(), collisions=False, coverage=0.2):
    covered = (ref["keys"] != RU.EMPTY).mean()
    assert covered >= coverage, f"only {covered:.3f} of the pixels covered"
    for rule in point_rules:
        assert ref["drops"][rule] >= 0.05 * ref["drops"]["pairs"], (rule, ref["drops"])
    edges = sum(ref["fates"].values())
    for rule in edge_rules:
        assert ref["fates"].get(rule, 0) >= 0.05 * edges, (rule, ref["fates"])
    if collisions:
        assert ref["count"].max() >= 2


def gpu_draw(H, W, V, calls, poses=None):
    """the calls on the device -> the Renderer"""
    from boxfusion_amd.render import Renderer
    ren = Renderer(H, W, pinhole(H, W), views=V, device=DEV)
    poses = cameras(V) if poses is None else poses
    for kind, kw in calls:
        if kind == "points":
            ren.draw_points(kw["xyz"], kw["rgb"], poses, radius=kw["r"], near=kw["near"], far=kw["far"], overlay=kw["overlay"])
        else:
            ren.draw_boxes(kw["corners"], kw["colors"], poses, half_width=kw["hw"], xray=kw["xray"], mask=kw["mask"],
                           near=kw["near"])
    return ren


def gpu_keys(ren):
    return ren.keys.cpu().numpy().view(np.uint64)


def compare(ren, ref, background=(0, 0, 0)):
    bg = torch.from_numpy(background).to(DEV) if isinstance(background, np.ndarray) else background
    rgb, depth = ren.resolve(bg)
    want_rgb, want_depth = RU.resolve(ref["keys"], background)
    assert rgb.dtype == torch.uint8 and depth.dtype == torch.float32
    assert torch.equal(rgb.cpu(), torch.from_numpy(want_rgb))
    assert torch.equal(depth.cpu().view(torch.int32), torch.from_numpy(want_depth).view(torch.int32))
    np.testing.assert_array_equal(gpu_keys(ren), ref["keys"])
    return rgb, depth


POINT_RULES = ("nonfinite", "near", "far", "outside")
_BACKDROP = {}


def backdrop(r=0):
    """the 5000-point scene every points picture starts from (computed once, never changed)"""
    if r not in _BACKDROP:
        _BACKDROP[r] = points_call(*random_points(5000, 11), r=r)
    return _BACKDROP[r]


# ---- points --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("n,r", [(0, 0), (1, 3), (63, 1), (64, 0), (65, 3), (5000, 0), (5000, 1), (5000, 3)])
def test_points_random(L, size, V, n, r):
    """n = 5000: the random scene alone; smaller n: n visible points drawn by a second call over it (n = 0:
    a valid call that launches nothing)"""
    H, W = size
    if n == 5000:
        calls = [backdrop(r)]
    else:
        calls = [backdrop(0), points_call(*visible_points(n, 100 + n), r=r, near=0.05, far=20.0)]
    ref = reference(H, W, V, calls)
    check_caps(ref, point_rules=POINT_RULES, collisions=True)
    if r == 3:       # the splats cross all four image borders
        k = ref["keys"] != RU.EMPTY
        assert k[:, 0].any() and k[:, -1].any() and k[:, :, 0].any() and k[:, :, -1].any()
    compare(gpu_draw(H, W, V, calls), ref)


@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("size", SIZES)
def test_points_collisions(L, size, V):
    """500 points forced onto sixteen pixels of view 0 at random depths, a fifth of them exact copies of
    others (the same pixel and exactly the same Z in every view) in other colours"""
    H, W = size
    K = pinhole(H, W)
    rng = np.random.default_rng(5)
    px = np.stack([rng.integers(2, W - 2, 16), rng.integers(2, H - 2, 16)], 1)
    which = rng.integers(0, 16, 400)
    z = rng.uniform(0.8, 5.0, 400)
    pc = np.stack([(px[which, 0] - K[0, 2]) / K[0, 0] * z, (px[which, 1] - K[1, 2]) / K[1, 1] * z, z], 1)
    xyz = to_world(pc)
    xyz = np.concatenate([xyz, xyz[rng.integers(0, 400, 100)]])
    rgb = rng.integers(0, 256, (500, 3), dtype=np.uint8)
    calls = [backdrop(0), points_call(xyz, rgb, r=0, near=0.05, far=20.0)]
    ref = reference(H, W, V, calls)
    check_caps(ref, point_rules=POINT_RULES, collisions=True)
    only = reference(H, W, 1, calls[1:])
    assert (only["keys"] != RU.EMPTY).sum() <= 16 and only["count"].max() >= 20      # sixteen pixels, deep piles
    same = np.unique(xyz, axis=0, return_counts=True)[1]
    assert (same >= 2).sum() >= 50
    compare(gpu_draw(H, W, V, calls), ref)


@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("size", SIZES)
def test_points_order_independence(L, size, V):
    H, W = size
    (_, kw), = [backdrop(1)]
    ref = reference(H, W, V, [backdrop(1)])
    check_caps(ref, point_rules=POINT_RULES, collisions=True)
    one = gpu_draw(H, W, V, [backdrop(1)])
    perm = np.random.default_rng(9).permutation(5000)
    permuted = gpu_draw(H, W, V, [points_call(kw["xyz"][perm], kw["rgb"][perm], r=1)])
    cuts = [0, 1667, 3334, 5000]
    thirds = gpu_draw(H, W, V, [points_call(kw["xyz"][a:b], kw["rgb"][a:b], r=1) for a, b in zip(cuts, cuts[1:])])
    assert torch.equal(one.keys, permuted.keys) and torch.equal(one.keys, thirds.keys)
    compare(one, ref)


# ---- edges ---------------------------------------------------------------------------------------------
def edge_scene():
    """boxes in camera-0 coordinates -> (corners [B,8,3] world, colours, names)"""
    b = dict(
        in_view=box((0.0, 0.0, 2.6), (1.6, 1.2, 1.0)),                     # axis-aligned: horizontal and vertical edges
        steep=box((-0.5, 0.1, 2.2), (0.9, 1.3, 0.7), yaw=0.5, pitch=1.2),
        shallow=box((0.6, -0.1, 3.0), (1.8, 0.5, 0.9), yaw=-0.4, pitch=0.1),
        tall=box((0.1, 0.0, 4.0), (2.4, 2.0, 1.0), yaw=0.8),
        corner_behind=box((0.9, 0.5, 0.55), (0.9, 0.8, 1.4), yaw=0.7, pitch=0.5),
        straddle=box((-0.6, 0.3, 0.9), (0.8, 0.6, 1.6)),                   # front face behind the near plane
        straddle_in_view=box((0.1, 0.05, 0.7), (0.3, 0.25, 1.0)),
        straddle_turned=box((-0.1, -0.1, 0.8), (0.3, 0.3, 1.2), yaw=0.3, pitch=0.2),
        graze=box((0.0, -0.1, 0.9), (4000.0, 0.1, 0.798)),                 # front edges 1 mm past the near plane, +-2 km wide
        behind=box((0.2, 0.1, -3.0), (1.0, 1.0, 1.0), yaw=0.3),
        off_screen=box((9.0, 0.3, 3.0), (1.0, 1.0, 1.0), yaw=0.2),
        nan_corner=box((0.0, 0.0, 2.0), (0.5, 0.5, 0.5)),
        after_nan=box((-0.2, -0.3, 1.8), (0.7, 0.5, 0.6), yaw=-0.9, pitch=-0.3),
    )
    names = list(b)
    corners = to_world(np.stack([b[k] for k in names]).reshape(-1, 3)).reshape(-1, 8, 3)
    corners[names.index("nan_corner"), 5, 1] = np.nan
    colors = np.random.default_rng(2).integers(0, 256, (len(names), 3), dtype=np.uint8)
    return corners, colors, names


EDGE_RULES = ("behind", "offscreen", "near_clipped", "bad_box")


@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("hw", [0, 1])
def test_edges(L, size, V, hw):
    H, W = size
    corners, colors, names = edge_scene()
    calls = [boxes_call(corners, colors, hw=hw)]
    ref = reference(H, W, V, calls)
    check_caps(ref, edge_rules=EDGE_RULES, collisions=True)
    # the grazing box: its front edges lie within 1 mm of the near plane and project +-1e6 pixels wide; the
    # restatement (which has the same cap) samples each at most max(W, H) + 1 times
    g = names.index("graze")
    cam = [RU.to_camera(RU.camera_rows(cameras(1))[0], *corners[g, k]) for k in range(8)]
    assert 0 < min(float(c[2]) for c in cam) - NEAR < 1.5e-3
    K = pinhole(H, W)
    s, fate = RU.edge_samples(cam[0], cam[1], (K[0, 0], K[1, 1], K[0, 2], K[1, 2]), H, W, NEAR)
    assert fate == "drawn" and len(s[0]) <= max(W, H) + 1 and abs(float(cam[1][0] - cam[0][0])) > 3000
    ren = gpu_draw(H, W, V, calls)                                          # the call returns
    compare(ren, ref)
    # boxes that draw nothing: the picture without them is the same picture
    for gone in ("behind", "off_screen", "nan_corner"):
        alone = reference(H, W, 1, [boxes_call(corners[names.index(gone)][None], colors[:1], hw=hw)])
        assert (alone["keys"] == RU.EMPTY).all()
    keep = np.array([n not in ("behind", "off_screen", "nan_corner") for n in names])
    assert torch.equal(gpu_draw(H, W, V, [boxes_call(corners[keep], colors[keep], hw=hw)]).keys, ren.keys)
    # the enable mask: unset entries skip their boxes, an all-set mask changes nothing
    mask = np.array([n not in ("steep", "after_nan") for n in names])
    masked = [boxes_call(corners, colors, hw=hw, mask=mask)]
    ref_m = reference(H, W, V, masked)
    check_caps(ref_m, edge_rules=EDGE_RULES, collisions=True)
    assert (ref_m["keys"] != ref["keys"]).any()
    compare(gpu_draw(H, W, V, masked), ref_m)
    assert torch.equal(gpu_draw(H, W, V, [boxes_call(corners, colors, hw=hw, mask=np.ones(len(names), bool))]).keys, ren.keys)
    assert torch.equal(gpu_draw(H, W, V, [boxes_call(corners, colors, hw=hw, mask=torch.from_numpy(mask).to(DEV))]).keys,
                       gpu_draw(H, W, V, masked).keys)


def test_edges_exactly_horizontal_and_vertical(L):
    """view 0 of the axis-aligned box: its front face's edges have equal v (or u) at both ends, bit for bit"""
    H, W = SIZES[0]
    corners, colors, names = edge_scene()
    K = pinhole(H, W)
    intr = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    cam = [RU.to_camera(RU.camera_rows(cameras(1))[0], *corners[0, k]) for k in range(8)]
    kinds = set()
    for i, j in RU.EDGES:
        s, fate = RU.edge_samples(cam[i], cam[j], intr, H, W, NEAR)
        assert fate == "drawn"
        if (s[1] == s[1][0]).all() and len(s[0]) > 5:
            kinds.add("horizontal")
        if (s[0] == s[0][0]).all() and len(s[0]) > 5:
            kinds.add("vertical")
    assert kinds == {"horizontal", "vertical"}
    calls = [boxes_call(corners[:1], colors[:1], hw=0)]
    compare(gpu_draw(H, W, 1, calls), reference(H, W, 1, calls))


# ---- layers --------------------------------------------------------------------------------------------
def wall(H, W, z=1.2):
    """a dense wall of points at depth z of camera 0, wider than the image"""
    K = pinhole(H, W)
    u, v = np.meshgrid(np.arange(-4, W + 4, 0.5), np.arange(-4, H + 4, 0.5))
    pc = np.stack([(u.ravel() - K[0, 2]) / K[0, 0] * z, (v.ravel() - K[1, 2]) / K[1, 1] * z, np.full(u.size, z)], 1)
    return to_world(pc), np.random.default_rng(4).integers(0, 256, (u.size, 3), dtype=np.uint8)


@pytest.mark.parametrize("size", SIZES)
def test_layers(L, size):
    H, W = size
    corners, colors, names = edge_scene()
    near_box, far_box = names.index("in_view"), names.index("tall")
    two = np.stack([corners[near_box], corners[far_box]])
    cols = np.array([[255, 0, 0], [0, 0, 255]], np.uint8)
    w = points_call(*wall(H, W), r=0, near=0.05, far=20.0)
    hidden = [w, boxes_call(two, cols, hw=1, xray=False)]
    shown = [w, boxes_call(two, cols, hw=1, xray=True)]
    ref_h, ref_s = reference(H, W, 1, hidden), reference(H, W, 1, shown)
    ref_w = reference(H, W, 1, [w])
    check_caps(ref_h, collisions=True, coverage=0.99)
    check_caps(ref_s, collisions=True, coverage=0.99)
    boxes_only = reference(H, W, 1, [boxes_call(two, cols, hw=1, xray=True)])
    on_box = boxes_only["keys"] != RU.EMPTY
    assert on_box.mean() > 0.1
    np.testing.assert_array_equal(ref_h["keys"], ref_w["keys"])             # the wall hides every pixel of the boxes
    rgb_h, depth_h = compare(gpu_draw(H, W, 1, hidden), ref_h)
    rgb_s, depth_s = compare(gpu_draw(H, W, 1, shown), ref_s)
    on = torch.from_numpy(on_box)
    assert (depth_h.cpu() < 1.3).all()                                      # the wall's depth everywhere
    assert (depth_s.cpu()[on] > 1.9).all() and (depth_s.cpu()[~on] < 1.3).all()   # the boxes' Z where they are
    box_z = RU.unpack_key(boxes_only["keys"][on_box])[1]
    np.testing.assert_array_equal(depth_s.cpu().numpy()[on_box], box_z)
    # two x-ray boxes sort by depth between themselves: where both have pixels the nearer (red) one shows
    a = reference(H, W, 1, [boxes_call(two[:1], cols[:1], hw=1, xray=True)])["keys"]
    b = reference(H, W, 1, [boxes_call(two[1:], cols[1:], hw=1, xray=True)])["keys"]
    both = (a != RU.EMPTY) & (b != RU.EMPTY)
    red = both & (a < b)
    assert red.sum() >= 4
    np.testing.assert_array_equal(gpu_keys(gpu_draw(H, W, 1, shown[1:]))[both], np.minimum(a, b)[both])
    assert (rgb_s.cpu()[torch.from_numpy(red)] == torch.tensor([255, 0, 0], dtype=torch.uint8)).all()


# ---- resolve -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("size", SIZES)
def test_resolve_backgrounds(L, size, V):
    H, W = size
    calls = [backdrop(0)]
    ref = reference(H, W, V, calls)
    check_caps(ref, point_rules=POINT_RULES)
    empty = ref["keys"] == RU.EMPTY
    assert empty.mean() > 0.2
    ren = gpu_draw(H, W, V, calls)
    rgb, depth = compare(ren, ref, (12, 250, 3))
    assert (rgb.cpu().numpy()[empty] == [12, 250, 3]).all() and (depth.cpu().numpy()[empty] == 0).all()
    assert (depth.cpu().numpy()[~empty] > NEAR).all()
    img = np.random.default_rng(8).integers(0, 256, (V, H, W, 3), dtype=np.uint8)
    rgb, depth = compare(ren, ref, img)
    assert (rgb.cpu().numpy()[empty] == img[empty]).all() and (depth.cpu().numpy()[empty] == 0).all()
    fresh = gpu_draw(H, W, V, [])                                           # a cleared target is all background
    rgb, depth = fresh.resolve((1, 2, 3))
    assert (rgb.cpu().numpy() == [1, 2, 3]).all() and (depth == 0).all()
    ren.clear()
    assert torch.equal(ren.keys, fresh.keys)


def test_argument_validation(L):
    from boxfusion_amd.render import Renderer
    H, W = SIZES[0]
    ren = Renderer(H, W, pinhole(H, W), views=1, device=DEV)
    xyz, rgb = visible_points(4, 0)
    corners, colors, _ = edge_scene()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    cams = t(RU.camera_rows(cameras(1)))
    intr = ren.intr
    with pytest.raises(ValueError):
        ren.draw_points(xyz, rgb, cameras(1), radius=5)
    with pytest.raises(ValueError):
        ren.draw_boxes(corners, colors, cameras(1), half_width=3)
    with pytest.raises(ValueError):
        ren.draw_points(xyz, rgb, cameras(3))                               # three cameras, one view
    with pytest.raises(ValueError):
        Renderer(H, W, pinhole(H, W), views=0, device=DEV)
    for bad in (dict(radius=5), dict(radius=-1), dict(near=0.0), dict(far=0.01), dict(layer=2)):
        kw = dict(near=0.05, far=20.0, radius=1, layer=1)
        kw.update(bad)
        with pytest.raises(L.HipError):
            L.render_points(ren.keys, t(xyz), t(rgb), cams, intr, kw["near"], kw["far"], kw["radius"], kw["layer"])
    for bad in (dict(half_width=3), dict(half_width=-1), dict(near=-1.0)):
        kw = dict(near=0.05, half_width=1)
        kw.update(bad)
        with pytest.raises(L.HipError):
            L.render_edges(ren.keys, t(corners), t(colors), None, cams, intr, kw["near"], kw["half_width"], 1)
    with pytest.raises(L.HipError):
        L.render_points(ren.keys, t(xyz), t(rgb), cams[:, :9].contiguous(), intr, 0.05, 20.0, 1, 1)
    # nothing above drew anything; empty inputs are valid calls
    ren.draw_points(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8), cameras(1))
    ren.draw_boxes(np.zeros((0, 8, 3), np.float32), np.zeros((0, 3), np.uint8), cameras(1))
    assert (ren.keys == -1).all()


# ---- plumbing ------------------------------------------------------------------------------------------
def test_renderer_poses_as_arrays_and_tensors(L):
    H, W = SIZES[1]
    calls = [backdrop(1), boxes_call(*edge_scene()[:2], hw=1, xray=True)]
    a = gpu_draw(H, W, 3, calls, poses=cameras(3))
    b = gpu_draw(H, W, 3, calls, poses=torch.from_numpy(cameras(3)))
    c = gpu_draw(H, W, 3, calls, poses=torch.from_numpy(cameras(3)).to(DEV).double())
    assert torch.equal(a.keys, b.keys) and torch.equal(a.keys, c.keys)
    compare(a, reference(H, W, 3, calls))


@pytest.fixture(scope="module")
def two_frame_cloud(L):
    """a SceneCloud that integrated two synthetic frames (as test_gpu_cloud.py feeds it)"""
    from boxfusion_amd.scene_cloud import SceneCloud
    from boxfusion_amd.synthetic import frame_rgbd
    from boxfusion_amd.tools_utils import unproject
    HD, WD = 48, 64
    K = np.array([[57.8, 0, 31.5], [0, 57.8, 23.5], [0, 0, 1]], np.float32)
    sc = SceneCloud(voxel=0.05, capacity=1 << 16, device=DEV)
    for i in range(2):
        rgb, depth = frame_rgbd(i, HD, WD)
        xyz, valid = unproject(torch.from_numpy(depth).to(DEV), K, U.upright_pose((0.1 * i, 0.0, 1.2)), max_depth=10.0)
        sc.integrate(xyz, valid, torch.from_numpy(rgb).to(DEV))
    return sc


def test_render_scene_on_a_scene_cloud(L, two_frame_cloud):
    from boxfusion_amd import render as R
    sc = two_frame_cloud
    xyz, rgb, _ = sc.points()
    assert xyz.shape[0] > 3000
    H, W = SIZES[0]
    K = pinhole(H, W)
    lo, hi = xyz.min(0).values.cpu().numpy(), xyz.max(0).values.cpu().numpy()
    poses = np.concatenate([R.orbit_poses(lo, hi, 2, K3=K, H=H, W=W), R.topdown_pose(lo, hi, K, H, W)[None]])
    corners = np.stack([box((lo + hi) / 2, (hi - lo) * 0.5, yaw=0.3), box((lo + hi) / 2, (hi - lo) * 0.9)]).astype(np.float32)
    got_rgb, got_depth = R.render_scene(sc, corners, poses, K, H, W, radius=1, half_width=1, background=(9, 9, 9), far=50.0)
    pair_rgb, pair_depth = R.render_scene((xyz, rgb), (corners, R.box_colors(2)), poses, K, H, W, radius=1, half_width=1,
                                          background=(9, 9, 9), far=50.0)
    assert torch.equal(got_rgb, pair_rgb) and torch.equal(got_depth, pair_depth)
    rows = RU.camera_rows(poses)
    keys, intr = RU.new_keys(3, H, W), (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    RU.draw_points(keys, xyz.cpu().numpy(), rgb.cpu().numpy(), rows, intr, 0.05, 50.0, 1, 1)
    RU.draw_edges(keys, corners, R.box_colors(2), rows, intr, 0.05, 1, 1)
    assert (keys != RU.EMPTY).mean() >= 0.2
    want_rgb, want_depth = RU.resolve(keys, (9, 9, 9))
    assert torch.equal(got_rgb.cpu(), torch.from_numpy(want_rgb))
    assert torch.equal(got_depth.cpu().view(torch.int32), torch.from_numpy(want_depth).view(torch.int32))
    # no points, no boxes: the background
    none_rgb, none_depth = R.render_scene(None, None, poses, K, H, W, background=(9, 9, 9))
    assert (none_rgb == 9).all() and (none_depth == 0).all()


def _read_png(path, H, W):
    im = np.array(Image.open(path))
    assert im.shape == (H, W, 3) and im.dtype == np.uint8
    return im


def test_snapshot_writer_overviews(L, two_frame_cloud, tmp_path):
    from boxfusion_amd import render as R
    H, W = SIZES[0]
    sw = R.SnapshotWriter(tmp_path / "o", pinhole(H, W), H, W, cloud_views=2)
    paths = sw.finish(two_frame_cloud, None)
    assert [p.split("/")[-1] for p in paths] == ["overview_0.png", "overview_1.png", "overview_top.png"]
    for p in paths:
        assert (_read_png(p, H, W).any(-1)).mean() > 0.05                  # the cloud is in the picture
    assert R.SnapshotWriter(tmp_path / "n", pinhole(H, W), H, W, cloud_views=0).finish(two_frame_cloud, None) == []
    with pytest.raises(ValueError):
        R.SnapshotWriter(tmp_path, pinhole(H, W), H, W, every="frames")


class _SceneDetect:
    """Pipeline.run's detect side: the synthetic scene's detections of each keyframe (what the pipeline
    tests' stand-in models return), no model"""
    B = 1

    def __init__(self, scene):
        self.scene, self.ids = scene, []

    def preprocess_frames(self, depth, poses):
        return None

    def __call__(self, rgb, depth, poses):
        from boxfusion_amd.pipeline import scene_instances
        return [scene_instances(self.scene.detections(self.ids.pop(0)), torch.device(DEV))]


def test_pipeline_snapshots(L, tmp_path):
    from tests import trace_util as TU
    from boxfusion_amd import render as R
    from boxfusion_amd.fusion_stage import FusionStage
    from boxfusion_amd.pipeline import Pipeline
    from boxfusion_amd.synthetic import SCANNET_K, Scene, frame_rgbd
    n, gap = 8, 3
    cfg = dict(TU.SCANNET_CFG, data=dict(gap=gap))
    scene = Scene(seed=0)
    host = {i: frame_rgbd(i)[0] for i in range(n)}
    depth = torch.zeros((1, 480, 640), device=DEV)

    def frames(ids):
        return (torch.from_numpy(np.stack([host[i] for i in ids])).to(DEV), depth.expand(len(ids), -1, -1),
                np.stack([scene.pose(i) for i in ids]))

    def run(snapshots):
        det = _SceneDetect(scene)
        det.ids = [i for i in range(n) if i % gap == 0]
        fusion = FusionStage(cfg, SCANNET_K, device=DEV)
        Pipeline(det, fusion, gap).run(frames, n, snapshots=snapshots)
        return fusion.all_pred_box.pred_boxes_3d.corners

    sw = R.SnapshotWriter(tmp_path / "snaps", SCANNET_K, 480, 640)
    with_snaps = run(sw)
    want = [f"snap_{i:06d}.png" for i in (0, 3, 6, 7)]                      # the keyframes and the last frame
    assert sorted(p.name for p in (tmp_path / "snaps").iterdir()) == want
    assert [p.split("/")[-1] for p in sw.written] == want
    assert with_snaps.shape[0] > 3
    for name, i in zip(want, (0, 3, 6, 7)):
        im = _read_png(tmp_path / "snaps" / name, 480, 640)
        changed = (im != host[i]).any(-1).mean()
        assert 0.001 < changed < 0.5, changed                               # the frame, with wireframes on it
    assert torch.equal(run(None), with_snaps)


def _tiny_sens(tmp_path):
    from boxfusion_amd.synthetic import frame_rgbd
    HC, WC, HD, WD, n = 96, 128, 48, 64, 4
    colors = [U.jpeg_bytes(frame_rgbd(i * 3, HC, WC)[0], quality=90) for i in range(n)]
    depths = [np.clip(frame_rgbd(i * 3, HD, WD)[1] * 1000.0, 0, 65535).astype(np.uint16) for i in range(n)]
    poses = [U.upright_pose((0.05 * i, 0.1, 1.2)) for i in range(n)]
    Kd = np.eye(4, dtype=np.float32)
    Kd[:2, :3] = [[57.8, 0, 31.5], [0, 57.8, 23.5]]
    path = tmp_path / "scene.sens"
    U.write_sens(path, colors, depths, poses, (HC, WC), intrinsic_depth=Kd)
    return path


def test_command_lines(L, tmp_path, capsys):
    """`python -m boxfusion_amd.sens render` on a tiny container, and `python -m boxfusion_amd.render` on
    the PLY that `sens cloud` writes of it: the same pictures"""
    from boxfusion_amd import render as R
    from boxfusion_amd import sens as S
    from boxfusion_amd.results import save_box
    path = _tiny_sens(tmp_path)
    # world coordinates: one box around the whole cloud (the camera looks along +y from (0, 0.1, 1.2) at depths up
    # to 4 m), so its wireframe is not hidden inside the random points, and one inside it
    boxes = np.stack([box((0.07, 2.3, 1.2), (6.0, 5.5, 4.5)), box((0.3, 1.5, 1.0), (1.0, 1.0, 1.0), yaw=0.4)])
    save_box([[(0, b, 1.0) for b in boxes]], str(tmp_path / "scene_boxes.pkl"))
    args = ["--boxes", str(tmp_path / "scene_boxes.pkl"), "--views", "2", "--size", "37", "53", "--radius", "2"]
    assert S.main(["render", str(path), str(tmp_path / "a"), "--voxel", "0.05", "--max-depth", "4"] + args) == 0
    names = ["overview_0.png", "overview_1.png", "overview_top.png"]
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == names
    assert "3 views in" in capsys.readouterr().out
    assert S.main(["cloud", str(path), str(tmp_path / "scene.ply"), "--voxel", "0.05", "--max-depth", "4"]) == 0
    assert R.main([str(tmp_path / "scene.ply"), str(tmp_path / "b")] + args) == 0
    for n in names:
        a, b = _read_png(tmp_path / "a" / n, 37, 53), _read_png(tmp_path / "b" / n, 37, 53)
        assert np.array_equal(a, b) and a.any(-1).mean() > 0.2
    plain = tmp_path / "c"
    assert R.main([str(tmp_path / "scene.ply"), str(plain), "--views", "1", "--size", "37", "53", "--radius", "2"]) == 0
    assert not np.array_equal(_read_png(plain / "overview_top.png", 37, 53), _read_png(tmp_path / "b" / "overview_top.png", 37, 53))
