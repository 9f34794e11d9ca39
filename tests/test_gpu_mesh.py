"""The scene mesh on the GPU (bf_tsdf.hip, scene_mesh.TsdfVolume) against the numpy restatement in
tests/mesh_ref.py, bit for bit: the volume's integers after dirty frames, their independence of frame
order and batching, a full table, a voxel at its cap, the surface-nets vertices / colours / faces, and
the plumbing into `sens mesh`, `scene_mesh`, `evaluation filter` and Pipeline.run."""
import json

import numpy as np
import pytest
import torch
from PIL import Image

from tests import mesh_ref as R
from tests import sens_util as U

pytestmark = pytest.mark.gpu

DEV = "cuda"
VOXEL, T, MAX_DEPTH = 0.05, 3, 1.2


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from boxfusion_amd import _lib
    _lib.lib()
    return _lib


def _volume(capacity=1 << 10, voxel=VOXEL, trunc=T, max_depth=MAX_DEPTH, **kw):
    from boxfusion_amd.scene_mesh import TsdfVolume
    return TsdfVolume(voxel=voxel, trunc_voxels=trunc, capacity=capacity, max_depth=max_depth, device=DEV, **kw)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _feed(vol, sc, depths, poses, rgbs=None):
    vol.integrate(_dev(np.stack(depths)), sc.K, np.stack(poses), None if rgbs is None else _dev(np.stack(rgbs)))


def _assert_raw(vol, ref):
    key, state = vol.raw()
    assert key.dtype == torch.int64 and state.dtype == torch.int32 and tuple(state.shape[1:]) == (6, 512)
    assert torch.equal(key.cpu(), torch.from_numpy(ref["key"]))
    assert torch.equal(state.cpu().long(), torch.from_numpy(ref["state"]))


def _assert_mesh(vol):
    """vol.mesh() equals the restatement's surface of vol.raw(); returns the restatement's mesh"""
    key, state = vol.raw()
    want = R.surface(key.cpu().numpy(), state.cpu().numpy().astype(np.int64), vol.voxel)
    got = vol.mesh()
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.uint8 and got[2].dtype == torch.int32
    for g, w in zip(got, want):
        assert tuple(g.shape) == w.shape and torch.equal(g.cpu(), torch.from_numpy(w))
    return want


@pytest.fixture(scope="module")
def small():
    """24x32 frames of a scene 1.5 m across that straddles the origin: a sphere of radius 3 voxels, the
    tilted wall and the shell, from six cameras 0.55 m from the sphere (inside the shell's
    blocks), with colour at twice the depth size"""
    sc = R.Scene(voxel=VOXEL, H=24, W=32, focal=30.0, dist=0.55, wall_at=-0.5, shell=0.75, radius_voxels=3)
    rng = np.random.default_rng(11)
    depths = sc.depths()
    big = rng.integers(0, 256, (len(depths), 48, 64, 3), dtype=np.uint8)
    rgbs = [np.array(Image.fromarray(im).resize((32, 24))) for im in big]        # as bf_resize_bicubic_u8 resizes
    return dict(scene=sc, depths=depths, poses=sc.poses, big=big, rgbs=rgbs)


# ---- 1. the volume ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dirty(small):
    sc, rng = small["scene"], np.random.default_rng(5)
    d0 = small["depths"][0].copy()
    d0[rng.random(d0.shape) < 0.2] = 0.0                     # holes
    d0[rng.random(d0.shape) < 0.1] = 5.0                     # beyond max_depth
    d0[0, 0] = MAX_DEPTH                                     # exactly max_depth: not valid
    d0[12, 10] = np.nan
    inside = sc.pose_on_wall()                               # frame 3: a camera inside the volume
    depths = [d0, np.zeros_like(d0), small["depths"][2], sc.depth(inside)]
    poses = [small["poses"][0], small["poses"][1], U.LOST.copy(), inside]
    poses[2][:] = small["poses"][2]
    poses[2][1, 3] = -np.inf                                 # one -inf entry: the frame is skipped
    seen = {}
    refs = {c: R.fuse(depths, poses, sc.K, VOXEL, T, MAX_DEPTH, small["rgbs"][:4] if c else None, seen=seen)
            for c in (False, True)}
    assert seen["behind"] > 0 and seen["outside"] > 0        # voxels with z <= 0, and voxels off the image
    blocks = R.key_block(refs[True]["key"])
    assert (blocks < 0).any() and (blocks > 0).any() and refs[True]["skipped_pose"] == 1
    return dict(depths=depths, poses=poses, refs=refs)


@pytest.mark.parametrize("colour", [False, True])
def test_volume_vs_restatement(L, small, dirty, colour):
    ref = dirty["refs"][colour]
    vol = _volume()
    vol.integrate(_dev(np.stack(dirty["depths"])), small["scene"].K, np.stack(dirty["poses"]),
                  _dev(small["big"][:4]) if colour else None)
    _assert_raw(vol, ref)
    st = vol.stats()
    assert st["blocks"] == len(ref["key"]) and st["observations"] == ref["observations"] > 1000
    assert st["skipped_pose"] == 1 and st["out_of_range"] == ref["out_of_range"] == 0
    assert st["dropped_full"] == 0 and st["saturated"] == 0
    assert (ref["state"][:, 2].sum() > 0) == colour
    vol.reset()
    assert vol.raw()[0].numel() == 0 and vol.stats()["observations"] == 0 and vol.mesh()[2].shape == (0, 3)


def test_out_of_range_is_counted(L, small):
    """a camera 60 km out: every sample's block index is past 2^20, counted and not stored"""
    vol = _volume(voxel=0.005, max_depth=10.0)
    pose = np.eye(4, dtype=np.float32)
    pose[0, 3] = 6.0e4
    depth = np.full((24, 32), 1.0, np.float32)
    vol.integrate(_dev(depth), small["scene"].K, pose)
    st = vol.stats()
    assert st["out_of_range"] == 24 * 32 * (2 * T + 1) and st["blocks"] == 0 and st["observations"] == 0


# ---- 2. order and batching -------------------------------------------------------------------------
def test_order_and_batching(L, small):
    sc, n = small["scene"], 5
    depths, poses, rgbs = small["depths"][:n], small["poses"][:n], list(small["big"][:n])

    def one_launch(vol):
        _feed(vol, sc, depths, poses, rgbs)

    def five_launches(vol):
        for j in range(n):
            _feed(vol, sc, depths[j:j + 1], poses[j:j + 1], rgbs[j:j + 1])

    def reversed_pairs(vol):
        order = list(range(n))[::-1]
        for a in range(0, n, 2):
            sel = order[a:a + 2]
            _feed(vol, sc, [depths[j] for j in sel], [poses[j] for j in sel], [rgbs[j] for j in sel])
    outs = []
    for feed in (one_launch, five_launches, reversed_pairs):
        vol = _volume()
        feed(vol)
        assert vol.stats()["saturated"] == 0 and vol.stats()["dropped_full"] == 0
        outs.append([t.cpu() for t in vol.raw() + vol.mesh()])
    assert outs[0][2].shape[0] > 500 and outs[0][4].shape[0] > 500
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert a.dtype == b.dtype and torch.equal(a, b)
    _assert_raw(vol, R.fuse(depths, poses, sc.K, VOXEL, T, MAX_DEPTH, small["rgbs"][:n]))


# ---- 3. full table ---------------------------------------------------------------------------------
def test_full_table_ends_cleanly(L, small):
    sc = small["scene"]
    depths, poses = small["depths"][:3], small["poses"][:3]
    ref = R.fuse(depths, poses, sc.K, VOXEL, T, MAX_DEPTH)
    assert len(ref["key"]) > 8
    vol = _volume(capacity=8)
    _feed(vol, sc, depths[:2], poses[:2])
    _feed(vol, sc, depths[2:], poses[2:])
    st = vol.stats()
    key, state = [t.cpu().numpy() for t in vol.raw()]
    assert len(key) == 8 == st["blocks"] and st["dropped_full"] > 0
    at = np.searchsorted(ref["key"], key)
    np.testing.assert_array_equal(ref["key"][at], key)
    np.testing.assert_array_equal(state, ref["state"][at])
    assert st["observations"] == int(state[:, 0].sum())
    vol.mesh()                                               # neighbour lookups in a full table end too


# ---- 4. saturation ---------------------------------------------------------------------------------
def test_saturation(L, small):
    sc = small["scene"]
    d, p = small["depths"][:1], small["poses"][:1]
    vol = _volume(max_weight=4)
    for _ in range(6):
        _feed(vol, sc, d, p, small["big"][:1])
    ref = R.fuse(d * 6, p * 6, sc.K, VOXEL, T, MAX_DEPTH, small["rgbs"][:1] * 6, max_weight=4)
    _assert_raw(vol, ref)
    st = vol.stats()
    w = vol.raw()[1][:, 0]
    assert int(w.max()) == 4 and st["saturated"] == ref["saturated"] == 2 * int((w == 4).sum()) > 0
    assert st["observations"] == int(w.sum())
    with pytest.raises(ValueError):
        _volume(max_weight=0)


# ---- 5. the surface ----------------------------------------------------------------------------------
def test_surface_wall_and_hole(L, small):
    """the wall and shell alone, then with a patch of every frame's depth missing: the surface has a
    boundary there and no face reaches into the unobserved cells"""
    sc = small["scene"]
    depths = [sc.depth(p, sphere=False) for p in sc.poses]
    vol = _volume()
    _feed(vol, sc, depths, sc.poses, list(small["big"]))
    v, _, f = _assert_mesh(vol)
    assert len(v) > 1000 and len(f) > 1000
    holed = [d.copy() for d in depths]
    for d in holed:
        d[8:16, 10:22] = 0.0
    vol = _volume()
    _feed(vol, sc, holed, sc.poses)
    v2, c2, f2 = _assert_mesh(vol)
    assert (c2 == 128).all() and 0 < len(f2) < len(f)
    # directly, from the volume's integers: every vertex a face uses lies in a cell whose 8 corners were observed
    key, state = [t.cpu().numpy() for t in vol.raw()]
    seen = set()
    for b, w in zip(R.key_block(key), state[:, 0].reshape(-1, 8, 8, 8)):        # w[z, y, x]
        z, y, x = np.nonzero(w > 0)
        seen.update(zip((b[0] * 8 + x).tolist(), (b[1] * 8 + y).tolist(), (b[2] * 8 + z).tolist()))

    def valid(cell):
        return all((cell[0] + c[0], cell[1] + c[1], cell[2] + c[2]) in seen for c in R.CORNERS.tolist())
    got_v, _, got_f = [t.cpu().numpy() for t in vol.mesh()]
    g = got_v.astype(np.float64) / VOXEL - 0.5                                   # in cells; a vertex lies in [i, i + 1]
    lo, hi = np.floor(g - 1e-4).astype(int), np.floor(g + 1e-4).astype(int)
    used = np.unique(got_f)
    assert len(used) > 1000
    for i in used:
        cells = {(a, b_, c) for a in (lo[i, 0], hi[i, 0]) for b_ in (lo[i, 1], hi[i, 1]) for c in (lo[i, 2], hi[i, 2])}
        assert any(valid(cell) for cell in cells), got_v[i]


def test_surface_sphere_48x64(L):
    """the host test's scene: the volume and the mesh of the restatement, on the GPU; the sphere
    crosses block boundaries on every axis"""
    sc = R.Scene()
    depths = sc.depths()
    vol = _volume(capacity=1 << 11, trunc=4, max_depth=3.5)
    _feed(vol, sc, depths, sc.poses)
    _assert_raw(vol, R.fuse(depths, sc.poses, sc.K, VOXEL, 4, 3.5))
    v, _, f = _assert_mesh(vol)
    on = np.linalg.norm(v.astype(np.float64) - sc.centre, axis=1) < sc.radius + 3 * VOXEL
    cells = np.floor(v[on] / np.float32(VOXEL) - 0.5).astype(np.int64)
    for ax in range(3):                                      # vertex cells on both sides of a block face, joined by faces
        assert (cells[:, ax] % 8 == 7).any() and (cells[:, ax] % 8 == 0).any()
    assert len(f) > 2 * on.sum() - 10


def test_surface_zero_is_outside(L, small):
    """corners whose sum q is set to exactly 0 count as outside"""
    sc = small["scene"]
    vol = _volume()
    _feed(vol, sc, small["depths"], small["poses"])
    before = [t.cpu() for t in vol.mesh()]
    w, q = vol.vox[:, 0], vol.vox[:, 1]
    shallow = (w > 0) & (q < 0) & (q > -300 * w)             # inside, by less than 0.3 of the truncation
    assert int(shallow.sum()) > 100
    q[shallow] = 0
    v, _, f = _assert_mesh(vol)
    assert len(v) != before[0].shape[0] or not np.array_equal(v, before[0].numpy())
    key, state = vol.raw()
    assert int(((state[:, 0] > 0) & (state[:, 1] == 0)).sum()) >= int(shallow.sum())


# ---- 6. plumbing -------------------------------------------------------------------------------------
def test_sens_mesh_command(L, tmp_path, capsys):
    from boxfusion_amd import sens as S
    from boxfusion_amd.evaluation import read_ply_points as eval_points
    from boxfusion_amd.synthetic import frame_rgbd
    from boxfusion_amd.visualize import read_ply_points
    HC, WC, HD, WD, n = 96, 128, 48, 64, 5
    colors = [U.jpeg_bytes(frame_rgbd(i * 3, HC, WC)[0], quality=90) for i in range(n)]
    v, u = np.mgrid[:HD, :WD]
    depths = [(1000.0 * (1.0 + 0.004 * u + 0.002 * v + 0.01 * i)).astype(np.uint16) for i in range(n)]
    poses = [U.LOST if i == 2 else U.upright_pose((0.05 * i, 0.1, 1.2)) for i in range(n)]
    Kd = np.eye(4, dtype=np.float32)
    Kd[:2, :3] = [[57.8, 0, 31.5], [0, 57.8, 23.5]]
    path = tmp_path / "scene.sens"
    U.write_sens(path, colors, depths, poses, (HC, WC), intrinsic_depth=Kd)
    out = tmp_path / "out" / "mesh.ply"
    assert S.main(["mesh", str(path), str(out), "--voxel", "0.05", "--trunc-voxels", "3", "--max-depth", "4",
                   "--capacity", "1024"]) == 0
    with S.SensFile(path) as f:
        vol = S.mesh(f, voxel=0.05, trunc_voxels=3, max_depth=4.0, capacity=1024, batch=2)
    st = vol.stats()
    assert st["skipped_pose"] == 1 and st["observations"] > 1000 and st["dropped_full"] == 0
    verts, rgb, faces = [t.cpu().numpy() for t in vol.mesh()]
    assert len(verts) > 200 and len(faces) > 200
    got_xyz, got_rgb = read_ply_points(str(out))
    np.testing.assert_array_equal(got_xyz, verts)
    np.testing.assert_array_equal(got_rgb, rgb)
    np.testing.assert_array_equal(eval_points(str(out)), verts.astype(np.float64))
    printed = capsys.readouterr().out
    assert f"{len(verts)} vertices, {len(faces)} faces -> {out}" in printed and f"observations={st['observations']}" in printed


def test_scene_mesh_command_and_filter(L, small, tmp_path, capsys):
    """a CA-1M sequence directory written here -> mesh.ply -> evaluation filter reads it"""
    from boxfusion_amd import evaluation as E
    from boxfusion_amd import scene_mesh as M
    sc, seq = small["scene"], tmp_path / "seq"
    (seq / "depth").mkdir(parents=True)
    (seq / "rgb").mkdir()
    scales = np.array([1.0, 2.0, 1.0, 0.5, 1.0, 1.25])                           # K_scales.npy: depth *= 1 / scale
    mm = [np.rint(d * 1000.0 * k).astype(np.uint16) for d, k in zip(small["depths"], scales)]
    np.save(seq / "K_scales.npy", scales)
    for i, (d, im) in enumerate(zip(mm, small["big"])):
        Image.fromarray(d).save(seq / "depth" / f"{i}.png")
        Image.fromarray(im).save(seq / "rgb" / f"{i}.png")
    np.savetxt(seq / "K_depth.txt", sc.K)
    np.save(seq / "all_poses.npy", np.stack(small["poses"]))
    on = sc.centre + sc.radius * np.array([0.0, 0.0, 1.0])                       # a box on the sphere, one far outside
    corners = lambda c, h: (c + h * (2.0 * R.CORNERS - 1.0)).tolist()            # noqa: E731
    (seq / "instances.json").write_text(json.dumps([{"corners": corners(on, 0.1)},
                                                    {"corners": corners(sc.centre + 5.0, 0.1)}]))
    assert M.main([str(seq), "--voxel", str(VOXEL), "--trunc-voxels", str(T), "--max-depth", str(MAX_DEPTH),
                   "--capacity", "1024"]) == 0
    vol = _volume()
    metres = [((m.astype(np.float32) / np.float32(1000.0)).astype(np.float64) * (1.0 / k)).astype(np.float32)
              for m, k in zip(mm, scales)]
    _feed(vol, sc, metres, small["poses"], list(small["big"]))
    verts, rgb, faces = [t.cpu().numpy() for t in vol.mesh()]
    from boxfusion_amd.visualize import read_ply_points
    got_xyz, got_rgb = read_ply_points(str(seq / "mesh.ply"))
    np.testing.assert_array_equal(got_xyz, verts)
    np.testing.assert_array_equal(got_rgb, rgb)
    printed = capsys.readouterr().out
    assert f"6 frames -> {len(verts)} vertices, {len(faces)} faces" in printed and "observations=" in printed
    assert "K_scales.npy" in printed
    (seq / "rgb" / "5.png").unlink()                         # rgb/ and depth/ no longer pair up
    with pytest.raises(SystemExit):
        M.main([str(seq)])
    with pytest.raises(ValueError):
        M.fuse_sequence(str(seq), vol)
    Image.fromarray(small["big"][5]).save(seq / "rgb" / "5.png")
    assert E.main(["filter", str(seq)]) == 0
    kept = np.load(seq / "after_filter_boxes.npy")
    assert kept.shape == (1, 8, 3)


class _Fusion:
    """Pipeline.run's fusion side: keeps what the detect stage handed over"""
    all_pred_box = None

    def __init__(self):
        self.got = []

    def keyframe(self, i, pose, preds):
        self.got.append((i, preds))

    def finish(self, *a, **k):
        pass


N_FRAMES, GAP, BATCH = 7, 3, 2


@pytest.fixture(scope="module")
def pipe(L):
    from boxfusion_amd.clip import VisionTransformer
    from boxfusion_amd.cubify_transformer import make_cubify_transformer
    from boxfusion_amd.pipeline import DetectStage
    from boxfusion_amd.synthetic import SCANNET_K, Scene, frame_rgbd
    from tests import trace_util as TU
    torch.manual_seed(0)
    with torch.device(DEV):
        cutr = make_cubify_transformer(192, True).eval()
        vis = VisionTransformer(224, 14, 1280, 2, 16, 1024).eval()
    det = DetectStage(cutr, vis, TU.SCANNET_CFG, BATCH, 480, 640, SCANNET_K, crop_source="top", crops_per_frame=4,
                      clip_capacity=8, device=DEV)
    scene = Scene(seed=0)
    host = {i: frame_rgbd(i) for i in range(N_FRAMES)}

    def frames(ids):
        return (torch.from_numpy(np.stack([host[i][0] for i in ids])).to(DEV),
                torch.from_numpy(np.stack([host[i][1] for i in ids])).to(DEV), np.stack([scene.pose(i) for i in ids]))
    return dict(det=det, frames=frames, host=host, scene=scene, K=SCANNET_K)


def _flat(x):
    if torch.is_tensor(x):
        return [x.detach().cpu()]
    if isinstance(x, dict):
        return [t for k in sorted(x) for t in _flat(x[k])]
    if isinstance(x, (list, tuple)):
        return [t for v in x for t in _flat(v)]
    if hasattr(x, "__dict__"):
        return _flat(vars(x))
    return [torch.as_tensor(np.asarray(x))] if isinstance(x, (np.ndarray, int, float)) else []


@pytest.mark.parametrize("which", ["keyframes", "all"])
def test_pipeline_mesh(L, pipe, which):
    from boxfusion_amd.pipeline import Pipeline
    plain = _Fusion()
    Pipeline(pipe["det"], plain, GAP).run(pipe["frames"], N_FRAMES)
    fused = _Fusion()
    vol = _volume(capacity=1 << 13, voxel=0.08, trunc=3, max_depth=10.0)
    Pipeline(pipe["det"], fused, GAP).run(pipe["frames"], N_FRAMES, mesh=vol, mesh_frames=which)
    ids = [i for i in range(N_FRAMES) if which == "all" or i % GAP == 0]
    want = _volume(capacity=1 << 13, voxel=0.08, trunc=3, max_depth=10.0)
    for i in ids:
        rgb, depth = pipe["host"][i]
        want.integrate(_dev(depth), pipe["K"], pipe["scene"].pose(i), _dev(rgb))
    assert vol.stats()["observations"] > 0 and want.stats()["saturated"] == 0 and want.stats()["dropped_full"] == 0
    for a, b in zip(vol.raw(), want.raw()):
        assert torch.equal(a, b)
    # the boxes handed to fusion do not depend on mesh=
    assert [i for i, _ in plain.got] == [i for i, _ in fused.got] == [i for i in range(N_FRAMES) if i % GAP == 0]
    for (_, a), (_, b) in zip(plain.got, fused.got):
        fa, fb = _flat(a), _flat(b)
        assert len(fa) == len(fb) > 0
        for x, y in zip(fa, fb):
            assert torch.equal(x, y)
    with pytest.raises(ValueError):
        Pipeline(pipe["det"], _Fusion(), GAP).run(pipe["frames"], N_FRAMES, mesh=vol, mesh_frames="some")
    with pytest.raises(ValueError):
        Pipeline(pipe["det"], _Fusion(), GAP).run(pipe["frames"], N_FRAMES, mesh=vol, mesh_frames="all", per_frame=False)


def test_pipeline_mesh_depth_ratio(L):
    """a CA-1M-shaped stage (depth at half the image's resolution): the mesh is fused with the depth
    map's intrinsics, the image's at 1/2, and equals a volume fed with them directly"""
    from boxfusion_amd.clip import VisionTransformer
    from boxfusion_amd.cubify_transformer import make_cubify_transformer
    from boxfusion_amd.pipeline import DetectStage, Pipeline
    from boxfusion_amd.synthetic import Scene
    from tests import trace_util as TU
    K = np.array([[360.0, 0.0, 191.5], [0.0, 360.0, 255.5], [0.0, 0.0, 1.0]], np.float32)
    B, H, W, n = 2, 512, 384, 4
    torch.manual_seed(0)
    with torch.device(DEV):
        cutr = make_cubify_transformer(192, True).eval()
        vis = VisionTransformer(224, 14, 1280, 2, 16, 1024).eval()
    det = DetectStage(cutr, vis, TU.SCANNET_CFG, B, H, W, K, crop_source="top", crops_per_frame=4, clip_capacity=8,
                      device=DEV, depth_ratio=2)
    scene = Scene(seed=0)
    rng = np.random.default_rng(2)
    v, u = np.mgrid[:H // 2, :W // 2].astype(np.float32)
    host = {i: (rng.integers(0, 256, (H, W, 3), dtype=np.uint8),
                (1.6 + 0.3 * np.sin(u / 40.0 + i) * np.cos(v / 50.0)).astype(np.float32)) for i in range(n)}

    def frames(ids):
        return (_dev(np.stack([host[i][0] for i in ids])), _dev(np.stack([host[i][1] for i in ids])),
                np.stack([scene.pose(i) for i in ids]))
    kw = dict(capacity=1 << 12, voxel=0.05, trunc=3, max_depth=10.0)
    vol = _volume(**kw)
    Pipeline(det, _Fusion(), 1).run(frames, n, mesh=vol)
    Kd = K.copy()
    Kd[:2] /= 2
    want, wrong = _volume(**kw), _volume(**kw)
    for i in range(n):
        want.integrate(_dev(host[i][1]), Kd, scene.pose(i), _dev(host[i][0]))
        wrong.integrate(_dev(host[i][1]), K, scene.pose(i), _dev(host[i][0]))
    assert want.stats()["observations"] > 10000 and want.stats()["dropped_full"] == 0
    for a, b in zip(vol.raw(), want.raw()):
        assert torch.equal(a, b)
    assert vol.stats() == want.stats()
    assert not torch.equal(want.raw()[0], wrong.raw()[0])    # the image's K would give another volume
