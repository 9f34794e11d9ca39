"""The coloured scene point cloud on the GPU: bf_resize_bicubic_u8 against Pillow, bf_cloud_pack
against the reference's expression (demo.py:124-127), the voxel map (bf_cloud_integrate /
bf_cloud_extract, SceneCloud) against integer sums grouped in numpy, its independence of the order
of arrival, its behaviour when the table is full, and the plumbing into Pipeline.run, FrameLogger and
`python -m boxfusion_amd.sens cloud`."""
import numpy as np
import pytest
import torch
from PIL import Image

from tests import sens_util as U

pytestmark = pytest.mark.gpu

VOXEL = 0.02
FINE = np.float32(VOXEL / 256.0)


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from boxfusion_amd import _lib
    _lib.lib()
    return _lib


DEV = "cuda"


# ---- (a) bicubic ---------------------------------------------------------------------------------
def pil_resize(imgs, H, W):
    return np.stack([np.array(Image.fromarray(im).resize((W, H))) for im in imgs])


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("src,dst", [((48, 64), (24, 32)), ((48, 64), (12, 16)), ((48, 64), (48, 32)),
                                     ((64, 48), (32, 24)), ((40, 56), (13, 19)), ((24, 32), (48, 64))])
def test_bicubic_vs_pillow(L, src, dst, batch):
    rng = np.random.default_rng(src[0] * 100 + dst[0] + batch)
    imgs = rng.integers(0, 256, (batch, *src, 3), dtype=np.uint8)
    got = L.resize_bicubic_u8(torch.from_numpy(imgs).to(DEV), *dst)
    assert got.shape == (batch, *dst, 3) and got.dtype == torch.uint8
    assert torch.equal(got.cpu(), torch.from_numpy(pil_resize(imgs, *dst)))


@pytest.mark.parametrize("src,dst", [((48, 64), (24, 32)), ((40, 56), (13, 19)), ((24, 32), (48, 64))])
def test_bicubic_clip_ends(L, src, dst):
    """a constant 255 image and a 0 / 255 checkerboard: the overshoot of the negative lobes is
    clipped at both ends as Pillow clips it"""
    yy, xx = np.mgrid[:src[0], :src[1]]
    board = (((yy + xx) % 2) * 255).astype(np.uint8)[..., None].repeat(3, -1)
    blocks = ((((yy // 3) + (xx // 5)) % 2) * 255).astype(np.uint8)[..., None].repeat(3, -1)
    imgs = np.stack([np.full((*src, 3), 255, np.uint8), board, blocks])
    got = L.resize_bicubic_u8(torch.from_numpy(imgs).to(DEV), *dst)
    assert torch.equal(got.cpu(), torch.from_numpy(pil_resize(imgs, *dst)))
    one = L.resize_bicubic_u8(torch.from_numpy(imgs[2]).to(DEV), *dst)          # [H,W,3]: a batch of one
    assert torch.equal(one.cpu(), torch.from_numpy(pil_resize(imgs[2:], *dst)[0]))


# ---- (b) pack ------------------------------------------------------------------------------------
def _depth_batch(H, W, seed):
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.3, 6.0, (3, H, W)).astype(np.float32)
    d[0][rng.random((H, W)) < 0.2] = 0.0            # holes
    d[0][rng.random((H, W)) < 0.1] = 12.0           # beyond max_depth
    d[0, 0, 0] = 10.0                               # exactly max_depth: not valid
    d[0, H // 2, W // 3] = np.nan
    d[1] = 0.0                                      # a frame with no valid pixel
    return d                                        # frame 2: every pixel valid


@pytest.mark.parametrize("hw", [(13, 19), (24, 32)])
def test_pack_vs_reference_expression(L, hw):
    from boxfusion_amd.scene_cloud import frame_cloud
    from boxfusion_amd.tools_utils import unproject
    H, W = hw
    depth = _depth_batch(H, W, H)
    K = np.array([[0.9 * W, 0, W / 2 - 0.5], [0, 0.9 * W, H / 2 - 0.5], [0, 0, 1]], np.float32)
    poses = [U.upright_pose((0.1 * b, -0.2, 1.3)) for b in range(3)]
    got = [unproject(torch.from_numpy(depth[b]).to(DEV), K, poses[b], max_depth=10.0) for b in range(3)]
    xyz = torch.stack([g[0] for g in got])
    valid = torch.stack([g[1] for g in got])
    xyz_h, valid_h = xyz.cpu(), valid.cpu()
    counts = valid_h.flatten(1).sum(1).tolist()
    assert counts[1] == 0 and counts[2] == H * W and 0 < counts[0] < H * W
    rng = np.random.default_rng(7)
    for ih, iw in ((H, W), (2 * H, 2 * W), (4 * H, 4 * W), (40, 56)):
        imgs = rng.integers(0, 256, (3, ih, iw, 3), dtype=np.uint8)
        rows, offsets = frame_cloud(xyz, valid, torch.from_numpy(imgs).to(DEV))
        assert offsets.dtype == torch.int32 and offsets.cpu().tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
        want = []
        for b in range(3):     # demo.py:124-127
            matched = torch.tensor(np.array(Image.fromarray(imgs[b]).resize((W, H))))
            want.append(torch.cat((xyz_h[b], matched / 255.0), dim=-1)[valid_h[b]])
        want = torch.cat(want)
        assert rows.dtype == torch.float32 and rows.shape == want.shape
        # NaN-free by construction (a NaN depth is not valid), so equal means bit-equal up to +-0
        assert torch.equal(rows.cpu(), want)
    # [H,W,...] inputs are a batch of one
    rows1, off1 = frame_cloud(xyz[0], valid[0], torch.from_numpy(imgs[0]).to(DEV))
    assert off1.cpu().tolist() == [0, counts[0]] and torch.equal(rows1.cpu(), want[:counts[0]])


# ---- (c) / (d) the voxel map ---------------------------------------------------------------------
def np_voxels(xyz, valid, rgb):
    """the map's contents by numpy: f32 floor(x / fine_step), int64 sums grouped by np.unique ->
    dict(key, count, sums [n,6], n_nonfinite, n_out_of_range)"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    rgb = np.asarray(rgb, np.uint8).reshape(-1, 3)
    valid = np.asarray(valid, bool).reshape(-1)
    fin = np.isfinite(xyz).all(1)
    with np.errstate(all="ignore"):
        f = np.floor(xyz / FINE)
    assert f.dtype == np.float32
    lim = np.float32(2.0 ** 28)
    inr = ((f >= -lim) & (f < lim)).all(1)
    use = valid & fin & inr
    fi = np.where(use[:, None], f, 0).astype(np.int64)
    idx, q = fi >> 8, fi & 255
    key = ((idx[:, 0] + (1 << 20)) << 42) | ((idx[:, 1] + (1 << 20)) << 21) | (idx[:, 2] + (1 << 20))
    uniq, inv = np.unique(key[use], return_inverse=True)
    vals = np.concatenate([q, rgb.astype(np.int64)], 1)[use]
    sums = np.zeros((len(uniq), 6), np.int64)
    np.add.at(sums, inv, vals)
    return dict(key=uniq, count=np.bincount(inv, minlength=len(uniq)).astype(np.int64), sums=sums,
                n_nonfinite=int((valid & ~fin).sum()), n_out_of_range=int((valid & fin & ~inr).sum()))


def np_points(ref):
    idx = np.stack([(ref["key"] >> 42) & 0x1FFFFF, (ref["key"] >> 21) & 0x1FFFFF, ref["key"] & 0x1FFFFF], 1) - (1 << 20)
    c = ref["count"][:, None]
    xyz = (idx * 256 + ref["sums"][:, :3] / c + 0.5) * float(FINE)
    return xyz, (ref["sums"][:, 3:] + c // 2) // c


def _points(seed=0):
    """~20 000 points in +-3 m: clusters of 1-8 consecutive points a few millimetres apart (runs of
    equal voxels in adjacent lanes, and many duplicates), points exactly on voxel boundaries, exact
    repeats, invalid pixels, NaN / inf and one point beyond the index range"""
    rng = np.random.default_rng(seed)
    centers = rng.uniform(-3, 3, (4000, 3))
    reps = rng.integers(1, 9, 4000)
    cl = np.repeat(centers, reps, 0) + rng.uniform(-0.004, 0.004, (reps.sum(), 3))
    k = rng.integers(-150, 150, (1500, 3))
    on_edge = (k.astype(np.float32) * np.float32(VOXEL)).astype(np.float32)      # k * voxel in f32
    on_edge[::3, 1] += np.float32(0.007)
    xyz = np.concatenate([cl.astype(np.float32), on_edge, cl[:800].astype(np.float32)])
    xyz = xyz[np.concatenate([np.arange(len(cl)), rng.permutation(len(xyz) - len(cl)) + len(cl)])]
    bad = rng.choice(len(xyz), 7, replace=False)
    xyz[bad[0], 0] = np.nan
    xyz[bad[1], 2] = np.nan
    xyz[bad[2], 1] = np.inf
    xyz[bad[3], 0] = -np.inf
    xyz[bad[4]] = (3.0e4, 0.0, 0.0)                  # index 1.5e6 > 2^20
    xyz[bad[5]] = (0.0, -2.2e4, 1.0)
    xyz[bad[6]] = (1.0, 1.0, 3.0e38)
    rgb = rng.integers(0, 256, (len(xyz), 3), dtype=np.uint8)
    valid = rng.random(len(xyz)) > 0.1
    valid[bad] = True
    assert 18000 < len(xyz) < 24000 and (xyz[:, 0] < 0).any()
    return xyz, valid, rgb


def _cloud(capacity, merge=True):
    from boxfusion_amd.scene_cloud import SceneCloud
    return SceneCloud(voxel=VOXEL, capacity=capacity, device=DEV, merge=merge)


def _feed(sc, xyz, valid, rgb):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    sc.integrate(t(xyz)[:, None], t(valid)[:, None], t(rgb)[:, None])       # [n,1,...]: one frame of n x 1 pixels


@pytest.fixture(scope="module")
def cloud_ref(L):
    xyz, valid, rgb = _points()
    return dict(xyz=xyz, valid=valid, rgb=rgb, ref=np_voxels(xyz, valid, rgb))


@pytest.mark.parametrize("merge", [True, False])
def test_integrate_vs_numpy(L, cloud_ref, merge):
    d, ref = cloud_ref, cloud_ref["ref"]
    assert 4 * len(ref["key"]) <= 1 << 17 and (ref["count"] > 1).sum() > 1000
    sc = _cloud(1 << 17, merge)
    _feed(sc, d["xyz"], d["valid"], d["rgb"])
    key, count, sums = [t.cpu().numpy() for t in sc.raw()]
    np.testing.assert_array_equal(key, ref["key"])
    np.testing.assert_array_equal(count, ref["count"])
    np.testing.assert_array_equal(sums, ref["sums"])
    st = sc.stats()
    assert st["nonfinite"] == ref["n_nonfinite"] == 4 and st["out_of_range"] == ref["n_out_of_range"] == 3
    assert st["stored"] + st["nonfinite"] + st["out_of_range"] == int(d["valid"].sum())
    assert st["stored"] == int(ref["count"].sum()) and st["dropped_full"] == 0 and st["saturated"] == 0
    # the run merge issues fewer sets of adds for the same contents; without it, one per stored point
    assert (st["runs"] < st["stored"]) if merge else (st["runs"] == st["stored"])
    xyz, rgb, cnt = sc.points()
    want_xyz, want_rgb = np_points(ref)
    assert xyz.dtype == torch.float32 and rgb.dtype == torch.uint8 and cnt.dtype == torch.int32
    np.testing.assert_array_equal(rgb.cpu().numpy(), want_rgb)
    np.testing.assert_array_equal(cnt.cpu().numpy(), ref["count"])
    np.testing.assert_allclose(xyz.cpu().numpy(), want_xyz, rtol=0, atol=4e-6)
    # every stored mean lies inside its voxel
    lo = np.floor(want_xyz / VOXEL)
    assert (np.abs(xyz.cpu().numpy().astype(np.float64) / VOXEL - (lo + 0.5)) <= 0.5 + 1e-3).all()


def test_integrate_order_independent(L, cloud_ref):
    d = cloud_ref
    n = len(d["xyz"])
    perm = np.random.default_rng(5).permutation(n)
    cuts = [0, n // 5, n // 2 + 13, n]

    def one_call(sc):
        _feed(sc, d["xyz"], d["valid"], d["rgb"])

    def three_calls(sc):
        for a, b in zip(cuts[:-1], cuts[1:]):
            _feed(sc, d["xyz"][a:b], d["valid"][a:b], d["rgb"][a:b])

    def permuted(sc):
        _feed(sc, d["xyz"][perm], d["valid"][perm], d["rgb"][perm])

    outs = []
    for feed in (one_call, one_call, three_calls, permuted):
        sc = _cloud(1 << 17)
        feed(sc)
        outs.append([t.cpu() for t in sc.raw() + sc.points()])
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert a.dtype == b.dtype and torch.equal(a, b)
    sc.reset()                                       # reset() empties the map and the counters
    assert sc.points()[0].shape == (0, 3) and sc.stats()["stored"] == 0
    one_call(sc)
    assert torch.equal(sc.raw()[2].cpu(), outs[0][2])


def test_full_table_ends_cleanly(L):
    """capacity 64 and ~200 distinct voxels: the call returns, a voxel is kept whole or not at all,
    and every point is accounted for"""
    rng = np.random.default_rng(3)
    centers = (rng.integers(-40, 40, (200, 3)) + 0.5) * VOXEL
    xyz = (np.repeat(centers, 6, 0) + rng.uniform(-0.008, 0.008, (1200, 3))).astype(np.float32)
    xyz = xyz[rng.permutation(len(xyz))]
    rgb = rng.integers(0, 256, (len(xyz), 3), dtype=np.uint8)
    valid = rng.random(len(xyz)) > 0.05
    ref = np_voxels(xyz, valid, rgb)
    assert 150 < len(ref["key"]) <= 200
    sc = _cloud(64)
    half = len(xyz) // 2
    _feed(sc, xyz[:half], valid[:half], rgb[:half])
    _feed(sc, xyz[half:], valid[half:], rgb[half:])
    key, count, sums = [t.cpu().numpy() for t in sc.raw()]
    st = sc.stats()
    assert 0 < len(key) <= 64
    assert st["stored"] == int(count.sum()) and st["stored"] + st["dropped_full"] == int(valid.sum())
    assert st["dropped_full"] > 0 and st["nonfinite"] == st["out_of_range"] == st["saturated"] == 0
    pos = np.searchsorted(ref["key"], key)
    np.testing.assert_array_equal(ref["key"][pos], key)
    np.testing.assert_array_equal(count, ref["count"][pos])
    np.testing.assert_array_equal(sums, ref["sums"][pos])


# ---- pipeline ------------------------------------------------------------------------------------
class _NoFusion:
    """Pipeline.run's fusion side, not under test here"""
    all_pred_box = None

    def keyframe(self, *a, **k):
        pass

    def finish(self, *a, **k):
        pass


N_FRAMES, GAP, BATCH = 7, 3, 2


@pytest.fixture(scope="module")
def pipe(L):
    from boxfusion_amd.clip import VisionTransformer
    from boxfusion_amd.cubify_transformer import make_cubify_transformer
    from boxfusion_amd.pipeline import DetectStage, Pipeline
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
    return dict(pipe=Pipeline(det, _NoFusion(), GAP), frames=frames, host=host, scene=scene, K=SCANNET_K)


def _by_hand(p, ids):
    """(xyz, valid, rgb) of frames ids through tools_utils.unproject, as demo.py:123-126"""
    from boxfusion_amd.tools_utils import unproject
    out = []
    for i in ids:
        rgb, depth = p["host"][i]
        xyz, valid = unproject(torch.from_numpy(depth).to(DEV), p["K"], p["scene"].pose(i), max_depth=10.0)
        out.append((xyz, valid, torch.from_numpy(rgb).to(DEV)))
    return out


@pytest.mark.parametrize("which", ["keyframes", "all"])
def test_pipeline_cloud(L, pipe, which):
    ids = [i for i in range(N_FRAMES) if which == "all" or i % GAP == 0]
    # the synthetic depth is random per pixel, so nearly every point is a voxel of its own: 7 frames
    # are ~2 M voxels, and the default capacity (2^22) holds them all
    sc = _cloud(1 << 22)
    pipe["pipe"].run(pipe["frames"], N_FRAMES, cloud=sc, cloud_frames=which)
    want = _cloud(1 << 22)
    for xyz, valid, rgb in _by_hand(pipe, ids):
        want.integrate(xyz, valid, rgb)
    assert want.stats()["stored"] > 100000 * len(ids)
    for a, b in zip(sc.points(), want.points()):
        assert torch.equal(a, b)
    st, sw = sc.stats(), want.stats()              # but for the runs, which the batching may cut elsewhere
    assert sw["dropped_full"] == 0
    assert {k: v for k, v in st.items() if k != "runs"} == {k: v for k, v in sw.items() if k != "runs"}


def _records(rec, skip=None):
    out = []
    for path, t, kind, a in rec.records:
        if path == skip:
            continue
        out.append((path, t, kind, {k: (np.asarray(v).tolist() if isinstance(v, np.ndarray) else
                                        [np.asarray(x).tolist() for x in v] if isinstance(v, list) else v)
                                    for k, v in a.items()}))
    return out


def test_pipeline_viz_points_and_defaults(L, pipe):
    from boxfusion_amd.scene_cloud import frame_cloud
    from boxfusion_amd.visualize import FrameLogger, Recording

    def run(**kw):
        rec = Recording(forward=False)
        viz = FrameLogger(rec, pipe["K"], (640, 480), K_depth=pipe["K"], depth_size=(640, 480), fps=1.0,
                          log_images=False)
        pipe["pipe"].run(pipe["frames"], N_FRAMES, viz=viz, **kw)
        return rec
    plain = run()
    assert not [r for r in plain.records if r[0] == "/world/xyz"]
    assert _records(plain) == _records(run(cloud=None, cloud_frames="keyframes", viz_points=False))
    rec = run(viz_points=True)
    pts = [(t, a) for p_, t, k, a in rec.records if p_ == "/world/xyz"]
    assert len(pts) == N_FRAMES and all(k == "Points3D" for p_, _, k, _ in rec.records if p_ == "/world/xyz")
    assert [t[1] for t, _ in pts] == [float(i) for i in range(N_FRAMES)]          # one per frame, in frame order
    for (t, a), (xyz, valid, rgb) in zip(pts, _by_hand(pipe, range(N_FRAMES))):
        rows = frame_cloud(xyz, valid, rgb)[0].cpu().numpy()
        np.testing.assert_array_equal(a["positions"], rows[:, :3])
        np.testing.assert_array_equal(a["colors"], rows[:, 3:])
    # the other records are the default run's, in its order
    assert _records(plain) == _records(rec, skip="/world/xyz")
    with pytest.raises(ValueError):
        pipe["pipe"].run(pipe["frames"], N_FRAMES, cloud=_cloud(64), cloud_frames="some")


# ---- sens cloud ----------------------------------------------------------------------------------
def test_sens_cloud_command(L, tmp_path, capsys):
    from boxfusion_amd import sens as S
    from boxfusion_amd.synthetic import frame_rgbd
    from boxfusion_amd.tools_utils import unproject
    from boxfusion_amd.visualize import read_ply_points
    HC, WC, HD, WD, n = 96, 128, 48, 64, 5
    colors = [U.jpeg_bytes(frame_rgbd(i * 3, HC, WC)[0], quality=90) for i in range(n)]
    depths = [np.clip(frame_rgbd(i * 3, HD, WD)[1] * 1000.0, 0, 65535).astype(np.uint16) for i in range(n)]
    poses = [U.LOST if i == 2 else U.upright_pose((0.05 * i, 0.1, 1.2)) for i in range(n)]
    Kd = np.eye(4, dtype=np.float32)
    Kd[:2, :3] = [[57.8, 0, 31.5], [0, 57.8, 23.5]]
    path = tmp_path / "scene.sens"
    U.write_sens(path, colors, depths, poses, (HC, WC), intrinsic_depth=Kd)
    out = tmp_path / "out" / "scene.ply"
    assert S.main(["cloud", str(path), str(out), "--voxel", "0.05", "--start", "1", "--max-depth", "4"]) == 0
    from boxfusion_amd.scene_cloud import SceneCloud
    sc = SceneCloud(voxel=0.05, capacity=1 << 16, device=DEV)
    with S.SensFile(path) as f:
        for s in S.SensFrameStream(f, batch=2, start=1):
            gt = s["sensor_info"].gt
            xyz, valid = unproject(s["wide"]["depth"][-1], gt.depth.K[-1], gt.RT[-1], max_depth=4.0)
            sc.integrate(xyz, valid, s["wide"]["image"][-1].permute(1, 2, 0).contiguous())
    xyz, rgb, _ = sc.points()
    assert xyz.shape[0] > 500
    got_xyz, got_rgb = read_ply_points(str(out))
    np.testing.assert_array_equal(got_xyz, xyz.cpu().numpy())
    np.testing.assert_array_equal(got_rgb, rgb.cpu().numpy())
    printed = capsys.readouterr().out
    assert f"{xyz.shape[0]} points -> {out}" in printed and f"stored={sc.stats()['stored']}" in printed
