"""The tracker's photometric term on the GPU (bf_grey_u8, bf_photo_reduce, tracking.IcpTracker with an image) against
the numpy restatement in tests/photo_ref.py: the intensity bit for bit, the sums within the gap two summation orders
can have, the tracker along the textured wall (which the geometry alone cannot place) and the room, and `sens track
--photometric` on a capture of the wall.  The reference numbers are those of test_photo_host.py."""
import ctypes

import numpy as np
import pytest
import torch

from tests import mesh_ref as R
from tests import photo_ref as P
from tests import sens_util as U
from tests import track_ref as TR

pytestmark = pytest.mark.gpu

DEV = "cuda"
RV = TR.ROOM_VOLUME
JPEG_QUALITY = 90       # sens_util's default: the restatement on images through it stays at 0.34 mm and 0.031 degrees on the wall


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from boxfusion_amd import _lib
    _lib.lib()
    return _lib


def _volume(capacity=1 << 11):
    from boxfusion_amd.scene_mesh import TsdfVolume
    return TsdfVolume(voxel=RV["voxel"], trunc_voxels=RV["T"], capacity=capacity, max_depth=RV["max_depth"], device=DEV)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- 1. the intensity --------------------------------------------------------------------------------------------
def test_grey_u8_is_the_restatement(L):
    rng = np.random.default_rng(5)
    one, two = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8), rng.integers(0, 256, (2, 37, 53, 3), dtype=np.uint8)
    one[0, :3] = [[255, 255, 255], [0, 0, 0], [255, 0, 255]]
    for rgb in (one, two):
        got = L.grey_u8(_dev(rgb))
        want = P.grey(rgb)
        assert got.dtype == torch.float32 and tuple(got.shape) == rgb.shape[:-1]
        assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
    with pytest.raises(L.HipError):
        L.grey_u8(_dev(one[..., :2]))
    with pytest.raises(L.HipError):
        L.grey_u8(_dev(one).float())
    p, i = ctypes.c_void_p, ctypes.c_int
    src, dst = _dev(one), torch.zeros((37, 53), dtype=torch.float32, device=DEV)
    f = L.lib().bf_grey_u8
    assert f(p(None), i(1), i(37), i(53), p(dst.data_ptr()), L._stream()) == -1
    assert f(p(src.data_ptr()), i(1), i(37), i(53), p(None), L._stream()) == -1
    assert f(p(src.data_ptr()), i(0), i(37), i(53), p(dst.data_ptr()), L._stream()) == -1
    assert f(p(src.data_ptr()), i(1), i(-1), i(53), p(dst.data_ptr()), L._stream()) == -1
    assert f(p(src.data_ptr()), i(1), i(1 << 15), i(1 << 15), p(dst.data_ptr()), L._stream()) == -3
    torch.cuda.synchronize()
    assert not dst.any()


# ---- 2. the reduction --------------------------------------------------------------------------------------------
def _photo_case(H, W):
    """a live frame and a reference frame of the textured room at H x W, from the restatement: holes in the reference
    depth and a patch of another depth there, a band of invalid live depth, a white patch and salt in the live image, an
    estimate 3 degrees and 5 cm off"""
    room = TR.Room()
    K = room.K.copy()
    K[0] *= W / room.W
    K[1] *= H / room.H
    rng = np.random.default_rng(H)
    dr = room.depth(room.poses[2], H, W, K)
    ir = P.grey(P.render_texture(room.poses[2], K, dr))
    dr[rng.random((H, W)) < 0.1] = 0.0
    dr[5, 7] = np.nan
    dr[H // 2:H - 6, W // 2:W - 8] += 1.0                   # something that stood nearer when the reference was taken
    depth = room.depth(room.poses[3], H, W, K)
    rgb = P.render_texture(room.poses[3], K, depth)
    rgb[24:32, 16:40] = 255
    rgb[rng.random((H, W)) < 0.03] = 0
    depth[10:14] = 0.0
    depth[20, 5] = np.nan
    lv, _ = TR.vertex_normal(depth, K, RV["max_depth"], 0.15)
    T = TR.perturb(room.poses[3], 3.0, 0.05, seed=1).astype(np.float64)[:3]
    return dict(K=K, lv=lv, il=P.grey(rgb), ir=ir, dr=dr, T=T, M=TR.w2c(room.poses[2]))


def _assert_sums(L, c, stride, T, lv=None):
    lv = c["lv"] if lv is None else lv
    terms, n_s = P.photo_terms(lv, c["il"], stride, T, c["ir"], c["dr"], c["M"], c["K"], 0.6, 0.3)
    want = TR.icp_sums(terms)
    args = (_dev(lv), _dev(c["il"]), stride, T, _dev(c["ir"]), _dev(c["dr"]), c["M"], R.intrinsics(c["K"]), 0.6, 0.3)
    a = L.photo_reduce(*args).cpu().numpy()
    b = L.photo_reduce(*args).cpu().numpy()
    assert a.tobytes() == b.tobytes()                           # the same bits on every run
    assert a[28] == want[28] and not a[29:].any() and np.isfinite(a).all()
    bound = max(len(terms) - 1, 0) * 2.0 ** -52 * np.abs(terms).sum(0)
    gap = np.abs(a[:28] - want[:28])
    assert (gap <= bound).all(), (stride, gap / np.maximum(bound, 1e-300))
    return a, n_s


@pytest.mark.parametrize("H,W", [(48, 64), (37, 53)])
def test_photo_reduce_vs_restatement(L, H, W):
    c = _photo_case(H, W)
    for stride in (1, 2, 4):
        a, n_s = _assert_sums(L, c, stride, c["T"])
        assert n_s == -(-H // stride) * -(-W // stride) and 0.2 * n_s < a[28] < 0.8 * n_s
        # each gate is at work in this case: without it the count is larger
        for over in (dict(dr=np.where(c["dr"] > 0, c["dr"], 1.0)), dict(il=c["ir"]), dict(dist_max=1e9)):
            k = {**c, **{k: v for k, v in over.items() if k != "dist_max"}}
            more, _ = P.photo_terms(k["lv"], k["il"], stride, c["T"], k["ir"], k["dr"], c["M"], c["K"],
                                    over.get("dist_max", 0.6), 0.3 if "il" not in over else 1e9)
            assert len(more) > a[28], over.keys()
    # nothing valid: the count and every sum are exactly zero
    zv, _ = TR.vertex_normal(np.zeros((H, W), np.float32), c["K"], RV["max_depth"], 0.15)
    a, _ = _assert_sums(L, c, 1, c["T"], lv=zv)
    assert not a.any()
    # a live frame wholly outside the reference: turned half round
    away = c["T"].copy()
    away[:, :3] = away[:, :3] @ np.diag([-1.0, 1.0, -1.0])
    a, _ = _assert_sums(L, c, 1, away)
    assert not a.any()
    # and one that looks past its edge: every pixel projects beyond the last column
    aside = c["T"].copy()
    aside[:, :3] = aside[:, :3] @ R.rotation(1, 80.0)
    _assert_sums(L, c, 1, aside)


def test_photo_reduce_arguments(L):
    c = _photo_case(37, 53)
    t = dict(lv=_dev(c["lv"]), il=_dev(c["il"]), ir=_dev(c["ir"]), dr=_dev(c["dr"]),
             partials=torch.zeros((L.icp_blocks(37, 53, 1), 32), dtype=torch.float64, device=DEV),
             out=torch.zeros(32, dtype=torch.float64, device=DEV))
    T, M = np.ascontiguousarray(c["T"]), np.ascontiguousarray(c["M"])
    fx, fy, cx, cy = [float(v) for v in R.intrinsics(c["K"])]

    def call(**over):
        a = dict(lv=t["lv"].data_ptr(), il=t["il"].data_ptr(), H=37, W=53, stride=1, T=T.ctypes.data, ir=t["ir"].data_ptr(),
                 dr=t["dr"].data_ptr(), Hr=37, Wr=53, M=M.ctypes.data, fx=fx, fy=fy, cx=cx, cy=cy, dist_max=0.6,
                 intensity_max=0.3, partials=t["partials"].data_ptr(), out=t["out"].data_ptr())
        a.update(over)
        p, d, i = ctypes.c_void_p, ctypes.c_double, ctypes.c_int
        rc = L.lib().bf_photo_reduce(p(a["lv"]), p(a["il"]), i(a["H"]), i(a["W"]), i(a["stride"]), p(a["T"]), p(a["ir"]),
                                     p(a["dr"]), i(a["Hr"]), i(a["Wr"]), p(a["M"]), d(a["fx"]), d(a["fy"]), d(a["cx"]),
                                     d(a["cy"]), d(a["dist_max"]), d(a["intensity_max"]), p(a["partials"]), p(a["out"]),
                                     L._stream())
        torch.cuda.synchronize()
        return rc

    bad = [dict(lv=None), dict(il=None), dict(T=None), dict(ir=None), dict(dr=None), dict(M=None), dict(partials=None),
           dict(out=None), dict(H=0), dict(W=-1), dict(stride=0), dict(Hr=0), dict(Wr=0), dict(fx=0.0), dict(fy=float("nan")),
           dict(dist_max=-1.0), dict(dist_max=float("nan")), dict(intensity_max=-0.1), dict(intensity_max=float("nan"))]
    for over in bad:
        assert call(**over) == -1, over                         # BF_ERR_ARG
    for over in (dict(H=1 << 15, W=1 << 15), dict(Hr=1 << 15, Wr=1 << 15)):
        assert call(**over) == -3, over                         # BF_ERR_CAPACITY
    assert not t["out"].any() and not t["partials"].any()       # nothing above launched anything
    assert call() == 0 and t["out"][28] > 0
    # the binding refuses what it can see
    args = (t["lv"], t["il"], 1, c["T"], t["ir"], t["dr"], c["M"], R.intrinsics(c["K"]), 0.6, 0.3)
    for at, wrong in ((0, t["il"]), (1, t["il"][:-1]), (2, 0), (3, c["T"][:2]), (4, t["ir"][:-1]), (5, t["dr"].double())):
        with pytest.raises(L.HipError):
            L.photo_reduce(*[wrong if k == at else v for k, v in enumerate(args)])
    with pytest.raises(L.HipError):
        L.photo_reduce(*args, out=torch.zeros(32, dtype=torch.float32, device=DEV))


# ---- 3. the tracker follows the wall and the room ----------------------------------------------------------------
# the allowance tests/test_gpu_track.py grants one borderline association
POSE_VS_RESTATEMENT_M, POSE_VS_RESTATEMENT_DEG = 1e-5, 1e-3


def _assert_follows(poses, infos, ref, what):
    scene = ref["scene"]
    assert poses.dtype == np.float32 and poses.shape == ref["poses"].shape
    assert [bool(i["lost"]) for i in infos] == [bool(i["lost"]) for i in ref["infos"]]
    assert [bool(i["tracked"]) for i in infos] == [bool(i["tracked"]) for i in ref["infos"]]
    placed = [k for k, i in enumerate(infos) if not i["lost"]]
    diff = [TR.pose_error(poses[k], ref["poses"][k]) for k in placed]
    et, er, _, _ = TR.trajectory_errors(poses[placed], [scene.poses[k] for k in placed])
    wt, wr, _, _ = TR.trajectory_errors(ref["poses"][placed], [scene.poses[k] for k in placed])
    print(f"{what}: against the restatement max {max(d[0] for d in diff):.3e} m {max(d[1] for d in diff):.3e} deg; against the "
          f"truth max {et * 1000:.3f} mm {er:.4f} deg (restatement {wt * 1000:.3f} mm {wr:.4f} deg)")
    for a, b in zip(infos, ref["infos"]):
        if a["tracked"]:
            assert abs(a["inliers"] - b["inliers"]) <= 2 and a["iterations"] == b["iterations"]     # as test_gpu_track.py
            assert a.get("photo_inliers") == b.get("photo_inliers")
            if "photo_rms" in b and np.isfinite(b["photo_rms"]):
                # intensities of 0 .. 1 at estimates that agree to 1e-5 m, gradients below 1 per pixel at 40 pixels
                # per metre: 4e-4 at the very most
                assert abs(a["photo_rms"] - b["photo_rms"]) <= 4e-4
    assert max(d[0] for d in diff) <= POSE_VS_RESTATEMENT_M and max(d[1] for d in diff) <= POSE_VS_RESTATEMENT_DEG
    assert np.isneginf(poses[[k for k in range(len(infos)) if k not in placed]]).all()


@pytest.mark.parametrize("which", ["wall", "room"])
def test_tracker_follows_with_the_image(L, which):
    """measured on an MI355X: the f32 poses equal the restatement tracker's (0 m, 0 degrees); against the truth 0.240 mm
    and 0.0151 degrees on the wall, 0.451 mm and 0.0232 degrees on the room"""
    from boxfusion_amd.tracking import IcpTracker
    ref = P.reference(which, "scratch")
    scene = ref["scene"]
    vol = _volume()
    tr = IcpTracker(vol, scene.K, scene.H, scene.W, **TR.TRACKER)
    poses, infos, last = [], [], None
    for k, (d, rgb) in enumerate(zip(ref["depths"], ref["rgbs"])):
        if k == 0:
            pose, info = scene.poses[0], dict(lost=False, tracked=False)
            tr.set_reference(_dev(rgb), _dev(d), pose)
        else:
            pose, info = tr.track(_dev(d), last, _dev(rgb))
            info["tracked"] = True
            assert "photo_inliers" in info and "photo_rms" in info
        poses.append(pose)
        infos.append(info)
        assert not info["lost"]
        vol.integrate(_dev(d), scene.K, pose[None])
        last = pose
    _assert_follows(np.stack(poses), infos, ref, which)
    for s in range(1, len(poses)):
        et, er = TR.pose_error(poses[s], scene.poses[s])
        if which == "wall":                                      # a tenth of what the stale pose is off by
            assert et < 0.0035 and er < 0.11, (s, et, er)


def test_reference_rules(L):
    """without an image or a reference track() is the geometry's path; a lost frame and a non-finite pose leave no
    reference behind"""
    from boxfusion_amd.tracking import IcpTracker
    s = P.wall_scene()
    wall, d, rgb = s["scene"], [_dev(a) for a in s["depths"]], [_dev(a) for a in s["rgbs"]]
    vol = _volume()
    vol.integrate(d[0], wall.K, wall.poses[0][None])
    tr = IcpTracker(vol, wall.K, wall.H, wall.W, **TR.TRACKER)
    plain, pi = tr.track(d[1], wall.poses[0])
    again, ai = tr.track(d[1], wall.poses[0], rgb[1])            # no reference yet: the same path, and lost the same way
    assert pi["lost"] and ai == pi and "photo_inliers" not in ai and tr._ref is None
    tr.set_reference(rgb[0], d[0], wall.poses[0])
    pose, info = tr.track(d[1], wall.poses[0], rgb[1])
    assert not info["lost"] and info["photo_inliers"] > 2800 and tr._ref is not None
    assert tr.track(d[1], wall.poses[0])[1] == pi               # and without the image it is lost as before
    grey = torch.full_like(rgb[2], 128)
    tr.set_reference(grey, d[0], wall.poses[0])
    held = tr._ref
    pose, info = tr.track(d[1], wall.poses[0], grey)             # no texture: lost, and the reference stays
    assert info["lost"] and info["iterations"] == 1 and info["photo_inliers"] > 0.9 * info["sampled"]
    assert info["photo_rms"] == 0 and tr._ref is held
    assert info["cond"] == pi["cond"] and info["inliers"] == pi["inliers"]
    tr.set_reference(rgb[0], d[0], TR.LOST)
    assert tr._ref is None
    # an image of another size is resized to the depth's, as TsdfVolume.integrate does
    big = torch.from_numpy(np.ascontiguousarray(np.repeat(np.repeat(s["rgbs"][0], 2, 0), 2, 1))).to(DEV)
    tr.set_reference(big, d[0], wall.poses[0])
    assert tuple(tr._ref[0].shape) == (wall.H, wall.W)
    with pytest.raises(ValueError):
        tr.set_reference(rgb[0].float(), d[0], wall.poses[0])
    with pytest.raises(ValueError):
        IcpTracker(vol, wall.K, wall.H, wall.W, photo_weight=-1.0)


# ---- 4. track_sequence -------------------------------------------------------------------------------------------
def test_track_sequence_places_the_wall(L):
    from boxfusion_amd.tracking import track_sequence
    ref = P.reference("wall", "known")
    wall = ref["scene"]
    depths, colours = _dev(np.stack(ref["depths"])), _dev(np.stack(ref["rgbs"]))
    unknown = list(P.WALL_UNKNOWN)
    poses, infos = track_sequence(depths, wall.K, known_poses=ref["known"], volume=_volume(), colours=colours, photometric=True,
                                  **TR.TRACKER)
    _assert_follows(poses, infos, ref, "wall, three poses unknown")
    assert np.isfinite(poses).all()
    for s in unknown:
        et, er = TR.pose_error(poses[s], wall.poses[s])
        assert et < 0.0035 and er < 0.11, (s, et, er)
    vol = _volume()
    poses, infos = track_sequence(depths, wall.K, known_poses=ref["known"], volume=vol, colours=colours, **TR.TRACKER)
    assert np.isneginf(poses[unknown]).all() and all(infos[s]["lost"] for s in unknown)
    assert np.array_equal(np.delete(poses, unknown, 0), np.delete(ref["known"], unknown, 0))
    with pytest.raises(ValueError):
        track_sequence(depths, wall.K, known_poses=ref["known"], volume=vol, photometric=True, **TR.TRACKER)


# ---- 5. through a .sens file -------------------------------------------------------------------------------------
def test_sens_track_photometric(L, tmp_path, capsys):
    import types
    from boxfusion_amd import sens as S
    s = P.wall_scene()
    wall = s["scene"]
    # the capture's world has z up and the camera upright (the stream turns frames by the pose's roll): the wall's
    # poses behind one rigid transform, the images and depths as they are
    G = U.upright_pose().astype(np.float64)
    truth = [(G @ p.astype(np.float64)).astype(np.float32) for p in wall.poses]
    scene = types.SimpleNamespace(K=wall.K, poses=truth)
    known = np.stack(truth)
    unknown = list(P.WALL_UNKNOWN)
    known[unknown] = TR.LOST
    Kd = np.eye(4, dtype=np.float32)
    Kd[:3, :3] = wall.K
    path = tmp_path / "wall.sens"
    U.write_sens(path, [U.jpeg_bytes(im, JPEG_QUALITY) for im in s["rgbs"]], [TR.quantise_mm(d)[0] for d in s["depths"]], known,
                 (wall.H, wall.W), intrinsic_depth=Kd)
    args = dict(voxel=RV["voxel"], trunc_voxels=RV["T"], max_depth=RV["max_depth"], capacity=2048)
    with S.SensFile(path) as f:
        poses, ids, infos, _ = S.track(f, photometric=True, **args, **TR.TRACKER)
        without, _, winfos, _ = S.track(f, **args, **TR.TRACKER)
        decoded = [m["wide"]["image"][-1].permute(1, 2, 0).cpu().numpy() for m in S.SensFrameStream(f, batch=4)]
    assert ids == list(range(6)) and np.isfinite(poses).all() and np.isneginf(without[unknown]).all()
    # the restatement on what the file holds: the depth in millimetres, the images as the stream decodes them
    assert decoded[0].dtype == np.uint8 and decoded[0].shape == (wall.H, wall.W, 3)
    assert 0 < max(np.abs(a.astype(int) - b.astype(int)).max() for a, b in zip(decoded, s["rgbs"])) <= 8
    want, winf = P.run_sequence(scene, [TR.quantise_mm(d)[1] for d in s["depths"]], decoded, known)
    _assert_follows(poses, infos, dict(scene=scene, poses=want, infos=winf), f"wall.sens, JPEG quality {JPEG_QUALITY}")
    for k in unknown:
        for got in (want[k], poses[k]):
            et, er = TR.pose_error(got, truth[k])
            assert et < 0.0035 and er < 0.11, (k, et, er)
    out = tmp_path / "poses.npy"
    argv = ["track", str(path), str(out), "--voxel", "0.05", "--trunc-voxels", "3", "--max-depth", "4", "--capacity", "2048"]
    assert S.main(argv + ["--photometric"]) == 0
    assert "6 frames: 3 tracked, 0 lost" in capsys.readouterr().out and np.isfinite(np.load(out)).all()
    assert S.main(argv) == 0
    assert "6 frames: 0 tracked, 3 lost" in capsys.readouterr().out and np.isneginf(np.load(out)[unknown]).all()
