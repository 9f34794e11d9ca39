"""Camera tracking on the GPU (bf_tsdf_raycast, bf_track.hip, boxfusion_amd/tracking.py) against the numpy
restatement in tests/track_ref.py: the raycast bit for bit, the ICP sums within the gap two summation orders can
have, the tracker along the box room, what it reports as lost, and `sens track` bringing back a capture's lost
frames.  The reference numbers are those of test_track_host.py."""
import numpy as np
import pytest
import torch

from tests import mesh_ref as R
from tests import sens_util as U
from tests import track_ref as TR

pytestmark = pytest.mark.gpu

DEV = "cuda"
SV, RV = TR.SCENE_VOLUME, TR.ROOM_VOLUME
STATS = ("hits", "behind", "left_range", "skipped_pose", "no_normal")


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from boxfusion_amd import _lib
    _lib.lib()
    return _lib


def _volume(v, capacity=1 << 11):
    from boxfusion_amd.scene_mesh import TsdfVolume
    return TsdfVolume(voxel=v["voxel"], trunc_voxels=v["T"], capacity=capacity, max_depth=v["max_depth"], device=DEV)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t, want):
    """a device tensor equals a numpy array bit for bit (f32 compared as int32: -0.0 and NaN included)"""
    got = t.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float32:
        got, want = got.view(np.int32), np.ascontiguousarray(want).view(np.int32)
    bad = np.argwhere(got != want)
    assert not len(bad), (len(bad), bad[:5])


@pytest.fixture(scope="module")
def scene_volumes(L):
    out = {}
    for colour in (False, True):
        s = TR.scene_reference(colour)
        sc = s["scene"]
        vol = _volume(SV)
        vol.integrate(_dev(np.stack(sc.depths())), sc.K, np.stack(sc.poses), _dev(np.stack(s["rgbs"])) if colour else None)
        key, state = vol.raw()
        assert np.array_equal(key.cpu().numpy(), s["ref"]["key"]) and np.array_equal(state.cpu().numpy(), s["ref"]["state"])
        out[colour] = vol
    return out


@pytest.fixture(scope="module")
def room_volume(L):
    room = TR.Room()
    vol = _volume(RV)
    vol.integrate(_dev(np.stack(room.depths())), room.K, np.stack(room.poses))
    return room, vol


# ---- 1. the raycast equals the restatement ---------------------------------------------------------------------
def _assert_raycast(got, wants, colour):
    d, v, n, c, counters = got
    assert d.dtype == v.dtype == n.dtype == torch.float32 and counters.dtype == torch.int64
    _bits(d, np.stack([w["depth"] for w in wants]))
    _bits(v, np.stack([w["vertex"] for w in wants]))
    _bits(n, np.stack([w["normal"] for w in wants]))
    if colour:
        _bits(c, np.stack([w["rgb"] for w in wants]))
    else:
        assert c is None
    counters = counters.cpu().tolist()
    assert counters[:5] == [sum(w[k] for w in wants) for k in STATS] and counters[5:] == [0, 0, 0]
    hit = d.cpu().numpy() > 0
    assert np.array_equal(hit, n.cpu().numpy().any(-1)) and int(hit.sum()) == counters[0]


@pytest.mark.parametrize("colour", [False, True])
def test_raycast_vs_restatement(L, scene_volumes, colour):
    s, vol = TR.scene_reference(colour), scene_volumes[colour]
    sc = s["scene"]
    six = s["views"][:6]
    got = vol.raycast(np.stack([v[1] for v in six]), sc.K, sc.H, sc.W, colour=colour)          # six views in one launch
    wants = [TR.scene_raycast(v[0], colour) for v in six]
    assert sum(w["hits"] for w in wants) > 6 * 2400
    _assert_raycast(got, wants, colour)
    for name, pose, H, W, K, mw in s["views"][6:]:
        want = TR.scene_raycast(name, colour)
        got = vol.raycast(pose, K, H, W, min_weight=mw, colour=colour)
        _assert_raycast(got, [want], colour)
        if name in ("behind_wall", "lost_pose", "heavy"):
            assert not got[0].any() and not got[1].any() and not got[2].any() and int(got[4][0]) == 0
            assert int(got[4][3]) == (name == "lost_pose")
    # a lost view among good ones: zero and counted, the others untouched
    three = np.stack([six[0][1], s["views"][9][1], six[1][1]])
    assert s["views"][9][0] == "lost_pose"
    _assert_raycast(vol.raycast(three, sc.K, sc.H, sc.W, colour=colour),
                    [wants[0], TR.scene_raycast("lost_pose", colour), wants[1]], colour)


def test_raycast_from_outside_ends_behind(L, room_volume):
    room, vol = room_volume
    want = TR.raycast(TR.fuse_room(room, room.depths(), room.poses)[0], TR.outside_pose(), room.K, room.H, room.W,
                      RV["voxel"], RV["T"], 0.05, RV["max_depth"])
    assert want["behind"] == room.H * room.W
    _assert_raycast(vol.raycast(TR.outside_pose(), room.K, room.H, room.W), [want], False)
    # near and far are honoured: a range that ends before the walls leaves every ray without a hit
    got = vol.raycast(room.poses[0], room.K, room.H, room.W, near=0.1, far=0.6)
    want = TR.raycast(TR.fuse_room(room, room.depths(), room.poses)[0], room.poses[0], room.K, room.H, room.W, RV["voxel"],
                      RV["T"], 0.1, 0.6)
    assert want["left_range"] == room.H * room.W
    _assert_raycast(got, [want], False)


def test_raycast_arguments(L, room_volume):
    room, vol = room_volume
    with pytest.raises(ValueError):
        vol.raycast(room.poses[0], room.K, 48, 64, near=1.0, far=0.5)
    with pytest.raises(ValueError):
        vol.raycast(room.poses[0], room.K, 48, 64, min_weight=0)
    with pytest.raises(L.HipError):
        L.tsdf_raycast(vol.keys, vol.vox, torch.zeros((1, 3, 4), device=DEV), (1, 1, 0, 0), 4, 4, 0.05, 3, 0.0, 1.0, 1, 16,
                       torch.zeros(8, dtype=torch.int64, device=DEV))


# ---- 2. the raycast against the analytic surface ----------------------------------------------------------------
def test_raycast_vs_analytic(L, scene_volumes):
    """measured on the GPU: the restatement's figures exactly (the depth is the same bits): max 2.051 voxels with the
    rays that pass the sphere within its band left out, 35.06 with them; mean 0.173 - 0.210; hit share 0.923 - 0.951"""
    s, vol = TR.scene_reference(), scene_volumes[False]
    sc = s["scene"]
    depth = vol.raycast(np.stack(sc.poses), sc.K, sc.H, sc.W)[0].cpu().numpy()
    for pose, d in zip(sc.poses, depth):
        err, share, _ = TR.analytic_error(sc, pose, d)
        print(f"analytic on the GPU: max {err.max():.3f} ({err[err < 10].max():.3f} off the sphere's band), mean "
              f"{err[err < 10].mean():.3f}, hits {share:.3f}")
        assert err.max() <= 1.5 * TR.ANALYTIC_MAX_ALL and err[err < 10].max() <= 1.5 * TR.ANALYTIC_MAX
        assert err[err < 10].mean() < 0.25                       # the mesh path's figure on a wall is 0.15 voxel
        assert share >= 0.9


# ---- 3. the reduction equals the restatement -----------------------------------------------------------------------
def _icp_case(H, W):
    """live and model maps of the room at H x W, from the restatement: model maps with holes, a live frame with a band
    of invalid depth, an estimate 3 degrees and 5 cm off"""
    room = TR.Room()
    K = room.K.copy()
    K[0] *= W / room.W
    K[1] *= H / room.H
    vol, _ = TR.fuse_room(room, room.depths(), room.poses)
    model = TR.raycast(vol, room.poses[2], K, H, W, RV["voxel"], RV["T"], 0.05, RV["max_depth"])
    rng = np.random.default_rng(H)
    holes = rng.random((H, W)) < 0.1
    mv, mn = model["vertex"].copy(), model["normal"].copy()
    mv[holes], mn[holes] = 0, 0
    depth = room.depth(room.poses[3], H, W, K)
    depth[10:14] = 0.0
    depth[20, 5] = np.nan
    T = TR.perturb(room.poses[3], 3.0, 0.05, seed=1).astype(np.float64)[:3]
    return dict(K=K, mv=mv, mn=mn, depth=depth, T=T, M=TR.w2c(room.poses[2]))


def _assert_sums(L, c, lv, ln, stride, T):
    terms, n_s = TR.icp_terms(lv, ln, stride, T, c["mv"], c["mn"], c["M"], c["K"], 0.6, 0.8)
    want = TR.icp_sums(terms)
    args = (_dev(lv), _dev(ln), stride, T, _dev(c["mv"]), _dev(c["mn"]), c["M"], R.intrinsics(c["K"]), 0.6, 0.8)
    a = L.icp_reduce(*args).cpu().numpy()
    b = L.icp_reduce(*args).cpu().numpy()
    assert a.tobytes() == b.tobytes()                           # the same bits on every run
    assert a[28] == want[28] and not a[29:].any() and np.isfinite(a).all()
    bound = max(len(terms) - 1, 0) * 2.0 ** -52 * np.abs(terms).sum(0)
    gap = np.abs(a[:28] - want[:28])
    assert (gap <= bound).all(), (stride, gap / np.maximum(bound, 1e-300))
    return a, n_s


@pytest.mark.parametrize("H,W", [(48, 64), (37, 53)])
def test_icp_reduce_vs_restatement(L, H, W):
    c = _icp_case(H, W)
    lv, ln = TR.vertex_normal(c["depth"], c["K"], RV["max_depth"], 0.15)
    gv, gn = L.depth_vertex_normal(_dev(c["depth"]), R.intrinsics(c["K"]), RV["max_depth"], 0.15)
    _bits(gv, lv)
    _bits(gn, ln)
    assert not ln[10:14].any() and not ln[9].any() and ln[15].any()
    for stride in (1, 2, 4):
        a, n_s = _assert_sums(L, c, lv, ln, stride, c["T"])
        assert n_s == -(-H // stride) * -(-W // stride) and 0.3 * n_s < a[28] < 0.9 * n_s
        assert L.icp_blocks(H, W, stride) == -(-n_s // 1024)
    # nothing valid: the count and every sum are exactly zero
    zv, zn = TR.vertex_normal(np.zeros((H, W), np.float32), c["K"], RV["max_depth"], 0.15)
    a, _ = _assert_sums(L, c, zv, zn, 1, c["T"])
    assert not a.any()
    # a live frame wholly outside the model's view: turned half round
    away = c["T"].copy()
    away[:, :3] = away[:, :3] @ np.diag([-1.0, 1.0, -1.0])
    a, _ = _assert_sums(L, c, lv, ln, 1, away)
    assert not a.any()


# ---- 4. the tracker follows the room ----------------------------------------------------------------------------------
# measured on an MI355X against the restatement's tracker: 0 m and 0 degrees in both modes, the f32 poses are equal
# (the sums differ by parts in 1e16, the solve has a condition number of 20).  Ten times nothing bounds nothing, so
# the bound is what one borderline association may do: a pixel more or less among >= 1900 inliers with residuals
# below 1 cm moves the solution by about 0.01 / 1900 = 5e-6 m, or 1e-5 rad = 6e-4 degrees at the room's 0.6 m lever
POSE_VS_RESTATEMENT_M, POSE_VS_RESTATEMENT_DEG = 1e-5, 1e-3


@pytest.mark.parametrize("mode", ["scratch", "known"])
def test_tracker_follows_the_room(L, mode):
    from boxfusion_amd.tracking import track_sequence
    ref = TR.room_reference(mode)
    room = ref["room"]
    vol = _volume(RV)
    poses, infos = track_sequence(_dev(np.stack(ref["depths"])), room.K, first_pose=room.poses[0], known_poses=ref["known"],
                                  volume=vol, **TR.TRACKER)
    assert poses.dtype == np.float32 and poses.shape == (8, 4, 4) and not any(i["lost"] for i in infos)
    assert [bool(i["tracked"]) for i in infos] == [bool(i["tracked"]) for i in ref["infos"]]
    diff = [TR.pose_error(p, q) for p, q in zip(poses, ref["poses"])]
    et, er, ft, fr = TR.trajectory_errors(poses, room.poses)
    wt, wr, wft, wfr = TR.trajectory_errors(ref["poses"], room.poses)
    print(f"{mode}: against the restatement max {max(d[0] for d in diff):.3e} m {max(d[1] for d in diff):.3e} deg; against "
          f"the truth max {et * 1000:.3f} mm {er:.4f} deg, final {ft * 1000:.3f} mm {fr:.4f} deg (restatement {wt * 1000:.3f} "
          f"mm {wr:.4f} deg, {wft * 1000:.3f} mm {wfr:.4f} deg)")
    for a, b in zip(infos, ref["infos"]):
        if a["tracked"]:
            assert a["inliers"] == b["inliers"] or abs(a["inliers"] - b["inliers"]) <= 2
            assert a["iterations"] == b["iterations"] == 12 and abs(a["cond"] - b["cond"]) < 1e-3 * b["cond"]
    assert max(d[0] for d in diff) <= POSE_VS_RESTATEMENT_M and max(d[1] for d in diff) <= POSE_VS_RESTATEMENT_DEG
    assert et <= 2 * wt and er <= 2 * wr and ft <= 2 * wft + 1e-12 and fr <= 2 * wfr + 1e-12
    # every frame went into the volume
    whole = _volume(RV)
    whole.integrate(_dev(np.stack(ref["depths"])), room.K, poses)
    assert vol.stats()["observations"] == whole.stats()["observations"]


# ---- 5. failure is reported, not invented ----------------------------------------------------------------------------
def test_failures_are_lost(L):
    from boxfusion_amd.tracking import IcpTracker, track_sequence
    room = TR.Room()
    d0 = room.depths()[0]
    wall, eye = TR.plane_depth(room.H, room.W, room.K), np.eye(4, dtype=np.float32)
    cases = [("wall", wall, eye, wall, TR.perturb(eye, 1.0, 0.02)),
             ("turned", d0, room.poses[0], d0, TR.perturb(room.poses[0], 45.0, 0.0)),
             ("empty", d0, room.poses[0], np.zeros_like(d0), room.poses[0])]
    for name, first, first_pose, frame, guess in cases:
        vol = _volume(RV)
        vol.integrate(_dev(first), room.K, first_pose[None])
        before = vol.stats()
        pose, info = IcpTracker(vol, room.K, room.H, room.W, **TR.TRACKER).track(_dev(frame), guess)
        print(name, info)
        assert info["lost"] and pose.dtype == np.float32 and np.isneginf(pose).all(), name
        if name == "wall":
            assert info["inliers"] > 0.7 * info["sampled"] and info["cond"] > 1e6
        else:
            assert info["inliers"] < 0.4 * info["sampled"]
        assert vol.stats() == before
        if name == "turned":
            continue
        # through track_sequence: a lost frame is not integrated, and the next one starts from the last good pose
        vol2 = _volume(RV)
        poses, infos = track_sequence(_dev(np.stack([first, np.zeros_like(d0), first])), room.K, first_pose=first_pose,
                                      volume=vol2, **TR.TRACKER)
        assert np.array_equal(poses[0], first_pose) and np.isneginf(poses[1]).all() and infos[1]["lost"]
        if name == "wall":                                       # the wall again: still no pose, still nothing fused
            assert infos[2]["lost"] and np.isneginf(poses[2]).all() and vol2.stats() == before
        else:
            assert not infos[2]["lost"] and TR.pose_error(poses[2], first_pose)[0] < 0.002
            assert vol2.stats()["observations"] > before["observations"]


# ---- 6. lost frames come back ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def capture(L, tmp_path_factory):
    ref = TR.room_reference("quantised")
    room = ref["room"]
    rng = np.random.default_rng(2)
    colors = [U.jpeg_bytes(rng.integers(0, 256, (room.H, room.W, 3), dtype=np.uint8)) for _ in room.poses]
    mm = [TR.quantise_mm(d)[0] for d in room.depths()]
    Kd = np.eye(4, dtype=np.float32)
    Kd[:3, :3] = room.K
    path = tmp_path_factory.mktemp("track") / "room.sens"
    U.write_sens(path, colors, mm, ref["known"], (room.H, room.W), intrinsic_depth=Kd)
    return dict(path=path, ref=ref, room=room)


def test_sens_track_recovers_lost_frames(L, capture, tmp_path, capsys):
    from boxfusion_amd import sens as S
    room, ref = capture["room"], capture["ref"]
    out = tmp_path / "poses.npy"
    assert S.main(["track", str(capture["path"]), str(out), "--recover-lost", "--voxel", "0.05", "--trunc-voxels", "3",
                   "--max-depth", "4", "--capacity", "2048", "--mesh", str(tmp_path / "room.ply")]) == 0
    line = capsys.readouterr().out
    assert "8 frames: 3 tracked, 0 lost" in line and (tmp_path / "room.ply").stat().st_size > 1000
    poses = np.load(out)
    assert poses.dtype == np.float32 and poses.shape == (8, 4, 4) and np.isfinite(poses).all()
    lost = list(TR.LOST_FRAMES)
    keep = [i for i in range(8) if i not in lost]
    assert np.array_equal(poses[keep], np.stack(room.poses)[keep])
    # the bound of test 4 (twice the restatement's error against the truth) plus the depth quantisation's share,
    # measured with the restatement on the quantised frames: 0.61 mm / 0.044 deg, and 0.03 mm / 0.005 deg
    exact = TR.room_reference("known")
    wt, wr, _, _ = TR.trajectory_errors(exact["poses"], room.poses)
    share = [TR.pose_error(a, b) for a, b in zip(ref["poses"], exact["poses"])]
    bt, br = 2 * wt + max(s[0] for s in share), 2 * wr + max(s[1] for s in share)
    with S.SensFile(capture["path"]) as f:
        stale = f.poses_filled()
        for i in lost:
            et, er = TR.pose_error(poses[i], room.poses[i])
            st = TR.pose_error(stale[i], room.poses[i])[0]
            print(f"frame {i}: recovered to {et * 1000:.3f} mm {er:.4f} deg (bound {bt * 1000:.3f} mm {br:.4f} deg); the stale "
                  f"pose is {st * 1000:.1f} mm off")
            assert et <= bt and er <= br
            assert st > 0.03 and st > 20 * et                    # what poses_filled() hands the detector today
        got = list(S.SensFrameStream(f, batch=4, poses=poses))
        today = list(S.SensFrameStream(f, batch=4))
        for i in range(8):
            assert torch.equal(got[i]["sensor_info"].gt.RT[0].cpu(), torch.from_numpy(poses[i]))
            assert torch.equal(today[i]["sensor_info"].gt.RT[0].cpu(), torch.from_numpy(stale[i]))
        with pytest.raises(ValueError):
            S.SensFrameStream(f, poses=poses[:3])


def test_sens_track_from_scratch(L, capture, tmp_path, capsys):
    from boxfusion_amd import sens as S
    out = tmp_path / "poses.npy"
    assert S.main(["track", str(capture["path"]), str(out), "--from-scratch", "--voxel", "0.05", "--trunc-voxels", "3",
                   "--max-depth", "4", "--capacity", "2048"]) == 0
    line = capsys.readouterr().out
    assert "8 frames: 7 tracked, 0 lost" in line and "rms translation difference to the file's poses 0.00" in line
    poses = np.load(out)
    et, er, _, _ = TR.trajectory_errors(poses, capture["room"].poses)
    assert et < 0.004 and er < 0.3                               # test_track_host's bound for this mode


@pytest.mark.parametrize("argv", [["track", "nowhere.sens", "p.npy"], ["track", "SENS", "p.npy", "--step", "0"],
                                  ["track", "SENS", "p.npy", "--recover-lost", "--from-scratch"],
                                  ["track", "SENS", "p.npy", "--capacity", "1000"]])
def test_sens_track_argument_errors(L, capture, argv, capsys):
    from boxfusion_amd import sens as S
    with pytest.raises(SystemExit) as e:
        S.main([str(capture["path"]) if a == "SENS" else a for a in argv])
    assert e.value.code == 2 and "error" in capsys.readouterr().err
