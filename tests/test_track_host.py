"""The numpy restatement of camera tracking (tests/track_ref.py) on its own, on the CPU: it follows the box room
without losing a frame, reports what it cannot place as lost, and its raycast of the fused mesh_ref.Scene agrees with
the analytic depth.  The figures these tests print and bound are the reference numbers of test_gpu_track.py."""
import numpy as np
import pytest

from tests import track_ref as TR

V = TR.ROOM_VOLUME


# measured with the restatement (48 x 64, voxel 0.05, eight frames, 4 cm and 1.3 - 2.4 degrees between frames):
# from scratch the largest error against the true trajectory is 1.7 mm and 0.13 degrees (the last frame: 1.0 mm,
# 0.10 degrees); with three unknown poses 0.6 mm and 0.04 degrees.  J^T J's condition number is 18.8 - 22.0 and the
# inlier share 0.81 - 0.91.  The bounds leave a factor of two.
@pytest.mark.parametrize("mode,max_t,max_deg", [("scratch", 0.004, 0.3), ("known", 0.0015, 0.1), ("quantised", 0.0015, 0.1)])
def test_room_is_followed(mode, max_t, max_deg):
    ref = TR.room_reference(mode)
    room = ref["room"]
    assert not any(i["lost"] for i in ref["infos"])
    tracked = [i for i in ref["infos"] if i.get("tracked")]
    assert len(tracked) == (7 if mode == "scratch" else len(TR.LOST_FRAMES))
    et, er, ft, fr = TR.trajectory_errors(ref["poses"], room.poses)
    print(f"{mode}: max {et * 1000:.2f} mm {er:.3f} deg, final {ft * 1000:.2f} mm {fr:.3f} deg; cond "
          f"{min(i['cond'] for i in tracked):.1f}-{max(i['cond'] for i in tracked):.1f}, inlier share "
          f"{min(i['inliers'] / i['sampled'] for i in tracked):.2f}-{max(i['inliers'] / i['sampled'] for i in tracked):.2f}")
    assert et < max_t and er < max_deg
    for i in tracked:
        assert i["cond"] < 50 and i["inliers"] > 0.7 * i["sampled"] and i["rms"] < 0.01
    # the frames move: the stale pose poses_filled() would hand out is off by centimetres
    step = TR.pose_error(room.poses[2], room.poses[3])[0]
    assert step > 0.03 > 10 * et


def test_room_keeps_three_walls_in_view():
    room = TR.Room()
    for p in room.poses:
        d = room.depth(p)
        assert (d > 0.5).all() and (d < 2.0).all()
        P = np.asarray(p, np.float64)
        pts = TR.vertex_normal(d, room.K, 10.0, 1.0)[0].reshape(-1, 3).astype(np.float64) @ P[:3, :3].T + P[:3, 3]
        on = [np.isclose(pts[:, a], room.lo[a], atol=1e-4).mean() for a in range(3)]
        assert min(on) > 0.1, on                                # each of the three walls of the corner: > 10 % of the pixels


def test_perturbed_guess_converges():
    """up to 8 degrees and 15 cm from the truth, against a volume of one frame"""
    room = TR.Room()
    vol, _ = TR.fuse_room(room, room.depths()[:1], room.poses[:1])
    for k, (deg, m) in enumerate(((3.0, 0.05), (8.0, 0.15))):
        pose, info = TR.track(vol, room.depths()[0], TR.perturb(room.poses[0], deg, m, seed=k), room.K, V["voxel"], V["T"],
                              V["max_depth"], **TR.TRACKER)
        assert not info["lost"] and info["cond"] < 50
        et, er = TR.pose_error(pose, room.poses[0])
        assert et < 0.003 and er < 0.3, (deg, m, et, er)


def test_failures_are_lost():
    room = TR.Room()
    vol, _ = TR.fuse_room(room, room.depths()[:1], room.poses[:1])
    args = (room.K, V["voxel"], V["T"], V["max_depth"])
    # a single wall: three of the six directions are unobserved
    wall, eye = TR.plane_depth(room.H, room.W, room.K), np.eye(4, dtype=np.float32)
    wall_vol, _ = TR.fuse_room(room, [wall], [eye])
    pose, info = TR.track(wall_vol, wall, TR.perturb(eye, 1.0, 0.02), *args, **TR.TRACKER)
    assert info["lost"] and np.isneginf(pose).all() and info["inliers"] > 0.7 * info["sampled"]
    assert info["cond"] > 1e6                                   # the share is fine: the geometry is not
    # 45 degrees from the guess: the normals disagree
    pose, info = TR.track(vol, room.depths()[0], TR.perturb(room.poses[0], 45.0, 0.0), *args, **TR.TRACKER)
    assert info["lost"] and np.isneginf(pose).all() and info["inliers"] < 0.4 * info["sampled"]
    # nothing valid in the frame
    for bad in (np.zeros((room.H, room.W), np.float32), np.full((room.H, room.W), np.nan, np.float32)):
        pose, info = TR.track(vol, bad, room.poses[0], *args, **TR.TRACKER)
        assert info["lost"] and np.isneginf(pose).all() and info["inliers"] == 0 and info["iterations"] == 1


def test_icp_sums_of_nothing_are_zero():
    room = TR.Room()
    lv, ln = TR.vertex_normal(np.zeros((room.H, room.W), np.float32), room.K, 4.0, 0.15)
    assert not lv.any() and not ln.any()
    terms, n = TR.icp_terms(lv, ln, 2, np.eye(4)[:3], lv, ln, np.eye(4)[:3], room.K, 0.6, 0.8)
    out = TR.icp_sums(terms)
    assert n == 24 * 32 and terms.shape == (0, 28) and not out.any()


def test_vertex_normal_of_a_plane():
    K = TR.Room().K
    vert, nrm = TR.vertex_normal(np.full((12, 16), 2.0, np.float32), K, 4.0, 0.1)
    assert np.array_equal(nrm[:-1, :-1], np.broadcast_to(np.float32([0, 0, -1]), (11, 15, 3)))      # towards the camera
    assert not nrm[-1].any() and not nrm[:, -1].any() and (vert[..., 2] == 2.0).all()
    d = np.full((12, 16), 2.0, np.float32)
    d[5, 5], d[2, 3], d[8, 8] = 2.5, np.nan, 4.0                # a jump, a NaN, max_depth itself
    vert, nrm = TR.vertex_normal(d, K, 4.0, 0.1)
    for y, x in ((5, 5), (5, 4), (4, 5), (2, 3), (2, 2), (1, 3), (8, 8), (8, 7), (7, 8)):
        assert not nrm[y, x].any(), (y, x)
    assert not vert[2, 3].any() and not vert[8, 8].any() and nrm[5, 6].any() and np.isfinite(vert).all()


# ---- the raycast against the analytic scene ---------------------------------------------------------------------
# measured: over the six cameras the largest |depth - analytic| on pixels whose 3 x 3 neighbourhood is one surface
# is 2.05 voxels (the sphere of radius 8 voxels near its silhouette, where the projective distances of the other
# cameras overestimate), 0.58 on the wall, 0.28 on the shell; the mean is 0.17 - 0.21 voxel, and 92.3 - 95.1 % of
# those pixels are hits.  One ray in camera 5 passes the sphere within its truncation band and meets the fused sphere
# where the analytic ray goes on to the shell: 35.06 voxels; TR.ANALYTIC_MAX_ALL bounds the set with it,
# TR.ANALYTIC_MAX the set without such rays (differences of 10 voxels and more).


def test_raycast_against_the_analytic_scene():
    s = TR.scene_reference()
    sc = s["scene"]
    worst, means, shares, wall, worst_all = 0.0, [], [], 0.0, 0.0
    for name, pose, H, W, K, mw in s["views"][:6]:
        rc = TR.scene_raycast(name)
        err, share, sid = TR.analytic_error(sc, pose, rc["depth"])
        worst_all = max(worst_all, float(err.max()))
        err, sid = err[err < 10], sid[err < 10]
        worst, wall = max(worst, float(err.max())), max(wall, float(err[sid == 0].max()) if (sid == 0).any() else 0.0)
        means.append(float(err.mean()))
        shares.append(share)
        hit = rc["depth"] > 0
        assert rc["hits"] == int(hit.sum()) and rc["behind"] == 0 and rc["hits"] + rc["left_range"] + rc["no_normal"] == H * W
        n = rc["normal"].astype(np.float64)
        assert np.allclose(np.linalg.norm(n[hit], axis=1), 1.0, atol=1e-6) and not n[~hit].any()
        # the normals face the camera, and on the wall they are the wall's
        view = rc["vertex"].astype(np.float64) - np.asarray(pose, np.float64)[:3, 3]
        assert ((n * view).sum(-1)[hit] < 0).mean() > 0.99
        wall_px = hit & TR.one_surface(TR.scene_surface_ids(sc, pose)) & (TR.scene_surface_ids(sc, pose) == 0)
        if wall_px.any():
            side = np.sign(-(view[wall_px] @ sc.normal))
            assert ((n[wall_px] @ sc.normal) * side > 0.85).all()
    print(f"analytic: max {worst_all:.3f} / {worst:.3f} voxel (wall {wall:.3f}), mean {min(means):.3f}-{max(means):.3f}, hit share "
          f"{min(shares):.3f}-{max(shares):.3f}")
    assert worst <= TR.ANALYTIC_MAX and worst_all <= TR.ANALYTIC_MAX_ALL and max(means) < 0.25 and min(shares) >= 0.9


def test_raycast_edge_views():
    s = TR.scene_reference()
    rc = TR.scene_raycast("behind_wall")
    assert rc["hits"] == 0 and rc["left_range"] == 48 * 64 and not rc["depth"].any()
    rc = TR.scene_raycast("lost_pose")
    assert rc["skipped_pose"] == 1 and rc["hits"] == rc["left_range"] == 0 and not rc["depth"].any()
    rc = TR.scene_raycast("heavy")
    assert rc["hits"] == 0 and not rc["normal"].any()
    rc = TR.scene_raycast("on_wall")
    assert rc["hits"] > 300
    rc = TR.scene_raycast("odd")
    assert rc["depth"].shape == (37, 53) and rc["hits"] > 1000
    assert (s["ref"]["state"][:, 0] > 0).any()


def test_raycast_from_outside_ends_behind_the_surface():
    room = TR.Room()
    vol, _ = TR.fuse_room(room, room.depths(), room.poses)
    rc = TR.raycast(vol, TR.outside_pose(), room.K, room.H, room.W, V["voxel"], V["T"], 0.05, V["max_depth"])
    assert rc["behind"] == room.H * room.W and rc["hits"] == 0 and not rc["depth"].any()


def test_raycast_colour_is_the_voxels():
    s = TR.scene_reference(True)
    rc = TR.scene_raycast("camera0", True)
    hit = rc["depth"] > 0
    assert rc["rgb"].dtype == np.uint8 and not rc["rgb"][~hit].any() and rc["rgb"][hit].std() > 20
    plain = TR.scene_raycast("camera0")
    assert np.array_equal(plain["depth"], rc["depth"])          # colour changes nothing else
