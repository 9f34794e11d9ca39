"""The numpy restatement of the tracker's photometric term (tests/photo_ref.py) on its own, on the CPU: its Jacobian
against finite differences, the textured wall that the geometry alone loses and the two rows together place, the room
with and without the term, what an untextured wall adds (nothing), and each gate against a per-pixel recount.  The
figures these tests print and bound are the reference numbers of test_gpu_photo.py."""
import numpy as np

from tests import photo_ref as P
from tests import track_ref as TR

V = TR.ROOM_VOLUME


def _pair(scene=None, live=1, ref=0):
    """the maps of one live frame against one reference frame of the wall: dict(K, lv, il, ir, dr, M, T)"""
    s = P.wall_scene() if scene is None else scene
    w = s["scene"]
    lv, _ = TR.vertex_normal(s["depths"][live], w.K, V["max_depth"], 0.15)
    return dict(K=w.K, lv=lv, il=P.grey(s["rgbs"][live]), ir=P.grey(s["rgbs"][ref]), dr=s["depths"][ref].copy(),
                M=TR.w2c(w.poses[ref]), T=np.asarray(w.poses[live], np.float64)[:3], depth=s["depths"][live])


def _terms(c, stride=1, T=None, dist_max=0.6, intensity_max=0.3, **over):
    a = {**c, **over}
    return P.photo_terms(a["lv"], a["il"], stride, a["T"] if T is None else T, a["ir"], a["dr"], a["M"], a["K"], dist_max,
                         intensity_max, parts=True)


# ---- 1. the Jacobian --------------------------------------------------------------------------------------------
# measured: J^T r against the central difference of 1/2 sum r^2 along the six twist axes, 0.3 degrees and 5 mm from
# the truth, 2915 samples, the same inlier set at +-1e-6: the largest gap is 4e-11 of the largest component
# (inside a cell the interpolant is bilinear and the central difference has only the projection's third-order error)
def test_jacobian_against_finite_differences():
    c = _pair()
    T0 = np.concatenate([TR.perturb(P.wall_scene()["scene"].poses[1], 0.3, 0.005, seed=2).astype(np.float64)[:3],
                         [[0, 0, 0, 1.0]]])
    terms, n_s, ok, r, J = _terms(c, T=T0[:3], intensity_max=10.0)
    assert n_s == 48 * 64 and ok.sum() > 0.9 * n_s and np.abs(r).max() < 0.3   # intensity_max rejects nothing here
    b = TR.icp_sums(terms)[21:27]
    assert np.allclose(b, J.T @ r, rtol=1e-12, atol=0)
    eps, fd = 1e-6, np.zeros(6)
    for a in range(6):
        e = []
        for sgn in (1.0, -1.0):
            xi = np.zeros(6)
            xi[a] = sgn * eps
            t2, _, ok2, r2, _ = _terms(c, T=(TR.se3_exp(xi) @ T0)[:3], intensity_max=10.0)
            assert np.array_equal(ok2, ok), a                   # the same samples on both sides
            e.append(0.5 * float(r2 @ r2))
        fd[a] = (e[0] - e[1]) / (2 * eps)
    gap = np.abs(b + fd).max() / np.abs(b).max()                # r = I_live - c: d(1/2 r^2) / d xi = -J r
    print(f"finite differences: J^T r {b}, gap {gap:.2e} of the largest component")
    assert gap <= 1e-4


# ---- 2. the wall -------------------------------------------------------------------------------------------------
# measured with the restatement (48 x 64, a wall at 1 m, frames 35 mm and 1.1 degrees apart): the geometry alone is
# lost on every frame after the first (J^T J has rank 3: cond = inf); with the photometric term at weight 1 all five
# are placed, at most 0.240 mm and 0.0151 degrees from the truth, cond 31.2 - 37.0, 2915 - 2917 photometric inliers of
# 3072 with an rms of 0.0013 - 0.0014.  The bound is the issue's: a tenth of what the stale pose is off by
def test_wall_is_placed_only_with_the_image():
    geo = P.reference("wall", "geometry")
    assert [i["lost"] for i in geo["infos"]] == [False] + [True] * 5
    for i in geo["infos"][1:]:
        assert i["inliers"] > 0.7 * i["sampled"] and i["cond"] > TR.TRACKER["cond_max"] and i["iterations"] == 1
    ref = P.reference("wall", "scratch")
    wall = ref["scene"]
    assert not any(i["lost"] for i in ref["infos"])
    errs = [TR.pose_error(p, q) for p, q in zip(ref["poses"], wall.poses)]
    tracked = ref["infos"][1:]
    print(f"wall: max {max(e[0] for e in errs) * 1000:.3f} mm {max(e[1] for e in errs):.4f} deg; cond "
          f"{min(i['cond'] for i in tracked):.1f}-{max(i['cond'] for i in tracked):.1f}; photometric inliers "
          f"{min(i['photo_inliers'] for i in tracked)}-{max(i['photo_inliers'] for i in tracked)}, rms "
          f"{min(i['photo_rms'] for i in tracked):.4f}-{max(i['photo_rms'] for i in tracked):.4f}")
    for s in range(1, 6):
        stale = TR.pose_error(wall.poses[s - 1], wall.poses[s])
        assert stale[0] > 0.0349 and stale[1] > 1.09           # 35 mm and 1.1 degrees, through the f32 poses
        assert errs[s][0] < 0.0035 and errs[s][1] < 0.11, (s, errs[s])
    for i in tracked:
        assert i["cond"] < 100 and i["photo_inliers"] > 0.9 * i["sampled"] and i["photo_rms"] < 0.01
    # with three poses unknown (what track_sequence is asked on the GPU): the same bound
    known = P.reference("wall", "known")
    assert [bool(i.get("tracked")) for i in known["infos"]] == [False, False, True, True, True, False]
    for s in P.WALL_UNKNOWN:
        et, er = TR.pose_error(known["poses"][s], wall.poses[s])
        assert et < 0.0035 and er < 0.11, (s, et, er)


# ---- 3. the room -------------------------------------------------------------------------------------------------
# measured: weight 0 gives the geometry's poses bit for bit (1.711 mm, 0.1329 degrees at worst); weight 1 gives
# 0.451 mm and 0.0232 degrees, cond 43.2 - 54.0
def test_room_with_and_without_the_term():
    geo, zero, one = P.reference("room", "geometry"), P.reference("room", "scratch", 0.0), P.reference("room", "scratch")
    room = geo["scene"]
    assert np.array_equal(geo["poses"], zero["poses"]) and np.array_equal(geo["poses"], TR.room_reference("scratch")["poses"])
    assert not any(i["lost"] for i in one["infos"])
    gt, gr, _, _ = TR.trajectory_errors(geo["poses"], room.poses)
    et, er, _, _ = TR.trajectory_errors(one["poses"], room.poses)
    print(f"room: geometry {gt * 1000:.3f} mm {gr:.4f} deg, with the photometric term {et * 1000:.3f} mm {er:.4f} deg, cond "
          f"{max(i['cond'] for i in one['infos'][1:]):.1f}")
    assert et <= gt and er <= gr
    assert max(i["cond"] for i in one["infos"][1:]) < 100


# ---- 4. no texture, no term --------------------------------------------------------------------------------------
def test_uniform_colour_adds_exactly_nothing():
    s = P.wall_scene()
    wall = s["scene"]
    plain = dict(s, rgbs=P.images(wall, s["depths"], uniform=0.5))
    assert all((im == 128).all() for im in plain["rgbs"])
    terms, n_s, ok, r, J = _terms(_pair(plain))
    assert ok.sum() > 0.9 * n_s and not terms.any() and not TR.icp_sums(terms)[:28].any()
    poses, infos = P.run_sequence(wall, s["depths"][:2], plain["rgbs"][:2])
    geo = P.reference("wall", "geometry")["infos"][1]
    assert infos[1]["lost"] and np.isneginf(poses[1]).all() and infos[1]["photo_inliers"] > 0 and infos[1]["photo_rms"] == 0
    assert {k: infos[1][k] for k in geo} == geo                 # lost as without an image: the same count, the same cond


def test_photo_sums_of_nothing_are_zero():
    c = _pair()
    lv, _ = TR.vertex_normal(np.zeros((48, 64), np.float32), c["K"], 4.0, 0.15)
    terms, n = P.photo_terms(lv, c["il"], 2, c["T"], c["ir"], c["dr"], c["M"], c["K"], 0.6, 0.3)
    assert n == 24 * 32 and terms.shape == (0, 28) and not TR.icp_sums(terms).any()
    # a reference too small for a bilinear tap
    terms, n = P.photo_terms(c["lv"], c["il"], 1, c["T"], c["ir"][:1], c["dr"][:1], c["M"], c["K"], 0.6, 0.3)
    assert n == 48 * 64 and terms.shape == (0, 28)


# ---- 5. the gates ------------------------------------------------------------------------------------------------
def _recount(c, stride, dist_max=0.6, intensity_max=0.3):
    """the model pixel by pixel in Python floats: the sampled indices that pass every gate, and the reference pixel
    each one reads its depth from"""
    fx, fy, cx, cy = [float(a) for a in TR.R.intrinsics(c["K"])]
    T, M = np.asarray(c["T"], np.float64), np.asarray(c["M"], np.float64)
    Hr, Wr = c["ir"].shape
    H, W = c["il"].shape
    kept, at, k = [], {}, -1
    for y in range(0, H, stride):
        for x in range(0, W, stride):
            k += 1
            v = c["lv"][y, x].astype(np.float64)
            if not v[2] > 0:
                continue
            p = T[:, :3] @ v + T[:, 3]
            q = M[:, :3] @ p + M[:, 3]
            if not q[2] > 0:
                continue
            u, w = fx * q[0] / q[2] + cx, fy * q[1] / q[2] + cy
            if not (0 <= np.floor(u) <= Wr - 2 and 0 <= np.floor(w) <= Hr - 2):
                continue
            near = (int(np.floor(w + 0.5)), int(np.floor(u + 0.5)))
            at[k] = near
            d = float(c["dr"][near])
            if not (d > 0 and abs(d - q[2]) <= dist_max):
                continue
            u0, w0 = int(np.floor(u)), int(np.floor(w))
            fu, fv = u - u0, w - w0
            tap = c["ir"][w0:w0 + 2, u0:u0 + 2].astype(np.float64)
            val = (1 - fv) * ((1 - fu) * tap[0, 0] + fu * tap[0, 1]) + fv * ((1 - fu) * tap[1, 0] + fu * tap[1, 1])
            if not abs(float(c["il"][y, x]) - val) <= intensity_max:
                continue
            kept.append(k)
    return kept, at


def test_gates_remove_what_they_should():
    base = _pair(live=2, ref=0)                                # 70 mm and 2.2 degrees apart: part of the frame leaves the view
    for stride in (1, 2):
        Ws = -(-64 // stride)
        _, n_s, ok0, r0, _ = _terms(base, stride)
        kept0, at = _recount(base, stride)
        assert kept0 == list(np.flatnonzero(ok0)) and 0.7 * n_s < len(kept0) < n_s
        # a band of zeros in the reference depth: the samples whose nearest reference pixel is in it go, no others
        dr = base["dr"].copy()
        dr[20:24] = 0.0
        _, _, ok, _, _ = _terms(base, stride, dr=dr)
        gone = [k for k in kept0 if 20 <= at[k][0] < 24]
        assert gone and sorted(set(kept0) - set(np.flatnonzero(ok))) == gone and not (ok & ~ok0).any()
        assert _recount({**base, "dr": dr}, stride)[0] == list(np.flatnonzero(ok))
        # a band of invalid live depth (zero, and a NaN beside it)
        depth = base["depth"].copy()
        depth[10:14] = 0.0
        depth[30, 8] = np.nan
        lv, _ = TR.vertex_normal(depth, base["K"], V["max_depth"], 0.15)
        _, _, ok, _, _ = _terms(base, stride, lv=lv)
        rows = np.arange(n_s) // Ws * stride
        cols = np.arange(n_s) % Ws * stride
        band = ((rows >= 10) & (rows < 14)) | ((rows == 30) & (cols == 8))
        assert (ok0 & band).any() and np.array_equal(ok, ok0 & ~band)
        assert _recount({**base, "lv": lv}, stride)[0] == list(np.flatnonzero(ok))
        # a white patch in the live image: the samples in it whose residual now exceeds intensity_max
        il = base["il"].copy()
        il[6:42, 6:58] = 1.0
        _, _, ok, _, _ = _terms(base, stride, il=il)
        patch = (rows >= 6) & (rows < 42) & (cols >= 6) & (cols < 58)
        c0 = base["il"][::stride, ::stride].reshape(-1).astype(np.float64)[ok0] - r0       # the interpolated reference
        over = np.zeros(n_s, bool)
        over[np.flatnonzero(ok0)] = np.abs(1.0 - c0) > 0.3
        assert (ok0 & patch & over).sum() > 20 and (ok0 & patch & ~over).sum() > 20
        assert np.array_equal(ok, ok0 & ~(patch & over))
        assert _recount({**base, "il": il}, stride)[0] == list(np.flatnonzero(ok))


def test_grey_is_the_integer_luma():
    rgb = np.array([[[0, 0, 0], [255, 255, 255], [255, 0, 0]], [[0, 255, 0], [0, 0, 255], [12, 200, 77]]], np.uint8)
    want = np.array([[0, 255, 77], [149, 29, (77 * 12 + 150 * 200 + 29 * 77 + 128) >> 8]], np.float32) / np.float32(255)
    got = P.grey(rgb)
    assert got.dtype == np.float32 and np.array_equal(got, want) and got[0, 1] == 1.0
