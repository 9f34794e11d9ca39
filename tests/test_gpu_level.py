"""Levelling on the GPU: the four kernels of bf_level.hip against the numpy restatement in tests/level_ref.py, bit for
bit (centroids, normals, weights, histograms, scores, sums, height bins and the stats), and the layers above them:
level_mesh on a fused volume, `sens track --from-scratch --level` and the scene_level command line.

The bound of the tracked-and-levelled run is 1.5 x the restatement's own chain figures, which test_level_host.py
records and re-measures (CHAIN_HEIGHT 0.0644 voxels, CHAIN_GRAVITY 0.1022 degrees): the margin covers the device
tracker's different rounding, and the bound is never taken from the device's result."""
import json

import numpy as np
import pytest
import torch

from tests import level_ref as LR
from tests import sens_util as U
from tests import track_ref as TR
from tests.test_level_host import CHAIN_GRAVITY, CHAIN_HEIGHT, FLOOR_TOL, rotation_angle

pytestmark = pytest.mark.gpu

DEV = "cuda"
SIZES = [0, 1, 63, 64, 65, 4097]
AREA_UNIT = np.float32(LR.VOXEL ** 2 / 256)


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from boxfusion_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def SL(L):
    from boxfusion_amd import scene_level
    return scene_level


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(DEV)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _equal(got, ref):
    """a device tensor and the restatement's array: the same bits (NaN included)"""
    ref = np.ascontiguousarray(ref)
    g = got.cpu().numpy()
    if ref.dtype == np.uint32:
        g = g.view(np.uint32)
    assert g.shape == ref.shape and g.dtype == ref.dtype
    return torch.equal(torch.from_numpy(_bits(g).astype(np.int64)), torch.from_numpy(_bits(ref).astype(np.int64)))


def _stats_equal(L, got, ref):
    assert got.dtype == torch.int64 and got.numel() == L.LEVEL_STATS_WORDS
    return torch.equal(got.cpu(), torch.from_numpy(ref))


@pytest.fixture(scope="module")
def room_samples():
    """the tilted room's mesh as samples (the restatement's, uploaded: no fusion needed)"""
    m = LR.room_mesh(30.0, 2)
    p, n, w, _ = LR.face_samples(m["vertices"], m["faces"], AREA_UNIT)
    return dict(m=m, p=p, n=n, w=w)


# ---- face samples -------------------------------------------------------------------------------------------
def _soup(m, seed):
    """m random faces over random vertices; from 63 faces on: a zero-area face, faces with an index out of range, a face
    with a NaN vertex, a face with an infinite one and one large enough to saturate the weight"""
    rng = np.random.default_rng(seed)
    nv = max(3, m // 2 + 3)
    v = rng.uniform(-1.0, 1.0, (nv, 3)).astype(np.float32) * np.float32(0.3)
    f = rng.integers(0, nv, (m, 3)).astype(np.int32)
    planted = dict(face_zero_area=0, face_bad_index=0, face_nonfinite=0, face_saturated=0)
    if m >= 63:
        v = np.concatenate([v, [[np.nan, 0, 0], [np.inf, 0, 0], [-60, -60, 0], [60, -60, 0], [0, 60, 0]]]).astype(np.float32)
        f[5] = [7, 7, 9]
        f[11], f[12] = [0, 1, len(v)], [-1, 2, 3]
        f[20], f[21] = [0, nv, 1], [nv + 1, 2, 3]
        f[30] = [nv + 2, nv + 3, nv + 4]
        planted = dict(face_zero_area=1, face_bad_index=2, face_nonfinite=2, face_saturated=1)
    return v, f, planted


@pytest.mark.parametrize("m", SIZES)
def test_face_samples(L, m):
    v, f, planted = _soup(m, m)
    ref = LR.face_samples(v, f, AREA_UNIT)
    c, n, w, st = L.level_face_samples(_dev(v), _dev(f), AREA_UNIT)
    torch.cuda.synchronize()
    assert _equal(c, ref[0]) and _equal(n, ref[1]) and _equal(w, ref[2]) and _stats_equal(L, st, ref[3])
    named = dict(zip(L.LEVEL_STATS, ref[3].tolist()))
    assert named["faces"] == m
    for k, least in planted.items():
        assert named[k] >= least
    if m >= 63:
        assert named["face_saturated"] == 1 and int(ref[2][30]) == L.LEVEL_WEIGHT_CAP
        assert np.isnan(ref[1][[5, 11, 12, 20, 21]]).all() and (ref[2][[5, 11, 12, 20, 21]] == 0).all()


def test_face_samples_room_normals_point_to_free_space(L, room_samples):
    m = room_samples["m"]
    c, n, w, st = L.level_face_samples(_dev(m["vertices"]), _dev(m["faces"]), AREA_UNIT)
    assert _equal(c, room_samples["p"]) and _equal(n, room_samples["n"]) and _equal(w, room_samples["w"])
    eye = m["poses"][0][:3, 3]                                   # a camera inside the room sees every face's front
    fin = room_samples["w"] > 0
    assert (LR.dot(room_samples["n"][fin], (eye - room_samples["p"][fin])) > 0).mean() > 0.99


def test_face_samples_argument_errors(L):
    v, f, _ = _soup(4, 0)
    for unit in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(L.HipError):
            L.level_face_samples(_dev(v), _dev(f), unit)
    with pytest.raises(L.HipError):
        L.level_face_samples(_dev(v), _dev(f.astype(np.int64)), AREA_UNIT)


# ---- vote ---------------------------------------------------------------------------------------------------
SPECIAL = np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1], [1, 1, 0], [-1, 0, 1], [0, 1, -1], [1, 1, 1], [-1, -1, -1],
                    [1, 0.5, 0], [1, 0.0625, -0.5], [2, -1, 0.125], [0, 0, 0], [np.nan, 0, 1], [0, np.inf, 0]], np.float32)


def _normals(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, 3)).astype(np.float32)
    with np.errstate(all="ignore"):
        x = x / np.sqrt((x * x).sum(1, keepdims=True)).astype(np.float32)
    w = rng.integers(0, 300, n).astype(np.uint32)
    k = min(n, len(SPECIAL))
    x[:k] = SPECIAL[:k]                                         # on an axis, on a cube-face tie, on a bin edge, unusable
    if n > 20:
        w[:k] = 7
        w[15], w[16], w[17] = 0, 65536, 0xFFFFFFFF              # skipped; past the LDS table's width: straight to memory
    return x, w


@pytest.mark.parametrize("G", [4, 32])
@pytest.mark.parametrize("n", SIZES)
def test_vote(L, n, G):
    x, w = _normals(n, 100 + n)
    hist, st = LR.vote(x, w, G)
    got, gst = L.level_vote(_dev(x), _dev(w), G)
    torch.cuda.synchronize()
    assert got.dtype == torch.int64 and _equal(got, hist) and _stats_equal(L, gst, st)
    assert int(hist.sum()) == dict(zip(L.LEVEL_STATS, st.tolist()))["vote_weight"]
    if n == 4097:                                               # the same bits for any order of the samples
        perm = np.random.default_rng(n).permutation(n)
        again, _ = L.level_vote(_dev(x[perm]), _dev(w[perm]), G)
        assert torch.equal(again, got)
        twice, _ = L.level_vote(_dev(x), _dev(w), G, hist=got.clone())      # added to, not written
        assert torch.equal(twice, 2 * got)


@pytest.mark.parametrize("G", [4, 32])
def test_vote_one_bin(L, G):
    """every sample in one bin, small and large weights mixed: contention on one word"""
    n = 4097
    x = np.tile(np.array([[0.6, 0.0, 0.8]], np.float32), (n, 1))
    w = np.random.default_rng(5).integers(1, 1000, n).astype(np.uint32)
    w[::97] = 0xFFFFFFF0
    hist, st = LR.vote(x, w, G)
    assert (hist != 0).sum() == 1
    got, gst = L.level_vote(_dev(x), _dev(w), G)
    assert _equal(got, hist) and _stats_equal(L, gst, st)


def test_vote_room(L, room_samples):
    hist, st = LR.vote(room_samples["n"], room_samples["w"], 32)
    got, gst = L.level_vote(_dev(room_samples["n"]), _dev(room_samples["w"]), 32)
    assert _equal(got, hist) and _stats_equal(L, gst, st)


def test_vote_argument_errors(L):
    x, w = _normals(8, 0)
    for G in (0, 33):
        with pytest.raises(L.HipError):
            L.level_vote(_dev(x), _dev(w), G)
    with pytest.raises(L.HipError):
        L.level_vote(_dev(x), _dev(w[:5]), 4)


# ---- score --------------------------------------------------------------------------------------------------
def _score(L, hist, G, cand, cos_par, sin_perp):
    ref = LR.score(hist, G, cand, cos_par, sin_perp)
    got = L.level_score(_dev(hist), G, _dev(np.asarray(cand, np.int32)), cos_par, sin_perp)
    torch.cuda.synchronize()
    assert got.dtype == torch.int64 and _equal(got, ref)
    return ref


def test_score_every_candidate(L):
    G = 4
    hist = np.random.default_rng(3).integers(0, 1 << 40, 6 * G * G).astype(np.int64)
    hist[::5] = 0
    tau = np.radians(20.0)
    ref = _score(L, hist, G, np.arange(6 * G * G), np.float32(np.cos(tau)), np.float32(np.sin(tau)))
    assert (ref[:, 0] >= hist).all() and (ref.sum(1) <= hist.sum()).all() and (ref[:, 1] > 0).any()
    # a candidate outside the table scores nothing
    out = _score(L, hist, G, [-1, 5, 6 * G * G, 0], np.float32(np.cos(tau)), np.float32(np.sin(tau)))
    assert (out[[0, 2]] == 0).all() and (out[1] == ref[5]).all()


def test_score_room_cone(L, SL, room_samples):
    G = 32
    hist, _ = LR.vote(room_samples["n"], room_samples["w"], G)
    prior = SL.prior_from_poses(room_samples["m"]["poses"])
    cand = np.nonzero(SL.bin_directions(G).astype(np.float64) @ prior >= np.cos(np.radians(40.0)))[0]
    assert 500 < len(cand) < 1000
    tau = np.radians(10.0)
    ref = _score(L, hist, G, cand, np.float32(np.cos(tau)), np.float32(np.sin(tau)))
    assert ref.sum(1).max() > 0.8 * hist.sum()                  # the room's up is in the cone


def test_score_empty_and_single_bin(L):
    G = 32
    hist = np.zeros(6 * G * G, np.int64)
    hist[1234] = (1 << 62) + 5
    assert _score(L, hist, G, np.zeros(0, np.int32), np.float32(0.9), np.float32(0.1)).shape == (0, 2)
    ref = _score(L, hist, G, np.arange(0, 6 * G * G, 7), np.float32(0.98), np.float32(0.17))
    assert set(np.unique(ref).tolist()) == {0, (1 << 62) + 5}
    with pytest.raises(L.HipError):
        L.level_score(_dev(hist), 4, _dev(np.zeros(1, np.int32)), 0.9, 0.1)


# ---- refine -------------------------------------------------------------------------------------------------
def _frame(SL, c):
    c = np.asarray(c, np.float64)
    c = c / np.linalg.norm(c)
    return np.concatenate([c, *SL.horizontal_basis(c)]).astype(np.float32)


def _refine(L, p, n, w, frame, cos_par, sin_perp, h0, hb, nb):
    ref = LR.refine(p, n, w, frame, cos_par, sin_perp, h0, hb, nb)
    got = L.level_refine(_dev(p), _dev(n), _dev(w), _dev(frame), cos_par, sin_perp, h0, hb, nb)
    torch.cuda.synchronize()
    assert _equal(got[0], ref[0]) and _equal(got[1], ref[1]) and _stats_equal(L, got[2], ref[2])
    return ref, got


def test_refine_room(L, SL, room_samples):
    s = room_samples
    up = s["m"]["A"][:3, :3] @ np.array([0.02, -0.03, 1.0])      # near the tilted room's up, not on it
    frame = _frame(SL, up)
    tau = np.radians(10.0)
    args = (frame, np.float32(np.cos(tau)), np.float32(np.sin(tau)))
    (sums, heights, st), got = _refine(L, s["p"], s["n"], s["w"], *args, np.float32(-3.0), np.float32(LR.VOXEL), 120)
    named = dict(zip(L.LEVEL_STATS, st.tolist()))
    assert named["refine_par"] > 500 and named["refine_perp"] > 1000 and named["refine_outside"] == 0
    assert heights[:, 0].sum() == named["refine_weight_up"] and sums[12] != 0 and sums[13] != 0
    # a range that misses the floor: the upward samples are counted as outside
    (_, narrow, st2), _ = _refine(L, s["p"], s["n"], s["w"], *args, np.float32(2.0), np.float32(LR.VOXEL), 3)
    assert dict(zip(L.LEVEL_STATS, st2.tolist()))["refine_outside"] == named["refine_up"] and not narrow.any()
    # no height histogram at all
    (_, none, st3), _ = _refine(L, s["p"], s["n"], s["w"], *args, np.float32(0.0), np.float32(1.0), 0)
    assert none.shape == (0, L.LEVEL_HEIGHT_WORDS) and dict(zip(L.LEVEL_STATS, st3.tolist()))["refine_outside"] == named["refine_up"]
    # the same bits when the samples are permuted
    perm = np.random.default_rng(9).permutation(len(s["w"]))
    again = L.level_refine(_dev(s["p"][perm]), _dev(s["n"][perm]), _dev(s["w"][perm]), _dev(frame), args[1], args[2],
                           np.float32(-3.0), np.float32(LR.VOXEL), 120)
    assert all(torch.equal(a, b) for a, b in zip(again, got))


@pytest.mark.parametrize("n", [0, 1, 65, 4097])
def test_refine_sizes(L, SL, n):
    rng = np.random.default_rng(n)
    x, w = _normals(n, 200 + n)
    p = rng.uniform(-2.0, 2.0, (n, 3)).astype(np.float32)
    if n > 20:
        p[3, 1], p[4, 0] = np.nan, 3.0e6                        # skipped; past the coordinate limit: outside
        w[18] = 0xFFFFFFFF
    frame = _frame(SL, [0.1, -0.2, 1.0])
    tau = np.radians(30.0)                                      # wide, so that random normals fill every set
    (sums, heights, st), _ = _refine(L, p, x, w, frame, np.float32(np.cos(tau)), np.float32(np.sin(tau)), np.float32(-1.0),
                                     np.float32(0.25), 6)
    if n == 4097:
        named = dict(zip(L.LEVEL_STATS, st.tolist()))
        assert named["refine_outside"] > 0 and heights[:, 0].all() and named["refine_skipped"] >= 3 and sums.all()


def test_refine_argument_errors(L, SL):
    x, w = _normals(8, 0)
    frame = _frame(SL, [0, 0, 1])
    for h0, hb, nb in ((0.0, 0.0, 4), (0.0, -1.0, 4), (float("nan"), 0.1, 4), (0.0, 0.1, L.LEVEL_MAX_HEIGHT_BINS + 1),
                       (0.0, 2048.0, 1024)):
        with pytest.raises(L.HipError):
            L.level_refine(_dev(x), _dev(x), _dev(w), _dev(frame), 0.9, 0.1, h0, hb, nb)


# ---- the layers above -----------------------------------------------------------------------------------------
def test_level_mesh_on_a_volume(L, SL):
    """a TsdfVolume fused on the device from the tilted room: the restatement's Levelling, sum for sum"""
    from boxfusion_amd.scene_mesh import TsdfVolume
    m = LR.room_mesh(30.0, 2)
    vol = TsdfVolume(voxel=LR.VOXEL, trunc_voxels=TR.ROOM_VOLUME["T"], capacity=2048, max_depth=TR.ROOM_VOLUME["max_depth"])
    vol.integrate(_dev(np.stack(m["room"].depths())), m["room"].K, m["poses"])
    got = SL.level_mesh(vol, poses=m["poses"])
    ref = LR.level_mesh((m["vertices"], m["faces"]), poses=m["poses"], voxel=LR.VOXEL)
    assert got.ok and ref.ok
    for k in ("hist", "candidates", "scores", "vote_stats"):
        assert np.array_equal(got.trace[k], ref.trace[k])
    assert len(got.trace["passes"]) == len(ref.trace["passes"]) == 4
    for a, b in zip(got.trace["passes"], ref.trace["passes"]):
        assert np.array_equal(a["frame"], b["frame"]) and np.array_equal(a["sums"], b["sums"]) and np.array_equal(a["stats"], b["stats"])
    assert np.array_equal(got.trace["passes"][-1]["heights"], ref.trace["passes"][-1]["heights"])
    assert np.array_equal(got.T, ref.T) and got.stats == ref.stats and got.floor == ref.floor and got.share == ref.share
    up, wall, floor = LR.room_errors(got, m["A"], m["room"])
    assert floor <= FLOOR_TOL
    # estimate over the same samples, given as tensors
    v, _, f = vol.mesh()
    c, n, w, _ = L.level_face_samples(v, f, AREA_UNIT)
    again = SL.estimate(c, n, w, poses=m["poses"], height_bin=LR.VOXEL)
    assert np.array_equal(again.T, ref.T)
    with pytest.raises(ValueError):
        SL.estimate(c, n, w, (0, 0, 1), height_bin=LR.VOXEL, cone_deg=45.0)


@pytest.fixture(scope="module")
def capture(tmp_path_factory):
    """the room as a .sens file without poses: tracking starts at identity, in the first camera's frame"""
    room = TR.Room()
    rng = np.random.default_rng(2)
    colors = [U.jpeg_bytes(rng.integers(0, 256, (room.H, room.W, 3), dtype=np.uint8)) for _ in room.poses]
    mm = [TR.quantise_mm(d)[0] for d in room.depths()]
    Kd = np.eye(4, dtype=np.float32)
    Kd[:3, :3] = room.K
    path = tmp_path_factory.mktemp("level") / "room.sens"
    U.write_sens(path, colors, mm, np.tile(TR.LOST, (len(mm), 1, 1)), (room.H, room.W), intrinsic_depth=Kd)
    return dict(path=path, room=room)


TRACK_ARGS = ["--from-scratch", "--voxel", "0.05", "--trunc-voxels", "3", "--max-depth", "4", "--capacity", "2048"]


def test_sens_track_level(L, capture, tmp_path, capsys):
    from boxfusion_amd import sens as S
    from boxfusion_amd.sensor import camera_to_gravity
    from boxfusion_amd.visualize import read_ply_surface
    room = capture["room"]
    out, ply = tmp_path / "poses.npy", tmp_path / "room.ply"
    assert S.main(["track", str(capture["path"]), str(out), *TRACK_ARGS, "--level", "--mesh", str(ply)]) == 0
    lines = capsys.readouterr().out.splitlines()
    print("\n".join(lines))
    assert "8 frames: 7 tracked, 0 lost" in lines[0]
    assert lines[1].startswith("levelled: moved ") and lines[1].endswith("ok True")
    assert float(lines[1].split("share ")[1].split(",")[0]) >= 0.8 and "floor " in lines[1]
    poses = np.load(out)
    assert poses.dtype == np.float32 and poses.shape == (8, 4, 4) and np.isfinite(poses).all()
    height = max(abs(g[2, 3] - (t[2, 3] - room.lo[2])) for g, t in zip(poses, room.poses)) / LR.VOXEL
    gravity = max(rotation_angle(camera_to_gravity(g), camera_to_gravity(t)) for g, t in zip(poses, room.poses))
    print(f"camera height {height:.4f} voxels, gravity {gravity:.4f} deg")
    assert height <= 1.5 * CHAIN_HEIGHT and gravity <= 1.5 * CHAIN_GRAVITY
    # --mesh: the surface fused again from the levelled poses has its floor at z = 0
    v, _, f = read_ply_surface(str(ply))
    _, n, w, _ = LR.face_samples(v, f, AREA_UNIT)
    floor = np.unique(f[(n[:, 2] >= np.cos(np.radians(5.0))) & (w > 0)])
    assert len(floor) > 300 and abs(float(v[floor, 2].mean())) / LR.VOXEL <= 1.5 * CHAIN_HEIGHT


def test_sens_track_without_level_is_unchanged(L, capture, tmp_path, capsys):
    from boxfusion_amd import sens as S
    out = tmp_path / "poses.npy"
    assert S.main(["track", str(capture["path"]), str(out), *TRACK_ARGS]) == 0
    text = capsys.readouterr().out
    assert text == f"8 frames: 7 tracked, 0 lost -> {out}\n"
    with S.SensFile(str(capture["path"])) as s:
        plain = S.track(s, "from-scratch", 0.05, 3, max_depth=4.0, capacity=2048)
    assert len(plain) == 4
    again = tmp_path / "again.npy"
    np.save(again, plain[0])
    assert out.read_bytes() == again.read_bytes()
    assert np.array_equal(plain[0][0], np.eye(4, dtype=np.float32))             # unlevelled: the first camera's frame


def test_scene_level_command(L, SL, tmp_path, capsys):
    from boxfusion_amd.visualize import mesh_to_ply, read_ply_surface
    m = LR.room_mesh(15.0, 1)
    src, dst, js = tmp_path / "in.ply", tmp_path / "out.ply", tmp_path / "level.json"
    mesh_to_ply(m["vertices"], np.full((len(m["vertices"]), 3), 200, np.uint8), m["faces"], str(src))
    np.save(tmp_path / "poses.npy", m["poses"])
    assert SL.main([str(src), str(dst), "--voxel", str(LR.VOXEL), "--poses", str(tmp_path / "poses.npy"), "--poses-out",
                    str(tmp_path / "levelled.npy"), "--json", str(js)]) == 0
    assert capsys.readouterr().out.startswith("levelled: moved ")
    v, rgb, f = read_ply_surface(str(dst))
    assert np.array_equal(f, m["faces"]) and (rgb == 200).all()
    _, n, w, _ = LR.face_samples(v, f, AREA_UNIT)
    floor = np.unique(f[(n[:, 2] >= np.cos(np.radians(5.0))) & (w > 0)])
    assert len(floor) > 300 and abs(float(v[floor, 2].mean())) / LR.VOXEL <= FLOOR_TOL
    ref = LR.level_mesh((m["vertices"], m["faces"]), poses=m["poses"], voxel=LR.VOXEL)
    info = json.loads(js.read_text())
    assert set(info) == set(ref.to_json()) and info["ok"] is True and np.array_equal(np.array(info["T"]), ref.T)
    assert np.array_equal(np.load(tmp_path / "levelled.npy"), ref.apply(m["poses"]))
    # not a room: reported, nothing written
    flat = tmp_path / "ball.ply"
    rng = np.random.default_rng(0)
    bv = rng.normal(size=(300, 3)).astype(np.float32)
    mesh_to_ply(bv, np.zeros((300, 3), np.uint8), rng.integers(0, 300, (500, 3)).astype(np.int32), str(flat))
    assert SL.main([str(flat), str(tmp_path / "none.ply"), "--voxel", "0.5"]) == 1
    assert "warning" in capsys.readouterr().err and not (tmp_path / "none.ply").exists()
    with pytest.raises(SystemExit):
        SL.main([str(src), str(dst), "--cone", "45"])
