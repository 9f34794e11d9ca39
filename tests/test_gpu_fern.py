"""Fern relocalisation on the GPU (bf_fern.hip, tracking.Relocaliser, track_sequence(relocaliser=...), `sens track
--relocalise`) against the numpy restatement in tests/fern_ref.py.  Cell means, codes, distances, the top-k and the
conditional append are integers: they must equal the restatement bit for bit.  The kidnap scene shows the behaviour
gained: two views the tracker cannot place from the last good pose come back through the keyframes.

The issue's scene (frames 0-13) has the two new views back to back: under the loop's own rule the second is tracked
from the first one's relocalised pose (2882 of 3072 inliers in the restatement), so it needs no relocalisation.  That
run is held to the restatement as it is; the variant that shows the last wall view again between the two (frames 0-14,
fern_ref.kidnap_scene(twice=True)) is the one in which both are relocalised."""
import ctypes

import numpy as np
import pytest
import torch

from tests import fern_ref as FR
from tests import sens_util as U
from tests import track_ref as TR

pytestmark = pytest.mark.gpu

DEV = "cuda"
RV = TR.ROOM_VOLUME
KD = FR.KIDNAP
# the allowance tests/test_gpu_track.py grants one borderline association
POSE_VS_RESTATEMENT_M, POSE_VS_RESTATEMENT_DEG = 1e-5, 1e-3
# the restatement's own error against the true poses over the relocalised frames, measured on the CPU
# (test_fern_host.py: 0.388 mm / 0.0247 degrees and 0.252 mm / 0.0218 degrees), rounded up; the bound is 1.5 x
RESTATEMENT_M, RESTATEMENT_DEG = 0.00039, 0.025


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from boxfusion_amd import _lib
    _lib.lib()
    return _lib


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _volume(capacity=1 << 11):
    from boxfusion_amd.scene_mesh import TsdfVolume
    return TsdfVolume(voxel=RV["voxel"], trunc_voxels=RV["T"], capacity=capacity, max_depth=RV["max_depth"], device=DEV)


def _relocaliser():
    from boxfusion_amd.tracking import Relocaliser
    room = TR.Room()
    return Relocaliser(room.H, room.W, DEV, ferns=KD["ferns"], cell=KD["cell"], harvest=KD["harvest"], seed=KD["seed"],
                       depth_range=KD["depth_range"], max_depth=RV["max_depth"])


# ---- 1. encode -----------------------------------------------------------------------------------------------------
def _frames(B, H, W, seed):
    """depth that varies from block to block across the thresholds' range, and colour likewise, with pixel noise"""
    rng = np.random.default_rng(seed)
    up = np.ones((4, 4))
    hb, wb = -(-H // 4), -(-W // 4)
    depth = np.stack([np.kron(rng.uniform(0.3, 3.4, (hb, wb)), up)[:H, :W] for _ in range(B)]) + rng.normal(0, 0.01, (B, H, W))
    rgb = np.stack([np.stack([np.kron(rng.uniform(0, 255, (hb, wb)), up)[:H, :W] for _ in range(3)], -1) for _ in range(B)])
    rgb = np.clip(rgb + rng.normal(0, 6, rgb.shape), 0, 255)
    return depth.astype(np.float32), np.rint(rgb).astype(np.uint8)


def _assert_encode(L, depth, rgb, cell, ferns, max_depth=4.0, seed=0, dev_depth=None):
    from boxfusion_amd.tracking import fern_table
    B, H, W = depth.shape
    cells = (H // cell) * (W // cell)
    table = fern_table(ferns, cells, seed, (0.4, 3.0))
    dt = L.fern_upload(table, cells, DEV)
    d = _dev(depth) if dev_depth is None else dev_depth
    c = None if rgb is None else _dev(rgb)
    codes, means = L.fern_encode(d, c, cell, max_depth, dt, with_means=True)
    only = L.fern_encode(d, c, cell, max_depth, dt)
    assert codes.dtype == torch.int32 and tuple(codes.shape) == (B, ferns // 8) and tuple(means.shape) == (B, cells, 4)
    assert torch.equal(codes, only)
    want = [FR.encode(depth[b], None if rgb is None else rgb[b], cell, max_depth, table) for b in range(B)]
    assert np.array_equal(means.cpu().numpy(), np.stack([w[1] for w in want]))
    assert np.array_equal(_u32(codes), np.stack([w[0] for w in want]))
    if B == 1:                                                   # a single frame without the batch axis
        assert torch.equal(L.fern_encode(d[0], None if c is None else c[0], cell, max_depth, dt), codes)
    return np.stack([w[0] for w in want]), np.stack([w[1] for w in want])


@pytest.mark.parametrize("H,W,cell,ferns", [(48, 64, 4, 256), (48, 64, 16, 64), (37, 53, 4, 64), (48, 64, 5, 64), (48, 64, 8, 512)])
def test_encode_is_the_restatement(L, H, W, cell, ferns):
    depth, rgb = _frames(2, H, W, seed=H + cell)
    codes, means = _assert_encode(L, depth, rgb, cell, ferns)
    assert means.shape[1] == (H // cell) * (W // cell)
    nib = np.stack([FR.unpack(c) for c in codes])
    assert all((nib >> b & 1).any() and not (nib >> b & 1).all() for b in range(4))     # every bit takes both values
    _assert_encode(L, depth[:1], rgb[:1], cell, ferns, seed=1)
    # without an image the colour bits are zero
    codes, means = _assert_encode(L, depth, None, cell, ferns)
    assert not means[..., :3].any() and not (np.stack([FR.unpack(c) for c in codes]) & 7).any()


def test_encode_room_frames_and_an_unaligned_frame(L):
    s = FR.kidnap_scene()
    _assert_encode(L, np.stack(s["depths"][2:5]), np.stack(s["rgbs"][2:5]), 4, 256, max_depth=RV["max_depth"])
    # a depth map that starts 4 bytes into its buffer: the rows cannot be read as vectors
    depth, rgb = _frames(1, 48, 64, seed=9)
    buf = torch.zeros(48 * 64 + 1, dtype=torch.float32, device=DEV)
    buf[1:] = _dev(depth).reshape(-1)
    _assert_encode(L, depth, rgb, 16, 64, dev_depth=buf[1:].view(1, 48, 64))


def test_encode_invalid_depth(L):
    """a band of zero depth, NaN, depth at and beyond max_depth, a cell with exactly half its pixels valid (valid) and a
    cell with one pixel fewer (invalid)"""
    depth, rgb = _frames(3, 48, 64, seed=3)
    depth = np.clip(depth, 0.3, 3.9)
    depth[0, 10:22] = 0.0                                        # cells of rows 8-11 half, 12-19 wholly, 20-23 half empty
    depth[1, 5, 7] = depth[1, 6, 6] = np.nan
    depth[1, 16:20, 0:8] = np.nan
    depth[1, 24:32, 16:24] = 4.0                                 # at max_depth
    depth[1, 24:32, 24:32] = np.nextafter(np.float32(4.0), np.float32(0))
    depth[1, 32:40, 0:8] = 7.5
    depth[1, 40:44, 0:4] = -1.0
    depth[2, 0:2, 0:4] = 0.0                                     # cell (0, 0) of 4 x 4: 8 of 16 valid
    depth[2, 0:2, 4:8] = 0.0                                     # cell (0, 1): 7 of 16
    depth[2, 2, 4] = np.inf
    for cell, ferns in ((4, 256), (16, 64)):
        codes, means = _assert_encode(L, depth, rgb, cell, ferns)
        _assert_encode(L, depth, None, cell, ferns)
    m = FR.cell_means(depth[2], None, 4, 4.0).reshape(12, 16, 4)
    assert m[0, 0, 3] > 0 and m[0, 1, 3] == -1
    m = FR.cell_means(depth[0], None, 4, 4.0).reshape(12, 16, 4)
    assert (m[2, :, 3] > 0).all() and (m[3:5, :, 3] == -1).all() and (m[5, :, 3] > 0).all()
    m = FR.cell_means(depth[1], None, 4, 4.0).reshape(12, 16, 4)
    assert (m[6:8, 4:6, 3] == -1).all() and (m[6:8, 6:8, 3] == 4000).all() and (m[8:10, 0:2, 3] == -1).all() and m[10, 0, 3] == -1


def test_encode_out_of_range_cell_is_nibble_zero(L):
    """the upload check refuses such a table; a kernel handed one all the same reads no pixel for that fern"""
    from boxfusion_amd.tracking import fern_table
    depth, rgb = _frames(1, 48, 64, seed=4)
    table = fern_table(64, 12, 0, (0.4, 3.0))
    table[:, 1:] = -1                                            # every bit of a valid cell is set
    table[[5, 40], 0] = [12, -1]
    codes = L.fern_encode(_dev(depth), _dev(rgb), 16, 4.0, _dev(table))
    nib = FR.unpack(_u32(codes)[0])
    assert nib[5] == 0 and nib[40] == 0 and (np.delete(nib, [5, 40]) == 15).all()


# ---- 2. search -----------------------------------------------------------------------------------------------------
def _codes(rng, rows, words):
    return rng.integers(0, 1 << 32, (rows, words), dtype=np.uint64).astype(np.uint32)


@pytest.mark.parametrize("ferns", [64, 256])
@pytest.mark.parametrize("n", [1, 7, 65, 300])
def test_search_is_the_restatement(L, ferns, n):
    rng = np.random.default_rng(ferns + n)
    words, capacity = ferns // 8, 320
    table = _codes(rng, capacity, words)
    if n > 5:                                                    # duplicated rows: ties go to the lower index
        table[5] = table[2]
        table[n - 1] = table[0]
    # queries a few ferns away from rows of the table, so the nearest are near
    queries = table[[0, 2 % n, n // 2]].copy()
    for q in range(3):
        nib = FR.unpack(queries[q])
        at = rng.choice(ferns, 3 + 2 * q, replace=False)
        nib[at] = (nib[at] + rng.integers(1, 16, len(at))) % 16
        queries[q] = FR.pack(nib)
    dt = _dev(table.view(np.int32))
    for n_dev, n_upper in ((n, n), (n, min(n + 17, capacity)), (max(n - 3, 0), n)):
        nt = torch.tensor([n_dev], dtype=torch.int32, device=DEV)
        for Q in (1, 3):
            dq = _dev(queries[:Q].view(np.int32))
            for k in (1, 4, 8):
                top, rows = L.fern_search(dt, nt, n_upper, dq, k, with_rows=True)
                again, rows2 = L.fern_search(dt, nt, n_upper, dq, k, with_rows=True)
                plain = L.fern_search(dt, nt, n_upper, dq, k)
                assert torch.equal(top, again) and torch.equal(rows, rows2) and torch.equal(top, plain)
                want_top, want_rows = FR.search(table, n_dev, n_upper, queries[:Q], k)
                assert tuple(top.shape) == (Q, k, 2) and tuple(rows.shape) == (Q, n_upper)
                assert np.array_equal(rows.cpu().numpy(), want_rows), (n_dev, n_upper, Q, k)
                assert np.array_equal(top.cpu().numpy(), want_top), (n_dev, n_upper, Q, k)
    if n > 5:                                                    # the tie is there: rows 2 and 5 at the same distance
        top = L.fern_search(dt, torch.tensor([n], dtype=torch.int32, device=DEV), n, _dev(queries[1:2].view(np.int32)), 4)
        top = top.cpu().numpy()[0]
        assert top[0, 0] == top[1, 0] and top[:2, 1].tolist() == [2, 5]
    if n < 8:                                                    # the padding
        top = L.fern_search(dt, torch.tensor([n], dtype=torch.int32, device=DEV), n, _dev(queries[:1].view(np.int32)), 8)
        assert (top.cpu().numpy()[0, n:] == -1).all() and (top.cpu().numpy()[0, :n] >= 0).all()


def test_search_empty_table(L):
    rng = np.random.default_rng(0)
    table, q = _dev(_codes(rng, 16, 8).view(np.int32)), _dev(_codes(rng, 2, 8).view(np.int32))
    top, rows = L.fern_search(table, torch.zeros(1, dtype=torch.int32, device=DEV), 1, q, 4, with_rows=True)
    assert (top == -1).all() and (rows == -1).all()


# ---- 3. append -----------------------------------------------------------------------------------------------------
def test_append_rules(L):
    rng = np.random.default_rng(2)
    words, capacity, threshold = 8, 3, 6
    codes = _codes(rng, 6, words)
    table = torch.zeros((capacity, words), dtype=torch.int32, device=DEV)
    poses = torch.zeros((capacity, 16), dtype=torch.float32, device=DEV)
    ids = torch.full((capacity,), -7, dtype=torch.int32, device=DEV)
    state = torch.zeros(4, dtype=torch.int32, device=DEV)
    want = FR.Table(capacity, words)

    def offer(i, best):
        pose = np.arange(16, dtype=np.float32).reshape(4, 4) + 100 * i
        L.fern_append(table, state[:1], _dev(codes[i].view(np.int32)), torch.tensor([best, 0], dtype=torch.int32, device=DEV),
                      threshold, pose, 10 + i, poses, ids, state[1:])
        want.append(codes[i], best, threshold, pose, 10 + i)
        n = want.n
        assert state.cpu().tolist() == [want.n, want.observed, want.added, want.dropped_full]
        assert np.array_equal(_u32(table)[:n], want.codes[:n]) and np.array_equal(poses.cpu().numpy()[:n], want.poses[:n])
        assert np.array_equal(ids.cpu().numpy()[:n], want.ids[:n])
        return state.cpu().tolist()

    assert offer(0, -1) == [1, 1, 1, 0]                          # the first frame is always added, whatever `best` holds
    assert offer(1, threshold) == [1, 2, 1, 0]                   # distance = threshold: not added
    assert not _u32(table)[1:].any() and (ids.cpu().numpy()[1:] == -7).all()
    assert offer(1, threshold + 1) == [2, 3, 2, 0]               # one more fern: added
    assert offer(2, 0) == [2, 4, 2, 0]
    assert offer(3, 50) == [3, 5, 3, 0]
    held = (table.clone(), poses.clone(), ids.clone())
    assert offer(4, 60) == [3, 6, 3, 1]                          # full: counted, nothing else changes
    assert offer(5, 2) == [3, 7, 3, 1]                           # near a keyframe: not even a candidate for the table
    assert torch.equal(table, held[0]) and torch.equal(poses, held[1]) and torch.equal(ids, held[2])
    assert ids.cpu().tolist() == [10, 11, 13]


# ---- 4. the Relocaliser over the kidnap scene ------------------------------------------------------------------------
def test_relocaliser_harvest_and_query(L):
    s = FR.kidnap_scene()
    rl = _relocaliser()
    assert np.array_equal(rl.table, FR.kidnap_table()) and len(rl) == 0 and rl.query(_dev(s["depths"][0]), _dev(s["rgbs"][0])) == []
    want = FR.Relocaliser(48, 64, FR.kidnap_table(), KD["cell"], harvest=KD["harvest"], max_depth=RV["max_depth"])
    for i in range(12):
        rl.observe(_dev(s["depths"][i]), s["poses"][i], _dev(s["rgbs"][i]), frame=i)
        want.observe(s["depths"][i], s["poses"][i], s["rgbs"][i], frame=i)
    rl.observe(_dev(s["depths"][12]), TR.LOST, _dev(s["rgbs"][12]), frame=12)          # no pose: ignored
    poses, ids, codes = rl.keyframes()
    n = want.kf.n
    print("keyframes", ids.tolist(), rl.counters())
    assert len(rl) == n and 2 < n < 12 and rl.counters() == want.kf.counters() and rl.counters()["observed"] == 12
    assert np.array_equal(ids, want.kf.ids[:n]) and np.array_equal(poses.reshape(n, 16), want.kf.poses[:n])
    assert codes.dtype == np.uint32 and np.array_equal(codes, want.kf.codes[:n])
    for i in (12, 13, 3):
        for k in (1, 4, 8):
            got = rl.query(_dev(s["depths"][i]), _dev(s["rgbs"][i]), k)
            ref = want.query(s["depths"][i], s["rgbs"][i], k)
            assert len(got) == min(k, n) and [g[:2] + g[3:] for g in got] == [r[:2] + r[3:] for r in ref]
            assert all(np.array_equal(g[2], r[2]) and g[2].dtype == np.float32 for g, r in zip(got, ref))
    # arrays from the host and no image work as well
    assert rl.query(s["depths"][12], s["rgbs"][12], 4)[0][:2] == want.query(s["depths"][12], s["rgbs"][12], 4)[0][:2]
    plain, ref = _relocaliser(), FR.Relocaliser(48, 64, FR.kidnap_table(), KD["cell"], harvest=KD["harvest"], max_depth=RV["max_depth"])
    for i in range(12):
        plain.observe(s["depths"][i], s["poses"][i], frame=i)
        ref.observe(s["depths"][i], s["poses"][i], frame=i)
    assert np.array_equal(plain.keyframes()[1], ref.kf.ids[:ref.kf.n]) and not (plain.keyframes()[2] & 0x77777777).any()
    assert [g[:2] for g in plain.query(s["depths"][13])] == [r[:2] for r in ref.query(s["depths"][13])]
    # a full table drops and counts
    from boxfusion_amd.tracking import Relocaliser
    small = Relocaliser(48, 64, DEV, ferns=KD["ferns"], cell=KD["cell"], capacity=2, harvest=KD["harvest"], seed=KD["seed"],
                        depth_range=KD["depth_range"], max_depth=RV["max_depth"])
    for i in range(12):
        small.observe(_dev(s["depths"][i]), s["poses"][i], _dev(s["rgbs"][i]), frame=i)
    c = small.counters()
    assert c["keyframes"] == 2 and c["added"] == 2 and c["dropped_full"] > 0 and c["observed"] == 12
    assert small.keyframes()[1].tolist() == want.kf.ids[:2].tolist()


# ---- 5. track_sequence -------------------------------------------------------------------------------------------------
def _assert_run(poses, infos, ref, what):
    unknown = list(ref["unknown"])
    assert [bool(i["lost"]) for i in infos] == [bool(i["lost"]) for i in ref["infos"]]
    assert [bool(i["tracked"]) for i in infos] == [bool(i["tracked"]) for i in ref["infos"]]
    assert [i["relocalised"] for i in infos] == [i["relocalised"] for i in ref["infos"]]
    known = [k for k in range(len(infos)) if k not in unknown]
    assert np.array_equal(poses[known], ref["known"][known])
    for k in unknown:
        a, b = infos[k], ref["infos"][k]
        assert not a["lost"] and np.isfinite(poses[k]).all()
        if b["relocalised"]:
            assert (a["keyframe"], a["fern_distance"], a["candidates_tried"]) == (b["keyframe"], b["fern_distance"], b["candidates_tried"])
        assert abs(a["inliers"] - b["inliers"]) <= 2 and a["iterations"] == b["iterations"]            # as test_gpu_track.py
        dt, dr = TR.pose_error(poses[k], ref["got"][k])
        et, er = TR.pose_error(poses[k], ref["poses"][k])
        wt, wr = TR.pose_error(ref["got"][k], ref["poses"][k])
        print(f"{what}, frame {k}: relocalised {a['relocalised']} keyframe {a.get('keyframe')} at {a.get('fern_distance')}; against the "
              f"restatement {dt:.3e} m {dr:.3e} deg; against the truth {et * 1000:.3f} mm {er:.4f} deg (restatement "
              f"{wt * 1000:.3f} mm {wr:.4f} deg)")
        assert dt <= POSE_VS_RESTATEMENT_M and dr <= POSE_VS_RESTATEMENT_DEG
        assert wt <= 1.5 * RESTATEMENT_M and wr <= 1.5 * RESTATEMENT_DEG


@pytest.mark.parametrize("twice", [False, True])
def test_track_sequence_relocalises(L, twice):
    from boxfusion_amd.tracking import track_sequence
    ref = FR.kidnap_reference(twice)
    room, unknown = ref["room"], list(ref["unknown"])
    depths, colours = _dev(np.stack(ref["depths"])), _dev(np.stack(ref["rgbs"]))
    # today's behaviour: the camera moved on while it was lost, and the frames stay lost
    without, winfos = track_sequence(depths, room.K, known_poses=ref["known"], volume=_volume(), colours=colours, **TR.TRACKER)
    assert np.isneginf(without[unknown]).all() and all(winfos[k]["lost"] for k in unknown)
    assert all("relocalised" not in i for i in winfos)
    rl = _relocaliser()
    poses, infos = track_sequence(depths, room.K, known_poses=ref["known"], volume=_volume(), colours=colours, relocaliser=rl,
                                  **TR.TRACKER)
    _assert_run(poses, infos, ref, "twice" if twice else "kidnap")
    assert infos[12]["relocalised"] and not any(infos[k]["relocalised"] for k in range(12))
    if twice:                                                    # each new view arrives while the camera is at the wall
        assert all(infos[k]["relocalised"] for k in unknown)
    assert rl.counters() == ref["rl"].kf.counters() and np.array_equal(rl.keyframes()[1], ref["rl"].kf.ids[:ref["rl"].kf.n])


def test_relocalise_gives_up_beyond_max_distance(L):
    """no candidate within max_distance: nothing is tried and the frame stays lost"""
    from boxfusion_amd.tracking import IcpTracker
    s = FR.kidnap_scene()
    room = s["room"]
    vol, rl = _volume(), _relocaliser()
    for i in range(12):
        vol.integrate(_dev(s["depths"][i]), room.K, s["poses"][i][None])
        rl.observe(_dev(s["depths"][i]), s["poses"][i], _dev(s["rgbs"][i]), i)
    tr = IcpTracker(vol, room.K, room.H, room.W, **TR.TRACKER)
    nearest = rl.query(_dev(s["depths"][12]), _dev(s["rgbs"][12]), 1)[0][0]
    assert nearest > 0.1 * KD["ferns"]
    pose, info = rl.relocalise(tr, _dev(s["depths"][12]), _dev(s["rgbs"][12]), max_distance=0.1)
    assert np.isneginf(pose).all() and info["lost"] and not info["relocalised"] and info["candidates_tried"] == 0
    assert tr._ref is None
    pose, info = rl.relocalise(tr, _dev(s["depths"][12]), _dev(s["rgbs"][12]), k=1)
    assert not info["lost"] and info["relocalised"] and info["fern_distance"] == nearest and info["candidates_tried"] == 1
    assert TR.pose_error(pose, s["poses"][12])[0] <= 1.5 * RESTATEMENT_M + POSE_VS_RESTATEMENT_M and tr._ref is not None


# ---- 6. through a .sens file -------------------------------------------------------------------------------------------
def test_sens_track_relocalise(L, tmp_path, capsys):
    from boxfusion_amd import sens as S
    ref = FR.kidnap_reference(True)
    room, unknown = ref["room"], list(ref["unknown"])
    Kd = np.eye(4, dtype=np.float32)
    Kd[:3, :3] = room.K
    path = tmp_path / "kidnap.sens"
    U.write_sens(path, [U.jpeg_bytes(im) for im in ref["rgbs"]], [TR.quantise_mm(d)[0] for d in ref["depths"]], ref["known"],
                 (room.H, room.W), intrinsic_depth=Kd)
    out = tmp_path / "poses.npy"
    argv = ["track", str(path), str(out), "--voxel", "0.05", "--trunc-voxels", "3", "--max-depth", "4", "--capacity", "2048"]
    assert S.main(argv) == 0
    line = capsys.readouterr().out
    assert "15 frames: 0 tracked, 2 lost" in line and "relocalised" not in line and np.isneginf(np.load(out)[unknown]).all()
    assert S.main(argv + ["--relocalise", "--ferns", str(KD["ferns"]), "--fern-cell", str(KD["cell"]), "--harvest",
                          str(KD["harvest"])]) == 0
    line = capsys.readouterr().out
    assert "15 frames: 2 tracked, 0 lost, 2 relocalised" in line
    poses = np.load(out)
    assert np.isfinite(poses).all()
    for k in unknown:
        et, er = TR.pose_error(poses[k], ref["poses"][k])
        print(f"frame {k}: {et * 1000:.3f} mm {er:.4f} deg")
        # the restatement's bound plus what depth in whole millimetres can add: half a millimetre, and that over the
        # metre the view spans as an angle
        assert et <= 1.5 * RESTATEMENT_M + 0.0005 and er <= 1.5 * RESTATEMENT_DEG + np.degrees(0.0005)
    for bad in (["--ferns", "100"], ["--fern-cell", "0"], ["--harvest", "1.5"]):
        with pytest.raises(SystemExit) as e:
            S.main(argv + ["--relocalise"] + bad)
        assert e.value.code == 2 and "error" in capsys.readouterr().err


# ---- 7. argument errors ------------------------------------------------------------------------------------------------
def test_argument_errors(L):
    from boxfusion_amd.tracking import Relocaliser, fern_table
    depth, rgb = _frames(1, 48, 64, seed=5)
    d, c = _dev(depth), _dev(rgb)
    table = fern_table(64, 12, 0)
    dt = L.fern_upload(table, 12, DEV)
    lib = L.lib()
    p, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    codes = torch.zeros((1, 8), dtype=torch.int32, device=DEV)
    means = torch.zeros((1, 12, 4), dtype=torch.int32, device=DEV)

    def encode(**over):
        a = dict(depth=d.data_ptr(), rgb=c.data_ptr(), B=1, H=48, W=64, cell=16, max_depth=4.0, ferns=dt.data_ptr(), F=64,
                 means=means.data_ptr(), codes=codes.data_ptr())
        a.update(over)
        return lib.bf_fern_encode(p(a["depth"]), p(a["rgb"]), i(a["B"]), i(a["H"]), i(a["W"]), i(a["cell"]), f(a["max_depth"]),
                                  p(a["ferns"]), i(a["F"]), p(a["means"]), p(a["codes"]), L._stream())
    for over in (dict(depth=None), dict(B=0), dict(H=0), dict(W=-1), dict(cell=0), dict(cell=65), dict(cell=64), dict(F=12),
                 dict(F=0), dict(ferns=None), dict(max_depth=0.0), dict(max_depth=66.0), dict(max_depth=float("nan")),
                 dict(means=None, codes=None)):
        assert encode(**over) == -1, over                        # BF_ERR_ARG; cell 64 exceeds the 48 rows
    torch.cuda.synchronize()
    assert not codes.any() and not means.any()                   # nothing above launched anything
    assert encode() == 0 and encode(rgb=None, means=None) == 0 and encode(codes=None, ferns=None, F=0) == 0
    # the table check
    ip = ctypes.POINTER(ctypes.c_int32)
    bad = table.copy()
    bad[7, 0] = 12
    assert lib.bf_fern_table_check(table.ctypes.data_as(ip), i(64), i(12)) == 0
    assert lib.bf_fern_table_check(bad.ctypes.data_as(ip), i(64), i(12)) == -1
    assert lib.bf_fern_table_check(table.ctypes.data_as(ip), i(64), i(11)) == (-1 if table[:, 0].max() == 11 else 0)
    assert lib.bf_fern_table_check(table.ctypes.data_as(ip), i(60), i(12)) == -1
    assert lib.bf_fern_table_check(None, i(64), i(12)) == -1
    bad[7, 0] = -1
    for t in (bad, table[:12], table[:, :4]):
        with pytest.raises(L.HipError):
            L.fern_upload(t, 12, DEV)
    # the binding refuses what it can see
    for args in ((d.double(), c), (d, c.float()), (d, c[:, :, :-1]), (d.cpu(), c.cpu()), (d[0, 0], None)):
        with pytest.raises(L.HipError):
            L.fern_encode(args[0], args[1], 16, 4.0, dt)
    for ferns in (dt.long(), dt[:, :4], dt.cpu(), dt[:12]):
        with pytest.raises(L.HipError):
            L.fern_encode(d, c, 16, 4.0, ferns)
    with pytest.raises(L.HipError):
        L.fern_encode(d, c, 64, 4.0, dt)                         # larger than the image
    # search
    kt = torch.zeros((16, 8), dtype=torch.int32, device=DEV)
    n = torch.zeros(1, dtype=torch.int32, device=DEV)
    q = torch.zeros((1, 8), dtype=torch.int32, device=DEV)
    for k in (0, 9):
        with pytest.raises(L.HipError):
            L.fern_search(kt, n, 4, q, k)
    for args in ((kt.long(), n, 4, q), (kt, n.long(), 4, q), (kt, n, 4, q.float()), (kt, n, 4, q[:, :4]), (kt, n, 0, q), (kt, n, 17, q),
                 (kt.cpu(), n.cpu(), 4, q.cpu()), (kt, n.cpu(), 4, q)):
        with pytest.raises(L.HipError):
            L.fern_search(*args, 4)
    part = torch.zeros((1, 1, 8), dtype=torch.int64, device=DEV)
    top = torch.zeros((1, 8, 2), dtype=torch.int32, device=DEV)
    assert lib.bf_fern_search(p(kt.data_ptr()), i(16), i(12), p(n.data_ptr()), i(4), p(q.data_ptr()), i(1), i(4),
                              p(part.data_ptr()), p(top.data_ptr()), p(None), L._stream()) == -1
    assert lib.bf_fern_search(p(kt.data_ptr()), i(16), i(64), p(n.data_ptr()), i(4), p(q.data_ptr()), i(1), i(9),
                              p(part.data_ptr()), p(top.data_ptr()), p(None), L._stream()) == -1
    # append
    poses, ids = torch.zeros((16, 16), dtype=torch.float32, device=DEV), torch.zeros(16, dtype=torch.int32, device=DEV)
    cnt = torch.zeros(3, dtype=torch.int32, device=DEV)
    good = (kt, n, q[0], top[0, 0], 3, np.eye(4, dtype=np.float32), 0, poses, ids, cnt)
    for at, wrong in ((0, kt.long()), (2, q[0, :4]), (3, top[0, 0].float()), (5, np.eye(3)), (7, poses[:8]), (8, ids.long()),
                      (9, cnt[:2]), (1, n.cpu())):
        with pytest.raises(L.HipError):
            L.fern_append(*[wrong if j == at else v for j, v in enumerate(good)])
    torch.cuda.synchronize()
    assert not kt.any() and not n.any() and not cnt.any()
    # the class
    for over in (dict(ferns=100), dict(ferns=0), dict(cell=0), dict(cell=64), dict(cell=65), dict(capacity=0), dict(harvest=1.5),
                 dict(max_depth=70.0)):
        with pytest.raises(ValueError):
            Relocaliser(48, 64, DEV, **over)
    rl = _relocaliser()
    with pytest.raises(ValueError):
        rl.observe(d[0, :40], np.eye(4))
    with pytest.raises(ValueError):
        rl.query(d[0], c[0].float())
    with pytest.raises(ValueError):
        rl.query(d[0], c[0], k=9)
