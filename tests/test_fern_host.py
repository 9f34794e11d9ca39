"""The fern relocaliser on the host: tracking.fern_table, the packing of tests/fern_ref.py, and the kidnap scene under
the numpy restatement: the codes order the frames as the camera moved, the two new views cannot be tracked from the
last wall view, and fern_ref's relocalise places them."""
import numpy as np
import pytest

from tests import fern_ref as FR
from tests import track_ref as TR


def test_fern_table_is_deterministic_and_in_range():
    from boxfusion_amd.tracking import fern_table
    a, b = fern_table(256, 192, 3, (0.4, 3.0)), fern_table(256, 192, 3, (0.4, 3.0))
    assert a.dtype == np.int32 and a.shape == (256, 5) and np.array_equal(a, b)
    assert not np.array_equal(a, fern_table(256, 192, 4, (0.4, 3.0)))
    assert a[:, 0].min() >= 0 and a[:, 0].max() < 192 and len(np.unique(a[:, 0])) > 96
    assert a[:, 1:4].min() >= 0 and a[:, 1:4].max() <= 254          # both outcomes of mean > t are possible
    assert a[:, 4].min() >= 400 and a[:, 4].max() < 3000
    one = fern_table(8, 1, 0)
    assert not one[:, 0].any() and one[:, 4].min() >= 400 and one[:, 4].max() < 4000
    for bad in (dict(ferns=12), dict(ferns=0), dict(cells=0), dict(depth_range_m=(1.0, 1.0)), dict(depth_range_m=(0.4, 70.0)),
                dict(depth_range_m=(-0.1, 1.0))):
        with pytest.raises(ValueError):
            fern_table(**{**dict(ferns=64, cells=12, seed=0, depth_range_m=(0.4, 4.0)), **bad})


def test_packing_round_trips():
    rng = np.random.default_rng(0)
    nib = rng.integers(0, 16, 64).astype(np.uint8)
    code = FR.pack(nib)
    assert code.dtype == np.uint32 and code.shape == (8,) and np.array_equal(FR.unpack(code), nib)
    assert code[0] == sum(int(v) << (4 * i) for i, v in enumerate(nib[:8]))
    other = nib.copy()
    other[[3, 17, 63]] ^= np.array([1, 8, 15], np.uint8)                             # one bit, the depth bit, all four: one fern each
    assert FR.distance(code, FR.pack(other)) == 3 and FR.distance(code, code) == 0
    assert FR.distance(FR.pack(np.zeros(64, np.uint8)), FR.pack(np.full(64, 15, np.uint8))) == 64


def test_cell_means_rules():
    d = np.full((9, 10), 1.0005, np.float32)                         # 1000.5 mm rounds half to even: 1000
    d[0, :2] = [2.0015, np.nan]
    rgb = np.zeros((9, 10, 3), np.uint8)
    rgb[:4, :4, 0] = 255
    rgb[:4, :4, 1] = np.arange(16).reshape(4, 4)                     # mean 7.5 -> 8
    m = FR.cell_means(d, rgb, 4, 4.0).reshape(2, 2, 4)
    want = (2 * (int(np.rint(np.float32(2.0015) * np.float32(1000.0))) + 14 * int(np.rint(np.float32(1.0005) * np.float32(1000.0))))
            + 15) // 30
    assert m[0, 0].tolist() == [255, 8, 0, want] and m[1, 1].tolist() == [0, 0, 0, int(np.rint(np.float32(1.0005) * np.float32(1000.0)))]
    d[4:8, 4:8] = 0.0
    d[4:6, 4:8] = 4.0                                                # at max_depth: invalid
    assert FR.cell_means(d, None, 4, 4.0).reshape(2, 2, 4)[1, 1].tolist() == [0, 0, 0, -1]
    d[4:6, 4:8] = 3.0                                                # exactly half the cell: valid
    assert FR.cell_means(d, None, 4, 4.0).reshape(2, 2, 4)[1, 1, 3] == 3000
    d[4, 4] = 0.0                                                    # one fewer: invalid
    assert FR.cell_means(d, None, 4, 4.0).reshape(2, 2, 4)[1, 1, 3] == -1
    with pytest.raises(ValueError):
        FR.cell_means(d, None, 16, 4.0)


def test_search_and_append_rules():
    rng = np.random.default_rng(1)
    codes = rng.integers(0, 1 << 32, (7, 8), dtype=np.uint64).astype(np.uint32)
    codes[5] = codes[2]
    top, rows = FR.search(codes, 6, 7, codes[[2]], 8)
    assert top[0, :2].tolist() == [[0, 2], [0, 5]] and (top[0, 6:] == -1).all() and rows[0, 6] == -1
    assert (np.diff(top[0, :6, 0]) >= 0).all()
    t = FR.Table(2, 8)
    assert t.append(codes[0], -1, 5, np.eye(4), 10) and not t.append(codes[1], 5, 5, np.eye(4), 11)
    assert t.append(codes[1], 6, 5, np.eye(4), 12) and not t.append(codes[3], 60, 5, np.eye(4), 13)
    assert t.counters() == dict(keyframes=2, observed=4, added=2, dropped_full=1) and t.ids.tolist() == [10, 12]


def test_kidnap_scene_codes_follow_the_camera():
    s, table = FR.kidnap_scene(), FR.kidnap_table()
    codes = [FR.encode(d, c, FR.KIDNAP["cell"], TR.ROOM_VOLUME["max_depth"], table)[0] for d, c in zip(s["depths"], s["rgbs"])]
    D = np.array([[int(FR.distance(a, b)) for b in codes] for a in codes])
    print(D)
    for i in range(8):                                               # a trajectory frame: its neighbour before any wall frame
        near = min(D[i, j] for j in (i - 1, i + 1) if 0 <= j < 8)
        assert near < D[i, 8:12].min(), (i, D[i])
    for i in (12, 13):                                               # and the new views: the trajectory before the wall
        assert D[i, :8].min() < D[i, 8:12].min() and D[i, :8].min() <= 0.5 * FR.KIDNAP["ferns"]


def test_kidnapped_frames_are_lost_and_relocalised():
    """measured with this restatement: keyframes [0, 2, 4, 6, 8, 9, 10] before the new views; frame 12 goes to keyframe
    1 (frame 2) at distance 40 of 256 and is placed to 0.388 mm and 0.0247 degrees; the second new view (frame 14 here)
    to keyframe 7, which is frame 12, at 29, 0.252 mm and 0.0218 degrees"""
    ref = FR.kidnap_reference(twice=True)
    kf = ref["rl"].kf
    print("keyframes", kf.ids[:kf.n].tolist(), kf.counters())
    assert set(kf.ids[:kf.n]) >= {0, 8} and kf.observed == 15 and kf.dropped_full == 0
    for i in ref["unknown"]:
        info = ref["infos"][i]
        first = info["first"]                                        # tracked from poses[11], the last wall view
        assert first["lost"] and first["inliers"] < 0.01 * first["sampled"] + 6
        assert not info["lost"] and info["relocalised"] and info["candidates_tried"] == 1
        assert kf.ids[info["keyframe"]] not in (8, 9, 10, 11, 13) and info["fern_distance"] <= 0.25 * FR.KIDNAP["ferns"]
        et, er = TR.pose_error(ref["got"][i], ref["poses"][i])
        print(f"frame {i}: keyframe {info['keyframe']} (frame {kf.ids[info['keyframe']]}) at {info['fern_distance']}, placed to "
              f"{et * 1000:.3f} mm {er:.4f} deg")
        assert et < 0.001 and er < 0.05                              # the tracker's own accuracy in this room (test_track_host)
    # without a relocaliser both stay lost
    s = ref
    poses, infos, _ = FR.run_sequence(s["room"], s["depths"][:13], s["rgbs"][:13], s["known"][:13], relocalise=False)
    assert infos[12]["lost"] and np.isneginf(poses[12]).all() and "relocalised" not in infos[12]
