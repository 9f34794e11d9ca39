"""Objects in the scene on the GPU: bf_label_points (bf_objects.hip) against the numpy restatement in
tests/objects_ref.py, bit for bit (labels, counts, the extents' keys and the stats), with and without the
per-wave cull, and the layers above it: label_mesh on a fused volume, instance_maps through the renderer
and the command line."""
import json
import pickle

import numpy as np
import pytest
import torch
from PIL import Image

from tests import objects_ref as OR

pytestmark = pytest.mark.gpu

DEV = "cuda"
K48 = np.array([[50.0, 0.0, 31.5], [0.0, 50.0, 23.5], [0.0, 0.0, 1.0]], np.float32)
H48, W48 = 48, 64
GRID_POINTS = 2048 * 256          # the points one pass of the largest grid covers: beyond it a block walks tiles


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from boxfusion_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def SO(L):
    from boxfusion_amd import scene_objects
    return scene_objects


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(L, xyz, rows, margin=0.0, cull=None):
    labels, counts, keys, stats = L.label_points(_dev(np.asarray(xyz, np.float32).reshape(-1, 3)),
                                                 _dev(np.asarray(rows, np.float32).reshape(-1, 16)), margin, cull=cull)
    torch.cuda.synchronize()
    assert labels.dtype == torch.int32 and counts.dtype == torch.int64 and keys.dtype == torch.int32
    assert stats.dtype == torch.int64 and stats.numel() == L.STATS_WORDS
    s = stats.cpu().tolist()
    assert s[len(L.OBJ_STATS):] == [0] * (L.STATS_WORDS - len(L.OBJ_STATS))
    return dict(labels=labels.cpu().numpy(), counts=counts.cpu().numpy(), keys=keys.cpu().numpy().view(np.uint32),
                stats=dict(zip(L.OBJ_STATS, s)))


def _same(got, ref):
    assert (got["labels"] == ref["labels"]).all()
    assert (got["counts"] == ref["counts"]).all()
    assert (got["keys"] == ref["keys"]).all()
    assert {k: got["stats"][k] for k in ref["stats"]} == ref["stats"]


def _check(L, xyz, rows, margin=0.0):
    """the product's call, and the hook with the cull off and on, all against the restatement"""
    ref = OR.label_ref(xyz, rows, margin)
    full = ref["finite"] * len(np.asarray(rows).reshape(-1, 16))
    for cull in (None, False, True):
        got = _run(L, xyz, rows, margin, cull)
        _same(got, ref)
        if cull is False:
            assert got["stats"]["pair_tests"] == full
        else:
            assert got["stats"]["pair_tests"] <= full
    return ref


def _rows(centres, halves, volumes=None):
    """axis-aligned rows written directly, every word exactly as given"""
    c, h = np.asarray(centres, np.float32).reshape(-1, 3), np.asarray(halves, np.float32).reshape(-1, 3)
    rows = np.zeros((len(c), 16), np.float32)
    rows[:, 0:3], rows[:, 3], rows[:, 7], rows[:, 11], rows[:, 12:15] = c, 1.0, 1.0, 1.0, h
    rows[:, 15] = 8.0 * h.prod(1) if volumes is None else volumes
    return rows


@pytest.fixture(scope="module")
def room(SO):
    """300 rotated boxes of 0.1..0.8 m within +-1.5 m and GRID_POINTS + 77 points within +-2 m"""
    rng = np.random.default_rng(7)
    rows, degenerate = SO.box_rows(OR.random_boxes(rng, 300, (0.1, 0.8), 1.5))
    assert not degenerate.any()
    return dict(rows=rows, xyz=rng.uniform(-2.0, 2.0, size=(GRID_POINTS + 77, 3)).astype(np.float32))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 5000])
def test_point_and_box_counts(L, room, n):
    C = L.OBJ_CHUNK
    for B in (0, 1, 3, C - 1, C, C + 1, 300):
        ref = _check(L, room["xyz"][:n], room["rows"][:B])
        if B == 0:
            assert (ref["labels"] == -1).all()
    if n == 5000:
        assert ref["stats"]["labelled"] > 1000 and ref["stats"]["shared"] > 100


def test_more_points_than_one_pass_of_the_grid(L, room):
    """a block walks several tiles, and with more boxes than a chunk restages the rows for each"""
    ref = _check(L, room["xyz"], room["rows"][:L.OBJ_CHUNK + 1])
    assert ref["stats"]["points"] == GRID_POINTS + 77 and (ref["labels"][-77:] >= 0).any()


def test_nested_boxes_the_small_one_owns(L):
    rows = _rows([[0, 0, 0], [0.1, 0, 0]], [[1, 1, 1], [0.25, 0.25, 0.25]])
    xyz = np.array([[0.2, 0.1, 0.0], [0.9, 0.0, 0.0], [3.0, 0.0, 0.0]], np.float32)
    ref = _check(L, xyz, rows)
    assert ref["labels"].tolist() == [1, 0, -1]
    assert ref["counts"].tolist() == [[2, 1], [1, 1]] and ref["stats"]["shared"] == 1
    _check(L, xyz, rows[::-1].copy())                            # the order of the rows does not decide


def test_identical_boxes_the_lower_index_owns(L):
    rows = _rows([[0, 0, 0]] * 3, [[0.5, 0.5, 0.5]] * 3)
    ref = _check(L, np.array([[0.1, 0.2, 0.3], [0.0, 0.0, 0.0]], np.float32), rows)
    assert ref["labels"].tolist() == [0, 0] and ref["counts"].tolist() == [[2, 2], [2, 0], [2, 0]]
    assert ref["stats"]["shared"] == 2


def test_a_point_on_a_face_is_inside(L):
    rows = _rows([[1.0, 2.0, 3.0]], [[0.5, 0.25, 0.125]])       # every number exactly representable
    out = np.nextafter(np.float32(1.5), np.float32(2.0))
    xyz = np.array([[1.5, 2.0, 3.0], [out, 2.0, 3.0], [0.5, 2.25, 2.875], [1.0, 1.75, 3.125],
                    [1.0, np.nextafter(np.float32(1.75), np.float32(0.0)), 3.0]], np.float32)
    ref = _check(L, xyz, rows)
    assert ref["labels"].tolist() == [0, -1, 0, 0, -1]
    # the extents reach exactly to the faces: t = -0.5 .. 0.5, -0.25 .. 0.25, -0.125 .. 0.125
    assert (ref["keys"][0] == OR.keys_of(np.array([-0.5, 0.5, -0.25, 0.25, -0.125, 0.125], np.float32))).all()


def test_margin_moves_a_point_in(L):
    rows = _rows([[0, 0, 0]], [[0.5, 0.5, 0.5]])
    xyz = np.array([[0.53, 0.0, 0.0], [0.0, -0.58, 0.0]], np.float32)
    assert _check(L, xyz, rows, 0.0)["labels"].tolist() == [-1, -1]
    assert _check(L, xyz, rows, 0.05)["labels"].tolist() == [0, -1]
    assert _check(L, xyz, rows, 0.1)["labels"].tolist() == [0, 0]


def test_nonfinite_points_and_a_nan_row(L, room):
    xyz = room["xyz"][:400].copy()
    xyz[5, 0], xyz[64, 1], xyz[65, 2], xyz[399] = np.nan, np.inf, -np.inf, np.nan
    xyz[128:192] = np.nan                                        # a whole wave with nothing finite
    rows = room["rows"][:40].copy()
    rows[7] = np.nan
    rows[11, 13] = np.nan                                        # one half-length: the row still contains nothing
    ref = _check(L, xyz, rows)
    assert ref["stats"]["nonfinite"] == 68 and (ref["labels"][[5, 64, 65, 399]] == -1).all()
    assert (ref["labels"][128:192] == -1).all()
    assert ref["counts"][[7, 11]].tolist() == [[0, 0], [0, 0]] and ref["stats"]["labelled"] > 50
    assert (ref["keys"][7] == np.array([0xFFFFFFFF, 0] * 3, np.uint32)).all()


def test_a_permutation_of_the_points_permutes_the_labels_only(L, room):
    xyz, rows = room["xyz"][:5000], room["rows"][:150]
    perm = np.random.default_rng(1).permutation(len(xyz))
    for cull in (False, True):
        a, b = _run(L, xyz, rows, 0.0, cull), _run(L, xyz[perm], rows, 0.0, cull)
        assert (b["labels"] == a["labels"][perm]).all()
        assert (a["counts"] == b["counts"]).all() and (a["keys"] == b["keys"]).all()
        for k in ("points", "nonfinite", "labelled", "shared") + (() if cull else ("pair_tests",)):
            assert a["stats"][k] == b["stats"][k]


def test_cull_gives_the_same_on_sorted_and_shuffled_points(L, room):
    """sorted by a 0.25 m voxel key, as both callers hand their points over, the cull skips most rows;
    shuffled it skips few; neither changes a label, a count or an extent"""
    xyz, rows = room["xyz"][:20000], room["rows"]
    cell = np.floor((xyz + 2.0) / 0.25).astype(np.int64)
    order = np.argsort((cell[:, 0] * 64 + cell[:, 1]) * 64 + cell[:, 2], kind="stable")
    srt = xyz[order]
    ref = OR.label_ref(srt, rows)
    on, off = _run(L, srt, rows, 0.0, True), _run(L, srt, rows, 0.0, False)
    _same(on, ref)
    _same(off, ref)
    shuffled = _run(L, xyz, rows, 0.0, True)
    assert (shuffled["labels"][order] == on["labels"]).all()
    assert (shuffled["counts"] == on["counts"]).all() and (shuffled["keys"] == on["keys"]).all()
    assert off["stats"]["pair_tests"] == len(xyz) * len(rows)
    print("pair tests: sorted", on["stats"]["pair_tests"], "shuffled", shuffled["stats"]["pair_tests"], "all",
          off["stats"]["pair_tests"])
    assert on["stats"]["pair_tests"] < shuffled["stats"]["pair_tests"] <= off["stats"]["pair_tests"]


def test_too_many_boxes_raise(L):
    xyz = _dev(np.zeros((4, 3), np.float32))
    with pytest.raises(L.HipError):
        L.label_points(xyz, _dev(np.zeros((L.MAX_BOXES + 1, 16), np.float32)))
    with pytest.raises(L.HipError):
        L.label_points(xyz, _dev(np.zeros((2, 12), np.float32)))
    with pytest.raises(L.HipError):
        L.label_points(xyz.double(), _dev(np.zeros((2, 16), np.float32)))
    # the entry point itself refuses what the wrapper lets through
    lab = torch.empty(4, dtype=torch.int32, device=DEV)
    st = torch.zeros(8, dtype=torch.int64, device=DEV)
    assert L.lib().bf_label_points(L._ptr(xyz), 4, None, 2, 0.0, L._ptr(lab), None, None, L._ptr(st), None) == -1


def test_label_points_api(SO, L):
    """the layer above the binding: decoded extents, fill, stats by name"""
    corners = OR.axis_boxes([[0, 0, 0], [5, 5, 5], [0.1, 0, 0]], [[1, 1, 1], [0.5, 0.5, 0.5], [0.25, 0.25, 0.0]])
    xyz = np.array([[-0.5, -1.0, 0.25], [0.5, 0.5, -0.75], [9, 9, 9]], np.float32)
    out = SO.label_points(xyz, corners)
    assert out.labels.is_cuda and out.labels.cpu().tolist() == [0, 0, -1]
    assert out.support.tolist() == [2, 0, 0] and out.owned.tolist() == [2, 0, 0]
    assert out.degenerate.tolist() == [False, False, True] and out.boxes == 3
    assert out.extents.shape == (3, 3, 2) and np.isnan(out.extents[1:]).all()
    got = np.sort(np.abs(out.extents[0]), axis=None)             # the axes' order and signs are box_rows' business
    assert got.tolist() == [0.25, 0.5, 0.5, 0.5, 0.75, 1.0]
    assert out.fill[0] == pytest.approx(1.0 * 1.5 * 1.0 / 8.0) and out.fill[1:].tolist() == [0.0, 0.0]
    assert out.stats == dict(points=3, nonfinite=0, labelled=2, shared=0, pair_tests=out.stats["pair_tests"])
    assert SO.supported(out).tolist() == [True, False, False]


def _box_on_floor_depth():
    """a camera 2 m above a floor looking straight down at a 0.8 x 0.6 x 0.5 m box in the middle"""
    v, u = np.mgrid[:H48, :W48].astype(np.float64)
    a, b = (u - K48[0, 2]) / K48[0, 0], (v - K48[1, 2]) / K48[1, 1]
    on_top = (np.abs(a * 1.5) <= 0.4) & (np.abs(b * 1.5) <= 0.3)
    pose = np.array([[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 2.0], [0, 0, 0, 1]], np.float32)
    return np.where(on_top, 1.5, 2.0).astype(np.float32), pose


def test_label_mesh_on_a_fused_volume(SO, L):
    from boxfusion_amd.scene_mesh import TsdfVolume
    depth, pose = _box_on_floor_depth()
    vol = TsdfVolume(voxel=0.05, trunc_voxels=3, capacity=1 << 12, max_depth=4.0, device=DEV)
    vol.integrate(_dev(depth), K48, pose[None])
    corners = OR.axis_boxes([[0, 0, 0.25], [3, 3, 3]], [[0.4, 0.3, 0.25], [0.2, 0.2, 0.2]])
    out = SO.label_mesh(vol, corners, margin=0.05)
    v, _, f = (t.cpu().numpy() for t in vol.mesh())
    lab, fl = out.labels.cpu().numpy(), out.face_labels.cpu().numpy()
    assert len(lab) == len(v) > 500 and len(fl) == len(f) > 500
    top = (np.abs(v[:, 0]) < 0.3) & (np.abs(v[:, 1]) < 0.2) & (np.abs(v[:, 2] - 0.5) < 0.04)
    floor = (np.abs(v[:, 0]) > 0.7) & (np.abs(v[:, 2]) < 0.04)
    assert top.sum() > 20 and floor.sum() > 20
    assert (lab[top] == 0).all() and (lab[floor] == -1).all()
    assert out.owned.tolist() == [int((lab == 0).sum()), 0] and out.support[1] == 0
    rows, _ = SO.box_rows(corners)
    assert (lab == OR.label_ref(v, rows, 0.05)["labels"]).all()
    assert (fl == SO.face_labels(lab, f)).all()
    top_faces = top[f].all(1)
    assert top_faces.sum() > 20 and (fl[top_faces] == 0).all() and (fl[floor[f].all(1)] == -1).all()
    assert SO.supported(out, 10).tolist() == [True, False]
    assert 0.0 < out.fill[0] <= 0.9 * 0.7 * 0.6 / (0.8 * 0.6 * 0.5) + 1e-6 and out.extents[0, :, 1].max() <= 0.45 + 1e-6


def _pixels(xyz):
    """seen from the identity pose: the image position of each point, its pixel, and how far the
    position is from where the pixel changes"""
    p = np.asarray(xyz, np.float64)
    u, v = K48[0, 0] * p[:, 0] / p[:, 2] + K48[0, 2], K48[1, 1] * p[:, 1] / p[:, 2] + K48[1, 2]
    pu, pv = np.floor(u + 0.5).astype(int), np.floor(v + 0.5).astype(int)
    edge = np.minimum(np.abs(u + 0.5 - np.round(u + 0.5)), np.abs(v + 0.5 - np.round(v + 0.5)))
    return u, v, pu, pv, edge


def test_instance_map_of_a_labelled_cloud(SO, L):
    rng = np.random.default_rng(2)
    a = rng.uniform(-0.15, 0.15, size=(150, 3)) + [-0.5, 0.0, 2.0]
    b = rng.uniform(-0.15, 0.15, size=(150, 3)) + [0.5, 0.1, 2.4]
    stray = rng.uniform(-0.1, 0.1, size=(40, 3)) + [-0.45, 0.0, 1.5]       # unlabelled, in front of part of a
    xyz = np.concatenate([a, b, stray]).astype(np.float32)
    corners = OR.axis_boxes([[-0.5, 0.0, 2.0], [0.5, 0.1, 2.4]], [[0.2, 0.2, 0.2], [0.2, 0.2, 0.2]])
    labels = SO.label_points(xyz, corners)
    lab = labels.labels.cpu().numpy()
    assert lab[:150].tolist() == [0] * 150 and lab[150:300].tolist() == [1] * 150 and (lab[300:] == -1).all()
    maps = SO.instance_maps((xyz, np.zeros((len(xyz), 3), np.uint8)), labels, np.eye(4, dtype=np.float32)[None], K48, H48,
                            W48, radius=1)
    assert maps.is_cuda and maps.dtype == torch.int32 and tuple(maps.shape) == (1, H48, W48)
    m = maps[0].cpu().numpy()
    assert set(np.unique(m)) == {-1, 0, 1}
    u, v, pu, pv, edge = _pixels(xyz)
    checked = 0
    for i in np.where((lab >= 0) & (edge > 0.01))[0]:
        # the points no farther away whose 3 x 3 splat may cover this point's pixel
        near = (xyz[:, 2] <= xyz[i, 2]) & (np.abs(u - pu[i]) <= 1.51) & (np.abs(v - pv[i]) <= 1.51)
        assert m[pv[i], pu[i]] in set(lab[near].tolist()), i
        checked += 1
    assert checked > 250
    assert (m[:, W48 // 2 - 3:W48 // 2 + 3] == -1).all()                    # between the two objects: nothing


def test_instance_map_of_a_mesh_is_one_face_per_pixel(SO, L):
    # a quad of two triangles that share an edge and carry different labels
    v = np.array([[-0.4, -0.3, 2.0], [0.4, -0.3, 2.0], [0.4, 0.3, 2.0], [-0.4, 0.3, 2.0]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    for ids in ((0, 1), (0, 300)):
        B = max(ids) + 1
        labels = SO.ObjectLabels(labels=_dev(np.zeros(4, np.int32)), support=np.zeros(B, np.int64), owned=np.zeros(B, np.int64),
                                 extents=np.zeros((B, 3, 2), np.float32), fill=np.zeros(B), degenerate=np.zeros(B, bool),
                                 stats={}, face_labels=_dev(np.array(ids, np.int32)))
        m = SO.instance_maps((v, None, f), labels, np.eye(4, dtype=np.float32)[None], K48, H48, W48)[0].cpu().numpy()
        assert set(np.unique(m)) == {-1, ids[0], ids[1]}
        assert (m == ids[0]).sum() > 100 and (m == ids[1]).sum() > 100 and (m == -1).sum() > 1000


def test_an_unlabelled_wall_hides_the_object_behind_it(SO, L):
    rng = np.random.default_rng(4)
    obj = (rng.uniform(-0.1, 0.1, size=(200, 3)) + [0.0, 0.0, 3.0]).astype(np.float32)
    g = np.arange(-0.5, 0.5001, 0.02)
    wall = np.stack(np.meshgrid(g, g, [1.5], indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    corners = OR.axis_boxes([[0, 0, 3.0]], [[0.15, 0.15, 0.15]])
    pose = np.eye(4, dtype=np.float32)[None]
    alone = SO.label_points(obj, corners)
    m = SO.instance_maps(obj, alone, pose, K48, H48, W48)[0].cpu().numpy()
    assert (m == 0).sum() >= 9 and set(np.unique(m)) == {-1, 0}
    both = np.concatenate([obj, wall])
    labels = SO.label_points(both, corners)
    assert labels.owned.tolist() == [200] and labels.stats["labelled"] == 200
    m = SO.instance_maps(both, labels, pose, K48, H48, W48)[0].cpu().numpy()
    assert (m == -1).all()


def _write_boxes(path, corners):
    with open(path, "wb") as fh:
        pickle.dump([[(0, np.asarray(c, np.float64), 0.9) for c in corners]], fh)


def test_command_line_on_a_cloud_and_a_mesh(SO, L, tmp_path):
    from boxfusion_amd.visualize import mesh_to_ply, points_to_ply
    rng = np.random.default_rng(6)
    xyz = np.concatenate([rng.uniform(-0.2, 0.2, size=(300, 3)) + [1.0, 0.0, 0.3],
                          rng.uniform(-0.2, 0.2, size=(300, 3)) + [-1.0, 0.5, 0.3],
                          rng.uniform(-2.0, 2.0, size=(400, 3)) * [1, 1, 0.01]]).astype(np.float32)
    rgb = rng.integers(0, 256, size=(len(xyz), 3), dtype=np.uint8)
    corners = OR.axis_boxes([[1.0, 0.0, 0.3], [-1.0, 0.5, 0.3], [0.0, -1.5, 1.5]],
                            [[0.25, 0.25, 0.25], [0.3, 0.25, 0.2], [0.1, 0.1, 0.1]])
    _write_boxes(tmp_path / "seq_boxes.pkl", corners)
    points_to_ply(xyz, rgb, str(tmp_path / "cloud.ply"))
    out = tmp_path / "out"
    assert SO.main([str(tmp_path / "cloud.ply"), str(tmp_path / "seq_boxes.pkl"), str(out), "--views", "2", "--size", "48",
                    "64", "--min-points", "5"]) == 0
    names = sorted(p.name for p in out.iterdir())
    assert names == ["labels.txt", "object_0000.ply", "object_0001.ply", "objects.json", "objects_0.png", "objects_1.png",
                     "objects_top.png"]
    want = SO.label_points(xyz, corners.astype(np.float32)).labels.cpu().numpy()
    assert (np.loadtxt(out / "labels.txt", dtype=np.int32) == want).all() and (want[:600] >= 0).all()
    for n in ("objects_0.png", "objects_1.png", "objects_top.png"):
        assert Image.open(out / n).size == (64, 48)
    meta = json.load(open(out / "objects.json"))
    assert meta["kind"] == "cloud" and [b["owned"] for b in meta["boxes"]] == [300, 300, 0]
    assert meta["stats"]["points"] == 1000

    # the same scene with faces: a mesh, one PLY of faces per object
    faces = np.concatenate([np.arange(0, 300).reshape(-1, 3), np.arange(300, 600).reshape(-1, 3),
                            np.array([[0, 1, 300], [600, 601, 602]])]).astype(np.int32)
    mesh_to_ply(xyz, rgb, faces, str(tmp_path / "mesh.ply"))
    out = tmp_path / "out_mesh"
    assert SO.main([str(tmp_path / "mesh.ply"), str(tmp_path / "seq_boxes.pkl"), str(out), "--views", "0"]) == 0
    assert sorted(p.name for p in out.iterdir()) == ["labels.txt", "object_0000.ply", "object_0001.ply", "objects.json"]
    from boxfusion_amd.visualize import read_ply_surface
    ov, _, of = read_ply_surface(str(out / "object_0001.ply"))
    assert len(ov) == 300 and len(of) == 100 and (ov == xyz[300:600]).all()
    assert json.load(open(out / "objects.json"))["kind"] == "mesh"
