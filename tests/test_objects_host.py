"""Objects in the scene, the parts that need no GPU: the host restatement against an f64 brute force, the
box rows, the two small codes, the second public header, the build entry and the file writers."""
import argparse
import ctypes

import numpy as np
import pytest

from boxfusion_amd import _abi, build as B, scene_objects as SO
from tests import objects_ref as OR

OBJECTS_HEADER = _abi.EXTENSION_HEADERS[0]


def test_f32_rule_agrees_with_f64_brute_force_away_from_faces():
    rng = np.random.default_rng(11)
    rows, degenerate = SO.box_rows(OR.random_boxes(rng, 24))
    assert not degenerate.any()
    xyz = rng.uniform(-4.0, 4.0, size=(20000, 3)).astype(np.float32)
    ref = OR.label_ref(xyz, rows)
    labels, member, face_dist = OR.label_f64(xyz, rows)
    far = face_dist > 1e-3
    excluded = 1.0 - far.mean()
    print(f"excluded share {excluded:.5f}, mismatches inside the band {(ref['labels'] != labels)[~far].sum()}")
    assert excluded <= 0.01
    assert (ref["labels"] == labels)[far].all()
    assert (ref["inside"] == member.sum(1))[far].all()
    assert ref["stats"]["labelled"] > 500 and ref["stats"]["shared"] > 20        # the draw exercises both


def test_box_rows_do_not_depend_on_the_corner_order():
    rng = np.random.default_rng(5)
    half = np.array([[0.9, 0.5, 0.2], [0.31, 0.3, 0.1], [1.1, 0.7, 0.05]])
    centre, R = rng.uniform(-2, 2, size=(3, 3)), OR.random_rotations(rng, 3)
    corners = OR.corners_of(centre, R, half)
    rows, degenerate = SO.box_rows(corners)
    assert rows.dtype == np.float32 and rows.shape == (3, 16) and not degenerate.any()
    np.testing.assert_allclose(rows[:, :3], centre, atol=1e-6)
    np.testing.assert_allclose(rows[:, 12:15], half, rtol=1e-6)
    np.testing.assert_allclose(rows[:, 15], 8 * half.prod(1), rtol=1e-6)
    for k in range(3):                                           # unit axes: the columns of R up to sign
        dots = np.einsum("bj,bj->b", rows[:, 3 + 3 * k:6 + 3 * k], R[:, :, k])
        np.testing.assert_allclose(np.abs(dots), 1.0, atol=1e-6)
    perms = [np.arange(8)[::-1], np.roll(np.arange(8), 3), np.array([3, 6, 0, 5, 1, 7, 2, 4]),
             np.array([7, 0, 6, 1, 5, 2, 4, 3]), rng.permutation(8)]
    for p in perms:
        again, deg = SO.box_rows(corners[:, p])
        assert not deg.any()
        np.testing.assert_allclose(again[:, :3], rows[:, :3], atol=1e-6)
        np.testing.assert_allclose(again[:, 12:], rows[:, 12:], rtol=1e-6)
        for k in range(3):                                       # the same axis, either way round
            dots = np.einsum("bj,bj->b", again[:, 3 + 3 * k:6 + 3 * k], rows[:, 3 + 3 * k:6 + 3 * k])
            np.testing.assert_allclose(np.abs(dots), 1.0, atol=1e-6)


def test_box_rows_flat_and_nan_boxes_are_nan_rows():
    corners = OR.axis_boxes([[0, 0, 0], [1, 1, 1], [2, 2, 2]], [[0.5, 0.4, 0.0], [0.5, 0.4, 0.3], [0.2, 0.2, 0.2]])
    corners[2, 3, 1] = np.nan
    rows, degenerate = SO.box_rows(corners)
    assert degenerate.tolist() == [True, False, True]
    assert np.isnan(rows[0]).all() and np.isnan(rows[2]).all() and np.isfinite(rows[1]).all()
    # a NaN row contains nothing under the rule
    ref = OR.label_ref(np.array([[0, 0, 0], [1, 1, 1]], np.float32), rows)
    assert ref["labels"].tolist() == [-1, 1] and ref["counts"][:, 0].tolist() == [0, 1, 0]


def test_extent_keys_round_trip_and_keep_the_order():
    values = np.array([-np.inf, -3.0e38, -1.5, -1.0000001, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1e-30, 0.5, 1.0, 2.0, 3.0e38,
                       np.inf], np.float32)
    keys = SO.extent_keys(values)
    assert keys.dtype == np.uint32
    assert (keys == OR.keys_of(values)).all()
    assert (np.diff(keys.astype(np.int64)) > 0).all()            # strictly rising, -0 below +0
    back = SO.extent_values(keys)
    assert (back.view(np.uint32) == values.view(np.uint32)).all()
    rng = np.random.default_rng(3)
    v = rng.normal(size=4096).astype(np.float32) * np.float32(10.0) ** rng.integers(-20, 20, 4096).astype(np.float32)
    k = SO.extent_keys(v)
    assert (SO.extent_values(k).view(np.uint32) == v.view(np.uint32)).all()
    assert (np.argsort(k, kind="stable") == np.argsort(v, kind="stable")).all()
    # the caller's initial words decode to values no owned point's |t| reaches
    assert 0xFFFFFFFF > keys.max() and 0 < keys.min()


def test_id_colours_round_trip():
    ids = np.arange(-1, 4097)
    rgb = SO.id_colours(ids)
    assert rgb.dtype == np.uint8 and rgb.shape == (len(ids), 3)
    assert (rgb[0] == 0).all() and rgb[1].tolist() == [0, 0, 1] and rgb[256].tolist() == [0, 1, 0]
    assert (SO.colour_ids(rgb) == ids).all()
    import torch
    t = SO.id_colours(torch.from_numpy(ids))
    assert t.dtype == torch.uint8 and (t.numpy() == rgb).all() and (SO.colour_ids(t).numpy() == ids).all()
    with pytest.raises(ValueError):
        SO.id_colours(np.array([-2]))
    with pytest.raises(ValueError):
        SO.id_colours(np.array([1 << 24]))


def test_second_header_is_read_by_the_same_reader():
    core, ext = _abi.prototypes(), _abi.prototypes(header=OBJECTS_HEADER)
    assert "bf_label_points" in ext and "bf_label_points" not in core
    restype, argtypes = ext["bf_label_points"]
    assert restype is ctypes.c_int and len(argtypes) == 10
    v, f, i, ll = ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_longlong
    assert argtypes == [v, ll, v, i, f, v, v, v, v, v]
    assert not set(core) & set(ext)
    c = _abi.constants(header=OBJECTS_HEADER)
    assert c["BF_OBJ_BOX_WORDS"] == 16 and c["BF_OBJ_EXTENT_WORDS"] == 6 and c["BF_OBJ_COUNT_WORDS"] == 2
    assert c["BF_OBJ_CHUNK"] >= 64 and c["BF_OBJ_CHUNK"] % 64 == 0
    # the core header's numbers are included, not restated
    assert not {"BF_STATS_WORDS", "BF_MAX_BOXES", "BF_OK", "BF_ERR_ARG"} & set(c)
    assert not any(k.startswith("BF_OBJ_") for k in _abi.constants())
    assert _abi.enum_names("BF_OBJ_STAT_", header=OBJECTS_HEADER) == ("points", "nonfinite", "labelled", "shared",
                                                                     "pair_tests")
    with pytest.raises(KeyError, match="boxfusion_objects.h"):
        _abi.enum_names("BF_CLOUD_STAT_", header=OBJECTS_HEADER)
    with pytest.raises(KeyError, match="boxfusion_hip.h"):
        _abi.enum_names("BF_OBJ_STAT_")
    with pytest.raises(KeyError, match="boxfusion_objects.h"):
        _abi.struct("bf_nms_cfg", header=OBJECTS_HEADER)


def test_kernel_file_is_built_exact_and_exported():
    assert B.SOURCES["bf_objects.hip"] is B.EXACT
    lib = ctypes.CDLL(B.build())
    assert hasattr(lib, "bf_label_points") and hasattr(lib, "bf_label_points_ex")
    from boxfusion_amd import _lib
    fn = _lib.lib().bf_label_points
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 10
    assert len(_lib.lib().bf_label_points_ex.argtypes) == 11
    assert _lib.OBJ_STATS[-1] == "pair_tests" and _lib.OBJ_CHUNK == _abi.constants(header=OBJECTS_HEADER)["BF_OBJ_CHUNK"]
    # argument checks that need no device: nothing is launched for them
    assert fn(None, -1, None, 0, 0.0, None, None, None, None, None) == -1
    assert fn(None, 0, None, 0, 0.0, None, None, None, None, None) == 0
    assert fn(None, 5, None, 0, 0.0, None, None, None, None, None) == -1
    assert fn(None, 0, None, _lib.MAX_BOXES + 1, 0.0, None, None, None, None, None) == -1


def _two_object_mesh():
    # two quads (two triangles each) and one triangle that bridges them
    v = np.array([[0, 0, 0], [5, 0, 0], [1, 0, 0], [5, 1, 0], [1, 1, 0], [6, 0, 0], [0, 1, 0], [6, 1, 0]], np.float32)
    rgb = (np.arange(24).reshape(8, 3) * 10).astype(np.uint8)
    f = np.array([[0, 2, 4], [1, 5, 7], [0, 4, 6], [2, 1, 4], [1, 7, 3]], np.int32)
    vertex_labels = np.array([3, 0, 3, 0, 3, 0, 3, 0], np.int32)
    return v, rgb, f, vertex_labels


def test_object_meshes_reindex_their_faces():
    v, rgb, f, vl = _two_object_mesh()
    fl = SO.face_labels(vl, f)
    assert fl.tolist() == [3, 0, 3, -1, 0]                       # the bridge has two labels: nobody's
    out = SO.object_meshes((v, rgb, f), vl)
    assert sorted(out) == [0, 3]
    for b, faces_in in ((3, f[[0, 2]]), (0, f[[1, 4]])):
        ov, oc, of = out[b]
        used = np.unique(faces_in)
        assert of.dtype == np.int32 and of.min() == 0 and of.max() == len(ov) - 1 == 3
        assert (ov == v[used]).all() and (oc == rgb[used]).all()
        assert (ov[of] == v[faces_in]).all()                     # the same triangles, vertex for vertex
    import torch
    assert SO.face_labels(torch.from_numpy(vl), torch.from_numpy(f)).tolist() == fl.tolist()
    assert SO.face_labels(vl, np.array([[0, 2, 9]])).tolist() == [-1]        # an index outside the vertices


def test_save_objects_writes_the_listed_files(tmp_path):
    from boxfusion_amd.visualize import read_ply_surface
    v, rgb, f, vl = _two_object_mesh()
    ext = np.full((4, 3, 2), np.nan, np.float32)
    ext[0], ext[3] = [[-1, 1]] * 3, [[-0.5, 0.25]] * 3
    labels = SO.ObjectLabels(labels=vl, support=np.array([4, 0, 0, 5]), owned=np.array([4, 0, 0, 4]), extents=ext,
                             fill=np.array([0.5, 0, 0, 0.25]), degenerate=np.array([False, False, True, False]),
                             stats=dict(points=8, nonfinite=0, labelled=8, shared=0, pair_tests=32),
                             face_labels=SO.face_labels(vl, f))
    paths = SO.save_objects(str(tmp_path), (v, rgb, f), labels)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["labels.txt", "object_0000.ply", "object_0003.ply", "objects.json"]
    assert len(paths) == 4
    assert np.loadtxt(tmp_path / "labels.txt", dtype=np.int32).tolist() == vl.tolist()
    ov, oc, of = read_ply_surface(str(tmp_path / "object_0003.ply"))
    assert len(ov) == 4 and len(of) == 2
    import json
    meta = json.load(open(tmp_path / "objects.json"))
    assert meta["kind"] == "mesh" and len(meta["boxes"]) == 4 and meta["stats"]["pair_tests"] == 32
    assert meta["boxes"][3]["owned"] == 4 and meta["boxes"][2]["degenerate"] and meta["boxes"][1]["extents"][0] == [None, None]
    assert SO.supported(labels, 1).tolist() == [True, False, False, True]
    assert SO.supported(labels, 5).tolist() == [False, False, False, True]
    # a cloud: the points of each label
    labels.face_labels = None
    SO.save_objects(str(tmp_path / "cloud"), (v, rgb), labels)
    px, pc, pf = read_ply_surface(str(tmp_path / "cloud" / "object_0000.ply"))
    assert len(pf) == 0 and (px == v[vl == 0]).all() and (pc == rgb[vl == 0]).all()


def test_instance_colours_tint_only_labelled_points():
    from boxfusion_amd.render import box_colors
    rgb = np.array([[10, 20, 30], [200, 100, 0], [255, 255, 255]], np.uint8)
    out = SO.instance_colours(np.array([-1, 1, 0]), rgb, blend=0.6)
    assert out.dtype == np.uint8 and (out[0] == rgb[0]).all()
    want = np.rint(0.6 * box_colors(2)[[1, 0]].astype(np.float64) + 0.4 * rgb[1:]).astype(np.uint8)
    assert (out[1:] == want).all()
    assert (SO.instance_colours(np.array([-1, 1, 0]), rgb, blend=0.0) == rgb).all()


@pytest.mark.parametrize("argv", [["--size", "0", "64"], ["--size", "48", "20000"], ["--margin", "-0.1"],
                                  ["--margin", "nan"], ["--margin", "inf"], ["--views", "-1"], ["--min-points", "-1"]])
def test_cli_refuses_bad_arguments(argv, capsys):
    p = SO.parser()
    a = p.parse_args(["scene.ply", "boxes.pkl", "out"] + argv)
    with pytest.raises(SystemExit):
        SO.check_arguments(p, a)
    assert argv[0] in capsys.readouterr().err


def test_cli_accepts_its_defaults():
    p = SO.parser()
    a = p.parse_args(["scene.ply", "boxes.pkl", "out"])
    SO.check_arguments(p, a)
    assert (a.margin, a.min_points, a.views, a.size) == (0.0, 1, 8, [480, 640])
    assert isinstance(p, argparse.ArgumentParser)
