"""The C-ABI library builds for gfx950, loads without a GPU, and exports every entry point that
include/boxfusion_hip.h declares (no compute calls here)."""
import ctypes
import os
import re

import pytest

from boxfusion_amd import build as B

HEADER = os.path.join(os.path.dirname(B.HERE), "include", "boxfusion_hip.h")


def declared():
    src = open(HEADER).read()
    return sorted(set(re.findall(r"^\s*(?:const\s+char\*|int|size_t|void)\s+(bf_\w+)\s*\(", src, re.M)))


def test_header_declares_entry_points():
    names = declared()
    for must in ["bf_obb_iou_matrix", "bf_nms_scan", "bf_corr_assoc", "bf_fusion_fit",
                 "bf_depth_standardize", "bf_backproject", "bf_box_corners"]:
        assert must in names


def test_library_exports_all_symbols():
    path = B.build()
    lib = ctypes.CDLL(path)
    missing = [n for n in declared() if not hasattr(lib, n)]
    assert not missing, missing
    lib.bf_version.restype = ctypes.c_char_p
    assert b"gfx950" in lib.bf_version()


def test_gemm_abi_is_stateless():
    """no process-wide GEMM / attention knobs in the product ABI (round-5 verdict item 6): the
    options travel per call in bf_gemm_plan / the _ex variant argument, and the library no longer
    exports the old setters"""
    src = open(HEADER).read()
    assert not re.search(r"\bbf_(gemm|attention)_(set|get|force)_\w*\s*\(", src)
    lib = ctypes.CDLL(B.build())
    for gone in ["bf_gemm_set_variant", "bf_gemm_set_tile_rows", "bf_gemm_force_small_tiles",
                 "bf_gemm_set_group_m", "bf_gemm_set_balanced", "bf_gemm_set_cu_budget",
                 "bf_gemm_get_cu_budget", "bf_gemm_get_variant", "bf_attention_set_variant"]:
        assert not hasattr(lib, gone), gone
    # the Python mirror of bf_gemm_plan has the header's layout (six int32 fields)
    from boxfusion_amd import _lib
    body = re.search(r"typedef struct \{([^}]*)\} bf_gemm_plan;", src).group(1)
    fields = re.findall(r"int32_t\s+(\w+);", body)
    assert [f for f, _ in _lib.GemmPlan._fields_] == fields
    assert ctypes.sizeof(_lib.GemmPlan) == 4 * len(fields)


# ---- the binding takes its types from the header (boxfusion_amd/_abi.py) --------------------------
def param_counts():
    """{entry point: parameter count} by commas, with this file's own regular expressions"""
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(bf_\w+)\s*\(([^()]*)\)\s*;", src):
        out[name] = 0 if params.strip() in ("", "void") else params.count(",") + 1
    return out


def test_reader_finds_every_prototype_and_lib_types_it():
    from boxfusion_amd import _abi, _lib
    names = declared()
    assert len(names) == 110
    assert sorted(_abi.prototypes()) == names
    B.build()
    lib, counts = _lib.lib(), param_counts()
    assert sorted(counts) == names
    for n in names:
        f = getattr(lib, n)
        assert f.argtypes is not None and len(f.argtypes) == counts[n], n


def test_signatures_spot_checks():
    from boxfusion_amd import _lib
    B.build()
    lib = _lib.lib()
    c = ctypes
    assert (lib.bf_version.restype, list(lib.bf_version.argtypes)) == (c.c_char_p, [])
    f = lib.bf_obb_iou_workspace_size
    assert (f.restype, list(f.argtypes)) == (c.c_size_t, [c.c_int])
    f = lib.bf_cloud_blocks
    assert (f.restype, list(f.argtypes)) == (c.c_size_t, [c.c_longlong, c.c_int])
    assert lib.bf_fseq_destroy.restype is None and list(lib.bf_fseq_destroy.argtypes) == [c.c_void_p]
    a = list(lib.bf_icp_reduce.argtypes)
    assert len(a) == 20 and a[11:17] == [c.c_double] * 6 and a[-1] is c.c_void_p
    assert lib.bf_icp_reduce.restype is c.c_int
    assert a[:11] == [c.c_void_p, c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p,
                      c.c_int, c.c_int, c.c_void_p]


def test_host_entry_points_through_the_typed_handle():
    from boxfusion_amd import _lib
    B.build()
    lib = _lib.lib()
    assert lib.bf_icp_blocks(480, 640, 4) == 19
    assert lib.bf_cloud_blocks(1000, 3) == 12
    assert lib.bf_cloud_blocks(1 << 40, 1) == 1 << 32          # a size_t, not truncated to an int
    assert _lib.icp_blocks(480, 640, 4) == 19
    with pytest.raises(TypeError):
        lib.bf_icp_blocks(480, 640)
    with pytest.raises(ctypes.ArgumentError):
        lib.bf_icp_blocks(480, 640, 4.0)
    with pytest.raises(ctypes.ArgumentError):
        lib.bf_cloud_blocks(1000.0, 3)


I, I32, I64, F, D, P = (ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_double,
                        ctypes.c_void_p)
# written out from the hand-made mirrors the binding had before it read the header
STRUCTS = {
    "RowsField": [("a", P), ("b", P), ("dst", P), ("n_a", I64), ("n_b", I64), ("row_bytes", I32), ("pad", I32)],
    "FilterCfg": [("score_thresh", F), ("floor_ratio", F), ("floor_half", F), ("size_max", F), ("gap_w", I32),
                  ("gap_h", I32), ("W", I32), ("H", I32), ("use_score", I32), ("use_uv", I32), ("use_floor", I32),
                  ("use_large", I32)],
    "NmsCfg": [("iou_threshold", D), ("translation_gap", F), ("rotation_gap", F), ("center_gap", D),
               ("max_list", I), ("list_capacity", I)],
    "CorrCfg": [("small_size", D), ("threshold", D), ("translation_gap", F), ("rotation_gap", F), ("W", F), ("H", F),
                ("max_list", I), ("list_capacity", I)],
    "FuseCfg": [("iters", I), ("pst_size", I), ("max_accept", I), ("legacy_promotion", I), ("center_init", D),
                ("shape_init", D), ("center_coef", D), ("shape_coef", D), ("beta", D), ("min_scale", D),
                ("img_h", F), ("img_w", F), ("K", F * 16)],
    "FseqCfg": [("nms", "NmsCfg"), ("corr", "CorrCfg"), ("fuse", "FuseCfg"), ("use_fusion", I32),
                ("strict_hull", I32)],
    "GemmPlan": [("cu_budget", I32), ("tile_rows", I32), ("kernel", I32), ("variant", I32), ("group_m", I32),
                 ("balanced", I32), ("objective", I32)],
}


@pytest.mark.parametrize("name", sorted(STRUCTS))
def test_struct_mirror_has_the_hand_written_layout(name):
    from boxfusion_amd import _lib
    cls = getattr(_lib, name)
    assert issubclass(cls, ctypes.Structure)
    want = [(f, getattr(_lib, t) if isinstance(t, str) else t) for f, t in STRUCTS[name]]
    assert list(cls._fields_) == want


def test_struct_sizes_and_offsets():
    from boxfusion_amd import _lib
    assert ctypes.sizeof(_lib.NmsCfg) == 32 and ctypes.sizeof(_lib.CorrCfg) == 40
    assert ctypes.sizeof(_lib.FuseCfg) == 136
    assert _lib.FuseCfg.K.offset == 72
    assert ctypes.sizeof(_lib.FseqCfg) == 32 + 40 + 136 + 8 == 216
    assert ctypes.sizeof(_lib.RowsField) == 48 and ctypes.sizeof(_lib.FilterCfg) == 48


def test_reader_refuses_a_type_it_does_not_know():
    from boxfusion_amd import _abi
    assert _abi._ctype("const  float *", "bf_f, parameter 1", _abi._SCALAR) is ctypes.c_void_p
    with pytest.raises(TypeError, match=r"bf_s\.b.*'unsigned'"):
        _abi._ctype("unsigned", "bf_s.b", _abi._SCALAR)


def test_lib_py_assigns_no_signatures_of_its_own():
    from boxfusion_amd import _lib
    assert not re.search(r"\.(restype|argtypes)\b", open(_lib.__file__).read())


# ---- the layout constants are written once, in the header (boxfusion_amd/_abi.constants) ----------
CONSTANTS = {
    "BF_DEV_OK": 0, "BF_DEV_FUSION_LIST_OVERFLOW": 1, "BF_DEV_HULL_OVERFLOW": 2, "BF_DEV_VIEW_OVERFLOW": 4,
    "BF_DEV_INDEX_RANGE": 8, "BF_DEV_HULL_TRUNC": 16, "BF_MAX_BOXES": 4096, "BF_ROWS_MAX_FIELDS": 16,
    "BF_FSEQ_STATE_N": 16,
    "BF_OK": 0, "BF_ERR_ARG": -1, "BF_ERR_LAUNCH": -2, "BF_ERR_CAPACITY": -3, "BF_ERR_UNSUPPORTED": -4,
    "BF_KEY_BITS": 21, "BF_KEY_BIAS": 1048576, "BF_KEY_EMPTY": 0xFFFFFFFFFFFFFFFF, "BF_STATS_WORDS": 8,
    "BF_CLOUD_SLOT_WORDS": 5, "BF_CLOUD_MAX_COUNT": 16777216, "BF_CLOUD_FINE_STEPS": 256,
    "BF_CLOUD_STAT_STORED": 0, "BF_CLOUD_STAT_NONFINITE": 1, "BF_CLOUD_STAT_OUT_OF_RANGE": 2,
    "BF_CLOUD_STAT_DROPPED_FULL": 3, "BF_CLOUD_STAT_SATURATED": 4, "BF_CLOUD_STAT_RUNS": 5,
    "BF_TSDF_VOX": 512, "BF_TSDF_FIELDS": 6, "BF_TSDF_MAX_WEIGHT": 1048576, "BF_TSDF_MAX_FRAMES": 64,
    "BF_TSDF_MAX_TRUNC": 64,
    "BF_TSDF_STAT_OBSERVATIONS": 0, "BF_TSDF_STAT_SKIPPED_POSE": 1, "BF_TSDF_STAT_OUT_OF_RANGE": 2,
    "BF_TSDF_STAT_DROPPED_FULL": 3, "BF_TSDF_STAT_SATURATED": 4, "BF_TSDF_STAT_BLOCKS": 5,
    "BF_TSDF_RAY_HITS": 0, "BF_TSDF_RAY_BEHIND": 1, "BF_TSDF_RAY_LEFT_RANGE": 2, "BF_TSDF_RAY_SKIPPED_POSE": 3,
    "BF_TSDF_RAY_NO_NORMAL": 4,
    "BF_ICP_ROW": 32,
    "BF_FERN_K_MAX": 8, "BF_FERN_CELL_MAX": 64, "BF_FERN_COUNT_OBSERVED": 0, "BF_FERN_COUNT_ADDED": 1,
    "BF_FERN_COUNT_DROPPED_FULL": 2,
    "BF_PNG_BAD_SIGNATURE": 1, "BF_PNG_BAD_HEADER": 2, "BF_PNG_UNSUPPORTED": 4, "BF_PNG_BAD_CHUNK": 8,
    "BF_PNG_BAD_ZLIB": 16, "BF_PNG_BAD_ADLER": 32, "BF_PNG_BAD_FILTER": 64, "BF_PNG_SIZE": 128,
    "BF_JPG_BAD_MARKER": 1, "BF_JPG_UNSUPPORTED": 2, "BF_JPG_SIZE": 4, "BF_JPG_BAD_DATA": 8,
}


def test_constants_have_the_written_out_values():
    from boxfusion_amd import _abi
    assert _abi.constants() == CONSTANTS


def test_lib_py_takes_its_numbers_from_the_header():
    from boxfusion_amd import _lib, scene_cloud, scene_mesh
    assert (_lib.BF_DEV_FUSION_LIST_OVERFLOW, _lib.BF_DEV_HULL_OVERFLOW, _lib.BF_DEV_VIEW_OVERFLOW,
            _lib.BF_DEV_INDEX_RANGE, _lib.BF_DEV_HULL_TRUNC) == (1, 2, 4, 8, 16)
    assert (_lib.ROWS_MAX_FIELDS, _lib.FSEQ_STATE_N, _lib.STATS_WORDS, _lib.ICP_ROW) == (16, 16, 8, 32)
    assert (_lib.TSDF_VOX, _lib.TSDF_FIELDS, _lib.TSDF_MAX_WEIGHT, _lib.TSDF_MAX_FRAMES) == (512, 6, 1048576, 64)
    assert (_lib.CLOUD_SLOT_WORDS, _lib.FERN_K_MAX) == (5, 8)
    assert sorted(_lib.PNG_STATUS) == [1, 2, 4, 8, 16, 32, 64, 128]
    assert sorted(_lib.ZLIB_STATUS) == [8, 16, 32, 128] and sorted(_lib.JPEG_STATUS) == [1, 2, 4, 8]
    assert _lib.PNG_STATUS[64] == "bad row filter" and _lib.JPEG_STATUS[4] == "size mismatch"
    assert (scene_cloud.KEY_BIAS, scene_cloud.KEY_MASK, scene_mesh.MAX_FRAMES) == (1048576, 2097151, 64)


def test_counter_names_follow_the_header_enums():
    """the tuples _lib.py held as literals before it built them from the enums"""
    from boxfusion_amd import _lib
    assert _lib.CLOUD_STATS == ("stored", "nonfinite", "out_of_range", "dropped_full", "saturated", "runs")
    assert _lib.TSDF_STATS == ("observations", "skipped_pose", "out_of_range", "dropped_full", "saturated", "blocks")
    assert _lib.TSDF_RAYCAST_STATS == ("hits", "behind", "left_range", "skipped_pose", "no_normal")
    assert _lib.FERN_COUNTERS == ("observed", "added", "dropped_full")


def test_reader_reads_the_literal_forms_and_refuses_the_rest():
    from boxfusion_amd import _abi
    text = ("#ifndef BF_GUARD_H\n#define BF_GUARD 7\n#define BF_CALL(x) ((x) + 1)\n#define OTHER 1 + 2\n"
            "#define BF_A 0x1Full\n#define BF_B (1u << 24)\n#define BF_C ( 3 )\n#define BF_D 12L\n"
            "typedef enum { BF_E, BF_F = -2, BF_G, BF_H = 1 << 4, BF_I } bf_e;\n")
    assert _abi.constants(text) == {"BF_GUARD": 7, "BF_A": 31, "BF_B": 1 << 24, "BF_C": 3, "BF_D": 12, "BF_E": 0,
                                    "BF_F": -2, "BF_G": -1, "BF_H": 16, "BF_I": 17}
    with pytest.raises(ValueError, match=r"BF_BAD.*'BF_A \* 2'"):
        _abi.constants("#define BF_BAD BF_A * 2\n")
    with pytest.raises(ValueError, match=r"BF_OPEN.*'\(1 << 20'"):
        _abi.constants("#define BF_OPEN (1 << 20\n")
    with pytest.raises(ValueError, match=r"BF_EMPTY"):
        _abi.constants("#define BF_EMPTY\n")
    with pytest.raises(ValueError, match=r"BF_M.*'sizeof\(int\)'"):
        _abi.constants("enum { BF_L, BF_M = sizeof(int) };\n")


def test_python_retypes_no_key_arithmetic():
    from boxfusion_amd import _lib, scene_cloud, scene_mesh
    for mod in (_lib, scene_cloud, scene_mesh):
        # the one `1 << 20` left is scene_mesh.py's cap on a ray's step count: no key, no weight and not in the header
        src = "\n".join(ln for ln in open(mod.__file__).read().splitlines()
                        if not (mod is scene_mesh and ln.lstrip().startswith("steps = ")))
        for literal in ("1 << 20", "<< 42", "0x1FFFFF"):
            assert literal not in src, (mod.__name__, literal)


def test_a_define_cannot_join_a_counter_tuple():
    from boxfusion_amd import _abi
    text = "enum { BF_X_STAT_A, BF_X_STAT_B };\n#define BF_X_STAT_LATER 1\nenum { BF_X_RAY_C = 1, BF_X_RAY_D = 0 };\n"
    assert _abi.enum_names("BF_X_STAT_", text) == ("a", "b") and _abi.enum_names("BF_X_RAY_", text) == ("d", "c")
    with pytest.raises(KeyError, match="BF_X_NONE_"):
        _abi.enum_names("BF_X_NONE_", text)
    with pytest.raises(KeyError, match="2 enums"):
        _abi.enum_names("BF_X_", text)
