"""The seeded association cases of tests/assoc_cases.py reach the paths they claim, by the oracle
alone (CPU only).  tests/test_gpu_assoc.py compares the kernels with the oracle on these very
cases, so a case that stops reaching a path must fail here rather than pass silently there."""
import numpy as np
import pytest

from oracle import oracle as OR
from tests import assoc_cases as AC

SHOWN = ("ng", "events", "branch1", "branch2", "lists_grown", "b2_grew", "b2_replaced", "cur_new",
         "cur_glo", "zero_proj", "clamped", "best_pos")


@pytest.mark.parametrize("name", list(AC.CORR_CASES))
def test_corr_case_reaches_its_paths(name):
    case, ref = AC.corr_named(name)
    want = AC.CORR_CASES[name][2]
    p = AC.corr_paths(case, ref)
    print(name, {k: p[k] for k in SHOWN}, "visited", len(p["visited"]), "status", ref["status"])
    n = len(case["scores"])
    mask = case["mask"]
    assert (np.diff(mask) > 0).all() and (mask >= 0).all() and (mask < n).all()
    np.testing.assert_array_equal(case["init_id"], np.arange(n))
    assert all(0 <= v < n for row in case["fusion_list"] for v in row)
    # the oracle's status: the overflow bit in the overflow cases, else clean
    assert ref["status"] == (1 if want.get("overflow") else 0)
    # the numpy restatement of the argmax names the pairs the oracle recorded, in its order
    assert [tuple(int(x) for x in e[:2]) for e in ref["events"]] == p["pairs"]
    if want["events"] == 0:
        assert p["events"] == 0
        np.testing.assert_array_equal(ref["keep"], mask)
        np.testing.assert_array_equal(ref["valid_num"], case["valid_num"])
    else:
        assert p["events"] >= want["events"]
    for k in ("ng", "best_pos"):
        if k in want:
            assert p[k] == want[k], k
    if "visited" in want:
        assert len(p["visited"]) == want["visited"] and (mask >= case["n_glo"]).sum() >= 5
    if "n_mask" in want:
        assert len(mask) == want["n_mask"]
    if p["ng"] > 256:
        assert p["best_pos"] >= 256                 # a winner in the second trip of a lane's loop
    if "each_branch" in want:
        assert p["branch1"] >= want["each_branch"] and p["branch2"] >= want["each_branch"]
        assert p["b2_grew"] >= want["grow"] and p["b2_replaced"] >= want["replace"]
        assert p["cur_new"] >= 1 and p["cur_glo"] >= 1
        assert p["zero_proj"] >= 3 and p["clamped"] >= 3
    assert bool(case["edges"]) == AC.wants_edges(p["ng"], n - case["n_glo"], **AC.CORR_CASES[name][1])
    assert all(m in mask for _, m, _ in case["edges"])
    cfg = AC.corr_cfg()
    gpos = {int(g): k for k, g in enumerate(p["gk"])}
    b2d = OR.project_2d_box(case["corners"][p["gk"]], case["cur_pose"], case["K"], AC.W, AC.H) if p["ng"] else None
    for kind, m, g in case["edges"]:
        # each pair decides one edge of project_2d_box: see assoc_cases.EDGE_KINDS
        assert m in p["visited"] and case["dims"][g].max() < np.float32(cfg.small_size + 0.1)
        ev = [e for e in ref["events"] if m in e[:2]]
        row, v = b2d[gpos[g]], p["ious"][m]
        if kind in AC.EDGE_NO_MATCH:
            # no match with g; a projection without the test would give g an IoU of 1 (the new
            # box's 2-D box is that projection), above every other candidate's
            assert (row == 0).all() and v[gpos[g]] == 0 and v.max() < 0.99
            assert len(ev) <= 1 and not any(g in e[:2] for e in ev)
            continue
        assert len(ev) == 1 and g in ev[0][:2] and int(np.argmax(v)) == gpos[g]
        if kind in ("right", "bottom", "left", "top"):
            ax, hi = (0, kind == "right") if kind in ("right", "left") else (1, kind == "bottom")
            lim = (AC.W, AC.H)[ax]
            off = row.copy()                        # the same box clamped one pixel short
            assert row[ax + 2 if hi else ax] == (lim if hi else 0)
            off[ax + 2 if hi else ax] = lim - 1 if hi else 1
            assert AC.iou_2d(case["boxes2d"][m], off[None])[0] == 0 < cfg.threshold < v[gpos[g]]
        if kind == "behind":
            full = AC._project(*AC.edge_box(kind)[:3])[2]       # with the corners behind the camera
            assert AC.iou_2d(case["boxes2d"][m], AC.clamp_box(full)[None])[0] < cfg.threshold < v[gpos[g]]
    if want.get("overflow"):
        # rows filled to the capacity, and some lists still grew before that
        cap = case["cap"]
        assert max(len(r) for r in ref["fusion_list"]) == cap and p["lists_grown"] >= 1
    if want.get("tie"):
        d, lower_first = case["tie"]
        m, pos = case["pins"][0]
        v = p["ious"][m]
        assert v[pos] == v[pos + d] == v.max() and v[pos] > AC.corr_cfg().threshold
        assert int(np.argmax(v)) == pos and (v == v.max()).sum() == 2
        first, second = int(p["gk"][pos]), int(p["gk"][pos + d])
        assert (case["scores"][first] < case["scores"][m] < case["scores"][second]) == lower_first
        assert (case["scores"][second] < case["scores"][m] < case["scores"][first]) != lower_first
        ev = [e for e in ref["events"] if m in e[:2]]
        assert len(ev) == 1 and first in ev[0][:2] and second not in ev[0][:2]
        # the other copy would have changed the answer: cur and idx swap with the score order
        assert int(ev[0][0]) == (m if lower_first else first)


def test_corr_cases_cover_the_listed_shapes_and_paths():
    """the shapes and the degenerate cases the kernel tests rely on are all present, and over the
    whole set both keep edits of branch 2 and both kinds of cur occur"""
    shapes = {AC.CORR_CASES[k][0][:2] for k in AC.CORR_CASES}
    assert {(0, 3), (1, 1), (5, 0), (40, 12), (255, 20), (256, 20), (257, 20), (300, 40), (600, 60),
            (70, 150)} <= shapes
    tot = dict.fromkeys(SHOWN, 0)
    for name in AC.CORR_CASES:
        p = AC.corr_paths(*AC.corr_named(name))
        for k in SHOWN:
            tot[k] += p[k]
    print(tot)
    assert tot["branch1"] >= 20 and tot["branch2"] >= 20
    assert tot["b2_grew"] >= 5 and tot["b2_replaced"] >= 5


@pytest.mark.parametrize("n_glo,n_new,cap,workspace,form", AC.BLOCK_SCANS)
def test_block_scan_case_reaches_its_paths(n_glo, n_new, cap, workspace, form):
    """the cases of the 256-thread k_nms_scan: suppressions of both branches, lists grown, keep
    replaced, and branch 2 with source lists below, at and above max_list, no overflow"""
    case = AC.block_scan_case(n_glo, n_new)
    ref = AC.nms_oracle(case, OR.obb_iou_matrix(case["corners"]), cap)
    p = AC.nms_paths(case, ref)
    print(n_glo + n_new, cap, p)
    assert ref["status"] == 0 and max(len(r) for r in ref["fusion_list"]) < cap
    AC.assert_block_scan_paths(p)


@pytest.mark.parametrize("order", ["cur", "idx"])
def test_over_capacity_case_visits_the_full_row(order):
    """the row that the device test gives a length above the capacity is visited by exactly one
    event of the pinned new box, as cur (branch 1) or as idx (branch 2), and at that capacity no
    append is tried, so the oracle on the full row states what the clamped device run must give"""
    case, ref, g, m = AC.over_capacity_case(order)
    cap = case["cap"]
    assert ref["status"] == 0 and len(case["fusion_list"][g]) == cap >= case["max_list"]
    assert max(len(r) for i, r in enumerate(case["fusion_list"]) if i != g) < cap
    ev = [e for e in ref["events"] if m in e[:2]]
    assert len(ev) == 1 and g in ev[0][:2]
    assert int(ev[0][0]) == (g if order == "cur" else m) and int(ev[0][2]) == (1 if order == "cur" else 2)
    assert ref["fusion_list"][g] == case["fusion_list"][g]


@pytest.mark.parametrize("style", ["large", "small"])
def test_nms_case_is_seeded_and_well_formed(style):
    kw = dict() if style == "large" else dict(spread=2.0, n_centres=33, scene_seed=2, max_extra=3)
    a, b = AC.nms_case(97, 3, 5, **kw), AC.nms_case(97, 3, 5, **kw)
    for k in ("corners", "scores", "cam_poses", "valid_num"):
        np.testing.assert_array_equal(a[k], b[k])
    assert a["fusion_list"] == b["fusion_list"] and a["corners"].shape == (100, 8, 3)
    assert all(row == sorted(set(row)) and i in row for i, row in enumerate(a["fusion_list"]))
    assert all(a["fusion_list"][i] == [i] for i in range(97, 100))
    OR.pack_lists(a["fusion_list"], 8)
