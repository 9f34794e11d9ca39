"""bf_assoc.hip against the CPU oracle, bit for bit, on the seeded cases of tests/assoc_cases.py
(tests/test_assoc_cases_host.py asserts which paths each case reaches): k_corr_assoc through
bf_corr_assoc and bf_corr_assoc_chained, the 256-thread k_nms_scan in both its forms, and
bf_fusion_writeback.  Runs only on a HIP device."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import oracle as OR
from tests import assoc_cases as AC

pytestmark = pytest.mark.gpu

I32 = torch.int32
_t = AC.to_dev


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from boxfusion_amd import _lib
    return _lib


def corr_run(L, case, chained=False, items=None, lens=None):
    """one k_corr_assoc launch on a case; returns host arrays.  `chained`: through
    bf_corr_assoc_chained, with the counts on the device and poisoned buffer tails."""
    c = case
    n_all, n_glo, cap = len(c["scores"]), c["n_glo"], c["cap"]
    if items is None:
        items, lens = OR.pack_lists(c["fusion_list"], cap)
    it, ln, vn = _t(items, I32), _t(lens, I32), _t(c["valid_num"])
    args = (_t(c["corners"]), _t(c["dims"]), _t(c["scores"]), _t(c["boxes2d"]), _t(c["init_id"], I32),
            _t(c["cam_poses"]), _t(c["cur_pose"]), _t(c["K"]), n_glo)
    cfg = AC.as_cfg(L.CorrCfg, AC.corr_cfg(cap, c["max_list"]))
    # n_keep and n_events preset to a value no run gives: both must be written, also when no box
    # is kept and no kernel runs (status is OR-ed into and starts clear)
    counts = _t(np.array([7, 7, 0], np.int32), I32)
    if not chained:
        out = (torch.full((max(1, len(c["mask"])),), -5, dtype=I32, device="cuda"),
               torch.full((n_all + 1, 3), -5, dtype=I32, device="cuda"), counts)
        keep, ev, cnt = L.corr_assoc(*args, _t(c["mask"], I32), _t(c["success"], I32), it, ln, vn, cfg,
                                     out=out)
    else:
        # the buffers nms_scan leaves: n_all + 1 entries, the counts in device words.  A read
        # past the mask count would find a global index (one more kept global box), one past the
        # success count the pinned new box (its event would be skipped)
        mask = np.full(n_all + 1, AC.POISON, np.int32)
        mask[:len(c["mask"])] = c["mask"]
        succ = np.full(n_all + 1, n_glo, np.int32)
        succ[:len(c["success"])] = c["success"]
        out = (torch.full((n_all,), -5, dtype=I32, device="cuda"),
               torch.full((n_all + 1, 3), -5, dtype=I32, device="cuda"), counts)
        keep, ev, cnt = L.corr_assoc_chained(
            *args, _t(mask, I32), _t(np.array([len(c["mask"])], np.int32), I32), _t(succ, I32),
            _t(np.array([len(c["success"])], np.int32), I32), it, ln, vn, cfg, out)
    torch.cuda.synchronize()
    k = cnt.cpu().numpy()
    return dict(keep=keep.cpu().numpy()[:k[0]], events=ev.cpu().numpy()[:k[1]], status=int(k[2]),
                n_keep=int(k[0]), n_events=int(k[1]), items=it.cpu().numpy(), lens=ln.cpu().numpy(), valid_num=vn.cpu().numpy())


def corr_compare(case, got, ref):
    n_all, cap = len(case["scores"]), case["cap"]
    assert got["status"] == ref["status"]
    assert (got["n_keep"], got["n_events"]) == (len(ref["keep"]), len(ref["events"]))
    np.testing.assert_array_equal(got["keep"], ref["keep"], err_msg="keep")
    np.testing.assert_array_equal(got["events"], ref["events"], err_msg="events")
    np.testing.assert_array_equal(got["valid_num"], ref["valid_num"], err_msg="valid_num")
    # the whole padded array: lists, and -1 still in every entry at or beyond a row's length
    items, lens = OR.pack_lists(ref["fusion_list"], cap)
    np.testing.assert_array_equal(got["lens"], lens, err_msg="fl_len")
    np.testing.assert_array_equal(got["items"], items, err_msg="fl_items")
    assert OR.unpack_lists(got["items"], got["lens"], n_all) == ref["fusion_list"]


@pytest.mark.parametrize("name", list(AC.CORR_CASES))
def test_corr_assoc_vs_oracle(L, name):
    """bf_corr_assoc (k_corr_assoc, one 256-thread workgroup) against OR.corr_assoc on every seeded
    case: keep, the events and their count, the fusion lists as the whole padded array, all of
    valid_num and the status word (the overflow bit in the small-capacity cases).  The two counts
    are preset to 7, so they are compared as written, also on the empty mask's no-launch path"""
    case, ref = AC.corr_named(name)
    corr_compare(case, corr_run(L, case), ref)


@pytest.mark.parametrize("name", ["40x12", "300x40", "70x150", "empty_mask", "tie256_lower_first", "cap4"])
def test_corr_assoc_chained_vs_oracle(L, name):
    """bf_corr_assoc_chained (k_corr_assoc with the mask / success counts read on the device and
    LDS sized for n_all) against the same oracle results; the mask and success buffers carry
    poison past their counts, the out views are n_all / n_all + 1 rows, and an empty mask
    (device count 0) comes back with n_keep 0 and n_events 0"""
    case, ref = AC.corr_named(name)
    got = corr_run(L, case, chained=True)
    corr_compare(case, got, ref)
    if name == "empty_mask":
        assert got["n_keep"] == 0 and got["n_events"] == 0


@pytest.mark.parametrize("order", ["cur", "idx"])
def test_corr_assoc_input_list_longer_than_capacity(L, order):
    """an input fusion-list length above the row capacity (a caller error) on the global box that
    the pinned new box matches, as record_corr's cur (branch 1) and as its idx (branch 2): the
    length is clamped to the row, the overflow bit is set, and everything else -- every entry of
    the padded array and of a guard row behind it -- equals the oracle run on that row at its
    full capacity (where record_corr tries no append).  Device only: pack_lists refuses such input."""
    case, ref, g, m = AC.over_capacity_case(order)
    cap = case["cap"]
    items, lens = OR.pack_lists(case["fusion_list"] + [[]], cap)   # one guard row
    lens[g] = cap + 5
    got = corr_run(L, case, items=items, lens=lens)
    assert got["status"] == L.BF_DEV_FUSION_LIST_OVERFLOW
    want_items, want_lens = OR.pack_lists(ref["fusion_list"] + [[]], cap)
    want_lens[g] = cap + 5
    np.testing.assert_array_equal(got["items"], want_items)
    np.testing.assert_array_equal(got["lens"], want_lens)
    for k in ("keep", "events", "valid_num"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)


# ---------------------------------------------------------------------------------------------
# the 256-thread block scan
# ---------------------------------------------------------------------------------------------
def nms_run(L, case, cap, workspace):
    """the greedy scan on a case through _lib.nms_scan (with a workspace) or through the public
    bf_nms_scan (none), on the device IoU matrix"""
    c = case
    n = len(c["scores"])
    items, lens = OR.pack_lists(c["fusion_list"], cap)
    it, ln, vn = _t(items, I32), _t(lens, I32), _t(c["valid_num"])
    corners = _t(c["corners"])
    iou = L.obb_iou_matrix(corners)
    cfg = AC.as_cfg(L.NmsCfg, AC.nms_cfg(cap))
    a = (iou, corners, _t(c["scores"]), _t(c["init_id"], I32), _t(c["cam_poses"]), it, ln, vn)
    if workspace:
        keep, succ, ev, cnt = L.nms_scan(*a, cfg)
    else:
        keep = torch.empty(n + 1, dtype=I32, device="cuda")
        succ = torch.empty(n + 1, dtype=I32, device="cuda")
        ev = torch.empty((n + 1, 3), dtype=I32, device="cuda")
        cnt = torch.zeros(4, dtype=I32, device="cuda")
        p = L._ptr
        rc = L.lib().bf_nms_scan(p(a[0]), p(a[1]), p(a[2]), p(a[3]), p(a[4]), ctypes.c_int(n), p(it), p(ln),
                                 p(vn), p(keep), p(cnt[0:1]), p(succ), p(cnt[1:2]), p(ev), p(cnt[2:3]),
                                 p(cnt[3:4]), ctypes.byref(cfg), L._stream())
        assert rc == 0
    torch.cuda.synchronize()
    k = cnt.cpu().numpy()
    return iou.cpu().numpy(), dict(
        keep=keep.cpu().numpy()[:k[0]], success=succ.cpu().numpy()[:k[1]], events=ev.cpu().numpy()[:k[2]],
        status=int(k[3]), items=it.cpu().numpy(), lens=ln.cpu().numpy(), valid_num=vn.cpu().numpy())


@pytest.mark.parametrize("n_glo,n_new,cap,workspace,form", AC.BLOCK_SCANS)
def test_nms_block_scan_vs_oracle(L, n_glo, n_new, cap, workspace, form):
    """k_nms_scan (256 threads: the IoU matrix staged in LDS up to 120 boxes, read from global
    memory above; its own keep edit, lane 0's sorted list append and the block rank sort) against
    OR.nms_scan: keep, success, events, fusion lists as the whole padded array and valid_num.
    tests/test_assoc_cases_host.py asserts the paths these cases reach, on the oracle's IoU."""
    assert L.nms_scan_form(n_glo + n_new, cap, workspace) == form
    case = AC.block_scan_case(n_glo, n_new)
    iou, got = nms_run(L, case, cap, workspace)
    ref = AC.nms_oracle(case, iou, cap)
    assert ref["status"] == 0 and got["status"] == 0
    for k in ("keep", "success", "events", "valid_num"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    items, lens = OR.pack_lists(ref["fusion_list"], cap)
    np.testing.assert_array_equal(got["lens"], lens)
    np.testing.assert_array_equal(got["items"], items)
    AC.assert_block_scan_paths(AC.nms_paths(case, ref))      # on the device IoU too


def test_nms_scan_forms_at_the_switches(L):
    """bf_nms_scan_form at each threshold of the launcher: 96 | 97 boxes, the bit-mask scan's LDS
    budget (340 | 341 at capacity 64), 120 | 121 for the block scan's IoU staging, and the list
    capacity that pushes a small scan out of LDS"""
    f = L.nms_scan_form
    assert [f(n, 64, True) for n in (1, 96, 97, 340, 341, 4096)] == [0, 0, 1, 1, 3, 3]
    assert [f(n, 64, False) for n in (1, 96, 97, 120, 121, 4096)] == [0, 0, 2, 2, 3, 3]
    assert f(96, 512, True) == 2 and f(96, 512, False) == 2 and f(121, 512, True) == 3
    assert {0, 1, 2, 3} == {f(96, 64, True), f(340, 64, True), f(97, 64, False), f(341, 64, True)}


# ---------------------------------------------------------------------------------------------
# bf_fusion_writeback
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ld", [6, 9])
@pytest.mark.parametrize("n_jobs", [1, 11, 64, 65])
@pytest.mark.parametrize("mix", ["mixed", "none", "all"])
def test_fusion_writeback_vs_numpy(L, n_jobs, ld, mix):
    """target[rows[j], :6] = out_box[j] where updated[j], against numpy indexing; every other
    float of the target (rows not named, jobs not updated, columns 6 and above) bitwise unchanged"""
    rng = np.random.default_rng(100 * n_jobs + ld)
    n_rows = n_jobs + 9
    target = rng.integers(0, 2 ** 32, (n_rows, ld), dtype=np.uint32).view(np.float32)
    out_box = rng.integers(0, 2 ** 32, (n_jobs, 6), dtype=np.uint32).view(np.float32)
    rows = rng.permutation(n_rows)[:n_jobs].astype(np.int32)
    upd = dict(mixed=rng.integers(0, 2, n_jobs), none=np.zeros(n_jobs), all=np.ones(n_jobs))[mix].astype(np.int32)
    if mix == "mixed" and n_jobs > 1:
        upd[0], upd[-1] = 1, 0
    want = target.copy()
    want[rows[upd != 0], :6] = out_box[upd != 0]
    tgt = _t(target)
    L.fusion_writeback(_t(out_box), _t(upd, I32), _t(rows, I32), tgt)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(tgt.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_fusion_writeback_empty_and_bad_ld(L):
    """n_jobs = 0 returns OK and touches nothing; a row stride under 6 floats is BF_ERR_ARG"""
    rng = np.random.default_rng(3)
    target = rng.standard_normal((5, 6)).astype(np.float32)
    tgt = _t(target)
    e = torch.empty(0, dtype=I32, device="cuda")
    L.fusion_writeback(torch.empty((0, 6), device="cuda"), e, e, tgt)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(tgt.cpu().numpy(), target)
    t5 = _t(rng.standard_normal((5, 5)).astype(np.float32))
    one = torch.ones(1, dtype=I32, device="cuda")
    with pytest.raises(L.HipError, match="bf_status -1"):
        L.fusion_writeback(torch.zeros((1, 6), device="cuda"), one, torch.zeros(1, dtype=I32, device="cuda"), t5)
