"""ctypes binding of libboxfusion_hip.so (the C-ABI in include/boxfusion_hip.h).

Every wrapper takes/returns torch tensors that live on the HIP device and launches on the current
torch stream.  There is deliberately no CPU fallback: if the shared library is missing or the
tensors are not on the GPU, the call raises.
"""
from __future__ import annotations

import atexit
import ctypes
import functools
import threading
import weakref
import sys
import os

import numpy as np
import torch

from . import _abi

HERE = os.path.dirname(os.path.abspath(__file__))
# BF_LIB_PATH: a diagnostic build of the same sources (e.g. one that forces a rare kernel path)
LIB_PATH = os.environ.get("BF_LIB_PATH") or os.path.join(HERE, "libboxfusion_hip.so")
_LIB = None

c_float, c_void_p = ctypes.c_float, ctypes.c_void_p

_C = _abi.constants()           # the header's #defines and enum members: every layout number below is read here
BF_DEV_FUSION_LIST_OVERFLOW, BF_DEV_HULL_OVERFLOW, BF_DEV_VIEW_OVERFLOW, BF_DEV_INDEX_RANGE, BF_DEV_HULL_TRUNC = (
    _C["BF_DEV_" + n] for n in ("FUSION_LIST_OVERFLOW", "HULL_OVERFLOW", "VIEW_OVERFLOW", "INDEX_RANGE", "HULL_TRUNC"))
STATS_WORDS, ICP_ROW, ROWS_MAX_FIELDS, FSEQ_STATE_N = (      # STATS_WORDS: of every int64 stats / counters tensor
    _C["BF_" + n] for n in ("STATS_WORDS", "ICP_ROW", "ROWS_MAX_FIELDS", "FSEQ_STATE_N"))

# the header's structs (all-zero GemmPlan = the product defaults)
NmsCfg, CorrCfg, FuseCfg, FseqCfg, FilterCfg, RowsField, GemmPlan = map(_abi.struct, (
    "bf_nms_cfg", "bf_corr_cfg", "bf_fuse_cfg", "bf_fseq_cfg", "bf_filter_cfg", "bf_rows_field", "bf_gemm_plan"))


def _bits(prefix, **messages):                      # {status bit of the header: message}
    return {_C[prefix + k]: v for k, v in messages.items()}


class HipError(RuntimeError):
    pass


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise HipError(f"{LIB_PATH} is missing: build it with `python -m boxfusion_amd.build`")
        # every entry point the header declares gets its argtypes and restype here, once: a call
        # with the wrong number or kind of arguments raises instead of reading garbage
        _LIB = _abi.declare(ctypes.CDLL(LIB_PATH))
    return _LIB


def _ptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise HipError("boxfusion_amd kernels need device tensors (no CPU fallback)")
    if not t.is_contiguous():
        raise HipError("tensor must be contiguous")
    return c_void_p(t.data_ptr())


def _stream():
    # the raw handle of the calling thread's current stream (torch.cuda.current_stream() builds a
    # Stream object through several device-index lookups: ~10 us per call on the fusion path)
    return c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


def h2d(a, device, dtype=None):
    """host array -> device tensor without blocking the host: staged through pinned memory (torch's
    caching host allocator keeps the block until the copy is done) and copied asynchronously on
    the current stream.  A pageable copy waits until the stream has drained every earlier kernel,
    which on the fusion path is a hidden synchronisation per upload."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.pin_memory().to(device, non_blocking=True)


_SYNC_DEBUG = os.environ.get("BF_SYNC_DEBUG", "0") == "1"


def _check(rc, name):
    if rc != 0:
        raise HipError(f"{name} failed with bf_status {rc}")
    if _SYNC_DEBUG:   # debugging aid: attribute asynchronous faults to the launching entry point
        try:
            torch.cuda.synchronize()
        except Exception as e:  # noqa: BLE001
            raise HipError(f"{name}: device fault after launch: {e}") from e


def _need(t, dtype, name):
    if t.dtype != dtype:
        raise HipError(f"{name}: expected {dtype}, got {t.dtype}")
    return t


def _timed(work):
    """decorator of a wrapper that KernelTimer records: while a timer entered on this thread is
    active, work(*args, **kwargs) -> (tags, flops, bytes) of the call and the call runs between the
    timer's two events; otherwise the call goes straight through.  `work` declares the wrapper's
    own signature, so a parameter added to one and not the other raises instead of shifting."""
    def deco(fn):
        @functools.wraps(fn)
        def timed(*args, **kwargs):
            t = _timer()
            if t is None:
                return fn(*args, **kwargs)
            return t.record(*work(*args, **kwargs), lambda: fn(*args, **kwargs))
        return timed
    return deco


def version():
    return lib().bf_version().decode()


# ------------------------------------------------------------------------------------------
# geometry
# ------------------------------------------------------------------------------------------
def box_corners(xyzlhw, R):
    xyzlhw = _need(xyzlhw.contiguous(), torch.float32, "xyzlhw")
    R = _need(R.contiguous(), torch.float32, "R")
    n = xyzlhw.shape[0]
    out = torch.empty((n, 8, 3), dtype=torch.float32, device=xyzlhw.device)
    _check(lib().bf_box_corners(_ptr(xyzlhw), _ptr(R), n, _ptr(out), _stream()), "bf_box_corners")
    return out


def box_transform2world(xyzlhw, R, cam_pose):
    """in place on xyzlhw / R (both contiguous f32 device tensors)"""
    n = xyzlhw.shape[0]
    _check(lib().bf_box_transform2world(_ptr(xyzlhw), _ptr(R), _ptr(cam_pose.contiguous()), n,
                                        _stream()), "bf_box_transform2world")


def project_boxes(corners, cam_pose, K, W, H):
    n = corners.shape[0]
    uv = torch.empty((n, 8, 2), dtype=torch.float32, device=corners.device)
    _check(lib().bf_project_boxes(_ptr(corners.contiguous()), _ptr(cam_pose.contiguous()),
                                  _ptr(K.contiguous()), n, W, H, _ptr(uv), _stream()),
           "bf_project_boxes")
    return uv


def _obb_iou_work(corners):
    n = int(corners.shape[0])
    # work = box pairs (i < j) of the IoU matrix (gate + 25^3 grid count launches)
    return dict(kind="obb_iou", n=n), n * (n - 1) / 2.0, 96.0 * n + 8.0 * n * n


@_timed(_obb_iou_work)
def obb_iou_matrix(corners):
    corners = _need(corners.contiguous(), torch.float32, "corners")
    n = corners.shape[0]
    iou = torch.empty((n, n), dtype=torch.float64, device=corners.device)
    ws = torch.empty(max(1, int(lib().bf_obb_iou_workspace_size(n))), dtype=torch.uint8,
                     device=corners.device)
    _check(lib().bf_obb_iou_matrix(_ptr(corners), n, _ptr(iou), _ptr(ws), _stream()),
           "bf_obb_iou_matrix")
    return iou


# ------------------------------------------------------------------------------------------
# box-set rows (Instances3D.cat / __getitem__ over every field in one launch)
# ------------------------------------------------------------------------------------------
_ROWS_DT = np.dtype([("a", np.uint64), ("b", np.uint64), ("dst", np.uint64), ("n_a", np.int64),
                     ("n_b", np.int64), ("row_bytes", np.int32), ("pad", np.int32)])


_STATUS = {}


def status_word(device):
    """persistent int32 device word per (device, host thread) that rows_gather launches without a
    caller status OR their BF_DEV_* flags into (an out-of-range index skips its row);
    check_status() reads and clears it -- FusionStage does so at the read-back it already makes
    per keyframe.  One word per thread: the fusion worker's flags never mix with (or get cleared
    by) another thread's reads."""
    import threading
    d = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    key = (d, threading.get_ident())
    if key not in _STATUS:
        _STATUS[key] = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", d))
    return _STATUS[key]


def check_status(device, what="bf_rows_gather"):
    w = status_word(device)
    v = int(w.item())
    if v:
        w.zero_()
        if v & BF_DEV_INDEX_RANGE:
            raise HipError(f"{what}: index out of range (BF_DEV_INDEX_RANGE)")
        raise HipError(f"{what}: device status {v:#x}")


def rows_gather(pairs, idx=None, n_out=None, outs=None, status=None):
    """pairs: [(a, b or None[, narrow])] contiguous device tensors with the same row shape / dtype
    per pair (narrow=True: int64 rows written as int32);
    returns new tensors with rows idx of cat(a, b) (idx: int64 device tensor; None: the whole
    concatenation; int32 or int64); `outs`: write into these contiguous tensors instead (e.g. the
    tail rows of a preallocated table).  One bf_rows_gather launch for up to ROWS_MAX_FIELDS
    fields.  An index outside [0, len(a) + len(b)) sets BF_DEV_INDEX_RANGE in `status` (an int32
    device word the caller reads back), or else in the device's status_word()."""
    if idx is not None:
        n_out = int(idx.shape[0])
    elif n_out is None:
        a, b = pairs[0]
        n_out = a.shape[0] + (0 if b is None else b.shape[0])
    given, outs, recs = outs, [], []
    for k, pr in enumerate(pairs):
        a, b = pr[0], pr[1]
        narrow = len(pr) > 2 and pr[2]                  # int64 rows -> int32 output
        if given is not None:                           # caller's contiguous destinations
            out = given[k]
        else:
            out = torch.empty((n_out,) + a.shape[1:], dtype=torch.int32 if narrow else a.dtype,
                              device=a.device)
        nb = 0 if b is None else b.shape[0]
        # contiguous tensors: stride(0) = elements per row (also for 0-row tensors)
        recs.append((a.data_ptr(), b.data_ptr() if nb else 0, out.data_ptr(), a.shape[0], nb,
                     a.stride(0) * a.element_size() if a.dim() > 1 else a.element_size(),
                     1 if narrow else 0))
        outs.append(out)
    if pairs and n_out:
        arr = np.array(recs, dtype=_ROWS_DT)
        i32 = idx is not None and idx.dtype == torch.int32
        if status is None and idx is not None:
            status = status_word(outs[0].device)
        _check(lib().bf_rows_gather(arr.ctypes.data, len(pairs), _ptr(idx), int(i32), n_out,
                                    _ptr(status) if status is not None else None, _stream()),
               "bf_rows_gather")
    return outs


# ------------------------------------------------------------------------------------------
# association
# ------------------------------------------------------------------------------------------
def _nms_scan_work(iou, corners, scores, init_id, cam_poses, fl_items, fl_len, valid_num, cfg, out=None):
    n = int(scores.shape[0])
    return dict(kind="nms_scan", n=n), float(n), 8.0 * n * n


@_timed(_nms_scan_work)
def nms_scan(iou, corners, scores, init_id, cam_poses, fl_items, fl_len, valid_num, cfg: NmsCfg,
             out=None):
    """returns device tensors: keep, succ, events, counts (n_keep, n_success, n_events, status);
    `out` = (keep, succ, events, counts) preallocated views (e.g. of one buffer read back once)"""
    dev = iou.device
    n = scores.shape[0]
    i32 = dict(dtype=torch.int32, device=dev)
    if out is not None:
        keep, succ, events, counts = out
    else:
        keep = torch.empty(n + 1, **i32)
        succ = torch.empty(n + 1, **i32)
        events = torch.empty((n + 1, 3), **i32)
        counts = torch.zeros(4, **i32)  # n_keep, n_success, n_events, status
    L = lib()
    ws = torch.empty(max(L.bf_nms_scan_workspace_size(n), 8), dtype=torch.uint8, device=dev)
    _check(L.bf_nms_scan_ws(_ptr(iou), _ptr(corners), _ptr(scores), _ptr(init_id), _ptr(cam_poses), n,
                            _ptr(fl_items), _ptr(fl_len), _ptr(valid_num), _ptr(keep), _ptr(counts[0:1]),
                            _ptr(succ), _ptr(counts[1:2]), _ptr(events), _ptr(counts[2:3]),
                            _ptr(counts[3:4]), ctypes.byref(cfg), _ptr(ws), _stream()), "bf_nms_scan_ws")
    return keep, succ, events, counts


def nms_scan_form(n, list_capacity, has_workspace=True):
    """the scan bf_nms_scan_ws launches (bf_nms_scan_form): 0 one wave on the IoU matrix, 1 one
    wave on the bit masks, 2 block scan with the IoU matrix in LDS, 3 block scan reading it from
    global memory; nms_scan always passes a workspace, bf_nms_scan none"""
    return int(lib().bf_nms_scan_form(n, list_capacity, int(bool(has_workspace))))


def corr_assoc(corners, dims, scores, boxes2d, init_id, cam_poses, cur_pose, K, n_glo, mask,
               success, fl_items, fl_len, valid_num, cfg: CorrCfg, out=None):
    """returns device tensors keep, events, counts (n_keep, n_events, status); `out` as nms_scan"""
    dev = corners.device
    n_all = scores.shape[0]
    i32 = dict(dtype=torch.int32, device=dev)
    if out is not None:
        keep, events, counts = out
    else:
        keep = torch.empty(max(1, mask.shape[0]), **i32)
        events = torch.empty((n_all + 1, 3), **i32)
        counts = torch.zeros(3, **i32)  # n_keep, n_events, status
    succ = success if success.numel() else torch.zeros(1, **i32)
    _check(lib().bf_corr_assoc(_ptr(corners), _ptr(dims), _ptr(scores), _ptr(boxes2d),
                               _ptr(init_id), _ptr(cam_poses), _ptr(cur_pose), _ptr(K), n_all,
                               n_glo, _ptr(mask), mask.shape[0], _ptr(succ), success.numel(),
                               _ptr(fl_items), _ptr(fl_len), _ptr(valid_num), _ptr(keep),
                               _ptr(counts[0:1]), _ptr(events), _ptr(counts[1:2]),
                               _ptr(counts[2:3]), ctypes.byref(cfg), _stream()), "bf_corr_assoc")
    return keep, events, counts


def corr_assoc_chained(corners, dims, scores, boxes2d, init_id, cam_poses, cur_pose, K, n_glo,
                       mask, n_mask, success, n_success, fl_items, fl_len, valid_num,
                       cfg: CorrCfg, out):
    """bf_corr_assoc_chained: correspondence association on nms_scan's device outputs (mask /
    n_mask = its keep / counts[0:1], success / n_success = its succ / counts[1:2]); `out` =
    (keep [n_all], events [n_all + 1, 3], counts [3]) preallocated device views"""
    keep, events, counts = out
    _check(lib().bf_corr_assoc_chained(
        _ptr(corners), _ptr(dims), _ptr(scores), _ptr(boxes2d), _ptr(init_id), _ptr(cam_poses),
        _ptr(cur_pose), _ptr(K), scores.shape[0], n_glo, _ptr(mask), _ptr(n_mask), _ptr(success),
        _ptr(n_success), _ptr(fl_items), _ptr(fl_len), _ptr(valid_num), _ptr(keep),
        _ptr(counts[0:1]), _ptr(events), _ptr(counts[1:2]), _ptr(counts[2:3]), ctypes.byref(cfg),
        _stream()), "bf_corr_assoc_chained")
    return keep, events, counts


# ------------------------------------------------------------------------------------------
# fusion
# ------------------------------------------------------------------------------------------
def fusion_fit(view_off, n_views, view_box, view_R, view_score, view_pose, view_tc, pst,
               cfg: FuseCfg, trace=False, max_views=None, packed_out=False, packed=None):
    """max_views: host-known bound on n_views (avoids a device read when given).
    packed_out: return (out_box, packed, trace) with packed = int32 [updated(n_jobs),
    iterations(n_jobs), status] (one device->host copy for the caller); `packed` may be given
    (zeroed; its status word may already hold flags of an earlier launch: they are kept)."""
    dev = view_box.device
    n_jobs = view_off.shape[0]
    out_box = torch.empty((n_jobs, 6), dtype=torch.float32, device=dev)
    # updated flags, iteration counts and the status word in one buffer: one read-back
    if packed is None:
        packed = torch.zeros(2 * n_jobs + 1, dtype=torch.int32, device=dev)
    out_upd, out_it, status = packed[:n_jobs], packed[n_jobs:2 * n_jobs], packed[2 * n_jobs:]
    tr = (torch.empty((n_jobs, cfg.iters, cfg.pst_size), dtype=torch.float32, device=dev)
          if trace else None)
    if max_views is None:
        max_views = int(n_views.max().item()) if n_views.numel() else 1
    max_views = max(1, min(int(max_views), 32))
    L = lib()
    nbytes = L.bf_fusion_fit_workspace_size(n_jobs, max_views, cfg.pst_size)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    launch = lambda: _check(L.bf_fusion_fit(_ptr(view_off), _ptr(n_views), n_jobs, max_views,
                                            _ptr(view_box), _ptr(view_R), _ptr(view_score), _ptr(view_pose),
                                            _ptr(view_tc), _ptr(pst), ctypes.byref(cfg), _ptr(out_box),
                                            _ptr(out_upd), _ptr(out_it), _ptr(tr), _ptr(status), _ptr(ws),
                                            _stream()), "bf_fusion_fit")
    # KernelTimer, by hand (not _timed): the work is known only from what this launch writes
    t = _timer()
    if t is None:
        launch()
    else:
        P = int(cfg.pst_size)
        # work = particle-view fitness evaluations: sum over jobs of views * particles * iterations
        # (the iteration counts are read when the summary is taken)
        t.record(dict(kind="fusion_fit", jobs=n_jobs),
                 lambda: float((out_it.long() * n_views.long()).sum().item() * P), 0.0, launch)
    if packed_out:
        return out_box, packed, tr
    return out_box, out_upd, out_it, status, tr


def fusion_writeback(out_box, updated, rows, target):
    """target[rows[j], :6] = out_box[j] where updated[j] (bf_fusion_writeback); rows int32"""
    _need(target, torch.float32, "target")
    if not target.is_contiguous():
        raise HipError("fusion_writeback: target must be contiguous")
    _check(lib().bf_fusion_writeback(_ptr(out_box), _ptr(updated), _ptr(rows), rows.shape[0],
                                     _ptr(target), target.shape[1], _stream()),
           "bf_fusion_writeback")


def fusion_fitness(box, R, view_pose, view_tc, pst, search_size, cfg: FuseCfg):
    nv = view_pose.shape[0]
    out = torch.empty(pst.shape[0], dtype=torch.float32, device=box.device)
    _check(lib().bf_fusion_fitness(_ptr(box), _ptr(R), nv, _ptr(view_pose), _ptr(view_tc),
                                   _ptr(pst), pst.shape[0], _ptr(search_size), ctypes.byref(cfg),
                                   _ptr(out), _stream()), "bf_fusion_fitness")
    return out


# ------------------------------------------------------------------------------------------
# keyframe sequencer (bf_fseq_*)
# ------------------------------------------------------------------------------------------
class FusionSequencer:
    """Owner of one bf_fseq: the demo.py:200-305 keyframe sequence over batches of keyframes,
    all_pred_box on the device and BoxManager's lists in the library (include/boxfusion_hip.h).
    Calls launch on the calling thread's current stream."""

    def __init__(self):
        self._L = lib()
        self.h = c_void_p()
        _check(self._L.bf_fseq_create(ctypes.byref(self.h)), "bf_fseq_create")
        self._state = np.zeros(FSEQ_STATE_N, np.int64)
        _LIVE_SEQUENCERS.add(self)

    def close(self):
        """release the sequencer's device buffers and handle now (idempotent)"""
        h, L = getattr(self, "h", None), getattr(self, "_L", None)
        if h is not None and h.value and L is not None:
            L.bf_fseq_destroy(h)
        self.h = None

    def _rc(self, rc, name):
        if rc != 0:
            raise HipError(f"{name}: {self._L.bf_fseq_error(self.h).decode()} (bf_status {rc})")
        if _SYNC_DEBUG:
            torch.cuda.synchronize()

    def keyframes(self, cfg: FseqCfg, sizes, p_base, fields, K, pst):
        """sizes: int32 [n_kf]; fields: (box, R, score, box2d, pose, proj) of the per-frame table,
        contiguous f32 device tensors with p_rows rows"""
        sizes = np.ascontiguousarray(sizes, np.int32)
        p_rows = int(fields[0].shape[0])
        self._rc(self._L.bf_fseq_keyframes(
            self.h, ctypes.byref(cfg), len(sizes), sizes.ctypes.data_as(c_void_p), int(p_base),
            p_rows, *[_ptr(t) for t in fields], _ptr(K), _ptr(pst), _stream()), "bf_fseq_keyframes")

    def sync(self):
        self._rc(self._L.bf_fseq_sync(self.h), "bf_fseq_sync")

    def state(self):
        """bf_fseq_state (waits for the stream and applies a pending fusion result)"""
        self._rc(self._L.bf_fseq_state(self.h, self._state.ctypes.data_as(c_void_p)), "bf_fseq_state")
        return self._state.copy()

    def lists(self, which, rows, items):
        lens = np.zeros(max(rows, 1), np.int32)
        flat = np.zeros(max(items, 1), np.int32)
        self._rc(self._L.bf_fseq_lists(self.h, which, lens.ctypes.data_as(c_void_p),
                                       flat.ctypes.data_as(c_void_p)), "bf_fseq_lists")
        off = np.concatenate([[0], np.cumsum(lens[:rows])])
        fl = flat.tolist()
        return [fl[off[i]:off[i + 1]] for i in range(rows)]

    def flags(self, n):
        out = np.zeros(max(n, 1), np.int32)
        self._rc(self._L.bf_fseq_flags(self.h, out.ctypes.data_as(c_void_p)), "bf_fseq_flags")
        return out[:n].tolist()

    def global_rows(self, n, device):
        """all_pred_box's init_id (host int32), xyzlhw [n,6] and valid_num [n] (device copies)"""
        ids = np.zeros(max(n, 1), np.int32)
        xyz = torch.empty((n, 6), dtype=torch.float32, device=device)
        vn = torch.empty(n, dtype=torch.float32, device=device)
        self._rc(self._L.bf_fseq_global(self.h, ids.ctypes.data_as(c_void_p), _ptr(xyz) if n else None,
                                        _ptr(vn) if n else None, _stream()), "bf_fseq_global")
        return ids[:n], xyz, vn

    def __del__(self, _finalizing=sys.is_finalizing):
        if _finalizing():             # interpreter exit: _shutdown() already released it
            return
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter teardown: the process frees everything
            pass


def filter_cfg(det_cfg, W, H):
    """FilterCfg from a config's `detection` section (demo.py:138-148 keys)"""
    c = FilterCfg()
    c.use_score = 1
    c.score_thresh = float(np.float32(det_cfg.get("score_thresh", 0.0)))
    c.use_uv = int(bool(det_cfg.get("uv_bound", False)))
    ratio = float(det_cfg.get("uv_bound_value", 1.0))
    c.gap_w, c.gap_h = int((1 - ratio) * W), int((1 - ratio) * H)     # python float, as the reference
    c.W, c.H = int(W), int(H)
    c.use_floor = int(bool(det_cfg.get("floor_mask", False)))
    fr = float(det_cfg.get("floor_ratio", 20))
    c.floor_ratio, c.floor_half = float(np.float32(fr)), float(np.float32(fr / 2))
    lg = det_cfg.get("size_max_thres")
    c.use_large = int(bool(lg))
    c.size_max = float(np.float32(lg)) if lg else 0.0
    return c


def detection_filter(scores, proj_xy, box3d, cfg: FilterCfg, with_bits=False):
    """keep mask (bool, shape of scores) of the demo.py:138-148 filters (bf_detection_filter)"""
    n = scores.numel()
    keep = torch.empty(scores.shape, dtype=torch.uint8, device=scores.device)
    bits = torch.empty(scores.shape, dtype=torch.uint8, device=scores.device) if with_bits else None
    _check(lib().bf_detection_filter(_ptr(_need(scores.contiguous(), torch.float32, "scores")),
                                     _ptr(_need(proj_xy.contiguous(), torch.float32, "proj_xy")),
                                     _ptr(_need(box3d.contiguous(), torch.float32, "box3d")), n,
                                     ctypes.byref(cfg), _ptr(keep), _ptr(bits), _stream()),
           "bf_detection_filter")
    return (keep.bool(), bits) if with_bits else keep.bool()


# ------------------------------------------------------------------------------------------
# per-frame depth
# ------------------------------------------------------------------------------------------
_DS_WS = {}


def depth_workspace(b, h, w, device):
    """zero-filled workspace of bf_depth_standardize / bf_depth_preprocess, one per (device,
    stream, shape): the kernels leave it zeroed, so it is reused as is by stream-ordered calls.
    Not for graph captures: a captured launch keeps the address, so replays on another stream
    would race the eager users of the cached buffer -- depth_preprocess therefore requires an
    explicit caller-owned `ws` (new_depth_workspace) while the current stream is capturing."""
    dev = torch.device(device)
    stream = torch.cuda.current_stream(dev).cuda_stream
    key = (dev.index, stream, b, h, w)
    ws = _DS_WS.get(key)
    if ws is None:
        size = int(lib().bf_depth_standardize_workspace_size(b, h, w))
        ws = torch.zeros(max(size, 1), dtype=torch.uint8, device=dev)
        _DS_WS[key] = ws
    return ws


def depth_standardize(depth, out=None, params=None, ws=None):
    """depth f32[b,h,w] -> (standardised f32[b,h,w], params f32[b,2])"""
    return depth_preprocess(depth, out=out, params=params, ws=ws)


def depth_preprocess(depth, K=None, RT=None, max_depth=10.0, out=None, params=None, xyz=None, valid=None,
                     ws=None):
    """demo.py:121-131 per-frame depth work for a batch: depth f32[b,h,w] -> (standardised,
    params f32[b,2]) and, with K f32[b,3,3] / RT f32[b,4,4], the back-projection (xyz f32[b,h,w,3],
    valid bool[b,h,w]) from the same pass.  ws: a zero-filled workspace of
    bf_depth_standardize_workspace_size bytes owned by the caller (default: one per stream)"""
    depth = _need(depth.contiguous(), torch.float32, "depth")
    if not depth.is_cuda:
        raise HipError("bf_depth_preprocess: depth must be a device tensor (no CPU path)")
    b, h, w = depth.shape
    out = torch.empty_like(depth) if out is None else out
    params = torch.empty((b, 2), dtype=torch.float32, device=depth.device) if params is None else params
    bp = K is not None
    if bp:
        K = _need(K.contiguous(), torch.float32, "K")
        RT = _need(RT.contiguous(), torch.float32, "RT")
        if K.shape != (b, 3, 3) or RT.shape != (b, 4, 4):
            raise HipError(f"bf_depth_preprocess: K {tuple(K.shape)} / RT {tuple(RT.shape)} for {b} frames")
        xyz = torch.empty((b, h, w, 3), dtype=torch.float32, device=depth.device) if xyz is None else xyz
        valid = torch.empty((b, h, w), dtype=torch.uint8, device=depth.device) if valid is None else valid
    if ws is None:
        if torch.cuda.is_current_stream_capturing():
            raise HipError("bf_depth_preprocess under graph capture needs a caller-owned ws "
                           "(new_depth_workspace): the per-stream cached workspace is shared")
        ws = depth_workspace(b, h, w, depth.device)
    launch = lambda: _check(lib().bf_depth_preprocess(
        _ptr(depth), b, h, w, _ptr(out), _ptr(params), _ptr(K) if bp else None, _ptr(RT) if bp else None,
        max_depth if max_depth is not None else 0.0, _ptr(xyz) if bp else None, _ptr(valid) if bp else None,
        _ptr(ws), _stream()), "bf_depth_preprocess")
    # KernelTimer, by hand (not _timed): the outputs and the workspace above are allocated before
    # the start event, so the events bracket the launches only
    t = _timer()
    if t is None:
        launch()
    else:
        n = float(b * h * w)
        # algorithmic bytes: read the depth once, write the standardised map (+ xyz and
        # the valid mask when back-projecting)
        t.record(dict(kind="depth", backproject=bp, b=b, h=h, w=w), 0.0, 8.0 * n + (13.0 * n if bp else 0.0),
                 launch)
    if bp:
        return out, params, xyz, valid.view(torch.bool)
    return out, params


def backproject(depth, K, RT, max_depth=10.0):
    h, w = depth.shape
    xyz = torch.empty((h, w, 3), dtype=torch.float32, device=depth.device)
    valid = torch.empty((h, w), dtype=torch.uint8, device=depth.device)
    _check(lib().bf_backproject(_ptr(depth.contiguous()), _ptr(K.contiguous()),
                                _ptr(RT.contiguous()), h, w,
                                max_depth if max_depth is not None else 0.0, _ptr(xyz), _ptr(valid),
                                _stream()), "bf_backproject")
    return xyz, valid.bool()


# ------------------------------------------------------------------------------------------
# MFMA tower kernels
# ------------------------------------------------------------------------------------------
ACT = {None: 0, "none": 0, "gelu": 1, "relu": 2}


# The CU budget a thread's GEMMs pass in their plan (0 = every CU).  Host-side, per thread: the C
# library keeps no GEMM state; the thread that launches on a CU-masked detect stream sets it
# (partition_streams), a fusion worker thread keeps 0.
_TLS = threading.local()


def set_cu_budget(n):
    """CUs the calling thread's GEMMs size their persistent grid for (0 = all)"""
    _TLS.cu_budget = max(int(n), 0)


def cu_budget():
    return getattr(_TLS, "cu_budget", 0)


def set_knobs(**kw):
    """measurement hooks for scripts/ (not used by the product path): per-thread defaults merged into
    the bf_gemm_plan of every GEMM call made without a plan (GemmPlan field names) and into every
    attention call made without a variant (attn_variant=...).  set_knobs() with no arguments clears
    them."""
    _TLS.knobs = {**getattr(_TLS, "knobs", {}), **kw} if kw else {}


def _knobs():
    return getattr(_TLS, "knobs", {})


def _plan(plan):
    if plan is None:
        k = {f: v for f, v in _knobs().items() if f != "attn_variant"}
        b = cu_budget()
        if not b and not k:
            return None
        plan = GemmPlan(**{"cu_budget": b, **k})
    elif isinstance(plan, dict):
        plan = GemmPlan(**{"cu_budget": cu_budget(), **plan})
    return ctypes.byref(plan)


def gemm_tile_rows(M, N, K, plan=None):
    """tile height the persistent bf16 GEMM takes for this shape under `plan` (as gemm()'s plan
    argument); host-only, needs no GPU"""
    r = lib().bf_gemm_tile_rows_plan(M, N, K, _plan(plan))
    if r <= 0:
        raise HipError(f"bf_gemm_tile_rows_plan failed with bf_status {r}")
    return r


def gemm_grid(M, N, K, plan=None):
    """workgroups of the persistent grid at that height (CU-time = this x the GEMM's duration)"""
    r = lib().bf_gemm_grid_plan(M, N, K, _plan(plan))
    if r <= 0:
        raise HipError(f"bf_gemm_grid_plan failed with bf_status {r}")
    return r


def _gemm_work(a, w, bias=None, act=None, resid=None, resid_mod=0, out=None, out_dtype=torch.bfloat16,
               row_map=None, m=None, plan=None):
    M = a.shape[0] if m is None else m
    N, K = w.shape
    ob = (out.dtype if out is not None else out_dtype) == torch.bfloat16
    tags = dict(kind="gemm", act=ACT[act], out_bf16=ob, resid=resid is not None, M=M, N=N, K=K,
                large=bool(lib().bf_gemm_large_tiles(M, N, K)))
    nbytes = 2.0 * (M * K + N * K) + M * N * (2 if ob else 4)
    if resid is not None:
        nbytes += 4.0 * (M * N if not resid_mod else resid_mod * N)
    return tags, 2.0 * M * N * K, nbytes


@_timed(_gemm_work)
def gemm(a, w, bias=None, act=None, resid=None, resid_mod=0, out=None, out_dtype=torch.bfloat16,
         row_map=None, m=None, plan=None):
    """out[orow(r)] = resid[...] + act(a @ w.T + bias); a bf16 [M,K] (row stride a.stride(0)),
    w bf16 [N,K]. `out` may be given (its row stride is used).  plan: None (defaults + the
    thread's CU budget), a GemmPlan or a dict of its fields (measurement hooks)."""
    _need(a, torch.bfloat16, "a")
    _need(w, torch.bfloat16, "w")
    M = a.shape[0] if m is None else m
    N, K = w.shape
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype, device=a.device)
    c_bf16 = 1 if out.dtype == torch.bfloat16 else 0
    if not c_bf16 and out.dtype != torch.float32:
        raise HipError("gemm output must be bf16 or f32")
    if resid is not None:
        _need(resid, torch.float32, "resid")
    if bias is not None:
        _need(bias, torch.float32, "bias")
    if a.stride(1) != 1 or w.stride(1) != 1 or out.stride(1) != 1:
        raise HipError("gemm operands need unit column stride")
    _check(lib().bf_gemm_bf16_plan(a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0),
                                   _ptr(bias) if bias is not None else None,
                                   resid.data_ptr() if resid is not None else None,
                                   resid.stride(0) if resid is not None else 0, resid_mod,
                                   out.data_ptr(), out.stride(0), c_bf16,
                                   _ptr(row_map) if row_map is not None else None, M, N, K, ACT[act],
                                   _plan(plan), _stream()), "bf_gemm_bf16")
    return out


def _attention_work(q, k, v, o, batch, heads, sq, sk, head_dim, scale, q_bs=None, k_bs=None, v_bs=None,
                    o_bs=None, o_map=None, variant=0):
    bh = float(batch * heads)
    return (dict(kind="attn", D=head_dim, sq=sq, sk=sk, batch=batch, heads=heads),
            4.0 * bh * sq * sk * head_dim, 2.0 * bh * head_dim * (2 * sq + 2 * sk))


@_timed(_attention_work)
def attention(q, k, v, o, batch, heads, sq, sk, head_dim, scale, q_bs=None, k_bs=None, v_bs=None,
              o_bs=None, o_map=None, variant=0):
    """q/k/v/o are 2-D token-major views [batch*S, >= heads*head_dim] (any row stride).
    o_map: int32 [batch*sq] output row of each query (< 0: not stored).  variant: the per-call
    kernel-variant hook of bf_attention_bf16_ex (0 = default)."""
    for x, n in ((q, "q"), (k, "k"), (v, "v"), (o, "o")):
        _need(x, torch.bfloat16, n)
    q_bs = sq * q.stride(0) if q_bs is None else q_bs
    k_bs = sk * k.stride(0) if k_bs is None else k_bs
    v_bs = sk * v.stride(0) if v_bs is None else v_bs
    o_bs = sq * o.stride(0) if o_bs is None else o_bs
    if o_map is not None:
        _need(o_map, torch.int32, "o_map")
        if o_map.numel() < batch * sq:
            raise HipError(f"o_map has {o_map.numel()} rows < batch*sq = {batch * sq}")
    _check(lib().bf_attention_bf16_ex(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), batch,
                                      heads, sq, sk, head_dim, q.stride(0), k.stride(0),
                                      v.stride(0), o.stride(0), q_bs, k_bs, v_bs, o_bs, scale,
                                      _ptr(o_map) if o_map is not None else None,
                                      variant or _knobs().get("attn_variant", 0), _stream()),
           "bf_attention_bf16_ex")
    return o


def _attention_fp8out_work(q, k, v, o, batch, heads, sq, sk, head_dim, scale, out_qscale, q_bs=None,
                           k_bs=None, v_bs=None, o_bs=None, variant=0):
    bh = float(batch * heads)
    return (dict(kind="attn", D=head_dim, sq=sq, sk=sk, batch=batch, heads=heads, fp8out=True),
            4.0 * bh * sq * sk * head_dim, bh * head_dim * (2 * sq + 4 * sk + sq))


@_timed(_attention_fp8out_work)
def attention_fp8out(q, k, v, o, batch, heads, sq, sk, head_dim, scale, out_qscale, q_bs=None,
                     k_bs=None, v_bs=None, o_bs=None, variant=0):
    """attention() with an fp8 e4m3 output o = saturate(softmax(q k^T) v * out_qscale)"""
    for x, n in ((q, "q"), (k, "k"), (v, "v")):
        _need(x, torch.bfloat16, n)
    _need(o, FP8, "o")
    q_bs = sq * q.stride(0) if q_bs is None else q_bs
    k_bs = sk * k.stride(0) if k_bs is None else k_bs
    v_bs = sk * v.stride(0) if v_bs is None else v_bs
    o_bs = sq * o.stride(0) if o_bs is None else o_bs
    _check(lib().bf_attention_fp8out_ex(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), batch, heads,
                                        sq, sk, head_dim, q.stride(0), k.stride(0), v.stride(0), o.stride(0),
                                        q_bs, k_bs, v_bs, o_bs, scale, out_qscale,
                                        variant or _knobs().get("attn_variant", 0), _stream()),
           "bf_attention_fp8out_ex")
    return o


def layernorm(x, weight, bias, eps, out=None, row_map=None, out_dtype=torch.bfloat16):
    """x f32 [M, C] (any row stride) -> LayerNorm rows in bf16 (or f32: out / out_dtype), row r
    written to row_map[r] of out (< 0 skipped)"""
    _need(x, torch.float32, "x")
    M, C = x.shape
    if out is None:
        out = torch.empty((M, C), dtype=out_dtype, device=x.device)
    if out.dtype not in (torch.bfloat16, torch.float32) or x.stride(1) != 1 or out.stride(1) != 1:
        raise HipError("layernorm: f32 in, bf16 / f32 out, unit column stride")
    _check(lib().bf_layernorm_out(x.data_ptr(), x.stride(0), _ptr(weight), _ptr(bias), eps,
                                  out.data_ptr(), out.stride(0), int(out.dtype == torch.float32),
                                  _ptr(row_map) if row_map is not None else None, M, C, _stream()),
           "bf_layernorm_out")
    return out



def attention_causal(q, k, v, o, batch, heads, s, head_dim, scale):
    """causal self-attention (CLIP text tower): q/k/v/o token-major 2-D views [batch*s, >= heads*D]"""
    for x, n in ((q, "q"), (k, "k"), (v, "v"), (o, "o")):
        _need(x, torch.bfloat16, n)
    _check(lib().bf_attention_causal(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), batch, heads,
                                     s, head_dim, q.stride(0), k.stride(0), v.stride(0), o.stride(0),
                                     s * q.stride(0), s * k.stride(0), s * v.stride(0), s * o.stride(0),
                                     scale, _stream()), "bf_attention_causal")
    return o


def token_embed(ids, table, pos, out=None, status=None):
    """ids i32 [N, S] -> table[ids] + pos, f32 [N*S, W]; an out-of-range id raises HipError"""
    _need(ids, torch.int32, "ids")
    _need(table, torch.float32, "table")
    _need(pos, torch.float32, "pos")
    N, S = ids.shape
    W = table.shape[1]
    if pos.shape[0] < S or pos.shape[1] != W:
        raise HipError(f"token_embed: positional table {tuple(pos.shape)} for S={S}, W={W}")
    if out is None:
        out = torch.empty((N * S, W), dtype=torch.float32, device=ids.device)
    _need(out, torch.float32, "out")
    own = status is None
    if own:
        status = torch.zeros(1, dtype=torch.int32, device=ids.device)
    _check(lib().bf_token_embed(_ptr(ids), N * S, _ptr(table), table.shape[0], _ptr(pos), S, W, _ptr(out),
                                _ptr(status), _stream()), "bf_token_embed")
    if own and int(status.item()) & BF_DEV_INDEX_RANGE:
        raise HipError("bf_token_embed: a token id outside the vocabulary (BF_DEV_INDEX_RANGE)")
    return out


def text_pool(ids, x, out=None):
    """x f32 [N*S, W] -> x[n*S + argmax(ids[n])] f32 [N, W] (open_clip 'argmax' text pooling)"""
    _need(ids, torch.int32, "ids")
    _need(x, torch.float32, "x")
    N, S = ids.shape
    W = x.shape[1]
    if out is None:
        out = torch.empty((N, W), dtype=torch.float32, device=x.device)
    _need(out, torch.float32, "out")
    _check(lib().bf_text_pool(_ptr(ids), N, S, _ptr(x), W, _ptr(out), _stream()), "bf_text_pool")
    return out


def l2_normalize_rows(x, out=None):
    """x f32 [R, W] -> x / ||x||_2 per row (out may be x)"""
    _need(x, torch.float32, "x")
    if out is None:
        out = torch.empty_like(x)
    _need(out, torch.float32, "out")
    _check(lib().bf_l2_normalize_rows(_ptr(x), x.shape[0], x.shape[1], _ptr(out), _stream()),
           "bf_l2_normalize_rows")
    return out


def ingest_rgbd(bgr, depth_u16, depth_scale, rot_k=0, rgb_out=None, depth_out=None, src_bgr=True):
    """decoded frames -> sample tensors (capture_stream.py:194-311): bgr u8 [F,Hc,Wc,3], depth
    int16/uint16 [F,Hd,Wd] (or None) -> rgb u8 [F,3,Ho,Wo] (RGB, cv2-resized to the depth size,
    rot90 k) and depth f32 [F,Ho,Wo] = depth / depth_scale (rot90 k)"""
    _need(bgr, torch.uint8, "bgr")
    if bgr.dim() == 3:
        bgr = bgr[None]
    F_, Hc, Wc, C = bgr.shape
    if C != 3:
        raise HipError("ingest_rgbd: BGR frames [F,H,W,3]")
    if depth_u16 is not None:
        if depth_u16.dtype not in (torch.uint16, torch.int16):
            raise HipError(f"depth: expected a 16-bit PNG map, got {depth_u16.dtype}")
        if depth_u16.dim() == 2:
            depth_u16 = depth_u16[None]
        if depth_u16.shape[0] != F_:
            raise HipError("ingest_rgbd: one depth map per frame")
        Hd, Wd = depth_u16.shape[1:]
    else:
        Hd, Wd = Hc, Wc
    k = rot_k % 4
    Ho, Wo = (Wd, Hd) if k % 2 else (Hd, Wd)
    if rgb_out is None:
        rgb_out = torch.empty((F_, 3, Ho, Wo), dtype=torch.uint8, device=bgr.device)
    _need(rgb_out, torch.uint8, "rgb_out")
    if depth_u16 is not None and depth_out is None:
        depth_out = torch.empty((F_, Ho, Wo), dtype=torch.float32, device=bgr.device)
    _check(lib().bf_ingest_rgbd(_ptr(bgr), Hc, Wc, _ptr(depth_u16), Hd, Wd, F_, depth_scale, k, int(bool(src_bgr)),
                                _ptr(rgb_out), _ptr(depth_out) if depth_u16 is not None else None, _stream()),
           "bf_ingest_rgbd")
    return rgb_out, depth_out


PNG_STATUS = _bits("BF_PNG_", BAD_SIGNATURE="bad signature", BAD_HEADER="bad IHDR", UNSUPPORTED="unsupported PNG kind",
                   BAD_CHUNK="bad chunk list", BAD_ZLIB="bad zlib / deflate stream", BAD_ADLER="Adler-32 mismatch",
                   BAD_FILTER="bad row filter", SIZE="size mismatch")


def _decode_batch(name, entry, workspace_bytes, status_bits, noun, data, offsets, H, W, tail, dtype, out,
                  offsets_host, check, work, extra=(), sized=True):
    """the one front end of the batched decoders (png_decode_u16 / zlib_decode_u16 / png_decode_rgb /
    jpeg_decode_rgb, whose docstrings give the arguments): `data` u8 [total] holds F `noun`s back to
    back at `offsets` -> (out `dtype` [F,H,W,*tail], int32 status [F]); a status word's set bits read
    as `status_bits`.  Every host check runs before anything touches the device.  sized: `entry` and
    `workspace_bytes` take the total and the largest member's byte counts, which need the host
    offsets (read back when not given); otherwise host offsets are only validated when given.
    extra: C arguments that go between the sizes and `out`."""
    _need(data, torch.uint8, f"{name}: {noun}s")
    _need(offsets, torch.int64, f"{name}: offsets")
    F_ = offsets.numel() - 1
    if offsets_host is None and sized:
        offsets_host = offsets.cpu()
    oh = None if offsets_host is None else [int(v) for v in offsets_host]
    if F_ < 0 or (oh is not None and len(oh) != F_ + 1):
        raise HipError(f"{name}: offsets [F+1]")
    if oh is not None:
        member = [oh[i + 1] - oh[i] for i in range(F_)]
        if oh[0] < 0 or min(member, default=0) < 0:
            raise HipError(f"{name}: offsets must not decrease")
        if oh[-1] > data.numel():
            raise HipError(f"{name}: offsets run past the {noun} bytes")
    if out is None:
        out = torch.empty((F_, H, W, *tail), dtype=dtype, device=data.device)
    _need(out, dtype, f"{name}: out")
    if out.numel() != F_ * H * W * int(np.prod(tail)):
        raise HipError(f"{name}: out [{','.join(['F', 'H', 'W', *map(str, tail)])}]")
    status = torch.zeros(F_, dtype=torch.int32, device=data.device)
    if F_ == 0:
        return out, status
    sizes = (oh[-1], max(member)) if sized else ()
    wb = workspace_bytes(F_, H, W, *sizes[:1])
    if work is None or work.numel() < wb:
        work = torch.empty(max(wb, 1), dtype=torch.uint8, device=data.device)
    _check(entry(_ptr(data), _ptr(offsets), F_, H, W, *sizes, *extra, _ptr(out), _ptr(work), wb, _ptr(status),
                 _stream()), entry.__name__)
    if check:
        st = status.cpu()
        bad = torch.nonzero(st).flatten().tolist()
        if bad:
            f = bad[0]
            why = ", ".join(v for k, v in status_bits.items() if int(st[f]) & k)
            raise HipError(f"{name}: {len(bad)} of {F_} {noun}s did not decode ({noun} {f}: {why})")
    return out, status


def png_decode_u16(files, offsets, H, W, out=None, offsets_host=None, check=True, depth_scale=None, work=None):
    """cv2.imread(path, IMREAD_UNCHANGED) for F 16-bit greyscale PNGs (capture_stream.py:197/:405):
    files u8 [total] device bytes of the files back to back, offsets int64 [F+1] device (and the
    same offsets on the host, `offsets_host`, to size the launch) -> out u16 [F,H,W] and the int32
    status word per file.  depth_scale given: out f32 [F,H,W] = sample / depth_scale
    (capture_stream.py:203, bf_png_decode_depth).  check=True synchronises and raises on any file
    that did not decode."""
    L = lib()
    entry, dt, extra = ((L.bf_png_decode_u16, torch.uint16, ()) if depth_scale is None else
                        (L.bf_png_decode_depth, torch.float32, (depth_scale,)))
    return _decode_batch("png_decode_u16", entry, png_workspace_bytes, PNG_STATUS, "file", files, offsets, H, W, (),
                         dt, out, offsets_host, check, work, extra)


def png_workspace_bytes(F, H, W, total_file_bytes):
    return int(lib().bf_png_workspace_bytes(F, H, W, total_file_bytes))


ZLIB_STATUS = _bits("BF_PNG_", BAD_CHUNK="shorter than a zlib header + Adler-32", BAD_ZLIB="bad zlib / deflate stream",
                    BAD_ADLER="Adler-32 mismatch", SIZE="inflated length is not 2 H W")


def zlib_decode_u16(streams, offsets, H, W, out=None, offsets_host=None, check=True, depth_scale=None, work=None):
    """np.frombuffer(zlib.decompress(s), '<u2').reshape(H, W) for F bare zlib streams (the depth
    frames of a ScanNet .sens container): streams u8 [total] device bytes of the streams back to
    back at any byte offsets, offsets int64 [F+1] device (and the same offsets on the host,
    `offsets_host`, to size the launch) -> out u16 [F,H,W] and the int32 status word per stream
    (BF_PNG_* bits, ZLIB_STATUS).  depth_scale given: out f32 [F,H,W] = sample / depth_scale
    (bf_zlib_decode_depth).  check=True synchronises and raises on any stream that did not decode."""
    L = lib()
    entry, dt, extra = ((L.bf_zlib_decode_u16, torch.uint16, ()) if depth_scale is None else
                        (L.bf_zlib_decode_depth, torch.float32, (depth_scale,)))
    return _decode_batch("zlib_decode_u16", entry, zlib_workspace_bytes, ZLIB_STATUS, "stream", streams, offsets, H, W,
                         (), dt, out, offsets_host, check, work, extra)


def zlib_workspace_bytes(F, H, W, total_stream_bytes):
    return int(lib().bf_zlib_workspace_bytes(F, H, W, total_stream_bytes))


def png_decode_rgb(files, offsets, H, W, out=None, offsets_host=None, check=True, work=None):
    """cv2.imread(color_path) + cvtColor(BGR2RGB) for F 8-bit PNGs (CA-1M's rgb/*.png,
    capture_stream.py:402): grey, RGB, grey + alpha or RGBA, non-interlaced (transparency is dropped,
    not composited, as cv2's default flag does); files / offsets / offsets_host as png_decode_u16
    -> out u8 [F,H,W,3] in RGB order and the int32 status word per file (BF_PNG_* bits).  A batch may
    mix the four kinds.  check=True synchronises and raises on any file that did not decode."""
    return _decode_batch("png_decode_rgb", lib().bf_png_decode_rgb, png_rgb_workspace_bytes, PNG_STATUS, "file", files,
                         offsets, H, W, (3,), torch.uint8, out, offsets_host, check, work)


def png_rgb_workspace_bytes(F, H, W, total_file_bytes):
    return int(lib().bf_png_rgb_workspace_bytes(F, H, W, total_file_bytes))


JPEG_STATUS = _bits("BF_JPG_", BAD_MARKER="bad / missing marker segment",
                    UNSUPPORTED="unsupported JPEG kind (not baseline 1/3-component h2v2/h2v1/h1v1)", SIZE="size mismatch",
                    BAD_DATA="corrupt entropy-coded data")


def jpeg_decode_rgb(files, offsets, H, W, out=None, check=True, work=None, offsets_host=None):
    """cv2.imread(color_path) for F baseline JPEGs (capture_stream.py:194/:402), in RGB order (the
    cvtColor(BGR2RGB) of the streams folded in): files u8 [total] device bytes back to back, offsets
    int64 [F+1] device -> out u8 [F,H,W,3] and the int32 status word per file (BF_JPG_* bits).
    check=True synchronises and raises on any file that did not decode.  offsets_host: the same
    offsets on the host, checked against `files` when given (the launch needs no host sizes, so
    without them nothing is read back and the device offsets are trusted)."""
    return _decode_batch("jpeg_decode_rgb", lib().bf_jpeg_decode_rgb, jpeg_workspace_bytes, JPEG_STATUS, "file", files,
                         offsets, H, W, (3,), torch.uint8, out, offsets_host, check, work, sized=False)


def jpeg_workspace_bytes(F, H, W):
    return int(lib().bf_jpeg_workspace_bytes(F, H, W))


def cv2_resize_u8(src, Wd, Hd, out=None):
    """cv2.resize(src, (Wd, Hd)) (u8 INTER_LINEAR) of u8 images [H,W], [H,W,cn] or [F,H,W,cn]"""
    _need(src, torch.uint8, "src")
    x = src
    if x.dim() == 2:
        x = x[None, :, :, None]
    elif x.dim() == 3:
        x = x[None]
    F_, Hs, Ws, cn = x.shape
    if out is None:
        out = torch.empty((F_, Hd, Wd, cn), dtype=torch.uint8, device=src.device)
    _check(lib().bf_cv2_resize_u8(_ptr(x), Hs, Ws, cn, Hd, Wd, F_, _ptr(out), _stream()),
           "bf_cv2_resize_u8")
    if src.dim() == 2:
        return out[0, :, :, 0]
    return out[0] if src.dim() == 3 else out


# ------------------------------------------------------------------------------------------
# coloured scene point cloud (bf_cloud.hip)
# ------------------------------------------------------------------------------------------
def _pil_bicubic(x):
    # Pillow's bicubic_filter (a = -0.5), the same f64 expressions
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


@functools.lru_cache(maxsize=64)
def pil_bicubic_coeffs(n_in, n_out):
    """Pillow's 8-bit resample tables of one axis for Image.resize's default BICUBIC, n_in -> n_out
    pixels (precompute_coeffs + normalize_coeffs_8bpc, all in f64 on the host): (bounds int32
    [n_out,2] = first source pixel and tap count, coeffs int32 [n_out,ksize] = the normalised weights
    as int(w * 2^22 -+ 0.5), zero past the tap count).  The arrays are cached: do not write to them."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in <= 0 or n_out <= 0:
        raise HipError("pil_bicubic_coeffs: sizes must be positive")
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(np.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), np.int32)
    coeffs = np.zeros((n_out, ksize), np.int32)
    ss = 1.0 / fs
    for i in range(n_out):
        c = (i + 0.5) * scale
        xmin = max(int(c - support + 0.5), 0)
        xmax = min(int(c + support + 0.5), n_in) - xmin
        w = [_pil_bicubic((x + xmin - c + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[i] = (xmin, xmax)
        coeffs[i, :xmax] = [int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22)) for v in w]
    bounds.setflags(write=False)
    coeffs.setflags(write=False)
    return bounds, coeffs


_BICUBIC_DEV = {}


def _bicubic_tables(n_in, n_out, device):
    """pil_bicubic_coeffs on the device, uploaded once per (in, out, device)"""
    key = (int(n_in), int(n_out), torch.device(device).index)
    t = _BICUBIC_DEV.get(key)
    if t is None:
        b, k = pil_bicubic_coeffs(n_in, n_out)
        t = _BICUBIC_DEV[key] = (h2d(b.copy(), device), h2d(k.copy(), device))
    return t


def _resize_bicubic_work(src, Hd, Wd, out=None):
    n_in, n_out = float(src.numel()), float(src.numel() // (src.shape[-3] * src.shape[-2]) * Hd * Wd)
    return dict(kind="resize_bicubic", Hd=Hd, Wd=Wd), 0.0, n_in + n_out


@_timed(_resize_bicubic_work)
def resize_bicubic_u8(src, Hd, Wd, out=None):
    """Image.fromarray(img).resize((Wd, Hd)) (Pillow's default BICUBIC, 8-bit path, bit-exact) of RGB
    images u8 [H,W,3] or [F,H,W,3] on the device (bf_resize_bicubic_u8)"""
    _need(src, torch.uint8, "src")
    x = src[None] if src.dim() == 3 else src
    if x.dim() != 4 or x.shape[-1] != 3:
        raise HipError("resize_bicubic_u8: RGB images [F,H,W,3]")
    x = x.contiguous()
    F_, Hs, Ws, _ = x.shape
    Hd, Wd = int(Hd), int(Wd)
    if out is None:
        out = torch.empty((F_, Hd, Wd, 3), dtype=torch.uint8, device=x.device)
    _need(out, torch.uint8, "out")
    if out.numel() != F_ * Hd * Wd * 3:
        raise HipError("resize_bicubic_u8: out [F,Hd,Wd,3]")
    bx, kx = _bicubic_tables(Ws, Wd, x.device) if Ws != Wd else (None, None)
    by, ky = _bicubic_tables(Hs, Hd, x.device) if Hs != Hd else (None, None)
    tmp = (torch.empty((F_, Hs, Wd, 3), dtype=torch.uint8, device=x.device)
           if Ws != Wd and Hs != Hd else None)
    _check(lib().bf_resize_bicubic_u8(_ptr(x), F_, Hs, Ws, Hd, Wd, _ptr(kx), _ptr(bx),
                                      kx.shape[1] if kx is not None else 0, _ptr(ky), _ptr(by),
                                      ky.shape[1] if ky is not None else 0, _ptr(tmp), _ptr(out), _stream()),
           "bf_resize_bicubic_u8")
    return out[0] if src.dim() == 3 else out


def _cloud_blocks(items, groups):
    return max(lib().bf_cloud_blocks(int(items), int(groups)), 1)


def _cloud_inputs(name, xyz, valid, rgb):
    """(xyz f32 [B,H,W,3], valid u8 [B,H,W], rgb u8 [B,H,W,3]) contiguous, shapes checked"""
    xyz = _need(xyz, torch.float32, f"{name}: xyz").contiguous()
    if valid.dtype == torch.bool:
        valid = valid.contiguous().view(torch.uint8)
    valid = _need(valid, torch.uint8, f"{name}: valid").contiguous()
    rgb = _need(rgb, torch.uint8, f"{name}: rgb").contiguous()
    if xyz.dim() != 4 or xyz.shape[-1] != 3 or tuple(valid.shape) != tuple(xyz.shape[:3]) or rgb.shape != xyz.shape:
        raise HipError(f"{name}: xyz [B,H,W,3], valid [B,H,W], rgb [B,H,W,3]; got {tuple(xyz.shape)}, "
                       f"{tuple(valid.shape)}, {tuple(rgb.shape)}")
    return xyz, valid, rgb


def _cloud_pack_work(xyz, valid, rgb):
    n = float(valid.numel())
    # algorithmic bytes: the mask twice, xyz + rgb read and six floats written per pixel at most
    return dict(kind="cloud_pack", n=int(n)), 0.0, n * (2 + 12 + 3 + 24)


@_timed(_cloud_pack_work)
def cloud_pack(xyz, valid, rgb):
    """torch.cat((xyz, rgb / 255.0), -1)[valid] (demo.py:127) for a batch (bf_cloud_pack): xyz f32
    [B,H,W,3], valid bool / u8 [B,H,W], rgb u8 [B,H,W,3] -> (xyzrgb f32 [B*H*W,6], offsets int32
    [B+1]); frame b's rows are offsets[b]..offsets[b+1], rows past offsets[B] are not written"""
    xyz, valid, rgb = _cloud_inputs("cloud_pack", xyz, valid, rgb)
    B, H, W = valid.shape
    out = torch.empty((B * H * W, 6), dtype=torch.float32, device=xyz.device)
    offsets = torch.empty(B + 1, dtype=torch.int32, device=xyz.device)
    work = torch.empty(_cloud_blocks(H * W, B), dtype=torch.int32, device=xyz.device)
    _check(lib().bf_cloud_pack(_ptr(xyz), _ptr(valid), _ptr(rgb), B, H, W, _ptr(out), _ptr(offsets),
                               _ptr(work), _stream()), "bf_cloud_pack")
    return out, offsets


# CLOUD_SLOT_WORDS: int64 words of a voxel slot: key, then eight uint32 (bf_cloud_integrate)
CLOUD_SLOT_WORDS, CLOUD_STATS = _C["BF_CLOUD_SLOT_WORDS"], _abi.enum_names("BF_CLOUD_STAT_")


def cloud_table(capacity, device):
    """(table int64 [capacity,5] with every key empty, stats int64 [8] zeroed) for cloud_integrate"""
    capacity = int(capacity)
    if capacity <= 0 or capacity & (capacity - 1) or capacity >= 1 << 31:
        raise HipError("cloud_table: capacity must be a power of two below 2^31")
    table = torch.zeros((capacity, CLOUD_SLOT_WORDS), dtype=torch.int64, device=device)
    table[:, 0] = -1
    return table, torch.zeros(STATS_WORDS, dtype=torch.int64, device=device)


def _cloud_integrate_work(xyz, valid, rgb, fine_step, table, stats, merge=True):
    n = float(valid.numel())
    return dict(kind="cloud_integrate", n=int(n), merge=bool(merge)), 0.0, n * (1 + 12 + 3)


@_timed(_cloud_integrate_work)
def cloud_integrate(xyz, valid, rgb, fine_step, table, stats, merge=True):
    """the valid points of xyz f32 [...,3] / valid bool or u8 [...] / rgb u8 [...,3] into the voxel
    map `table` (cloud_table; bf_cloud_integrate); fine_step = voxel / 256 as an f32"""
    xyz = _need(xyz, torch.float32, "cloud_integrate: xyz").contiguous()
    if valid.dtype == torch.bool:
        valid = valid.contiguous().view(torch.uint8)
    valid = _need(valid, torch.uint8, "cloud_integrate: valid").contiguous()
    rgb = _need(rgb, torch.uint8, "cloud_integrate: rgb").contiguous()
    n = valid.numel()
    if xyz.numel() != 3 * n or rgb.numel() != 3 * n:
        raise HipError("cloud_integrate: xyz [...,3], valid [...], rgb [...,3] of the same points")
    _need(table, torch.int64, "cloud_integrate: table")
    _need(stats, torch.int64, "cloud_integrate: stats")
    if table.dim() != 2 or table.shape[1] != CLOUD_SLOT_WORDS or stats.numel() < STATS_WORDS:
        raise HipError("cloud_integrate: table [capacity,5] / stats [8] of cloud_table")
    _check(lib().bf_cloud_integrate(_ptr(xyz), _ptr(valid), _ptr(rgb), n, fine_step, _ptr(table), table.shape[0],
                                    _ptr(stats), int(bool(merge)), _stream()), "bf_cloud_integrate")


def _cloud_extract_work(table):
    return dict(kind="cloud_extract", capacity=int(table.shape[0])), 0.0, 48.0 * table.shape[0]


@_timed(_cloud_extract_work)
def cloud_extract(table):
    """the occupied slots of a voxel map in slot order (bf_cloud_extract): (key int64 [cap], count
    int32 [cap] holding the uint32 counts, sums int32 [cap,6] holding the uint32 sums, n int32 [1] on
    the device); rows past n are not written"""
    _need(table, torch.int64, "cloud_extract: table")
    cap, dev = table.shape[0], table.device
    key = torch.empty(cap, dtype=torch.int64, device=dev)
    count = torch.empty(cap, dtype=torch.int32, device=dev)
    sums = torch.empty((cap, 6), dtype=torch.int32, device=dev)
    n = torch.empty(1, dtype=torch.int32, device=dev)
    work = torch.empty(_cloud_blocks(cap, 1), dtype=torch.int32, device=dev)
    _check(lib().bf_cloud_extract(_ptr(table), cap, _ptr(key), _ptr(count), _ptr(sums), _ptr(n), _ptr(work),
                                  _stream()), "bf_cloud_extract")
    return key, count, sums, n


# ------------------------------------------------------------------------------------------
# scene mesh (bf_tsdf.hip)
# ------------------------------------------------------------------------------------------
# voxels of a block; int32 fields per voxel: w, sum q, cw, sum r g b; frames of one touch / update launch
TSDF_VOX, TSDF_FIELDS, TSDF_MAX_WEIGHT, TSDF_MAX_FRAMES = (
    _C["BF_TSDF_" + n] for n in ("VOX", "FIELDS", "MAX_WEIGHT", "MAX_FRAMES"))
TSDF_STATS, TSDF_RAYCAST_STATS = _abi.enum_names("BF_TSDF_STAT_"), _abi.enum_names("BF_TSDF_RAY_")


def tsdf_volume(capacity, device):
    """(keys int64 [capacity] all empty, touched int64 [capacity], vox int32 [capacity,6,512], stats
    int64 [8]) zeroed, for tsdf_touch / tsdf_update"""
    capacity = int(capacity)
    if capacity <= 0 or capacity & (capacity - 1) or capacity >= 1 << 31:
        raise HipError("tsdf_volume: capacity must be a power of two below 2^31")
    return (torch.full((capacity,), -1, dtype=torch.int64, device=device),
            torch.zeros(capacity, dtype=torch.int64, device=device),
            torch.zeros((capacity, TSDF_FIELDS, TSDF_VOX), dtype=torch.int32, device=device),
            torch.zeros(STATS_WORDS, dtype=torch.int64, device=device))


def _tsdf_frames(name, depth, poses, rgb=None):
    depth = _need(depth, torch.float32, f"{name}: depth").contiguous()
    poses = _need(poses, torch.float32, f"{name}: poses").contiguous()
    if depth.dim() != 3 or not 0 < depth.shape[0] <= TSDF_MAX_FRAMES or tuple(poses.shape) != (depth.shape[0], 4, 4):
        raise HipError(f"{name}: depth [B,H,W] and poses [B,4,4] of 1..{TSDF_MAX_FRAMES} frames; got {tuple(depth.shape)}, "
                       f"{tuple(poses.shape)}")
    if rgb is not None:
        rgb = _need(rgb, torch.uint8, f"{name}: rgb").contiguous()
        if tuple(rgb.shape) != (*depth.shape, 3):
            raise HipError(f"{name}: rgb [B,H,W,3] at the depth size, got {tuple(rgb.shape)}")
    return depth, poses, rgb


def _tsdf_arrays(name, keys, touched, vox=None, stats=None):
    _need(keys, torch.int64, f"{name}: keys")
    _need(touched, torch.int64, f"{name}: touched")
    cap = keys.shape[0]
    if keys.dim() != 1 or tuple(touched.shape) != (cap,):
        raise HipError(f"{name}: keys / touched [capacity] of tsdf_volume")
    if vox is not None and (vox.dtype != torch.int32 or tuple(vox.shape) != (cap, TSDF_FIELDS, TSDF_VOX)):
        raise HipError(f"{name}: vox int32 [capacity,6,512] of tsdf_volume")
    if stats is not None and (stats.dtype != torch.int64 or stats.numel() < STATS_WORDS):
        raise HipError(f"{name}: stats int64 [{STATS_WORDS}] of tsdf_volume")
    return cap


def _tsdf_touch_work(depth, poses, intr, voxel, trunc_voxels, max_depth, keys, touched, stats):
    n = float(depth.numel())
    return dict(kind="tsdf_touch", n=int(n)), 0.0, n * 4


@_timed(_tsdf_touch_work)
def tsdf_touch(depth, poses, intr, voxel, trunc_voxels, max_depth, keys, touched, stats):
    """claim and mark the blocks within the truncation band of depth f32 [B,H,W] seen from poses f32
    [B,4,4] (B <= 64) with the pinhole intr = (fx, fy, cx, cy) (bf_tsdf_touch)"""
    depth, poses, _ = _tsdf_frames("tsdf_touch", depth, poses)
    cap = _tsdf_arrays("tsdf_touch", keys, touched, stats=stats)
    B, H, W = depth.shape
    _check(lib().bf_tsdf_touch(_ptr(depth), _ptr(poses), B, H, W, *intr, voxel, int(trunc_voxels), max_depth,
                               _ptr(keys), _ptr(touched), cap, _ptr(stats), _stream()), "bf_tsdf_touch")


def _tsdf_update_work(depth, poses, intr, voxel, trunc_voxels, max_depth, keys, touched, vox, stats, rgb=None,
                      max_weight=TSDF_MAX_WEIGHT):
    return dict(kind="tsdf_update", n=int(depth.numel()), colour=rgb is not None), 0.0, float(depth.numel()) * 4


@_timed(_tsdf_update_work)
def tsdf_update(depth, poses, intr, voxel, trunc_voxels, max_depth, keys, touched, vox, stats, rgb=None,
                max_weight=TSDF_MAX_WEIGHT):
    """the frames of the tsdf_touch call before it into the voxels of the blocks it marked, and the
    marks cleared (bf_tsdf_update); rgb u8 [B,H,W,3] at the depth size, or None for no colour"""
    depth, poses, rgb = _tsdf_frames("tsdf_update", depth, poses, rgb)
    cap = _tsdf_arrays("tsdf_update", keys, touched, vox, stats)
    if not 1 <= int(max_weight) <= TSDF_MAX_WEIGHT:
        raise HipError(f"tsdf_update: max_weight in 1..{TSDF_MAX_WEIGHT}")
    B, H, W = depth.shape
    dev = depth.device
    slots = torch.empty(cap, dtype=torch.int32, device=dev)
    n = torch.empty(1, dtype=torch.int32, device=dev)
    work = torch.empty(_cloud_blocks(cap, 1), dtype=torch.int32, device=dev)
    _check(lib().bf_tsdf_update(_ptr(depth), _ptr(rgb), _ptr(poses), B, H, W, *intr, voxel,
                                int(trunc_voxels), max_depth, int(max_weight), _ptr(keys), _ptr(touched), _ptr(vox),
                                cap, _ptr(slots), _ptr(n), _ptr(work), _ptr(stats), _stream()), "bf_tsdf_update")


def _tsdf_extract_work(keys):
    return dict(kind="tsdf_extract", capacity=int(keys.shape[0])), 0.0, 20.0 * keys.shape[0]


@_timed(_tsdf_extract_work)
def tsdf_extract(keys):
    """the occupied slots of a volume in slot order (bf_tsdf_extract): (key int64 [cap], slot int32
    [cap], n int32 [1] on the device); rows past n are not written"""
    _need(keys, torch.int64, "tsdf_extract: keys")
    cap, dev = keys.shape[0], keys.device
    key = torch.empty(cap, dtype=torch.int64, device=dev)
    slot = torch.empty(cap, dtype=torch.int32, device=dev)
    n = torch.empty(1, dtype=torch.int32, device=dev)
    work = torch.empty(_cloud_blocks(cap, 1), dtype=torch.int32, device=dev)
    _check(lib().bf_tsdf_extract(_ptr(keys), cap, _ptr(key), _ptr(slot), _ptr(n), _ptr(work), _stream()),
           "bf_tsdf_extract")
    return key, slot, n


def _tsdf_surface_work(keys, vox, skey, sslot, voxel):
    return dict(kind="tsdf_surface", blocks=int(skey.shape[0])), 0.0, float(skey.shape[0]) * TSDF_VOX * TSDF_FIELDS * 4


@_timed(_tsdf_surface_work)
def tsdf_surface(keys, vox, skey, sslot, voxel):
    """naive surface nets over the occupied blocks sorted by key (skey int64 [n], sslot int32 [n]):
    (vertices f32 [nv,3], rgb u8 [nv,3], faces int32 [nf,3]) (bf_tsdf_surface_count, one read-back of
    the two totals, bf_tsdf_surface_write)"""
    _need(keys, torch.int64, "tsdf_surface: keys")
    _need(vox, torch.int32, "tsdf_surface: vox")
    skey = _need(skey, torch.int64, "tsdf_surface: skey").contiguous()
    sslot = _need(sslot, torch.int32, "tsdf_surface: sslot").contiguous()
    cap, dev, n = keys.shape[0], keys.device, int(skey.shape[0])
    if tuple(vox.shape) != (cap, TSDF_FIELDS, TSDF_VOX) or tuple(sslot.shape) != (n,) or n > cap:
        raise HipError("tsdf_surface: keys [capacity], vox [capacity,6,512], skey / sslot [n <= capacity]")
    empty = (torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0, 3), dtype=torch.uint8, device=dev),
             torch.empty((0, 3), dtype=torch.int32, device=dev))
    if n == 0:
        return empty
    rank = torch.empty(cap, dtype=torch.int32, device=dev)
    bitmap = torch.empty((n, 8), dtype=torch.int64, device=dev)
    eflags = torch.empty((n, TSDF_VOX), dtype=torch.uint8, device=dev)
    vprefix = torch.empty(n, dtype=torch.int32, device=dev)
    fprefix = torch.empty(n, dtype=torch.int32, device=dev)
    totals = torch.empty(2, dtype=torch.int32, device=dev)
    head = (_ptr(keys), cap, _ptr(vox), _ptr(skey), _ptr(sslot), n, _ptr(rank), _ptr(bitmap), _ptr(eflags),
            _ptr(vprefix), _ptr(fprefix))
    _check(lib().bf_tsdf_surface_count(*head, _ptr(totals), _stream()), "bf_tsdf_surface_count")
    nv, nq = totals.cpu().tolist()
    if nv == 0:
        return empty
    verts = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    vrgb = torch.empty((nv, 3), dtype=torch.uint8, device=dev)
    faces = torch.empty((max(2 * nq, 1), 3), dtype=torch.int32, device=dev)
    _check(lib().bf_tsdf_surface_write(*head, voxel, _ptr(verts), _ptr(vrgb), _ptr(faces), _stream()),
           "bf_tsdf_surface_write")
    return verts, vrgb, faces[:2 * nq]


def _tsdf_raycast_work(keys, vox, poses, intr, H, W, voxel, trunc_voxels, near, far, min_weight, max_steps, counters,
                       colour=False):
    n = float(poses.shape[0]) * H * W
    return dict(kind="tsdf_raycast", n=int(n), colour=bool(colour)), 0.0, n * 28


@_timed(_tsdf_raycast_work)
def tsdf_raycast(keys, vox, poses, intr, H, W, voxel, trunc_voxels, near, far, min_weight, max_steps, counters,
                 colour=False):
    """the volume seen from poses f32 [V,4,4] through the pinhole intr at H x W (bf_tsdf_raycast):
    (depth f32 [V,H,W], vertex f32 [V,H,W,3], normal f32 [V,H,W,3], rgb u8 [V,H,W,3] or None);
    counters int64 [8] is added to (TSDF_RAYCAST_STATS)"""
    _need(keys, torch.int64, "tsdf_raycast: keys")
    poses = _need(poses, torch.float32, "tsdf_raycast: poses").contiguous()
    cap, dev = keys.shape[0], keys.device
    if keys.dim() != 1 or vox.dtype != torch.int32 or tuple(vox.shape) != (cap, TSDF_FIELDS, TSDF_VOX):
        raise HipError("tsdf_raycast: keys [capacity] and vox int32 [capacity,6,512] of tsdf_volume")
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (4, 4) or poses.shape[0] < 1:
        raise HipError(f"tsdf_raycast: poses [V,4,4], got {tuple(poses.shape)}")
    if counters.dtype != torch.int64 or counters.numel() < STATS_WORDS:
        raise HipError(f"tsdf_raycast: counters int64 [{STATS_WORDS}]")
    V, H, W = int(poses.shape[0]), int(H), int(W)
    depth = torch.empty((V, H, W), dtype=torch.float32, device=dev)
    vertex = torch.empty((V, H, W, 3), dtype=torch.float32, device=dev)
    normal = torch.empty((V, H, W, 3), dtype=torch.float32, device=dev)
    rgb = torch.empty((V, H, W, 3), dtype=torch.uint8, device=dev) if colour else None
    _check(lib().bf_tsdf_raycast(_ptr(keys), _ptr(vox), cap, _ptr(poses), V, H, W, *intr, voxel,
                                 int(trunc_voxels), near, far, int(min_weight), int(max_steps), _ptr(depth),
                                 _ptr(vertex), _ptr(normal), _ptr(rgb), _ptr(counters), _stream()), "bf_tsdf_raycast")
    return depth, vertex, normal, rgb


# ------------------------------------------------------------------------------------------
# tracking (bf_track.hip)
# ------------------------------------------------------------------------------------------
def _depth_vertex_normal_work(depth, intr, max_depth, jump):
    return dict(kind="depth_vertex_normal", n=int(depth.numel())), 0.0, float(depth.numel()) * 28


@_timed(_depth_vertex_normal_work)
def depth_vertex_normal(depth, intr, max_depth, jump):
    """depth f32 [H,W] metres -> camera-frame (vertex f32 [H,W,3], normal f32 [H,W,3])
    (bf_depth_vertex_normal)"""
    depth = _need(depth, torch.float32, "depth_vertex_normal: depth").contiguous()
    if depth.dim() != 2:
        raise HipError(f"depth_vertex_normal: depth [H,W], got {tuple(depth.shape)}")
    H, W = depth.shape
    vertex = torch.empty((H, W, 3), dtype=torch.float32, device=depth.device)
    normal = torch.empty((H, W, 3), dtype=torch.float32, device=depth.device)
    _check(lib().bf_depth_vertex_normal(_ptr(depth), H, W, *intr, max_depth, jump, _ptr(vertex),
                                        _ptr(normal), _stream()), "bf_depth_vertex_normal")
    return vertex, normal


def icp_blocks(H, W, stride):
    """rows of bf_icp_reduce's partials for a live map of H x W sampled at `stride`"""
    n = lib().bf_icp_blocks(int(H), int(W), int(stride))
    if n <= 0:
        raise HipError(f"icp_blocks: H, W, stride = {H}, {W}, {stride}")
    return n


def _reduce_setup(name, live_vertex, stride, T, w2c, w2c_name, intr, out):
    """what icp_reduce and photo_reduce share: (stride, T and w2c as host f64 [12], the pinhole, the
    partials workspace, out f64 [32] checked or allocated).  The pinhole is rounded to f32 and then
    passed as doubles: the kernels' bits depend on it"""
    stride = int(stride)
    if stride < 1:
        raise HipError(f"{name}: stride >= 1")
    T = np.ascontiguousarray(np.asarray(T, np.float64).reshape(-1)[:12])
    M = np.ascontiguousarray(np.asarray(w2c, np.float64).reshape(-1)[:12])
    if T.size != 12 or M.size != 12:
        raise HipError(f"{name}: T and {w2c_name} f64 [3,4]")
    H, W = live_vertex.shape[:2]
    dev = live_vertex.device
    partials = torch.empty((icp_blocks(H, W, stride), ICP_ROW), dtype=torch.float64, device=dev)
    if out is None:
        out = torch.empty(ICP_ROW, dtype=torch.float64, device=dev)
    elif out.dtype != torch.float64 or out.numel() != ICP_ROW:
        raise HipError(f"{name}: out f64 [{ICP_ROW}]")
    return stride, T, M, [float(np.float32(v)) for v in intr], partials, out


def _icp_reduce_work(live_vertex, live_normal, stride, T, model_vertex, model_normal, model_w2c, intr, dist_max, cos_min,
                     out=None):
    n = float(live_vertex.shape[0] // stride) * (live_vertex.shape[1] // stride)
    return dict(kind="icp_reduce", n=int(n), stride=int(stride)), n * 120.0, n * 48.0


@_timed(_icp_reduce_work)
def icp_reduce(live_vertex, live_normal, stride, T, model_vertex, model_normal, model_w2c, intr, dist_max, cos_min,
               out=None):
    """the normal equations of one ICP iteration (bf_icp_reduce): out f64 [32] on the device = the 21
    upper-triangle entries of J^T J, the 6 of J^T r, sum r^2, the inlier count.  live maps f32 [H,W,3]
    (camera frame), T host f64 [3,4] camera-to-world, model maps f32 [Hm,Wm,3] (world) of the camera
    model_w2c (host f64 [3,4]) with the pinhole intr"""
    for t, name in ((live_vertex, "live_vertex"), (live_normal, "live_normal"), (model_vertex, "model_vertex"),
                    (model_normal, "model_normal")):
        _need(t, torch.float32, f"icp_reduce: {name}")
        if t.dim() != 3 or t.shape[2] != 3:
            raise HipError(f"icp_reduce: {name} [H,W,3], got {tuple(t.shape)}")
    if live_vertex.shape != live_normal.shape or model_vertex.shape != model_normal.shape:
        raise HipError("icp_reduce: a vertex and a normal map of one size each")
    stride, T, M, intr, partials, out = _reduce_setup("icp_reduce", live_vertex, stride, T, model_w2c, "model_w2c",
                                                      intr, out)
    H, W = live_vertex.shape[:2]
    Hm, Wm = model_vertex.shape[:2]
    _check(lib().bf_icp_reduce(_ptr(live_vertex.contiguous()), _ptr(live_normal.contiguous()), H, W, stride,
                               T.ctypes.data, _ptr(model_vertex.contiguous()), _ptr(model_normal.contiguous()), Hm, Wm,
                               M.ctypes.data, *intr, dist_max, cos_min, _ptr(partials), _ptr(out), _stream()),
           "bf_icp_reduce")
    return out


def _grey_u8_work(rgb, out=None):
    return dict(kind="grey_u8", n=int(rgb.numel() // 3)), 0.0, float(rgb.numel()) * 7 / 3


@_timed(_grey_u8_work)
def grey_u8(rgb, out=None):
    """RGB images u8 [H,W,3] or [B,H,W,3] -> intensity f32 [H,W] or [B,H,W] = ((77 R + 150 G + 29 B + 128)
    >> 8) / 255 (bf_grey_u8)"""
    _need(rgb, torch.uint8, "grey_u8: rgb")
    x = rgb[None] if rgb.dim() == 3 else rgb
    if x.dim() != 4 or x.shape[-1] != 3:
        raise HipError(f"grey_u8: RGB images [B,H,W,3], got {tuple(rgb.shape)}")
    x = x.contiguous()
    B, H, W, _ = x.shape
    if out is None:
        out = torch.empty((B, H, W), dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or out.numel() != B * H * W or not out.is_contiguous():
        raise HipError("grey_u8: out f32 [B,H,W]")
    _check(lib().bf_grey_u8(_ptr(x), B, H, W, _ptr(out), _stream()), "bf_grey_u8")
    out = out.view(B, H, W)
    return out[0] if rgb.dim() == 3 else out


def _photo_reduce_work(live_vertex, live_intensity, stride, T, ref_intensity, ref_depth, ref_w2c, intr, dist_max,
                       intensity_max, out=None):
    n = float(live_vertex.shape[0] // stride) * (live_vertex.shape[1] // stride)
    return dict(kind="photo_reduce", n=int(n), stride=int(stride)), n * 130.0, n * 36.0


@_timed(_photo_reduce_work)
def photo_reduce(live_vertex, live_intensity, stride, T, ref_intensity, ref_depth, ref_w2c, intr, dist_max, intensity_max,
                 out=None):
    """the normal equations of the photometric term (bf_photo_reduce): out f64 [32] on the device in
    icp_reduce's layout.  live_vertex f32 [H,W,3] (camera frame) and live_intensity f32 [H,W] of the new
    frame, T host f64 [3,4] camera-to-world; ref_intensity and ref_depth f32 [Hr,Wr] of the last placed
    frame, whose camera is ref_w2c (host f64 [3,4]) with the pinhole intr"""
    _need(live_vertex, torch.float32, "photo_reduce: live_vertex")
    if live_vertex.dim() != 3 or live_vertex.shape[2] != 3:
        raise HipError(f"photo_reduce: live_vertex [H,W,3], got {tuple(live_vertex.shape)}")
    for t, name in ((live_intensity, "live_intensity"), (ref_intensity, "ref_intensity"), (ref_depth, "ref_depth")):
        _need(t, torch.float32, f"photo_reduce: {name}")
        if t.dim() != 2:
            raise HipError(f"photo_reduce: {name} [H,W], got {tuple(t.shape)}")
    if live_intensity.shape != live_vertex.shape[:2] or ref_intensity.shape != ref_depth.shape:
        raise HipError("photo_reduce: an intensity map of the vertex map's size, and of the reference depth's")
    stride, T, M, intr, partials, out = _reduce_setup("photo_reduce", live_vertex, stride, T, ref_w2c, "ref_w2c", intr,
                                                      out)
    H, W = live_vertex.shape[:2]
    Hr, Wr = ref_intensity.shape
    _check(lib().bf_photo_reduce(_ptr(live_vertex.contiguous()), _ptr(live_intensity.contiguous()), H, W, stride,
                                 T.ctypes.data, _ptr(ref_intensity.contiguous()), _ptr(ref_depth.contiguous()), Hr, Wr,
                                 M.ctypes.data, *intr, dist_max, intensity_max, _ptr(partials), _ptr(out), _stream()),
           "bf_photo_reduce")
    return out


# ------------------------------------------------------------------------------------------
# relocalisation (bf_fern.hip)
# ------------------------------------------------------------------------------------------
FERN_COUNTERS, FERN_K_MAX = _abi.enum_names("BF_FERN_COUNT_"), _C["BF_FERN_K_MAX"]


def fern_upload(table, cells, device):
    """a host fern table i32 [F,5] (cell, tR, tG, tB, tD per fern; F a multiple of 8, every cell index
    below `cells`) checked by bf_fern_table_check and copied to the device"""
    t = np.ascontiguousarray(np.asarray(table, np.int32))
    if t.ndim != 2 or t.shape[1] != 5:
        raise HipError(f"fern_upload: table i32 [F,5], got {t.shape}")
    _check(lib().bf_fern_table_check(t.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), t.shape[0], int(cells)),
           "bf_fern_table_check")
    return h2d(t, device)


def _fern_frames(depth, rgb):
    _need(depth, torch.float32, "fern_encode: depth")
    d = depth[None] if depth.dim() == 2 else depth
    if d.dim() != 3:
        raise HipError(f"fern_encode: depth [H,W] or [B,H,W], got {tuple(depth.shape)}")
    if rgb is not None:
        _need(rgb, torch.uint8, "fern_encode: rgb")
        rgb = rgb[None] if rgb.dim() == 3 else rgb
        if tuple(rgb.shape) != tuple(d.shape) + (3,) or rgb.device != d.device:
            raise HipError(f"fern_encode: rgb u8 {tuple(d.shape) + (3,)} beside the depth, got {tuple(rgb.shape)}")
        rgb = rgb.contiguous()
    return d.contiguous(), rgb


def _fern_encode_work(depth, rgb, cell, max_depth, ferns, with_means=False, codes=None):
    return dict(kind="fern_encode", n=int(depth.numel())), 0.0, float(depth.numel()) * (4 if rgb is None else 7)


@_timed(_fern_encode_work)
def fern_encode(depth, rgb, cell, max_depth, ferns, with_means=False, codes=None):
    """frames (depth f32 [H,W] or [B,H,W] metres, rgb u8 of the same size with a last axis of 3, or None)
    -> codes u32-in-int32 [B, F/8] under the device fern table `ferns` i32 [F,5] (bf_fern_encode); with
    with_means=True (codes, means i32 [B, (H//cell) (W//cell), 4])"""
    d, rgb = _fern_frames(depth, rgb)
    _need(ferns, torch.int32, "fern_encode: ferns")
    if ferns.dim() != 2 or ferns.shape[1] != 5 or ferns.device != d.device:
        raise HipError(f"fern_encode: ferns i32 [F,5] on the depth's device, got {tuple(ferns.shape)}")
    B, H, W = d.shape
    F, cell = int(ferns.shape[0]), int(cell)
    if codes is None:
        codes = torch.empty((B, max(F // 8, 1)), dtype=torch.int32, device=d.device)
    elif codes.dtype != torch.int32 or codes.numel() != B * (F // 8) or not codes.is_contiguous():
        raise HipError("fern_encode: codes int32 [B, F/8]")
    means = None
    if with_means:
        means = torch.empty((B, max(H // cell, 0) * max(W // cell, 0) if cell > 0 else 0, 4), dtype=torch.int32, device=d.device)
    _check(lib().bf_fern_encode(_ptr(d), _ptr(rgb), B, H, W, cell, max_depth, _ptr(ferns.contiguous()), F, _ptr(means),
                                _ptr(codes), _stream()), "bf_fern_encode")
    return (codes, means) if with_means else codes


def _fern_search_work(table, n, n_upper, queries, k, with_rows=False, top=None):
    return dict(kind="fern_search", n=int(n_upper), q=int(queries.shape[0])), 0.0, float(n_upper) * table.shape[1] * 4


@_timed(_fern_search_work)
def fern_search(table, n, n_upper, queries, k, with_rows=False, top=None):
    """the k (<= 8) nearest keyframes of each query (bf_fern_search): table int32 [capacity, F/8] (the u32
    codes), n int32 [1] on the device (the rows held), n_upper the host's bound of it, queries int32
    [Q, F/8] -> top int32 [Q,k,2] of (distance, index), (-1, -1) beyond n; with_rows=True (top, rows
    int32 [Q, n_upper] with -1 at and beyond n)"""
    _need(table, torch.int32, "fern_search: table")
    _need(queries, torch.int32, "fern_search: queries")
    _need(n, torch.int32, "fern_search: n")
    if table.dim() != 2 or queries.dim() != 2 or queries.shape[1] != table.shape[1] or n.numel() < 1:
        raise HipError(f"fern_search: table [capacity, F/8], queries [Q, F/8], n [1]; got {tuple(table.shape)}, "
                       f"{tuple(queries.shape)}, {tuple(n.shape)}")
    if queries.device != table.device or n.device != table.device:
        raise HipError("fern_search: table, n and queries on one device")
    capacity, words = table.shape
    Q, k, n_upper = int(queries.shape[0]), int(k), int(n_upper)
    blocks = lib().bf_fern_search_blocks(n_upper)
    part = torch.empty((max(Q, 1), max(blocks, 1), max(k, 1)), dtype=torch.int64, device=table.device)
    if top is None:
        top = torch.empty((Q, max(k, 1), 2), dtype=torch.int32, device=table.device)
    elif top.dtype != torch.int32 or top.numel() != Q * k * 2 or not top.is_contiguous():
        raise HipError("fern_search: top int32 [Q,k,2]")
    rows = torch.empty((Q, max(n_upper, 1)), dtype=torch.int32, device=table.device) if with_rows else None
    _check(lib().bf_fern_search(_ptr(table), capacity, words * 8, _ptr(n), n_upper, _ptr(queries.contiguous()), Q, k,
                                _ptr(part), _ptr(top), _ptr(rows), _stream()), "bf_fern_search")
    return (top, rows) if with_rows else top


def _fern_append_work(table, n, code, best, threshold, pose, frame, poses, ids, counters):
    return dict(kind="fern_append"), 0.0, float(table.shape[1]) * 8 + 76


@_timed(_fern_append_work)
def fern_append(table, n, code, best, threshold, pose, frame, poses, ids, counters):
    """the conditional append of one code (bf_fern_append): `code` int32 [F/8] joins row n of table when
    n == 0 or best[0] (int32 on the device, the nearest distance of the search) > threshold; pose (host
    f32 [4,4]) and frame go to row n of poses f32 [capacity,16] and ids int32 [capacity]; counters
    int32 [3] (FERN_COUNTERS).  Launches only"""
    for t, dt, name in ((table, torch.int32, "table"), (n, torch.int32, "n"), (code, torch.int32, "code"),
                        (best, torch.int32, "best"), (poses, torch.float32, "poses"), (ids, torch.int32, "ids"),
                        (counters, torch.int32, "counters")):
        _need(t, dt, f"fern_append: {name}")
        if t.device != table.device:
            raise HipError(f"fern_append: {name} on the table's device")
    capacity, words = table.shape
    if code.numel() != words or best.numel() < 1 or poses.numel() != capacity * 16 or ids.numel() != capacity or \
            counters.numel() < 3 or n.numel() < 1:
        raise HipError("fern_append: code [F/8], best [>= 1], poses [capacity,16], ids [capacity], counters [3], n [1]")
    P = np.ascontiguousarray(np.asarray(pose, np.float32).reshape(-1))
    if P.size != 16:
        raise HipError("fern_append: pose f32 [4,4]")
    _check(lib().bf_fern_append(_ptr(table), capacity, words * 8, _ptr(n), _ptr(code), _ptr(best), int(threshold),
                                P.ctypes.data_as(ctypes.POINTER(c_float)), int(frame), _ptr(poses), _ptr(ids),
                                _ptr(counters), _stream()), "bf_fern_append")


# ------------------------------------------------------------------------------------------
# headless renderer (bf_render.hip)
# ------------------------------------------------------------------------------------------
def _render_target(name, keys):
    """(V, H, W) of a key buffer int64 [V,H,W] holding the uint64 keys"""
    _need(keys, torch.int64, f"{name}: keys")
    if keys.dim() != 3:
        raise HipError(f"{name}: keys [V,H,W], got {tuple(keys.shape)}")
    return tuple(int(s) for s in keys.shape)


def _render_cams(name, cams, V, intr):
    cams = _need(cams, torch.float32, f"{name}: cams").contiguous()
    if tuple(cams.shape) != (V, 12):
        raise HipError(f"{name}: cams [{V},12] (R row-major, t), got {tuple(cams.shape)}")
    return cams, tuple(intr)


def render_clear(keys):
    """every key of keys int64 [V,H,W] to empty (bf_render_clear)"""
    V, H, W = _render_target("render_clear", keys)
    _check(lib().bf_render_clear(_ptr(keys), V, H, W, _stream()), "bf_render_clear")


def _render_points_work(keys, xyz, rgb, cams, intr, near, far, radius, layer, stats=None):
    n, V = int(xyz.shape[0]), int(keys.shape[0])
    # algorithmic bytes: the points once per view, one 8-byte key per splat pixel
    return (dict(kind="render_points", n=n, views=V, radius=int(radius)), 0.0,
            float(n) * V * (15 + 8 * (2 * int(radius) + 1) ** 2))


@_timed(_render_points_work)
def render_points(keys, xyz, rgb, cams, intr, near, far, radius, layer, stats=None):
    """xyz f32 [n,3] / rgb u8 [n,3] into keys int64 [V,H,W] (bf_render_points); cams f32 [V,12], intr
    (fx, fy, cx, cy); stats: None or int64 [2] added to (pixels offered, atomics issued)"""
    V, H, W = _render_target("render_points", keys)
    xyz = _need(xyz, torch.float32, "render_points: xyz").contiguous()
    rgb = _need(rgb, torch.uint8, "render_points: rgb").contiguous()
    n = xyz.shape[0]
    if xyz.dim() != 2 or xyz.shape[1] != 3 or tuple(rgb.shape) != (n, 3):
        raise HipError(f"render_points: xyz [n,3] and rgb [n,3], got {tuple(xyz.shape)} and {tuple(rgb.shape)}")
    if stats is not None and (_need(stats, torch.int64, "render_points: stats").numel() < 2):
        raise HipError("render_points: stats int64 [2]")
    cams, (fx, fy, cx, cy) = _render_cams("render_points", cams, V, intr)
    _check(lib().bf_render_points(_ptr(xyz), _ptr(rgb), n, _ptr(cams), V, fx, fy, cx, cy, H, W, near, far,
                                  int(radius), int(layer), _ptr(keys), _ptr(stats), _stream()), "bf_render_points")


def _render_edges_work(keys, corners, colors, mask, cams, intr, near, half_width, layer):
    b, V = int(corners.shape[0]), int(keys.shape[0])
    return dict(kind="render_edges", boxes=b, views=V, half_width=int(half_width)), 0.0, float(b) * V * (96 + 3)


@_timed(_render_edges_work)
def render_edges(keys, corners, colors, mask, cams, intr, near, half_width, layer):
    """the wireframes of corners f32 [B,8,3] in colors u8 [B,3] (mask: None or u8 / bool [B]) into
    keys int64 [V,H,W] (bf_render_edges)"""
    V, H, W = _render_target("render_edges", keys)
    corners = _need(corners, torch.float32, "render_edges: corners").contiguous()
    colors = _need(colors, torch.uint8, "render_edges: colors").contiguous()
    b = corners.shape[0]
    if tuple(corners.shape) != (b, 8, 3) or tuple(colors.shape) != (b, 3):
        raise HipError(f"render_edges: corners [B,8,3] and colors [B,3], got {tuple(corners.shape)} and {tuple(colors.shape)}")
    if mask is not None:
        if mask.dtype == torch.bool:
            mask = mask.contiguous().view(torch.uint8)
        mask = _need(mask, torch.uint8, "render_edges: mask").contiguous()
        if tuple(mask.shape) != (b,):
            raise HipError(f"render_edges: mask [{b}], got {tuple(mask.shape)}")
    cams, (fx, fy, cx, cy) = _render_cams("render_edges", cams, V, intr)
    _check(lib().bf_render_edges(_ptr(corners), _ptr(colors), _ptr(mask), b, _ptr(cams), V, fx, fy, cx, cy, H, W, near,
                                 int(half_width), int(layer), _ptr(keys), _stream()), "bf_render_edges")


RENDER_COOP_PIXELS = 64       # DESIGN.md §4 "Renderer": the sweep of scripts/render_mesh_probe.py


def _render_triangles_work(keys, vertices, rgb, faces, cams, intr, near, far, cull, shade, layer, coop_pixels=None,
                           stats=None):
    m, V = int(faces.shape[0]), int(keys.shape[0])
    # algorithmic bytes: a face and its three vertices once per view; the pixels depend on the geometry
    return dict(kind="render_triangles", m=m, views=V), 0.0, float(m) * V * (12 + 3 * 15)


@_timed(_render_triangles_work)
def render_triangles(keys, vertices, rgb, faces, cams, intr, near, far, cull, shade, layer, coop_pixels=None, stats=None):
    """vertices f32 [n,3] / rgb u8 [n,3] / faces int32 [m,3] filled into keys int64 [V,H,W]
    (bf_render_triangles); cull / shade / layer 0 or 1; coop_pixels: None (RENDER_COOP_PIXELS) or the
    rectangle size from which a triangle is filled by its whole wave (the image does not depend on
    it); stats: None or int64 [6] added to (pairs drawn, dropped as not finite or outside near..far,
    dropped by index or guard band, culled or of zero area, pixels covered, atomics issued)"""
    V, H, W = _render_target("render_triangles", keys)
    vertices = _need(vertices, torch.float32, "render_triangles: vertices").contiguous()
    rgb = _need(rgb, torch.uint8, "render_triangles: rgb").contiguous()
    faces = _need(faces, torch.int32, "render_triangles: faces").contiguous()
    n, m = vertices.shape[0], faces.shape[0]
    if vertices.dim() != 2 or vertices.shape[1] != 3 or tuple(rgb.shape) != (n, 3) or faces.dim() != 2 or faces.shape[1] != 3:
        raise HipError(f"render_triangles: vertices [n,3], rgb [n,3] and faces [m,3], got {tuple(vertices.shape)}, "
                       f"{tuple(rgb.shape)} and {tuple(faces.shape)}")
    if stats is not None and (_need(stats, torch.int64, "render_triangles: stats").numel() < 6):
        raise HipError("render_triangles: stats int64 [6]")
    cams, (fx, fy, cx, cy) = _render_cams("render_triangles", cams, V, intr)
    coop = RENDER_COOP_PIXELS if coop_pixels is None else min(int(coop_pixels), 2 ** 31 - 1)
    _check(lib().bf_render_triangles(_ptr(vertices), _ptr(rgb), n, _ptr(faces), m, _ptr(cams), V, fx, fy, cx, cy, H, W,
                                     near, far, int(cull), int(shade), int(layer), coop, _ptr(keys), _ptr(stats),
                                     _stream()), "bf_render_triangles")


def _render_resolve_work(keys, background=(0, 0, 0)):
    return dict(kind="render_resolve", pixels=int(keys.numel())), 0.0, float(keys.numel()) * (8 + 3 + 4)


@_timed(_render_resolve_work)
def render_resolve(keys, background=(0, 0, 0)):
    """keys int64 [V,H,W] -> (rgb u8 [V,H,W,3], depth f32 [V,H,W]) (bf_render_resolve); background:
    an (r, g, b) constant or a u8 image [V,H,W,3] for the empty pixels"""
    V, H, W = _render_target("render_resolve", keys)
    image, const = None, (0, 0, 0)
    if torch.is_tensor(background):
        image = _need(background, torch.uint8, "render_resolve: background").contiguous()
        if tuple(image.shape) != (V, H, W, 3):
            raise HipError(f"render_resolve: background image [{V},{H},{W},3], got {tuple(image.shape)}")
    else:
        const = tuple(int(v) for v in background)
        if len(const) != 3:
            raise HipError("render_resolve: background (r, g, b)")
    rgb = torch.empty((V, H, W, 3), dtype=torch.uint8, device=keys.device)
    depth = torch.empty((V, H, W), dtype=torch.float32, device=keys.device)
    _check(lib().bf_render_resolve(_ptr(keys), V, H, W, _ptr(image), const[0], const[1], const[2], _ptr(rgb),
                                   _ptr(depth), _stream()), "bf_render_resolve")
    return rgb, depth


# ------------------------------------------------------------------------------------------
# evaluation against ground truth (bf_eval.hip; f64 throughout, off the timed path)
# ------------------------------------------------------------------------------------------
def _f64_rows(t, tail, name):
    t = _need(t, torch.float64, name).contiguous()
    if t.dim() != len(tail) + 1 or tuple(t.shape[1:]) != tuple(tail):
        raise HipError(f"{name}: expected [n,{','.join(map(str, tail))}], got {tuple(t.shape)}")
    return t


def gt_frustum_seen(corners, pose_inv, fx, fy, cx, cy, W, H, near, far):
    """bf_gt_frustum: corners f64 [N,8,3] (world), pose_inv f64 [M,4,4] -> seen u8 [N,8], 1 where the
    corner projects into at least one frame (filter_gt_boxes.py:24-62)"""
    corners = _f64_rows(corners, (8, 3), "gt_frustum_seen: corners")
    pose_inv = _f64_rows(pose_inv, (4, 4), "gt_frustum_seen: pose_inv")
    n, m = corners.shape[0], pose_inv.shape[0]
    seen = torch.zeros((n, 8), dtype=torch.uint8, device=corners.device)
    _check(lib().bf_gt_frustum(_ptr(corners), n, _ptr(pose_inv), m, fx, fy, cx, cy, int(W), int(H), near,
                               far, _ptr(seen), _stream()), "bf_gt_frustum")
    return seen


def nn_min_dist2(query, points):
    """bf_nn_min_dist2: query f64 [Q,3], points f64 [P,3] -> d2 f64 [Q], the squared distance to the
    nearest point (+inf when P == 0)"""
    query = _f64_rows(query, (3,), "nn_min_dist2: query")
    points = _f64_rows(points, (3,), "nn_min_dist2: points")
    q, p = query.shape[0], points.shape[0]
    d2 = torch.full((q,), float("inf"), dtype=torch.float64, device=query.device)
    _check(lib().bf_nn_min_dist2(_ptr(query), q, _ptr(points), p, _ptr(d2), _stream()), "bf_nn_min_dist2")
    return d2


def obb_iou_exact(a, b, with_inter=False):
    """bf_obb_iou_exact: a f64 [P,12], b f64 [G,12] (centre, three half-axis vectors) -> iou f64
    [P,G], and the intersection volumes f64 [P,G] when with_inter"""
    a = _f64_rows(a, (12,), "obb_iou_exact: a")
    b = _f64_rows(b, (12,), "obb_iou_exact: b")
    p, g = a.shape[0], b.shape[0]
    iou = torch.empty((p, g), dtype=torch.float64, device=a.device)
    inter = torch.empty((p, g), dtype=torch.float64, device=a.device) if with_inter else None
    _check(lib().bf_obb_iou_exact(_ptr(a), p, _ptr(b), g, _ptr(iou), _ptr(inter), _stream()),
           "bf_obb_iou_exact")
    return (iou, inter) if with_inter else iou


# ------------------------------------------------------------------------------------------
# objects in the scene (bf_objects.hip; include/boxfusion_objects.h)
# ------------------------------------------------------------------------------------------
OBJECTS_HEADER = _abi.EXTENSION_HEADERS[0]
_OC = _abi.constants(header=OBJECTS_HEADER)
OBJ_BOX_WORDS, OBJ_COUNT_WORDS, OBJ_EXTENT_WORDS, OBJ_CHUNK = (
    _OC["BF_OBJ_" + n] for n in ("BOX_WORDS", "COUNT_WORDS", "EXTENT_WORDS", "CHUNK"))
OBJ_STATS = _abi.enum_names("BF_OBJ_STAT_", header=OBJECTS_HEADER)
MAX_BOXES = _C["BF_MAX_BOXES"]


def _label_points_work(xyz, boxes16, margin=0.0, cull=None):
    n, b = int(xyz.shape[0]), int(boxes16.shape[0])
    # 21 f32 operations per point-box test; algorithmic bytes: the points once, a label each, the rows once
    return dict(kind="label_points", n=n, boxes=b), 21.0 * n * b, 16.0 * n + 4.0 * OBJ_BOX_WORDS * b


@_timed(_label_points_work)
def label_points(xyz, boxes16, margin=0.0, cull=None):
    """bf_label_points: xyz f32 [n,3], boxes16 f32 [B,16] (centre, three unit axes, half-lengths,
    volume) -> (labels int32 [n], counts int64 [B,2] = support, owned, extents int32 [B,6] holding the
    uint32 keys of min / max t_0, t_1, t_2 over the owned points, stats int64 [8] in the order of
    OBJ_STATS), allocated and initialised here; cull: None (the product's choice) or False / True
    (bf_label_points_ex, the test and benchmark hook)"""
    xyz = _need(xyz, torch.float32, "label_points: xyz").contiguous()
    boxes16 = _need(boxes16, torch.float32, "label_points: boxes16").contiguous()
    if xyz.dim() != 2 or xyz.shape[1] != 3 or boxes16.dim() != 2 or boxes16.shape[1] != OBJ_BOX_WORDS:
        raise HipError(f"label_points: xyz [n,3] and boxes16 [B,{OBJ_BOX_WORDS}], got {tuple(xyz.shape)} and "
                       f"{tuple(boxes16.shape)}")
    n, b, dev = xyz.shape[0], boxes16.shape[0], xyz.device
    if boxes16.device != dev:
        raise HipError("label_points: xyz and boxes16 on one device")
    if b > MAX_BOXES:
        raise HipError(f"label_points: {b} boxes, at most {MAX_BOXES} per call")
    labels = torch.full((n,), -1, dtype=torch.int32, device=dev)
    counts = torch.zeros((b, OBJ_COUNT_WORDS), dtype=torch.int64, device=dev)
    extents = torch.zeros((b, OBJ_EXTENT_WORDS), dtype=torch.int32, device=dev)
    extents[:, 0::2] = -1                                       # the min words: all ones
    stats = torch.zeros(STATS_WORDS, dtype=torch.int64, device=dev)
    args = (_ptr(xyz), n, _ptr(boxes16), b, float(margin), _ptr(labels), _ptr(counts), _ptr(extents), _ptr(stats))
    if cull is None:
        _check(lib().bf_label_points(*args, _stream()), "bf_label_points")
    else:
        _check(lib().bf_label_points_ex(*args, int(bool(cull)), _stream()), "bf_label_points_ex")
    return labels, counts, extents, stats


# ------------------------------------------------------------------------------------------
# levelling a scene (bf_level.hip; include/boxfusion_level.h)
# ------------------------------------------------------------------------------------------
LEVEL_HEADER = _abi.EXTENSION_HEADERS[1]
_LC = _abi.constants(header=LEVEL_HEADER)
(LEVEL_WEIGHT_CAP, LEVEL_MAX_G, LEVEL_MAX_CANDIDATES, LEVEL_MAX_HEIGHT_BINS, LEVEL_HEIGHT_WORDS, LEVEL_SUM_WORDS,
 LEVEL_NORMAL_SHIFT, LEVEL_METRE_SHIFT, LEVEL_COORD_LIMIT, LEVEL_STATS_WORDS) = (
    _LC["BF_LEVEL_" + n] for n in ("WEIGHT_CAP", "MAX_G", "MAX_CANDIDATES", "MAX_HEIGHT_BINS", "HEIGHT_WORDS", "SUM_WORDS",
                                   "NORMAL_SHIFT", "METRE_SHIFT", "COORD_LIMIT", "STATS_WORDS"))
LEVEL_STATS = _abi.enum_names("BF_LEVEL_STAT_", header=LEVEL_HEADER)


def _level_rows(t, dtype, width, name):
    t = _need(t, dtype, name).contiguous()
    if (t.dim() != 2 or t.shape[1] != width) if width else t.dim() != 1:
        raise HipError(f"{name}: {f'[n,{width}]' if width else '[n]'}, got {tuple(t.shape)}")
    return t


def _level_stats(stats, dev):
    if stats is None:
        return torch.zeros(LEVEL_STATS_WORDS, dtype=torch.int64, device=dev)
    if stats.dtype != torch.int64 or stats.numel() != LEVEL_STATS_WORDS or stats.device != dev:
        raise HipError(f"stats: int64 [{LEVEL_STATS_WORDS}] on the samples' device")
    return stats


def _level_face_samples_work(vertices, faces, area_unit, stats=None):
    m = int(faces.shape[0])
    # two differences, a cross product, a norm and three divisions, a centroid; a face reads 12 + 36 and writes 28 bytes
    return dict(kind="level_face_samples", faces=m), 40.0 * m, 76.0 * m


@_timed(_level_face_samples_work)
def level_face_samples(vertices, faces, area_unit, stats=None):
    """bf_level_face_samples: vertices f32 [n,3], faces int32 [m,3] -> (centroids f32 [m,3], unit normals
    f32 [m,3], weights int32 [m] holding uint32 = the area in units of area_unit, stats int64
    [LEVEL_STATS_WORDS] in the order of LEVEL_STATS, added to when given)"""
    vertices = _level_rows(vertices, torch.float32, 3, "level_face_samples: vertices")
    faces = _level_rows(faces, torch.int32, 3, "level_face_samples: faces")
    dev = faces.device
    if vertices.device != dev:
        raise HipError("level_face_samples: vertices and faces on one device")
    m = faces.shape[0]
    centroids = torch.empty((m, 3), dtype=torch.float32, device=dev)
    normals = torch.empty((m, 3), dtype=torch.float32, device=dev)
    weights = torch.empty((m,), dtype=torch.int32, device=dev)
    stats = _level_stats(stats, dev)
    _check(lib().bf_level_face_samples(_ptr(vertices), vertices.shape[0], _ptr(faces), m, float(area_unit), _ptr(centroids),
                                       _ptr(normals), _ptr(weights), _ptr(stats), _stream()), "bf_level_face_samples")
    return centroids, normals, weights, stats


def _level_vote_work(normals, weights, G=32, hist=None, stats=None):
    n = int(normals.shape[0])
    return dict(kind="level_vote", n=n, G=int(G)), 12.0 * n, 16.0 * n + 8.0 * 6 * G * G


@_timed(_level_vote_work)
def level_vote(normals, weights, G=32, hist=None, stats=None):
    """bf_level_vote: normals f32 [n,3], weights int32 [n] (uint32) -> (hist int64 [6 G G], stats), both
    added to when given"""
    normals = _level_rows(normals, torch.float32, 3, "level_vote: normals")
    weights = _level_rows(weights, torch.int32, 0, "level_vote: weights")
    dev, G = normals.device, int(G)
    if weights.shape[0] != normals.shape[0] or weights.device != dev:
        raise HipError("level_vote: one weight per normal, on one device")
    if not 1 <= G <= LEVEL_MAX_G:
        raise HipError(f"level_vote: G in 1..{LEVEL_MAX_G}")
    if hist is None:
        hist = torch.zeros(6 * G * G, dtype=torch.int64, device=dev)
    elif hist.dtype != torch.int64 or hist.numel() != 6 * G * G or hist.device != dev:
        raise HipError(f"level_vote: hist int64 [{6 * G * G}] on the samples' device")
    stats = _level_stats(stats, dev)
    _check(lib().bf_level_vote(_ptr(normals), _ptr(weights), normals.shape[0], G, _ptr(hist), _ptr(stats), _stream()),
           "bf_level_vote")
    return hist, stats


def _level_score_work(hist, G, candidates, cos_par, sin_perp):
    k = int(candidates.shape[0])
    return dict(kind="level_score", candidates=k, G=int(G)), 25.0 * k * 6 * G * G, 8.0 * 6 * G * G + 20.0 * k


@_timed(_level_score_work)
def level_score(hist, G, candidates, cos_par, sin_perp):
    """bf_level_score: hist int64 [6 G G], candidates int32 [k] (bin indices) -> scores int64 [k,2]: the
    weight parallel (|c.d| >= cos_par) and perpendicular (|c.d| <= sin_perp) to each candidate's centre"""
    hist = _level_rows(hist, torch.int64, 0, "level_score: hist")
    candidates = _level_rows(candidates, torch.int32, 0, "level_score: candidates")
    G, k = int(G), candidates.shape[0]
    if not 1 <= G <= LEVEL_MAX_G or hist.numel() != 6 * G * G:
        raise HipError(f"level_score: G in 1..{LEVEL_MAX_G} and hist [6 G G]")
    if k > LEVEL_MAX_CANDIDATES or candidates.device != hist.device:
        raise HipError(f"level_score: at most {LEVEL_MAX_CANDIDATES} candidates, on the histogram's device")
    scores = torch.zeros((k, 2), dtype=torch.int64, device=hist.device)
    _check(lib().bf_level_score(_ptr(hist), G, _ptr(candidates), k, float(cos_par), float(sin_perp), _ptr(scores),
                                _stream()), "bf_level_score")
    return scores


def _level_refine_work(points, normals, weights, frame, cos_par, sin_perp, h0=0.0, height_bin=1.0, n_bins=0, stats=None):
    n = int(points.shape[0])
    return dict(kind="level_refine", n=n, bins=int(n_bins)), 60.0 * n, 28.0 * n


@_timed(_level_refine_work)
def level_refine(points, normals, weights, frame, cos_par, sin_perp, h0=0.0, height_bin=1.0, n_bins=0, stats=None):
    """bf_level_refine: points, normals f32 [n,3], weights int32 [n] (uint32), frame f32 [9] = c, e1, e2 ->
    (sums int64 [LEVEL_SUM_WORDS], heights int64 [n_bins,LEVEL_HEIGHT_WORDS], stats)"""
    points = _level_rows(points, torch.float32, 3, "level_refine: points")
    normals = _level_rows(normals, torch.float32, 3, "level_refine: normals")
    weights = _level_rows(weights, torch.int32, 0, "level_refine: weights")
    frame = _need(frame, torch.float32, "level_refine: frame").contiguous()
    dev, n, n_bins = points.device, points.shape[0], int(n_bins)
    if normals.shape[0] != n or weights.shape[0] != n or frame.numel() != 9:
        raise HipError("level_refine: one normal and one weight per point, and a frame of 9 floats")
    if normals.device != dev or weights.device != dev or frame.device != dev:
        raise HipError("level_refine: every tensor on one device")
    if not 0 <= n_bins <= LEVEL_MAX_HEIGHT_BINS:
        raise HipError(f"level_refine: n_bins in 0..{LEVEL_MAX_HEIGHT_BINS}")
    sums = torch.zeros(LEVEL_SUM_WORDS, dtype=torch.int64, device=dev)
    heights = torch.zeros((n_bins, LEVEL_HEIGHT_WORDS), dtype=torch.int64, device=dev)
    stats = _level_stats(stats, dev)
    _check(lib().bf_level_refine(_ptr(points), _ptr(normals), _ptr(weights), n, _ptr(frame), float(cos_par), float(sin_perp),
                                 float(h0), float(height_bin), n_bins, _ptr(sums), _ptr(heights) if n_bins else None,
                                 _ptr(stats), _stream()), "bf_level_refine")
    return sums, heights, stats


FP8 = torch.float8_e4m3fn     # OCP e4m3 (gfx950's fp8; not the MI300 fnuz variant)
FP8_MAX = 448.0
_FP8_OUT = {torch.float32: 0, torch.bfloat16: 1, FP8: 2}


def _gemm_fp8_work(a, w, scale, bias=None, act=None, resid=None, out=None, out_dtype=torch.bfloat16,
                   out_qscale=1.0, plan=None):
    M, K = a.shape
    N = w.shape[0]
    od = out.dtype if out is not None else out_dtype
    tags = dict(kind="gemm_fp8", act=ACT[act], out=str(od), resid=resid is not None, M=M, N=N, K=K)
    nbytes = 1.0 * (M * K + N * K) + M * N * od.itemsize + (4.0 * M * N if resid is not None else 0.0)
    return tags, 2.0 * M * N * K, nbytes


@_timed(_gemm_fp8_work)
def gemm_fp8(a, w, scale, bias=None, act=None, resid=None, out=None, out_dtype=torch.bfloat16,
             out_qscale=1.0, plan=None):
    """out = resid + act(scale * (a @ w.T) + bias); a fp8 e4m3 [M,K], w fp8 [N,K] (per-tensor
    scales folded into `scale`); out f32 / bf16 / fp8 (fp8: saturate(value * out_qscale))."""
    _need(a, FP8, "a")
    _need(w, FP8, "w")
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise HipError(f"gemm_fp8: a K={K} vs w K={w.shape[1]}")
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype, device=a.device)
    if out.dtype not in _FP8_OUT:
        raise HipError("gemm_fp8 output must be f32, bf16 or fp8")
    if resid is not None:
        _need(resid, torch.float32, "resid")
    if bias is not None:
        _need(bias, torch.float32, "bias")
    if a.stride(1) != 1 or w.stride(1) != 1 or out.stride(1) != 1:
        raise HipError("gemm_fp8 operands need unit column stride")
    _check(lib().bf_gemm_fp8_plan(a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), scale,
                                  _ptr(bias) if bias is not None else None,
                                  resid.data_ptr() if resid is not None else None,
                                  resid.stride(0) if resid is not None else 0, out.data_ptr(), out.stride(0),
                                  _FP8_OUT[out.dtype], out_qscale, M, N, K, ACT[act], _plan(plan), _stream()),
           "bf_gemm_fp8")
    return out


def layernorm_fp8(x, weight, bias, eps, qscale, out=None):
    """x f32 [M, C] -> fp8 e4m3 saturate(LayerNorm(x) * qscale)"""
    _need(x, torch.float32, "x")
    M, C = x.shape
    if out is None:
        out = torch.empty((M, C), dtype=FP8, device=x.device)
    _need(out, FP8, "out")
    if x.stride(1) != 1 or out.stride(1) != 1:
        raise HipError("layernorm_fp8: unit column stride")
    _check(lib().bf_layernorm_fp8(x.data_ptr(), x.stride(0), _ptr(weight), _ptr(bias), eps,
                                  out.data_ptr(), out.stride(0), qscale, M, C, _stream()),
           "bf_layernorm_fp8")
    return out


def _f3(vals):
    return (c_float * 3)(*[float(v) for v in vals])


def im2col_rgb8(img, pad, patch, mean, std, out=None, chw=False):
    """img u8 [B,H,W,3] (chw=True: [B,3,H,W]) -> bf16 [B*(pad/patch)^2, 3*patch*patch]"""
    _need(img, torch.uint8, "img")
    if chw:
        B, _, H, W = img.shape
    else:
        B, H, W, _ = img.shape
    n = B * (pad // patch) ** 2
    if out is None:
        out = torch.empty((n, 3 * patch * patch), dtype=torch.bfloat16, device=img.device)
    _check(lib().bf_im2col_rgb8_chw(_ptr(img), B, H, W, int(chw), pad, patch, _f3(mean), _f3(std),
                                    out.data_ptr(), out.stride(0), _stream()), "bf_im2col_rgb8_chw")
    return out


def im2col_f32(x, pad, patch, out=None):
    _need(x, torch.float32, "x")
    B, H, W = x.shape
    n = B * (pad // patch) ** 2
    if out is None:
        out = torch.empty((n, patch * patch), dtype=torch.bfloat16, device=x.device)
    _check(lib().bf_im2col_f32(_ptr(x), B, H, W, pad, patch, out.data_ptr(), out.stride(0),
                               _stream()), "bf_im2col_f32")
    return out


def crop_resize_im2col(img, boxes, img_idx, size, patch, mean, std, kpad, out=None):
    """img u8 [F,H,W,3]; boxes i32 [N,4]; img_idx i32 [N] -> bf16 [N*(size/patch)^2, kpad]"""
    _need(img, torch.uint8, "img")
    F, H, W, _ = img.shape
    N = boxes.shape[0]
    if out is None:
        out = torch.empty((N * (size // patch) ** 2, kpad), dtype=torch.bfloat16,
                          device=img.device)
    _check(lib().bf_crop_resize_im2col(_ptr(img), H, W, _ptr(boxes),
                                       _ptr(img_idx) if img_idx is not None else None, N, size,
                                       patch, _f3(mean), _f3(std), out.data_ptr(), out.stride(0),
                                       _stream()), "bf_crop_resize_im2col")
    return out


class KernelTimer:
    """HIP-event timing of the MFMA tower launches (bench.py's roofline objects): while active,
    every bf_gemm_bf16 and bf_attention_bf16 launch made from Python is bracketed by two events
    on the launch stream and recorded with its algorithmic FLOPs and bytes:
      gemm       2*M*N*K FLOPs; bytes A + W + out (+ the f32 residual read)
      attention  4*Sq*Sk*D FLOPs per (batch, head); bytes Q + K + V read + O written
    `summary(pred)` aggregates the records selected by pred(tags)."""

    def __init__(self):
        self.records = []      # (tags, flops, bytes, start event, end event)
        self.active = False

    def __enter__(self):
        global _TIMER
        import threading
        self.thread = threading.get_ident()     # records launches made from this thread only
        _TIMER = self
        self.active = True
        return self

    def __exit__(self, *exc):
        global _TIMER
        _TIMER = None
        self.active = False

    def record(self, tags, flops, nbytes, fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        r = fn()
        e.record()
        self.records.append((tags, flops, nbytes, s, e))
        return r

    def summary(self, pred=lambda tags: True):
        torch.cuda.synchronize()
        sel = [r for r in self.records if pred(r[0])]
        if not sel:
            return dict(launches=0, flops=0.0, bytes=0.0, ms=0.0)
        ms = sum(s.elapsed_time(e) for _, _, _, s, e in sel)
        # work may be a callable resolved now (e.g. particle-views from the iteration counts a
        # fusion launch wrote)
        fl = sum(f() if callable(f) else f for _, f, _, _, _ in sel)
        nb = sum(b for _, _, b, _, _ in sel)
        return dict(launches=len(sel), flops=fl, bytes=nb, ms=ms, avg_us=1e3 * ms / len(sel),
                    tflops=fl / (ms * 1e-3) / 1e12, gbs=nb / (ms * 1e-3) / 1e9,
                    flops_per_launch=fl / len(sel), bytes_per_launch=nb / len(sel))


_TIMER = None


def _timer():
    """the active KernelTimer if it was entered on this thread (a fusion worker thread's
    launches are not recorded by the detect thread's timer)"""
    t = _TIMER
    if t is None:
        return None
    import threading
    return t if t.thread == threading.get_ident() else None


def new_depth_workspace(b, h, w, device):
    """a caller-owned zero-filled workspace for bf_depth_preprocess (one per concurrent user)"""
    size = int(lib().bf_depth_standardize_workspace_size(b, h, w))
    return torch.zeros(max(size, 1), dtype=torch.uint8, device=device)


# ------------------------------------------------------------------------------------------
# chip partitioning: CU-masked HIP streams (fusion on a few CUs, detection on the rest)
# ------------------------------------------------------------------------------------------
def cu_masked_stream(cus, device=None):
    """torch ExternalStream on a new HIP stream restricted to the CUs in `cus` (indices as the
    runtime enumerates them) via hipExtStreamCreateWithCUMask."""
    hip = ctypes.CDLL("libamdhip64.so")
    dev = torch.cuda.current_device() if device is None else device
    n = torch.cuda.get_device_properties(dev).multi_processor_count
    words = (ctypes.c_uint32 * ((n + 31) // 32))()
    for c in cus:
        if not 0 <= c < n:
            raise HipError(f"CU index {c} outside 0..{n - 1}")
        words[c // 32] |= 1 << (c % 32)
    s = ctypes.c_void_p()
    with torch.cuda.device(dev):
        rc = hip.hipExtStreamCreateWithCUMask(ctypes.byref(s), ctypes.c_uint32(len(words)), words)
    if rc != 0:
        raise HipError(f"hipExtStreamCreateWithCUMask failed ({rc})")
    _MASKED_STREAMS.append((dev, s.value))
    return torch.cuda.ExternalStream(s.value, device=dev)


_MASKED_STREAMS = []


def _destroy_masked_streams():
    """destroy the CU-masked streams while the HIP runtime is still up (interpreter exit, before
    the runtime's own static teardown: left to that teardown, a profiler's finalisation crashed)"""
    hip = ctypes.CDLL("libamdhip64.so")
    while _MASKED_STREAMS:
        dev, h = _MASKED_STREAMS.pop()
        with torch.cuda.device(dev):
            hip.hipStreamSynchronize(ctypes.c_void_p(h))
            hip.hipStreamDestroy(ctypes.c_void_p(h))


# Objects that hold HIP resources past their last use: fusion worker threads (which may still launch
# on a CU-masked stream) and keyframe sequencers (device buffers, a stored stream).  At interpreter
# exit they are released in dependency order while the HIP runtime is still up: workers stopped,
# then sequencers destroyed, then the masked streams.
_LIVE_WORKERS = weakref.WeakSet()
_LIVE_SEQUENCERS = weakref.WeakSet()


def register_worker(w):
    """an object with stop(timeout) that runs HIP work on a thread (fusion_stage.AsyncFusion)"""
    _LIVE_WORKERS.add(w)


def _shutdown():
    stuck = False
    for w in list(_LIVE_WORKERS):
        try:
            stuck |= w.stop(timeout=30.0) is False
        except Exception:  # noqa: BLE001 - exit path: keep releasing the rest
            pass
    if stuck:
        # a worker thread is still launching on the sequencers / masked streams: releasing them
        # now would be a use-after-free under it, so process teardown reclaims them instead
        return
    for q in list(_LIVE_SEQUENCERS):
        try:
            q.close()
        except Exception:  # noqa: BLE001
            pass
    _destroy_masked_streams()


atexit.register(_shutdown)


def partition_streams(n_reserved, device=None, masked=False):
    """(detect_stream, fusion_stream) for a rank that also runs the fusion state machine.
    The persistent GEMMs are told to leave `n_reserved` CUs free (their grid is n_cu - n_reserved
    workgroups, one per CU), so the fusion kernels always find CUs while a GEMM runs; the fusion
    stream gets high priority for the CUs that free up in between.  masked=True additionally
    confines each stream to its CUs with hipExtStreamCreateWithCUMask."""
    dev = torch.cuda.current_device() if device is None else device
    det, fus = partition_cus(n_reserved, dev)
    set_cu_budget(len(det))
    if not masked:
        return torch.cuda.current_stream(dev), torch.cuda.Stream(device=dev, priority=-1)
    return cu_masked_stream(det, dev), cu_masked_stream(fus, dev)


XCDS = 8


def cu_placement(stream, n_wg=4096, spin=20000):
    """{(xcc, se, sh, cu)} of the CUs that n_wg probe workgroups ran on when launched on `stream`
    (bf_cu_probe): what a CU mask really does on this chip"""
    out = torch.zeros(2 * n_wg, dtype=torch.int32, device=torch.device("cuda", stream.device_index))
    _check(lib().bf_cu_probe(_ptr(out), n_wg, spin, stream.cuda_stream), "bf_cu_probe")
    stream.synchronize()
    v = out.view(-1, 2).cpu().numpy()
    hw, xcc = v[:, 0], v[:, 1] & 0xF
    return {(int(x), int((h >> 13) & 7), int((h >> 12) & 1), int((h >> 8) & 0xF)) for h, x in zip(hw, xcc)}


def partition_cus(n_reserved, device=None, n_cu=None):
    """(detect CUs, fusion CUs) as CU-mask bit indices.  Mask bit i is CU i // 8 of XCD i % 8, and
    a mask that leaves an XCD without CUs is not applied at all (the stream then runs on every CU:
    measured with scripts/diag/cu_probe.py), so the fusion set takes the first n_reserved bits —
    n_reserved / 8 CUs on every XCD — and detection the rest."""
    if n_cu is None:
        dev = torch.cuda.current_device() if device is None else device
        n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    n = n_cu
    k = -(-max(1, n_reserved) // XCDS) * XCDS
    if k >= n:
        raise HipError(f"cannot reserve {n_reserved} of {n} CUs for the fusion stream")
    fus = list(range(k))
    det = list(range(k, n))
    return det, fus


# ------------------------------------------------------------------------------------------
# CuTR decoder: cross-attention position bias + clip + softmax
# ------------------------------------------------------------------------------------------
def cpb_mlp(ref, pos, axis, w1, b1, w2, out=None):
    """ref f32 [B,nq,4], pos f32 [n] -> f32 [B,nq,n,heads] (GlobalCrossAttention.rpe's MLP), written
    into `out` when a preallocated buffer of that shape is given"""
    ref = _need(ref.contiguous(), torch.float32, "ref")
    B, nq = ref.shape[0], ref.shape[1]
    heads, hidden = w2.shape
    if out is None:
        out = torch.empty((B, nq, pos.shape[0], heads), dtype=torch.float32, device=ref.device)
    _check(lib().bf_cpb_mlp(_ptr(ref), B, nq, _ptr(pos.contiguous()), pos.shape[0], axis,
                            _ptr(w1.contiguous()), _ptr(b1.contiguous()), _ptr(w2.contiguous()), hidden,
                            heads, _ptr(out), _stream()), "bf_cpb_mlp")
    return out


cpb_mlp_into = cpb_mlp      # the name decoder_engine calls it by, with `out` as the seventh argument


def xattn(q, k, v, rx, ry, hh, ww, q0, heads, scale, out=None):
    """fused global cross-attention (bf_xattn_f32): q f32 [B,Nq,C], k / v f32 [B,hh*ww,C] (any row
    stride, unit column stride), rx [B,Nq-q0,ww,heads], ry [B,Nq-q0,hh,heads] -> out f32 [B,Nq,C]"""
    for x, n in ((q, "q"), (k, "k"), (v, "v")):
        _need(x, torch.float32, n)
        if x.dim() != 3 or x.stride(2) != 1 or x.stride(0) != x.shape[1] * x.stride(1):
            raise HipError(f"xattn: {n} must be [B, rows, C] with unit column stride and packed batches")
    B, Nq, C = q.shape
    if C != heads * 32 or k.shape != (B, hh * ww, C) or v.shape != k.shape:
        raise HipError("xattn: head dim 32, k / v [B, hh*ww, C]")
    if out is None:
        out = torch.empty((B, Nq, C), dtype=torch.float32, device=q.device)
    if q0 < Nq:
        rx = _need(rx.contiguous(), torch.float32, "rx")
        ry = _need(ry.contiguous(), torch.float32, "ry")
    _check(lib().bf_xattn_f32(q.data_ptr(), q.stride(1), k.data_ptr(), k.stride(1), v.data_ptr(),
                              v.stride(1), _ptr(rx) if q0 < Nq else None,
                              _ptr(ry) if q0 < Nq else None, out.data_ptr(), out.stride(1), B, heads,
                              Nq, q0, hh, ww, scale, _stream()), "bf_xattn_f32")
    return out


def rpe_softmax(attn, rx, ry, hh, ww, q0):
    """attn f32 [B,H,Nq,hh*ww] in place: + bias on rows q >= q0, clip, softmax"""
    _need(attn, torch.float32, "attn")
    B, H, Nq, N = attn.shape
    _check(lib().bf_rpe_softmax(_ptr(attn), B, H, Nq, q0, _ptr(rx), _ptr(ry), hh, ww, _stream()),
           "bf_rpe_softmax")
    return attn


# ------------------------------------------------------------------------------------------
# CuTR decoder tail, f32 (bf_dec_native.hip + bf_self_attn_f32): thin pointer-level wrappers.
# Views with a row stride and unit column stride are accepted (the row stride is passed on).
# ------------------------------------------------------------------------------------------
def _rows(t, name, dtype=torch.float32):
    """(pointer, row stride) of a 2-D device view with unit column stride"""
    if t is None:
        return None, 0
    if not t.is_cuda:
        raise HipError("boxfusion_amd kernels need device tensors (no CPU fallback)")
    _need(t, dtype, name)
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise HipError(f"{name}: expected a 2-D view with unit column stride")
    return c_void_p(t.data_ptr()), t.stride(0)


def gemm_f32(a, w, bias=None, act=None, resid=None, out=None, a_map=None, c_map=None, m=None):
    """out[c_map[r]] = resid[c_map[r]] + act(a[a_map[r]] @ w.T + bias) for r < m (f32 MFMA);
    a_map / c_map int32 (< 0: zero row / dropped row); m defaults to len(a_map) or a.shape[0]"""
    N, K = w.shape
    M = m if m is not None else (a_map.shape[0] if a_map is not None else a.shape[0])
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    pa, lda = _rows(a, "a")
    pw, ldw = _rows(w, "w")
    pc, ldc = _rows(out, "out")
    pr, ldr = _rows(resid, "resid")
    for mp, n in ((a_map, "a_map"), (c_map, "c_map")):
        if mp is not None:
            _need(mp, torch.int32, n)
            if mp.shape[0] < M:
                raise HipError(f"gemm_f32: {n} shorter than M")
    if bias is not None:
        _need(bias, torch.float32, "bias")
    _check(lib().bf_gemm_f32(pa, lda, _ptr(a_map), pw, ldw, _ptr(bias), pr, ldr, pc, ldc, _ptr(c_map),
                             M, N, K, ACT[act], _stream()), "bf_gemm_f32")
    return out


def ln_rows(x, gamma, beta, eps, out=None, pos=None, out2=None, gelu=False):
    """out = LayerNorm(x rows) [GELU]; out2 = out + pos (optional).  C % 256 == 0, <= 1024"""
    M, C = x.shape
    if out is None:
        out = torch.empty((M, C), dtype=torch.float32, device=x.device)
    px, ldx = _rows(x, "x")
    po, ldo = _rows(out, "out")
    pp, ldp = _rows(pos, "pos")
    p2, ld2 = _rows(out2, "out2")
    _check(lib().bf_ln_rows_f32(px, ldx, _ptr(gamma), _ptr(beta), eps, po, ldo, pp, ldp, p2, ld2, M,
                                C, int(gelu), _stream()), "bf_ln_rows_f32")
    return out


def groupnorm_cl(x, frames, groups, gamma, beta, eps, out, pos=None, out2=None):
    """GroupNorm of a channel-last map x [frames*P, C] -> out (and out2 = out + pos)"""
    px, ldx = _rows(x, "x")
    po, ldo = _rows(out, "out")
    pp, ldp = _rows(pos, "pos")
    p2, ld2 = _rows(out2, "out2")
    P = x.shape[0] // frames
    _check(lib().bf_groupnorm_cl_f32(px, ldx, frames, P, x.shape[1], groups, _ptr(gamma), _ptr(beta), eps, po,
                                     ldo, pp, ldp, p2, ld2, _stream()), "bf_groupnorm_cl_f32")
    return out


def s2d(x, frames, H, W, out=None):
    """space-to-depth rows (kernel-2 stride-2 conv operand) of a channel-last map [frames*H*W, C]"""
    C = x.shape[1]
    if out is None:
        out = torch.empty((frames * (H // 2) * (W // 2), 4 * C), dtype=torch.float32, device=x.device)
    px, ldx = _rows(x, "x")
    _check(lib().bf_s2d_f32(px, ldx, frames, H, W, C, _ptr(out), _stream()), "bf_s2d_f32")
    return out


HEAD_MODES = {"class": 0, "box2d": 1, "box3d": 2, "scale": 3}


def row_heads(x, in_fs, in_off, rows, nq, w, b, mode, out=None, prop=None, params=None, boxes=None,
              clamp_wh=(0.0, 0.0), max_ratio=0.0):
    """the predictors' output linears + transforms (bf_row_heads_f32; see bf_dec_native.hip)"""
    px, ldx = _rows(x, "x")
    po, ldo = _rows(out, "out")
    _check(lib().bf_row_heads_f32(px, ldx, in_fs, in_off, rows, nq, w.shape[1], _ptr(w), _ptr(b),
                                  w.shape[0], _ptr(prop), _ptr(params), po, ldo, _ptr(boxes),
                                  clamp_wh[0], clamp_wh[1], max_ratio, HEAD_MODES[mode], _stream()),
           "bf_row_heads_f32")
    return out


def topk_rows(v, frames, n, k, ldv=1, idx=None, vals=None):
    """per-frame top-k of v[(f*n + i)*ldv] (descending, ties -> lower index): int32 idx [frames, k]"""
    if idx is None:
        idx = torch.empty((frames, k), dtype=torch.int32, device=v.device)
    _check(lib().bf_topk_rows_f32(v.data_ptr(), ldv, frames, n, k, _ptr(idx), _ptr(vals), _stream()),
           "bf_topk_rows_f32")
    return idx


def prop_select(boxes, frames, n, k, idx, ref, embs, max_e, qpos, qfs, qoff):
    """ref[f*k + j] = boxes[f*n + idx[f, j]]; qpos row f*qfs + qoff + j = the 4 box embeddings"""
    pq, ldq = _rows(qpos, "qpos")
    ex, ey, ew, eh = embs
    _check(lib().bf_prop_select_f32(_ptr(boxes), frames, n, k, _ptr(idx), _ptr(ref), _ptr(ex), _ptr(ey),
                                    _ptr(ew), _ptr(eh), ex.shape[1], max_e, pq, ldq, qfs, qoff,
                                    _stream()), "bf_prop_select_f32")


def infer_select(logits, frames, nq, nc, boxes, b3info, desc, desc_fs, desc_off, Kinv, Tg, img_wh, k, outs):
    """inference_single_image for every frame (bf_infer_select_f32); outs = dict of output buffers
    scores [F,k], classes int64 [F,k], logits [F,k,nc], boxes [F,k,4], proj [F,k,2], b3 [F,k,6],
    R [F,k,3,3], desc [F,k,C]"""
    pd, ldd = _rows(desc, "desc")
    _check(lib().bf_infer_select_f32(_ptr(logits), frames, nq, nc, _ptr(boxes), _ptr(b3info), pd, ldd,
                                     desc_fs, desc_off, desc.shape[1], _ptr(Kinv), _ptr(Tg), _ptr(img_wh),
                                     k, _ptr(outs["scores"]), _ptr(outs["classes"]), _ptr(outs["logits"]),
                                     _ptr(outs["boxes"]), _ptr(outs["proj"]), _ptr(outs["b3"]),
                                     _ptr(outs["R"]), _ptr(outs["desc"]), _stream()), "bf_infer_select_f32")


def ray_fourier(K3, W, H, feat, stride, scales, out):
    """CameraRayEmbedding's Fourier features of one camera into out [feat*feat, ld] (ld >= 3 * bands)"""
    K3 = np.asarray(K3, np.float32).reshape(3, 3)
    po, ld = _rows(out, "out")
    _check(lib().bf_ray_fourier_f32(K3[0, 0], K3[1, 1], K3[0, 2], K3[1, 2], W, H, feat, stride, _ptr(scales),
                                    scales.shape[0], po, ld, _stream()), "bf_ray_fourier_f32")
    return out


def self_attn(q, k, v, out, frames, heads, n, q0, scale):
    """decoder self-attention with the metric / box block mask (bf_self_attn_f32); q / k / v / out
    [frames*n, heads*32] row views"""
    pq, ldq = _rows(q, "q")
    pk, ldk = _rows(k, "k")
    pv, ldv = _rows(v, "v")
    po, ldo = _rows(out, "out")
    _check(lib().bf_self_attn_f32(pq, ldq, pk, ldk, pv, ldv, po, ldo, frames, heads, n, q0, scale, _stream()),
           "bf_self_attn_f32")
    return out
