"""bench.py --dump-outputs / --full: the flags (off by default), dump_outputs on host stand-ins for
the last step's DetectStage and the fusion owner (CPU), and one small plain run on the GPU that
writes its outputs and prints the headline line only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
from boxfusion_amd.boxes import GeneralInstance3DBoxes
from boxfusion_amd.instances import Instances3D

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("roofline", "roofline_components", "cpu_baseline", "decode")


def test_flags_default_off():
    a = bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert a.full is False and a.dump_outputs is None and a.steps == 3 and a.warmup == 1
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


class _Det:
    def __init__(self, B=2, n=5, crops=3, H=4, W=6):
        g = torch.Generator().manual_seed(0)
        res = []
        for _ in range(B):
            r = Instances3D((H, W))
            r.scores = torch.rand(n, generator=g)
            r.pred_boxes = torch.rand(n, 4, generator=g)
            r.pred_boxes_3d = GeneralInstance3DBoxes(torch.rand(n, 6, generator=g), torch.rand(n, 3, 3, generator=g))
            r.pred_proj_xy = torch.rand(n, 2, generator=g)
            res.append(r)
        valid = torch.rand(B, H, W, generator=g) > 0.3
        xyz = torch.rand(B, H, W, 3, generator=g)
        xyz[~valid] = float("nan")          # whatever an invalid pixel holds must not reach the file
        self.last = dict(res=res, keep=torch.rand(B, n, generator=g) > 0.5,
                         xyz=[(xyz[b], valid[b]) for b in range(B)],
                         clip=(None, None, torch.arange(B * crops), torch.rand(B * crops, 1024, generator=g),
                               torch.rand(B * crops, generator=g)))


class _Fusion:
    all_pred_box = None

    def boxes(self):
        return np.ones((3, 6), np.float32), np.ones((3, 3, 3), np.float32)


def test_dump_outputs_files(tmp_path):
    det = _Det()
    d = tmp_path / "o"
    bench.dump_outputs(str(d), det, _Fusion(), points=64)
    got = {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}
    assert set(got) == {"cutr_scores", "cutr_boxes", "cutr_boxes_3d", "cutr_R", "cutr_proj_xy", "filter_keep",
                        "clip_features", "clip_sims", "clip_class", "xyz_sample", "xyz_sample_valid",
                        "global_boxes", "global_R"}
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in got.values())
    np.testing.assert_array_equal(got["cutr_scores"], torch.stack([r.scores for r in det.last["res"]]).numpy())
    np.testing.assert_array_equal(got["cutr_R"][1], det.last["res"][1].pred_boxes_3d.R.numpy())
    np.testing.assert_array_equal(got["clip_features"], det.last["clip"][3].numpy())
    assert got["xyz_sample"].shape == (64, 3) and got["global_boxes"].shape == (3, 6)
    assert (got["xyz_sample"][got["xyz_sample_valid"] == 0] == 0).all()
    # the sample is drawn with a fixed seed: a second dump of the same outputs is the same file
    bench.dump_outputs(str(tmp_path / "p"), det, _Fusion(), points=64)
    np.testing.assert_array_equal(got["xyz_sample"], np.load(tmp_path / "p" / "xyz_sample.npy"))


@pytest.mark.gpu
def test_plain_run_dumps_and_prints_the_headline_only(tmp_path):
    """a small plain run: --steps sets the timed steps, the line carries the headline keys and none
    of the --full objects, and the dump holds finite float32 arrays of the last step (< 64 MB)"""
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, "-u", os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3",
                        "--warmup", "1", "--batch", "2", "--dim", "192", "--clip-layers", "2", "--crops", "2",
                        "--dump-outputs", str(d)], cwd=REPO, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert all(k in line for k in HEADLINE) and not any(k in line for k in FULL_ONLY), sorted(line)
    assert line["steps"] == 3 and line["config"]["frames"] == 3 * 2
    assert line["ms_per_step"] > 0 and abs(line["value"] * line["ms_per_step"] * 1e-3 - 2) < 1e-6
    got = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    assert {"cutr_scores", "cutr_boxes_3d", "clip_features", "xyz_sample", "global_boxes"} <= set(got)
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in got.values())
    assert sum(v.nbytes for v in got.values()) < 64 << 20
    assert got["cutr_scores"].shape[0] == 2 and got["clip_features"].shape == (2 * 2, 1024)
    assert len(got["global_boxes"]) == line["config"]["global_boxes"] > 0
