#!/bin/bash
# Diagnostic build of libboxfusion_hip.so that sends the refinement's hull IoU with more than 4
# candidates down its scratch fallback (iou_hull_pre).  The GPU tests run against it with
#   BF_LIB_PATH=boxfusion_amd/_build/diag/libboxfusion_hip_diag.so pytest tests/test_gpu_fusion.py
# to show that the fallback gives the same results as the LDS path.
set -e
cd "$(dirname "$0")/../boxfusion_amd/_build"
python3 -c "import sys; sys.path.insert(0, '../..'); from boxfusion_amd import build; build.build()"
mkdir -p diag
FL="--offload-arch=gfx950 -O3 -fPIC -std=c++17 -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -I../../include -Wno-unused-result"
/opt/rocm/bin/hipcc $FL -DFAST_CAND=4 -c ../csrc/bf_fusion.hip -o diag/bf_fusion.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o diag/libboxfusion_hip_diag.so \
    $(ls *.o | grep -v -e "^bf_fusion.o$") diag/bf_fusion.o
echo "$PWD/diag/libboxfusion_hip_diag.so"
