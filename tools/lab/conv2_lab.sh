#!/bin/bash
cd $GRAFT_REPO_ROOT; mkdir -p gpurun_out/conv2lab
o=gpurun_out/conv2lab/out.txt; : > $o
python -m pytest tests/test_gpu_gemm.py -x -q -k "im2col" 2>&1 | tail -2 >> $o
LAB_WHICH=wgrad python tools/lab/conv2_lab.py 2>&1 | grep -v amdgpu.ids >> $o
LAB_N=128 MT_WGRAD_BLOCKS_OLD=256 LAB_WHICH=wgrad python tools/lab/conv2_lab.py 2>&1 | grep -v amdgpu.ids >> $o
LAB_N=256 MT_WGRAD_BLOCKS_OLD=512 LAB_WHICH=wgrad python tools/lab/conv2_lab.py 2>&1 | grep -v amdgpu.ids >> $o
cat $o
