#!/bin/bash
# Builds the diagnostic probes (tools/duoprobe.cpp: plain and -DCOG_STAMPS) and the lone-wave
# instruction-cost probe (tools/chainprobe.hip) into tools/bin/ (git-ignored; they travel to the
# GPU box with the tree while present).
set -e
cd "$(dirname "$0")/.."
mkdir -p tools/bin
F="-w -O3 -std=c++17 -ffp-contract=off -mllvm -amdgpu-sched-strategy=max-ilp -falign-loops=64 -Iinclude -Igym-eldorado_amd/csrc"
# (cog_policy.hip: the ABI that duoprobe.cpp includes links the policy kernels' launchers)
P=gym-eldorado_amd/csrc/cog_policy.hip
/opt/rocm/bin/hipcc --offload-arch=gfx950 $F tools/duoprobe.cpp $P -o tools/bin/duoprobe &
a=$!
/opt/rocm/bin/hipcc --offload-arch=gfx950 $F -DCOG_STAMPS tools/duoprobe.cpp $P -o tools/bin/duoprobe_st &
b=$!
wait $a
wait $b
/opt/rocm/bin/hipcc --offload-arch=gfx950 -w -O3 tools/chainprobe.hip -o tools/bin/chainprobe
