#!/bin/bash
# ISA of one translation unit with source lines attached (for tools/isa_budget.py): tools/isa_dump.sh nn_grid [extra -D flags]  ->  $ISA_DIR/<unit>.s
# (ISA_DIR defaults to /tmp/mislam_isa)
u=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
d=${ISA_DIR:-/tmp/mislam_isa}
mkdir -p $d/$u && cd $d/$u || exit 1
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -gline-tables-only -w -I/opt/rocm/include -I$root/cuda-slam_amd/csrc -I$root/include "$@" \
    --save-temps -c $root/cuda-slam_amd/csrc/$u.hip -o $d/$u/$u.o 2>/dev/null
cp $d/$u/$u-hip-amdgcn-amd-amdhsa-gfx950.s $d/$u.s && echo $d/$u.s
