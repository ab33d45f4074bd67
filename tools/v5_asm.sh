#!/bin/bash
# dev tool (CPU): the gfx950 assembly of smx_agg_v5.hip with the product flags + -DSMX_V5_MARK + extra flags -> $1
# usage: tools/v5_asm.sh out.s [-Dflags...]        V5_ASM_MARK=0 in the environment: without the mark flag (the product's code)
# The 25 s compile is kept under _build/v5_asm/, keyed by the hash of the sources, this script, the compiler and the flags, so
# that the ISA lints (dpp_hazard_check.py, v5_handoff_check.py) and their tests share one compile per build.
# (tools/v5_handoff_check.py parses the hipcc line below and holds its flags against CXXFLAGS of csrc/Makefile)
set -e
ROOT=$(cd $(dirname $0)/.. && pwd); OUT=$(realpath $1); shift
MARK=-DSMX_V5_MARK; if [ "${V5_ASM_MARK:-1}" = 0 ]; then MARK=; fi
CSRC=$ROOT/stereo_matching_cuda_amd/csrc
KEY=$( (cat $CSRC/smx_agg_v5.hip $CSRC/*.h $ROOT/include/*.h $0; /opt/rocm/bin/hipcc --version; echo "$MARK" "$@") 2>&1 | sha256sum | cut -c1-32)
CACHE=$ROOT/stereo_matching_cuda_amd/_build/v5_asm
if [ -s $CACHE/$KEY.s ]; then cp $CACHE/$KEY.s $OUT; exit 0; fi
T=$(mktemp -d); cd $T
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -fno-fast-math \
  -fno-slp-vectorize -mllvm -amdgpu-atomic-optimizer-strategy=None -fvisibility=hidden $MARK "$@" -I$ROOT/include \
  --save-temps -c $CSRC/smx_agg_v5.hip -o x.o >/dev/null 2>&1
cp smx_agg_v5-hip-amdgcn-amd-amdhsa-gfx950.s $OUT
# (a tree that cannot be written to is no error: the next call compiles again)
if mkdir -p $CACHE 2>/dev/null && cp $OUT $CACHE/$KEY.tmp$$ 2>/dev/null; then mv $CACHE/$KEY.tmp$$ $CACHE/$KEY.s; fi
cd /; rm -rf $T
