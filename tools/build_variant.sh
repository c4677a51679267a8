#!/bin/bash
# Experiment builds of the fused candidate kernel: tools/build_variant.sh NAME [QM] [-DFLAG ...]
#   -> build/lib_NAME.so = the shipped objects (make them first) with the 8- and 10-bit slice QM of
#      rdo_cand_slice.hip recompiled with the flags, the two in parallel.  Without QM: slice 0 with the
#      headline sizes only (-DR1_HEADLINE_ONLY), well under a minute; QM = 2 with all sizes takes a few minutes.
# A/B on one GPU box: bash tools/gpu_lease.sh TAG bench_ab:build/lib_A.so,build/lib_B.so
set -e
NAME=$1; shift
case "$1" in [0-4]) QM=$1; shift ;; *) QM=0; set -- -DR1_HEADLINE_ONLY "$@" ;; esac
cd "$(dirname "$0")/../rav1e_amd/csrc"
mkdir -p ../../build
HIPCC=/opt/rocm/bin/hipcc
FLAGS=$(make -s flags)
for b in 8 10; do
  # the 8-bit coefficient slice is built with its MFMA results in VGPRs (MFMA_VGPR, csrc/Makefile)
  MX=""; [ "$b$QM" = 80 ] && MX="-mllvm -amdgpu-mfma-vgpr-form"
  $HIPCC $FLAGS $MX -DR1_RDO_TU_BD=$b -DR1_RDO_TU_QM=$QM "$@" -c rdo_cand_slice.hip -o ../../build/rdo_cand_b${b}_q${QM}_$NAME.o &
done
wait
OBJS=$(ls *.o | grep -v "^rdo_cand_b8_q${QM}.o\|^rdo_cand_b10_q${QM}.o\|_prof.o$")
$HIPCC --offload-arch=gfx950 -shared -fPIC -o ../../build/lib_$NAME.so $OBJS ../../build/rdo_cand_b8_q${QM}_$NAME.o ../../build/rdo_cand_b10_q${QM}_$NAME.o -ldl
ls -la ../../build/lib_$NAME.so
