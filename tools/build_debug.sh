#!/bin/bash
# Experiment builds of the two Winograd conv kernels -> tools/dbg/libfemasr_hip_<tag>.so  (FEMASR_SO=... python tools/bench_conv.py ... --wino)
#   tt       per-phase cycle stamps (-DFEMASR_WINO_TT, both Winograd kernels): bench_conv prints the per-wave cycle shares
#   <other>  the plain kernels with $EXTRA_DEFS (a one-off -D of a working copy), library tagged <other>
set -e
cd "$(dirname "$0")/.."; mkdir -p tools/dbg
F="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -Wno-unused-result"
O=femasr_amd/csrc
for tag in ${@:-tt}; do
  case $tag in tt) D="-DFEMASR_WINO_TT=1 $EXTRA_DEFS";; *) D="$EXTRA_DEFS";; esac
  /opt/rocm/bin/hipcc $F $D -c $O/kernels_wino.hip -o tools/dbg/kernels_wino_$tag.o
  /opt/rocm/bin/hipcc $F $D -c $O/kernels_wino_up2.hip -o tools/dbg/kernels_wino_up2_$tag.o
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o tools/dbg/libfemasr_hip_$tag.so $O/kernels_conv.o $O/kernels_gemm.o $O/kernels_gemm_bf16.o $O/kernels_vq.o tools/dbg/kernels_wino_$tag.o tools/dbg/kernels_wino_up2_$tag.o $O/kernels_conv_bf16.o $O/kernels_misc.o $O/model.o $O/lpips.o $O/psnr_ssim.o $O/niqe.o
done
