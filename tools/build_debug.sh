#!/bin/bash
# Experiment builds of the two Winograd conv kernels -> tools/dbg/libfemasr_hip_<tag>.so  (FEMASR_SO=... python tools/bench_conv.py ... --wino)
#   tt       per-phase cycle stamps (-DFEMASR_WINO_TT, both Winograd kernels): bench_conv prints the per-wave cycle shares
#   <other>  the plain kernels with $EXTRA_DEFS (a one-off -D of a working copy), library tagged <other>
# Sources and flags are those of femasr_amd/csrc/build.py; every other object is the one the regular build left there.
set -e
cd "$(dirname "$0")/.."; mkdir -p tools/dbg
O=femasr_amd/csrc
F=$(python3 -c "import sys; sys.path.insert(0, '$O'); import build; print(' '.join(build.FLAGS))")
OBJS=$(python3 -c "import sys; sys.path.insert(0, '$O'); import build; print(' '.join(s[:-4] for s in build.SOURCES if not s.startswith('kernels_wino')))")
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
for tag in ${@:-tt}; do
  case $tag in tt) D="-DFEMASR_WINO_TT=1 $EXTRA_DEFS";; *) D="$EXTRA_DEFS";; esac
  $HIPCC $F $D -c $O/kernels_wino.hip -o tools/dbg/kernels_wino_$tag.o
  $HIPCC $F $D -c $O/kernels_wino_up2.hip -o tools/dbg/kernels_wino_up2_$tag.o
  $HIPCC --offload-arch=gfx950 -shared -fPIC -o tools/dbg/libfemasr_hip_$tag.so $(for o in $OBJS; do echo $O/$o.o; done) tools/dbg/kernels_wino_$tag.o tools/dbg/kernels_wino_up2_$tag.o
done
