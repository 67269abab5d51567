#!/bin/bash
# Ablation timing of pstack_kernel: "build N..." (container) makes libcrank_hip_psabl<N>.so with -DPS_ABL=<N>; otherwise
# (GPU box) times the speaker classifier's forward + backward per variant with a kernel trace.
REPO=$(cd "$(dirname "$0")/.." && pwd)
if [ "$1" = "build" ]; then
  shift
  for n in "$@"; do
    bash $REPO/tools/build_variant.sh psabl$n pstack_kernels.hip -DPS_ABL=$n || exit 1
  done
  exit 0
fi
cd /tmp && export TMPDIR=/tmp
for n in "$@"; do
  lib=$REPO/crank_amd/libcrank_hip_psabl$n.so; [ "$n" = "0" ] && lib=$REPO/crank_amd/libcrank_hip.so
  rm -rf /tmp/psabl_$n
  CRANK_AMD_LIB=$lib rocprofv3 --kernel-trace --output-format csv -d /tmp/psabl_$n -- python $REPO/tools/prof_c.py 6 > /tmp/psabl.log 2>&1 || tail -3 /tmp/psabl.log
  echo "abl=$n"; python $REPO/tools/kstats.py /tmp/psabl_$n --by-grid | grep pstack_kernel | cut -c1-130
done
