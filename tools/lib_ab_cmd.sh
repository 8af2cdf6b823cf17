#!/bin/bash
# Run one command under the previous (tools/probes/libmtbt_prev.so) and the current build of libmtbt_hip.so on ONE box, alternating.
# The first run that ends with a non-zero status (a failure, a fault, the time limit) ends the script with that status, the current
# library back in place: nothing more is started on a GPU that may just have faulted.
#   bash tools/lib_ab_cmd.sh python3 tools/mlp384_probe.py
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
LIB=multitask_bonetumor_yolo_amd/csrc/libmtbt_hip.so
cp $LIB /tmp/lib_new.so || exit 1
for which in prev new prev new; do
  if [ $which = prev ]; then cp tools/probes/libmtbt_prev.so $LIB; else cp /tmp/lib_new.so $LIB; fi || { cp /tmp/lib_new.so $LIB; exit 1; }
  echo "== $which"
  timeout -k 10 300 "$@" 2>&1 | grep -v amdgpu.ids
  rc=${PIPESTATUS[0]}
  if [ $rc -ne 0 ]; then
    cp /tmp/lib_new.so $LIB
    echo "== $which ended with status $rc: stopped"
    exit $rc
  fi
done
cp /tmp/lib_new.so $LIB
