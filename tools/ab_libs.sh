#!/bin/bash
# Same-box A/B of two builds of libtinyrt.so on the three bench scenes: tools/ab_libs.sh <libA> <libB> [reps]
# (TRT_LIB_PATH picks the build; kernel time only: no CPU leg, no roofline pass.)  Every run has its own time limit, and the first run
# that fails ends the script: nothing more is started on a device that has just faulted or hung.
set -o pipefail
A=$1; B=$2; reps=${3:-3}
run() {
  local line
  line=$(TRT_LIB_PATH=$1 timeout -k 10 300 python3 bench.py --cpu-seconds 0 --no-roofline-pass "${@:2}" 2>/dev/null | tail -1) || return 1
  python3 -c "import sys,json; d=json.loads(sys.argv[1]); print('%9.1f' % d['value'])" "$line"
}
C="--steps 20 --warmup 3"
R="--scene random_spheres --width 1920 --height 1080 --spp-per-step 64 --steps 3 --warmup 1"
G="--scene sphere_grid --width 3840 --height 2160 --spp-per-step 16 --steps 2 --warmup 1"
for rep in $(seq $reps); do
  for lib in $A $B; do
    c=$(run $lib $C) && r=$(run $lib $R) && g=$(run $lib $G) || { echo "$(basename $lib): a run failed - stopping"; exit 1; }
    echo "$(basename $lib): cornell $c  random_spheres $r  sphere_grid $g"
  done
done
