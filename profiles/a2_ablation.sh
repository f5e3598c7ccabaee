#!/bin/bash
# What each part of stage A2 (cape_cell_plane_kernel) costs: one library per ablated part (results wrong by construction,
# timing only), the default bench workload, A2's mean launch time from the handle's HIP events.
# build (CPU box):  profiles/a2_ablation.sh build      run (GPU box): profiles/a2_ablation.sh run
set -e
ROOT="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
if [ "$1" = build ]; then
  for a in 1 2 4 8 15; do "$ROOT/profiles/build_variant.sh" a2abl$a -DCAPE_A2_ABLATE=$a | tail -1; done
  exit 0
fi
cd "$ROOT"
one() { env "$@" python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-parity-check --no-cylinders-on 2>/dev/null | python -c "import json,sys; k=json.loads(sys.stdin.read())['roofline']['kernel_ms']; print('A1 %.3f  A2 %.3f  B %.3f ms' % (k['cape_cell_moments_kernel'], k['cape_cell_plane_kernel'], k['cape_grow_kernel']))"; }
echo -n "full kernel                          "; one A=1
echo -n "without fit_plane (eigen-solver)     "; one CAPE_HIP_LIB=rgb-d-slam_amd/lib/exp/libcape_a2abl1.so
echo -n "without acos / atan2 (histogram bin) "; one CAPE_HIP_LIB=rgb-d-slam_amd/lib/exp/libcape_a2abl2.so
echo -n "without the four edge predicates     "; one CAPE_HIP_LIB=rgb-d-slam_amd/lib/exp/libcape_a2abl4.so
echo -n "without the merge tolerance          "; one CAPE_HIP_LIB=rgb-d-slam_amd/lib/exp/libcape_a2abl8.so
echo -n "loads + gates + stores only          "; one CAPE_HIP_LIB=rgb-d-slam_amd/lib/exp/libcape_a2abl15.so
