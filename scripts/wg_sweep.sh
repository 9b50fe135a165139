#!/bin/bash
# wavefronts per workgroup of the per-tick lane-group kernels, per shape (tick_wpg() in csrc/ismpc_b_group.hpp): variants go to
# build/variants/ (ISMPC_LIB), never in-tree.  The libraries are loaded alternately, ROUNDS times each, one bench.py process per run.
# usage: scripts/wg_sweep.sh build            (here, no GPU)
#        scripts/wg_sweep.sh run [leg ...]    (GPU box; default: the legs that take an 8-lane shape, then two that do not, as a control)
set -e
cd "$(dirname "$0")/.."
mkdir -p build/variants
VARIANTS=("8lane1:-DISMPC_WPG_8LANE=1" "8lane2:-DISMPC_WPG_8LANE=2" "8lane4:-DISMPC_WPG_8LANE=4" "16lane1:-DISMPC_WPG_16LANE=1" "16lane2:-DISMPC_WPG_16LANE=2")
ROUNDS=${ROUNDS:-5}
if [ "$1" = build ]; then
  for v in "${VARIANTS[@]}"; do
    python -c "from quadruped_gait_generation_ismpc_amd import build; build.build(out='build/variants/libismpc_wpg_${v%%:*}.so', flags='${v#*:}')"
  done; ls -la build/variants; exit 0
fi
shift || true
LEGS=${@:-headline shard_b32768 shard_b16384 sweep_k64_b65536 shard_b8192 config1_b1024}
: > build/variants/wg_sweep.log
for leg in $LEGS; do for r in $(seq $ROUNDS); do
  for n in default "${VARIANTS[@]}"; do n=${n%%:*}
    lib=$PWD/build/variants/libismpc_wpg_$n.so; [ $n = default ] && lib=""
    echo "$leg run $r $n $(ISMPC_LIB=$lib timeout -k 10 200 python bench.py --only $leg --no-cpu-baseline --no-extras --min-region-ms 20 | python -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('%.4e' % d['value'], 'kernel_ms', d['roofline']['kernel_ms'])")" | tee -a build/variants/wg_sweep.log
  done
done; done
