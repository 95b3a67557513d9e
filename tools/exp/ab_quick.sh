#!/bin/bash
# one library, three workloads: step and the kernels named on the command line.  usage: tools/exp/ab_quick.sh k_call_sites k_call_paths ...
R=$(cd "$(dirname "$0")/../.." && pwd); cd $R
O=${PF_OUT:-$R/bench_out}; mkdir -p "$O"
for wl in "--workload stress" "--workload stress --unitigs 1000000" ""; do
  python bench.py $wl --full --no-cpu --steps 8 > "$O/abq.json" 2> "$O/abq.log"
  python3 - "$O/abq.json" "$wl" "$@" <<'PY'
import json, sys
d = json.loads(open(sys.argv.pop(1)).read().strip().splitlines()[-1])
ks = " ".join("%s %.3f x%g" % (k, d['kernels'][k]['avg_ms'], d['kernels'][k]['launches_per_step']) for k in sys.argv[2:] if k in d['kernels'])
print((sys.argv[1] or 'default').ljust(40), 'step', d['ms_per_step'], 'median', d['ms_per_step_median'], 'excl', d['ms_per_step_excl_join'], 'align_s', d['host_phases_s_per_step']['align_s'], '|', ks, '| ok', d['output_check'].get('identical_to_reference'))
PY
done
