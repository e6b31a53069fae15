#!/bin/bash
# Round 5 check on one box: the GPU suite, the default bench with every leg (--full) and configs[2]'s
# per-GPU share. Output under $OUT (default bench_out). usage: bash tools/gpu_r5_check.sh TAG
set -o pipefail
cd "$(dirname "$0")/.."
O=${OUT:-bench_out}; mkdir -p "$O"
T=${1:-r5c}
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread -p no:cacheprovider \
  > $O/${T}_gputests.txt 2>&1 || { tail -40 $O/${T}_gputests.txt; exit 1; }
tail -1 $O/${T}_gputests.txt
timeout -k 10 400 python bench.py --full --steps 20 --warmup 5 > $O/${T}_bench.json 2> $O/${T}_bench.err \
  || { tail -30 $O/${T}_bench.err; exit 1; }
python -c "import json;d=json.loads(open('$O/${T}_bench.json').read().strip().splitlines()[-1]);print(round(d['value']),round(d['roofline']['frac'],3),{k:round(v,3) for k,v in d['breakdown_ms_per_step_rank0'].items()}, d['cpu_baseline']['value'])"
timeout -k 10 400 python bench.py --reps 1250 --steps 20 --warmup 5 --cpu-seconds 0 --no-e2e \
  > $O/${T}_share1250.json 2> $O/${T}_share1250.err || { tail -30 $O/${T}_share1250.err; exit 1; }
python -c "import json;d=json.loads(open('$O/${T}_share1250.json').read().strip().splitlines()[-1]);print('share1250',round(d['value']),{k:round(v,3) for k,v in d['breakdown_ms_per_step_rank0'].items()})"
