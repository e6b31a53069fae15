#!/bin/bash
# The non-headline bench lines at HEAD (configs[3] RIF multi-tau, Heckman, configs[4] Machado-Mata),
# one after another, each under its own time limit, Heckman and MM with their CPU baselines (--full).
# -> $OUT/TAG_{rif3,heckman,mm}.json (OUT defaults to bench_out)
set -o pipefail
cd "$(dirname "$0")/.."
O=${OUT:-bench_out}; mkdir -p "$O"
TAG=${1:-side}
timeout -k 10 300 python bench.py --taus 0.1,0.5,0.9 --reps 5000 > $O/${TAG}_rif3.json 2> $O/${TAG}_rif3.err || exit $?
tail -c 600 $O/${TAG}_rif3.json; echo
timeout -k 10 300 python bench.py --full --heckman > $O/${TAG}_heckman.json 2> $O/${TAG}_heckman.err || exit $?
tail -c 600 $O/${TAG}_heckman.json; echo
timeout -k 10 400 python bench.py --full --mm > $O/${TAG}_mm.json 2> $O/${TAG}_mm.err || exit $?
tail -c 600 $O/${TAG}_mm.json; echo
