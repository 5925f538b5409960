#!/bin/bash
# round-6 GPU step 2: the drop-in kernel probe, the 2-rank same-device rehearsal of the
# result gather, and the N=1 bench (every leg)
# usage: scripts/r6_run2.sh [outdir]
set -o pipefail
out=${1:-$(mktemp -d)}
mkdir -p "$out"
timeout -k 10 300 python -u scripts/dropin_kernel_probe.py > "$out/probe.log" 2>&1 || { cat "$out/probe.log"; exit 1; }
cat "$out/probe.log"
RL_BENCH_SAME_DEVICE=1 RL_BENCH_BACKEND=gloo timeout -k 10 300 python -u bench.py --gpus 2 --steps 5 --warmup 1 --full --no-extras \
  > "$out/rehearsal.log" 2>&1 || { tail -30 "$out/rehearsal.log"; exit 1; }
grep '"metric"' "$out/rehearsal.log" | python -c "import json,sys; d=json.loads(sys.stdin.read()); print(json.dumps({k: d.get(k) for k in ('n_gpus','value','ms_per_step','result_gather','parity')}))"
timeout -k 10 600 python -u bench.py --full > "$out/bench.log" 2> "$out/bench.err" || { tail -30 "$out/bench.err"; exit 1; }
tail -c 3000 "$out/bench.log"
