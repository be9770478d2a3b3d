# Pipelined C3 bench over CU partitions between the front half and the walkers (SG_FRONT_SIXTEENTHS).
# Logs go to $OUT (default build/sweep_logs).
OUT=${OUT:-build/sweep_logs}
mkdir -p "$OUT"
for k in ${SWEEP:-0 4 6 8}; do
  SG_FRONT_SIXTEENTHS=$k timeout -k 10 200 python -u bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --e2e-batches 0 > "$OUT/front_$k.log" 2>&1 || exit 1
  python -c "import json,sys; d=json.loads(open('$OUT/front_$k.log').read().strip().splitlines()[-1]); print($k, round(d['ms_per_step'],4), d['phases_ms'])"
done
