cd "$(dirname "$0")/../.."
OUT=${1:?usage: tools/lab/final.sh OUTDIR}
mkdir -p "$OUT/profiles_r05"
bash tools/profile_round.sh r05 > "$OUT/profile_round.log" 2>&1; echo profile rc=$?
timeout 2400 bash tools/round_extras.sh r05 > "$OUT/round_extras.log" 2>&1; echo extras rc=$?
timeout 900 python bench.py --full > "$OUT/profiles_r05/r05_bench.json" 2> "$OUT/bench_final.err"; echo bench rc=$?
