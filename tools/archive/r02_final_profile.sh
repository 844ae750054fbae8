# round-2 final artefacts: kernel trace of the benchmark command + the full bench line (one box call)
set -x
cd "$(dirname "$0")/../.."
ROOT=$PWD
export TMPDIR=/tmp
OUT=${OUT:?set OUT to an output directory}; mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd)
rm -rf "$OUT/prof_r02f"
(cd "$TMPDIR" && rocprofv3 --kernel-trace --stats -d "$OUT/prof_r02f" -o r02f -- python "$ROOT/bench.py" --full --steps 5 --warmup 2 --cpu-baseline 0 --small-graphs 0 > "$OUT/r02f_bench_under_rocprof.json" 2> "$OUT/r02f_rocprof.err")
DB=$(find "$OUT/prof_r02f" -name '*.db' | head -1)
python profiles/summarize_rocpd.py "$DB" "round 2 (f, final tree): python bench.py --full --steps 5 --warmup 2 --cpu-baseline 0 --small-graphs 0, C5, 1x MI355X" > "$OUT/r02_f_kernel_stats.txt"
find "$OUT/prof_r02f" -name '*.db' -size +40M -delete
timeout 600 python bench.py --full > "$OUT/r02_f_bench.json" 2> "$OUT/r02_f_bench.err"
head -5 "$OUT/r02_f_kernel_stats.txt"; head -c 400 "$OUT/r02_f_bench.json"
