TAG=${1:-r05}
OUT=${2:?directory the lines are written to}
set -o pipefail
mkdir -p "$OUT"
# full lines (bench.py --full): what profiles/ keeps quotes the CPU baselines, the oracle's parity, the steady state and the accounting legs
python bench.py --full > $OUT/${TAG}_bench_line.json 2> $OUT/${TAG}_bench_line.err
for w in ecsample30x-like hifi-half dense-repeats-25th dense-repeats-8th hifi-k31; do
  python bench.py --full --workload $w --steps 10 --warmup 2 --no-cpu-full > $OUT/${TAG}_bench_line_$w.json 2> $OUT/${TAG}_bench_line_$w.err
done
