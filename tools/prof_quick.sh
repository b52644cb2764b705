# quick state check on the GPU box: feast parity tests, bench line, per-kernel stats
set -e
cd "$(dirname "$0")/.."
OUT=${OUT:-profile_out}; mkdir -p "$OUT"
TAG=${1:-q}
timeout -k 10 900 python -m pytest tests/test_gpu_kernels.py tests/test_gpu_properties.py -m gpu -q -x -k "feast or properties" > $OUT/${TAG}_tests.log 2>&1 || { tail -30 $OUT/${TAG}_tests.log; exit 1; }
tail -2 $OUT/${TAG}_tests.log
timeout -k 10 660 python bench.py --full --steps 20 --warmup 3 --no-cpu-baseline > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_prof -- python3 bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-roofline > $OUT/${TAG}_bench_under_rocprof.json 2> $OUT/${TAG}_prof.err
cat $OUT/${TAG}_bench.json
