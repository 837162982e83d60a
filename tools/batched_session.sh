set -u
OUT=${OUT:-bench_out/batched}
mkdir -p "$OUT"
timeout -k 10 300 python bench.py --full --batch 8 --variant shared --no-cpu-baseline --steps 50 --warmup 5 > "$OUT/shared_b8.log" 2>&1 && \
timeout -k 10 300 python bench.py --full --batch 32 --variant shared --no-cpu-baseline --steps 20 --warmup 3 > "$OUT/shared_b32.log" 2>&1
