cd "$(dirname "$0")/.." && export TMPDIR=/tmp; O=${1:?usage: bash scripts/round4_final_runs.sh OUT_DIR}; mkdir -p $O
timeout 900 python bench.py --full > $O/21_bench_N1_default.json 2> $O/21.err
timeout 1200 python bench.py --full --steps 20 --warmup 2 > $O/20_bench_N1_steps20.json 2> $O/20.err
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -o p64 -- python3 bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --no-vit-extra --no-traffic > $O/22_bench_under_rocprof.json 2> $O/22.err
ls $O $O/prof/* | head -30
