cd "$(dirname "$0")/.." && export TMPDIR=/tmp; O=${1:?usage: bash scripts/round5_final_runs.sh OUT_DIR}; mkdir -p $O
timeout 1500 python -m pytest tests -x -q -m gpu > $O/20_final_pytest_gpu.txt 2>&1; tail -4 $O/20_final_pytest_gpu.txt
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/20_final_smoke.txt 2>&1; tail -3 $O/20_final_smoke.txt
timeout 1200 python bench.py --full > $O/21_bench_N1_default.json 2> $O/21.err; tail -c 300 $O/21.err
timeout 1500 python bench.py --full --steps 20 --warmup 2 --no-traffic > $O/22_bench_N1_steps20.json 2> $O/22.err
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -o p64 -- python3 bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --no-vit-extra --no-traffic --no-strong-share > $O/23_bench_under_rocprof.json 2> $O/23.err
ROWS=1,2,4,8,16,32,64 STEPS=48 timeout 600 python scripts/decode_rows.py child > $O/24_final_decode_rows.txt 2>&1
timeout 600 python scripts/config3.py > $O/25_config3_phases.txt 2>&1; tail -2 $O/25_config3_phases.txt
ls $O $O/prof | head -30
