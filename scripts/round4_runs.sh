cd "$(dirname "$0")/.." && export TMPDIR=/tmp; O=${1:?usage: bash scripts/round4_runs.sh OUT_DIR}; mkdir -p $O
timeout 900 python bench.py --full > $O/07_bench_N1_default.json 2> $O/07.err
timeout 1200 python bench.py --full --steps 20 --warmup 2 > $O/06_bench_N1_steps20.json 2> $O/06.err
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -o p64 -- python3 bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --no-vit-extra --no-traffic > $O/08_bench_under_rocprof.json 2> $O/08.err
timeout 200 python scripts/config3.py > $O/09_config3_phases.txt 2>&1
(timeout 200 python scripts/vit_config2.py 32 10; timeout 200 python scripts/vit_config2.py 255 5) > $O/10_config2.txt 2>&1
timeout 300 python scripts/decode_bench.py 64 48 > $O/11_decode_bench_64.txt 2>&1
timeout 200 python scripts/attn_bench.py > $O/12_attn_bench.txt 2>&1
timeout 300 python scripts/decode_gemm_bench.py 1 2 4 8 16 > $O/03_decode_gemm_bench.txt 2>&1
ls $O $O/prof/* | head -30
