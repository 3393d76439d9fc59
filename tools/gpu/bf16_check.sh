set -e
cd $GRAFT_REPO_ROOT
O=${OUT:-bench_out}  # output directory
mkdir -p $O
timeout -k 10 300 python -u -m pytest tests/test_step_parity_gpu.py -m gpu -q -k bf16 --timeout 200 --timeout-method thread > $O/tb.log 2>&1
timeout -k 10 300 python bench.py --full --no-cpu-baseline --config c5 > $O/b_c5.json 2> $O/b_c5.err
