# all GPU tests, the C2 / C5 bench lines, the bf16 GEMM micro-benchmark (developer script)
set -e
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
O=${OUT:-bench_out}  # output directory
mkdir -p $O
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $O/gt.log 2>&1
timeout -k 10 300 python bench.py --full --no-cpu-baseline > $O/b_c2.json 2> $O/b_c2.err
timeout -k 10 300 python bench.py --full --no-cpu-baseline --config c5 > $O/b_c5.json 2> $O/b_c5.err
timeout -k 10 60 two-tower-augmented-with-adaptive-mimic-mechanism_amd/build/gemm_bench_bf16 > $O/gb16.txt 2>&1
