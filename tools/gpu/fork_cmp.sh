set -e
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
O=${OUT:-bench_out}  # output directory
mkdir -p $O
timeout -k 10 300 python bench.py --full --no-cpu-baseline --config c5 > $O/fk_late.json 2> $O/fk.err
TTAMM_EARLY_FORK=1 timeout -k 10 300 python bench.py --full --no-cpu-baseline --config c5 > $O/fk_early.json 2> $O/fk.err
timeout -k 10 300 python bench.py --full --no-cpu-baseline --config c5 > $O/fk_late2.json 2> $O/fk.err
timeout -k 10 300 python -u -m pytest -q --timeout 200 --timeout-method thread tests/test_step_parity_gpu.py -k bf16 > $O/fk_tests.log 2>&1
