set -e
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
O=${OUT:-bench_out}  # output directory
mkdir -p $O
timeout -k 10 300 python bench.py --full --no-cpu-baseline --config c4 > $O/b_c4.json 2> $O/b_c4.err
timeout -k 10 600 python -u -m pytest -q --timeout 300 --timeout-method thread tests/test_fullsize_gpu.py > $O/fullsize.log 2>&1
