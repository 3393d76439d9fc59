# GPU tests, then the C2 and C5 bench lines (developer script)
set -e
cd $GRAFT_REPO_ROOT
O=${OUT:-bench_out}  # output directory
mkdir -p $O
export TMPDIR=/tmp
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $O/gt.log 2>&1
timeout -k 10 300 python bench.py --full --no-cpu-baseline > $O/b_c2.json 2> $O/b_c2.err
timeout -k 10 300 python bench.py --full --no-cpu-baseline --config c5 > $O/b_c5.json 2> $O/b_c5.err
