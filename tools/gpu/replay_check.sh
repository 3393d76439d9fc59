set -e
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
O=${OUT:-bench_out}  # output directory
mkdir -p $O
timeout -k 10 600 python -u -m pytest -q --timeout 200 --timeout-method thread tests/test_deferred_gpu.py tests/test_fullsize_gpu.py tests/test_c1_gpu.py > $O/replay.log 2>&1
for cfg in c2 c4 c5; do
  timeout -k 10 300 python bench.py --full --no-cpu-baseline --config $cfg > $O/rp_${cfg}.json 2> $O/rp.err
done
