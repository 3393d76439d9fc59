set -e
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
O=${OUT:-bench_out}  # output directory
mkdir -p $O
for cfg in c4 c2 c5; do
  timeout -k 10 300 python bench.py --full --no-cpu-baseline --config $cfg > $O/sc_${cfg}_aux.json 2> $O/sc.err
  TTAMM_SLICE_MAIN=1 timeout -k 10 300 python bench.py --full --no-cpu-baseline --config $cfg > $O/sc_${cfg}_main.json 2> $O/sc.err
done
