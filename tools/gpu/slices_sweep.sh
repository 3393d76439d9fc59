set -e
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
O=${OUT:-bench_out}  # output directory
mkdir -p $O
for n in 32 64 128 200; do
  timeout -k 10 300 python bench.py --full --no-cpu-baseline --replay-slices $n > $O/sl_$n.json 2> $O/sl.err
done
for n in 32 128; do
  timeout -k 10 300 python bench.py --full --no-cpu-baseline --config c4 --replay-slices $n > $O/sl4_$n.json 2> $O/sl.err
done
