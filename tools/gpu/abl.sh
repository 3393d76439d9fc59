set -e
cd $GRAFT_REPO_ROOT
O=${OUT:-bench_out}  # output directory
mkdir -p $O
for v in 0 1 2; do
  if [ $v = 0 ]; then export -n TTAMM_LIBRARY; unset TTAMM_LIBRARY; else export TTAMM_LIBRARY=$PWD/tools/gpu/libttamm_abl$v.so; fi
  timeout -k 10 200 python bench.py --full --no-cpu-baseline --config c5 --steps 10 --warmup 3 > $O/abl_$v.json 2> $O/abl_$v.err
done
