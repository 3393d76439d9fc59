# rocprofv3 kernel stats of short bench runs of the given configs (developer script)
# usage: bash tools/gpu/stats_cfg.sh c5 c4 ...
set -e
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
O=${OUT:-bench_out}  # output directory
mkdir -p $O
for cfg in "$@"; do
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/st_$cfg -o run -- python3 bench.py --full --no-cpu-baseline --config $cfg --steps 30 --warmup 3 > $O/st_${cfg}_bench.json 2> $O/st_${cfg}.err
  find $O/st_$cfg -name "*kernel_stats.csv" -exec cp {} $O/st_${cfg}_kernel_stats.csv \;
  rm -rf $O/st_$cfg
done
