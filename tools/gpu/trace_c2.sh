set -e
cd $GRAFT_REPO_ROOT
O=${OUT:-bench_out}  # output directory
mkdir -p $O
export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d $O/trace_c2 -o run -- python3 bench.py --full --no-cpu-baseline --steps 10 --warmup 3 $BENCH_ARGS > $O/trace_c2_bench.json 2> $O/trace_c2.err
find $O/trace_c2 -name "*kernel_trace.csv" -exec cp {} $O/trace_c2_kernels.csv \;
rm -rf $O/trace_c2
