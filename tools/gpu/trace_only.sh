set -e
cd $GRAFT_REPO_ROOT
O=${OUT:-bench_out}  # output directory
mkdir -p $O
export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d $O/trace_x -o run -- python3 bench.py --full --no-cpu-baseline --steps 10 --warmup 3 $BENCH_ARGS > $O/trace_x_bench.json 2> $O/trace_x.err
find $O/trace_x -name "*kernel_trace.csv" -exec cp {} $O/trace_x_kernels.csv \;
rm -rf $O/trace_x
