# kernel trace of a steady-state C2 run (120 timed steps; developer script)
set -e
cd $GRAFT_REPO_ROOT
O=${OUT:-bench_out}  # output directory
mkdir -p $O
export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d $O/trace_l -o run -- python3 bench.py --full --no-cpu-baseline --steps 120 --warmup 3 $BENCH_ARGS > $O/trace_l_bench.json 2> $O/trace_l.err
find $O/trace_l -name "*kernel_trace.csv" -exec cp {} $O/trace_l_kernels.csv \;
rm -rf $O/trace_l
