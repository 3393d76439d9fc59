# C2 bench line + steady-state kernel trace (developer script)
set -e
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
O=${OUT:-bench_out}  # output directory
mkdir -p $O
timeout -k 10 300 python bench.py --full --no-cpu-baseline > $O/b_c2.json 2> $O/b_c2.err
timeout -k 10 300 python bench.py --full --no-cpu-baseline --config c5 > $O/b_c5.json 2> $O/b_c5.err
bash tools/gpu/trace_long.sh
