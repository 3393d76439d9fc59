# FETCH_SIZE / WRITE_SIZE passes + a bench line (developer script)
set -e
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
O=${OUT:-bench_out}  # output directory
mkdir -p $O
run_pass() {
    local name=$1; shift
    timeout -s KILL 240 rocprofv3 --pmc "$@" --output-format csv -d $O/pmc_$name -o run -- python3 bench.py --full --no-cpu-baseline --steps 40 --warmup 3 $BENCH_ARGS > $O/pmc_${name}_bench.json 2> $O/pmc_${name}.err
    find $O/pmc_$name -name "*counter_collection.csv" -exec cp {} $O/pmc_${name}.csv \;
    rm -rf $O/pmc_$name
}
run_pass fetch FETCH_SIZE
run_pass write WRITE_SIZE
timeout -k 10 300 python bench.py --full --no-cpu-baseline > $O/b_c2.json 2> $O/b_c2.err
