# round-end evidence: default bench line, rocprofv3 kernel stats of the same command, and the two PMC passes
# (FETCH_SIZE / WRITE_SIZE, each in a run of its own) behind profiles/traffic.json
set -e
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
O=${1:?usage: bash scripts/run_profile.sh OUTDIR}; mkdir -p "$O"
timeout -k 10 400 python bench.py --full > $O/final_bench.json 2> $O/final_bench.err
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $O/final_prof -o f --output-format csv -- python3 bench.py --full > $O/final_bench_under_rocprof.json 2>> $O/final_bench.err
python3 profiles/summarize_stats.py $O/final_prof/f_kernel_stats.csv 12
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE -d $O/pmc_fetch -o p --output-format csv -- python3 bench.py --full --steps 100 --warmup 300 --cpu-steps 0 > $O/pmc_fetch.json 2>> $O/final_bench.err
python3 profiles/summarize_pmc.py $O/pmc_fetch/p_counter_collection.csv k_step > $O/pmc_fetch_summary.txt
cat $O/pmc_fetch_summary.txt
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE -d $O/pmc_write -o p --output-format csv -- python3 bench.py --full --steps 100 --warmup 300 --cpu-steps 0 > $O/pmc_write.json 2>> $O/final_bench.err
python3 profiles/summarize_pmc.py $O/pmc_write/p_counter_collection.csv k_step > $O/pmc_write_summary.txt
cat $O/pmc_write_summary.txt
cat $O/final_bench.json
