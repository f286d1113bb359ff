set -x
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
O=${OUT:-prof_out}; mkdir -p $O
timeout 600 python -m pytest tests -m gpu -q 2>&1 | tail -5 > $O/gpu_tests.log
timeout 600 python bench.py --full > $O/bench_final.log 2>&1
rm -rf $O/prof_kt $O/prof_fetch $O/prof_write
timeout 400 rocprofv3 --kernel-trace --stats -d $O/prof_kt -- python bench.py --steps 5 --warmup 2 > $O/prof_kt.log 2>&1
DB=$(find $O/prof_kt -name "*.db" | head -1)
python profiles/summarize_rocpd.py $DB > $O/kernel_stats.txt 2>&1
timeout 400 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $O/prof_fetch -- python bench.py --steps 2 --warmup 1 > $O/prof_fetch.log 2>&1
F=$(find $O/prof_fetch -name "*counter_collection.csv" | head -1)
python profiles/summarize_pmc.py $F > $O/pmc_fetch.txt 2>&1
timeout 400 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $O/prof_write -- python bench.py --steps 2 --warmup 1 > $O/prof_write.log 2>&1
F=$(find $O/prof_write -name "*counter_collection.csv" | head -1)
python profiles/summarize_pmc.py $F > $O/pmc_write.txt 2>&1
find $O/prof_kt $O/prof_fetch $O/prof_write -type f -size +2M -delete
