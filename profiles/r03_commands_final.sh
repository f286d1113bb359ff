# r03 (HEAD): rocprofv3 evidence of the driver's bench command -- kernel trace + separate PMC passes -> r03_traffic.json -> the bench
# lines of every workload; full GPU test suite
set -x
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
O=gpurun_out/r03final
rm -rf $O; mkdir -p $O
(timeout 1500 python -m pytest tests -m gpu -q 2>&1 | tail -6) > $O/gpu_tests.log
B="python bench.py --no-cpu-baseline --no-roofline"
timeout 300 rocprofv3 --kernel-trace --stats -d $O/kt -- $B --steps 7 --warmup 2 > $O/kt.log 2>&1
DB=$(find $O/kt -name "*.db" | head -1)
python profiles/summarize_rocpd.py $DB > $O/kernel_stats.txt 2>&1
python profiles/gap_report.py $DB 5 rollout_init_kernel 2 > $O/gaps.txt 2>&1
timeout 300 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $O/fetch -- $B --steps 2 --warmup 1 > $O/fetch.log 2>&1
python profiles/summarize_pmc.py $(find $O/fetch -name "*counter_collection.csv" | head -1) > $O/pmc_fetch_size.txt 2>&1
timeout 300 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $O/write -- $B --steps 2 --warmup 1 > $O/write.log 2>&1
python profiles/summarize_pmc.py $(find $O/write -name "*counter_collection.csv" | head -1) > $O/pmc_write_size.txt 2>&1
timeout 300 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_WAIT_INST_LDS SQ_ACTIVE_INST_LDS SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT --kernel-trace --output-format csv -d $O/sq -- $B --steps 1 --warmup 1 > $O/sq.log 2>&1
python profiles/summarize_pmc.py $(find $O/sq -name "*counter_collection.csv" | head -1) > $O/pmc_sq_waits.txt 2>&1
python profiles/make_traffic.py $O/pmc_fetch_size.txt $O/pmc_write_size.txt $O/kernel_stats.txt > $O/traffic.json 2>> $O/fetch.log
find $O -type f -size +1M -delete
cp $O/traffic.json profiles/r03_traffic.json          # (this run's own counters feed bench.py's `traffic` fields below)
python bench.py --full --steps 20 --warmup 5 > $O/bench_line.json 2> $O/bench.err
$B --full --workload adv > $O/bench_line_adv.json 2>> $O/bench.err
$B --full --workload adv --planner hardcode > $O/bench_line_adv_hardcode.json 2>> $O/bench.err
$B --full --scenes 1 --agents 8 --steps 20 > $O/bench_line_1x8.json 2>> $O/bench.err
$B --full --workload train --steps 10 --warmup 3 > $O/bench_line_train.json 2>> $O/bench.err
$B --full --workload sample --steps 5 > $O/bench_line_sample.json 2>> $O/bench.err
$B --full --workload sharded4096 --steps 5 > $O/bench_line_sharded4096_1gpu.json 2>> $O/bench.err
timeout 400 rocprofv3 --kernel-trace --stats -d $O/ktt -- $B --workload train --steps 3 --warmup 1 > $O/ktt.log 2>&1
DB=$(find $O/ktt -name "*.db" | head -1)
python profiles/summarize_rocpd.py $DB | head -60 > $O/train_kernel_stats.txt 2>&1
find $O -type f -size +1M -delete
tail -c 300 $O/bench_line.json
