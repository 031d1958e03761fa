#!/bin/bash
# The commands behind profiles/rNN_*: run on the GPU box from the repo root as `bash tools/profile_round.sh rNN [OUT]`;
# everything lands in OUT (default tools/_run/rNN); copy what is to be kept into profiles/.
#   rNN_gputest_final.txt      python -m pytest tests -m gpu
#   rNN_bench_kernel_stats.txt rocprofv3 --kernel-trace --stats over a short bench.py --full run (per-kernel average durations)
#   pmc_dominant.json          separate --pmc passes (FETCH_SIZE, WRITE_SIZE) over tools/pmc_head.py -> HBM bytes of the dominant kernel
#   rNN_pmc_mfma_busy.txt      --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE over the same command -> matrix-pipe busy fraction
#   rNN_bench_line.json        the full bench line, python bench.py --full --steps 20 --warmup 5
# (PMC passes carry --kernel-trace only: counters are collected in runs of their own, without the other trace domains)
set -u
TAG=${1:-r06}
R=${GRAFT_REPO_ROOT:-$PWD}
OUT=$(realpath -m "${2:-$R/tools/_run/$TAG}")
mkdir -p $OUT
cd $R
python -m pytest tests -m gpu -x -q > $OUT/${TAG}_gputest_final.txt 2>&1; tail -2 $OUT/${TAG}_gputest_final.txt
python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.txt 2>&1; tail -1 $OUT/${TAG}_smoke.txt
export PYTHONPATH=$R
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o $TAG -- python $R/bench.py --full --steps 6 --warmup 2 --no-cpu-baseline --no-extras --no-configs > $OUT/${TAG}_prof_bench.log 2>&1
cd $R; DB=$(find $OUT/prof_$TAG -name "*_results.db" | head -1); python tools/rocpd_summary.py $DB > $OUT/${TAG}_bench_kernel_stats.txt 2>&1; rm -rf $OUT/prof_$TAG
cd /tmp
rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $OUT/pmc_fetch -o p --output-format csv -- python $R/tools/pmc_head.py > $OUT/${TAG}_pmc_fetch.log 2>&1
rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $OUT/pmc_write -o p --output-format csv -- python $R/tools/pmc_head.py > $OUT/${TAG}_pmc_write.log 2>&1
rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_BUSY_CYCLES -d $OUT/pmc_busy -o p --output-format csv -- python $R/tools/pmc_head.py > $OUT/${TAG}_pmc_busy.log 2>&1
cd $R
python tools/pmc_traffic.py $OUT/pmc_fetch $OUT/pmc_write --commit "$(cat tools/_run/HEAD 2>/dev/null || echo $TAG)" > $OUT/${TAG}_pmc_traffic.txt 2>&1
cp profiles/pmc_dominant.json $OUT/pmc_dominant.json
python tools/pmc_busy.py $OUT/pmc_busy > $OUT/${TAG}_pmc_mfma_busy.txt 2>&1
rm -rf $OUT/pmc_fetch $OUT/pmc_write $OUT/pmc_busy
python bench.py --full --steps 20 --warmup 5 > $OUT/${TAG}_bench_line.json 2> $OUT/${TAG}_bench_line.err
tail -c 200 $OUT/${TAG}_bench_line.err
