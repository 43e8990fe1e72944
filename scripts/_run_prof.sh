# headline profile set: kernel stats, SQ PMC pass, FETCH / WRITE passes (separate passes, as the guide prescribes),
# then the summaries the bench line reads (profiles/current_*.json are copies of <TAG>_pmc.json / <TAG>_traffic.json)
#   CVHIP_GIT_HEAD=<hash> PROF_OUT=<dir> bash scripts/_run_prof.sh r03      (results in PROF_OUT, default prof_out/)
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
TAG=${1:-r03}
O=${PROF_OUT:-prof_out}
mkdir -p $O
# --full: the runs keep the instrumented step after the timed one that the collectors count
B="python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-extras --no-count-step"
rocprofv3 --kernel-trace --stats -d $O/${TAG}_stats -o s --output-format csv -- python3 bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-extras > $O/${TAG}_stats.log 2>&1
rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_ACTIVE_INST_VALU SQ_WAIT_ANY SQ_ACTIVE_INST_ANY GRBM_GUI_ACTIVE -d $O/${TAG}_pmcS -o q --output-format csv -- $B > $O/${TAG}_pmcS.log 2>&1
rocprofv3 --pmc FETCH_SIZE -d $O/${TAG}_pmcF -o f --output-format csv -- $B > $O/${TAG}_pmcF.log 2>&1
rocprofv3 --pmc WRITE_SIZE -d $O/${TAG}_pmcW -o w --output-format csv -- $B > $O/${TAG}_pmcW.log 2>&1
# three identical bench steps per profiled run (--no-count-step): one warm-up step, the timed step, the instrumented step
python3 scripts/collect_pmc.py $O/${TAG}_pmcS $O/${TAG}_pmc.json 3 > $O/${TAG}_collect.log 2>&1
python3 scripts/collect_traffic.py $O/${TAG}_pmcF $O/${TAG}_pmcW $O/${TAG}_traffic.json 3 >> $O/${TAG}_collect.log 2>&1
cp $O/${TAG}_stats/*/*kernel_stats.csv $O/${TAG}_kernel_stats.csv 2>/dev/null || find $O/${TAG}_stats -name "*kernel_stats.csv" -exec cp {} $O/${TAG}_kernel_stats.csv \;
# the bulky raw counter dumps are not kept
rm -rf $O/${TAG}_pmcS $O/${TAG}_pmcF $O/${TAG}_pmcW $O/${TAG}_stats
tail -4 $O/${TAG}_collect.log | cut -c1-300
