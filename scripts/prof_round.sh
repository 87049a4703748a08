# Round profile on the GPU box: bench line (with PMC traffic), rocprofv3 kernel stats of the same command, all configs.
# usage (from the repo root on the box): [OUT_DIR=<dir>] bash scripts/prof_round.sh <prefix>     -> files $OUT_DIR/<prefix>_*
P=${1:-x}
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
D=${OUT_DIR:-$R/profile_out}   # where everything goes (OUT_DIR, or profile_out/ in the repository)
mkdir -p $D/prof_$P
cd $R
timeout -k 10 500 python bench.py --steps 100 --warmup 10 --full --traffic-dir $D/traffic > $D/${P}_bench.json 2> $D/${P}_bench.err
echo bench-done
cd /tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $D/prof_$P -- python3 $R/bench.py --steps 100 --warmup 10 --full --no-cpu-baseline --no-traffic > $D/${P}_bench_under_rocprof.json 2> $D/${P}_rocprof.err
echo rocprof-done
cd $R
timeout -k 10 600 python scripts/bench_configs.py --frames 100 > $D/${P}_configs.jsonl 2> $D/${P}_configs.err
echo configs-done
timeout -k 10 300 python scripts/bench_cache.py --candidates 32 --distinct 8 > $D/${P}_cache_ticks.jsonl 2> $D/${P}_cache.err
echo cache-done
timeout -k 10 300 python bench.py --steps 100 --warmup 10 --group --full --no-traffic --no-cpu-baseline > $D/${P}_bench_group.json 2> $D/${P}_bench_group.err
echo group-done
cd /tmp
TAIL_STEPS=12 timeout -k 10 200 rocprofv3 --kernel-trace --output-format csv -d $D/tail_$P -- python3 $R/scripts/tail_profile.py > $D/${P}_tail.log 2>&1
cd $R
python3 scripts/tail_fit.py $D/tail_$P $D/${P}_tail_table.json > /dev/null
echo tail-done
# keep the summaries, drop the raw traces (tens of MB)
cp $(find $D/prof_$P -name "*kernel_stats.csv" | head -1) $D/${P}_kernel_stats.csv
rm -rf $D/prof_$P $D/tail_$P $D/traffic
ls -la $D | head -40
