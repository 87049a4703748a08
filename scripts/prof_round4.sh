# Round-4 profile on the GPU box: the bench line (upstream order timed; PMC traffic; cpu_baseline; parity gate), rocprofv3 kernel stats of the
# same command, SQ counters of the timed kernel, every config in both orders (+ cfg5_batched with traffic), the group form, the fast order.
# usage (repo root on the box): [OUT_DIR=<dir>] bash scripts/prof_round4.sh <prefix>   -> $OUT_DIR/<prefix>_*
P=${1:-r04}
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
D=${OUT_DIR:-$R/profile_out}   # where everything goes (OUT_DIR, or profile_out/ in the repository)
cd $R
mkdir -p $D
timeout -k 10 700 python bench.py --steps 100 --warmup 10 --full --traffic-dir $D/traffic > $D/${P}_bench.json 2> $D/${P}_bench.err
echo bench-done
mkdir -p $D/prof_$P
cd /tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $D/prof_$P -- python3 $R/bench.py --steps 100 --warmup 10 --full --no-cpu-baseline --no-traffic > $D/${P}_bench_under_rocprof.json 2> $D/${P}_rocprof.err
echo rocprof-done
cd $R
cp $(find $D/prof_$P -name "*kernel_stats.csv" | head -1) $D/${P}_kernel_stats.csv
rm -rf $D/prof_$P
OUT_DIR=$D NPASS=5 PMC_CMD="bench.py --steps 2 --warmup 1 --full --no-cpu-baseline --no-traffic" bash scripts/pmc_round.sh ${P} > $D/${P}_pmc.log 2>&1
echo pmc-done
cd $R
timeout -k 10 900 python scripts/bench_configs.py --frames 100 > $D/${P}_configs.jsonl 2> $D/${P}_configs.err
echo configs-done
timeout -k 10 300 python bench.py --steps 100 --warmup 10 --group --full --no-traffic --no-cpu-baseline > $D/${P}_bench_group.json 2> $D/${P}_bench_group.err
echo group-done
timeout -k 10 300 python bench.py --steps 100 --warmup 10 --order 0 --full --no-traffic --no-cpu-baseline > $D/${P}_bench_fast_order.json 2> $D/${P}_bench_fast.err
echo fast-done
ls -la $D | grep ${P}_
