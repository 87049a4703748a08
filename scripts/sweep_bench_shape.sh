# the bench workload (32 candidates per step) over the launch-shape knobs of the experiments build: points per thread, floor of blocks per pair
export DGS_REG_LIB=$PWD/delta_graph_slam_amd/libdgs_reg_exp.so
D=${1:-$(mktemp -d)}   # the bench line and its stderr of the last setting: the directory given, or a new temporary one
for cfg in "2 64" "4 64" "4 32" "3 64" "1 64" "2 128"; do set -- $cfg; DGS_NDT_PPT=$1 DGS_NDT_MIN_BLOCKS=$2 python bench.py --steps 60 --full --no-traffic --no-cpu-baseline > $D/sh.json 2> $D/sh.err; python -c "
import json
d=json.loads(open('$D/sh.json').read().strip().splitlines()[-1])
print('ppt $1 min_blocks $2:', round(d['value']), round(d['ms_per_step'],4), round(d['roofline']['frac'],4))"; done
