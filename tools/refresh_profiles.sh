#!/bin/bash
# Run ON THE GPU BOX: regenerates the raw profile evidence for the current build under $OUT (default: profile_raw/ in the repository).
#   kernel-trace stats of the --full bench run and of --in-flight 1 --lanes 1, PMC FETCH_SIZE / WRITE_SIZE passes (separate, as the
#   guide prescribes) with the per-launch op list.  Copy the summaries into profiles/ afterwards (tools/pmc_traffic.py).
set -e
R=${GRAFT_REPO_ROOT:-/root/repo}
TAG=${1:-r06}
OUT=$(realpath -m "${OUT:-$R/profile_raw}")
mkdir -p $OUT
python3 -c "import sys; sys.path.insert(0, '$R'); import bench; print(bench.source_hash())" > $OUT/${TAG}_source_hash.txt
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $OUT/prof_default -o d --output-format csv -- python3 $R/bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-variants --no-configs --no-train --no-extras --no-live-traffic > $OUT/prof_default.log 2>&1
rocprofv3 --kernel-trace --stats -d $OUT/prof_lanes1 -o l --output-format csv -- python3 $R/bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-variants --no-configs --no-train --no-extras --no-live-traffic --in-flight 1 --lanes 1 > $OUT/prof_lanes1.log 2>&1
rocprofv3 --kernel-trace --stats -d $OUT/prof_f16 -o h --output-format csv -- python3 $R/bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-variants --no-configs --no-train --no-extras --no-live-traffic --res 512 --batch 128 --dtype f16 > $OUT/prof_f16.log 2>&1
rocprofv3 --kernel-trace --stats -d $OUT/prof_f16x3 -o x --output-format csv -- python3 $R/bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-variants --no-configs --no-train --no-extras --no-live-traffic --dtype f16x3 > $OUT/prof_f16x3.log 2>&1
rocprofv3 --kernel-trace --stats -d $OUT/prof_f16x3_512 -o y --output-format csv -- python3 $R/bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-variants --no-configs --no-train --no-extras --no-live-traffic --res 512 --batch 128 --dtype f16x3 > $OUT/prof_f16x3_512.log 2>&1
rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $OUT/pmc_fetch -o f --output-format csv -- python3 $R/bench.py --full --launch-repeats 1 --steps 3 --warmup 1 --no-cpu-baseline --no-variants --no-configs --no-train --no-extras --no-live-traffic --in-flight 1 --lanes 1 --dump-ops $OUT/ops.json > $OUT/pmc_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --kernel-trace -d $OUT/pmc_write -o w --output-format csv -- python3 $R/bench.py --full --launch-repeats 1 --steps 3 --warmup 1 --no-cpu-baseline --no-variants --no-configs --no-train --no-extras --no-live-traffic --in-flight 1 --lanes 1 > $OUT/pmc_write.log 2>&1
rocprofv3 --kernel-trace --stats -d $OUT/prof_train -o t --output-format csv -- python3 $R/tools/train_bench.py --batch 16 --steps 20 > $OUT/prof_train.log 2>&1
rocprofv3 --kernel-trace --stats -d $OUT/prof_train256 -o u --output-format csv -- python3 $R/tools/train_bench.py --batch 256 --steps 5 > $OUT/prof_train256.log 2>&1
# the headline loop ALONE under the kernel trace (two batches in flight, the default scheduling): what tools/trace_overlap.py reads
rocprofv3 --kernel-trace -d $OUT/prof_headline -o hl --output-format csv -- python3 $R/bench.py --steps 20 --warmup 5 --regions 1 --headline-only --no-live-traffic > $OUT/prof_headline.log 2>&1
ls $OUT/prof_default $OUT/pmc_fetch $OUT/prof_train $OUT/prof_headline
