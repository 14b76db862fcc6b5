#!/bin/bash
# kernel trace of the default four-lane bench (no stats, no per-launch events): input of scripts/experiments/lane_overlap.py
cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
OUT=${1:?usage: scripts/experiments/prof_lanes.sh <output directory, relative to the repository root>}
rm -rf $OUT && mkdir -p $OUT
rocprofv3 --kernel-trace --output-format csv -d $OUT -- python3 bench.py --full --no-cpu-baseline --no-single --no-kernel-events --steps 10 --warmup 3 > $OUT/bench.json 2> $OUT/bench.err
ls -la $OUT/*/ | head
