#!/bin/bash
# rocprofv3 kernel trace + stats of the bench command with one launch sequence in flight (--streams 1: a launch's duration is the
# kernel's own), minus the CPU leg, the single-pair tail and the output check (--no-verify: its reference runs go through a
# single-pair plan and would add launches of other shapes to the per-symbol averages); then the plain bench line on the same box
cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
OUT=${1:?usage: scripts/prof.sh <output directory, relative to the repository root>}
rm -rf $OUT && mkdir -p $OUT
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT -- python3 bench.py --full --no-cpu-baseline --no-single --no-verify --streams 1 > $OUT/bench_under_rocprof.json 2> $OUT/bench_under_rocprof.err
python bench.py --full --verbose > $OUT/bench.json 2> $OUT/bench.err
tail -2 $OUT/bench.err
