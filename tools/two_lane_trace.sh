#!/bin/bash
# rocprofv3 kernel trace of the two blocks of a --full bench line (one lane, then two lanes): how long do the kernels of the
# headline schedule take beside each other?  Output $OUT/<tag>_2lane (tag = $1); summarise with tools/two_lane_trace.py
tag=${1:-r04}
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mkdir -p "${OUT:?set OUT to an output directory}" && cd "$OUT" && pwd)
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --output-format csv -d $OUT/${tag}_2lane -- python3 $R/bench.py --full --steps 20 --warmup 3 --no-cpu-baseline --no-other-configs --repeats 2 > $OUT/${tag}_2lane.log 2>&1 || exit 1
grep -h '"metric"' $OUT/${tag}_2lane.log | cut -c1-200
