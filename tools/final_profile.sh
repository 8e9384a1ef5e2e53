#!/bin/bash
# artefacts committed under profiles/: default bench line (every leg: --full), rocprofv3 kernel
# statistics of the same command, smoke().  usage: tools/final_profile.sh OUT_DIR
set -e
O=$(realpath -m "${1:?usage: tools/final_profile.sh OUT_DIR}")
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
mkdir -p $O
timeout -k 10 300 python3 -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $O/smoke.log 2>&1
timeout -k 10 500 python3 bench.py --full > $O/bench_default.json 2> $O/bench_default.err
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -o bench -- python3 bench.py --cpu-sample 0 --steps 8 --worst-case-steps 0 --bounded-gb 0 --gen-workers 1 > $O/bench_under_rocprof.json 2> $O/rocprof.err
