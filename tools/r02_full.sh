#!/bin/sh
# end-of-round evidence: whole GPU suite, smoke, the full bench line, profiles.  usage: sh tools/r02_full.sh OUTDIR
D=$(mkdir -p "${1:?usage: sh tools/r02_full.sh OUTDIR}" && cd "$1" && pwd) || exit 2
cd "$(dirname "$0")/.."
timeout 1500 python -m pytest tests -m gpu -x -q > $D/gputest_r02.txt 2>&1; echo "pytest rc=$?" >> $D/gputest_r02.txt
timeout 300 python -c "import __graft_entry__ as g; g.smoke(); print('SMOKE OK')" > $D/smoke_r02.txt 2>&1
timeout 900 python bench.py --full > $D/bench_r02.json 2> $D/bench_r02.err
sh tools/profile_r02.sh > $D/profile_r02.log 2>&1
SIZES=64000000 sh tools/r02_pmc.sh > $D/pmc64.txt 2>&1
tail -3 $D/gputest_r02.txt; tail -2 $D/smoke_r02.txt; tail -c 3000 $D/bench_r02.json
