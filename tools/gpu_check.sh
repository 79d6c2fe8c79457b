#!/bin/bash
# one GPU round: parity tests -> smoke -> bench; each step time-boxed, the
# chain stops at the first failure (no GPU work after a fault).  OUT names
# the directory the logs go to (default: out).
set -o pipefail
O=${OUT:-out}; mkdir -p $O
export TMPDIR=/tmp
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread -p no:cacheprovider > $O/pytest_gpu.log 2>&1
rc=$?; echo "pytest rc=$rc"; tail -8 $O/pytest_gpu.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1
rc=$?; echo "smoke rc=$rc"; tail -3 $O/smoke.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 400 python bench.py --full --steps 20 --warmup 5 > $O/bench.log 2>&1
rc=$?; echo "bench rc=$rc"; tail -c 3000 $O/bench.log
exit $rc
