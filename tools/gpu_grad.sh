#!/bin/bash
# differentiable rollout on the GPU: parity tests, bench (config 5), profile.
# OUT names the directory the logs go to (default: out).
set -o pipefail
O=${OUT:-out}; mkdir -p $O/prof_grad
export TMPDIR=/tmp
timeout -k 10 900 python -m pytest tests -m gpu -x -q -p no:cacheprovider > $O/pytest_gpu.log 2>&1
rc=$?; echo "pytest rc=$rc"; tail -8 $O/pytest_gpu.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python bench.py --full --mode grad --steps 10 --warmup 2 > $O/bench_grad.log 2>&1
rc=$?; echo "bench grad rc=$rc"; tail -2 $O/bench_grad.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python bench.py --full --cpu-baseline off > $O/bench.log 2>&1
rc=$?; echo "bench rc=$rc"; tail -1 $O/bench.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/prof_grad/trace -o run --output-format csv -- python bench.py --mode grad --steps 5 --warmup 1 > $O/prof_grad/bench.json 2> $O/prof_grad/trace.err || { tail $O/prof_grad/trace.err; exit 2; }
echo "profile ok"
