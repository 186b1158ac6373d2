#!/bin/bash
# One GPU call: the parity suite, an optional same-box A/B of variant builds
# (scripts/gpu_ab.sh: PKGS single cubes, HPKGS the helix batch) and the bench
# line without its profiler child. Stops at the first failure; every GPU step
# has its own time limit. Results under gpurun_out/<TAG>/.
#   TAG=r6b HPKGS="variants/a variants/b" bash scripts/gpu_check.sh   (NOTEST=1 / NOBENCH=1 skip;
#   PYTEST_K="golden or vspace" selects tests)
set -o pipefail
cd "$GRAFT_REPO_ROOT"; TAG=${TAG:-chk}; O=gpurun_out/$TAG; mkdir -p $O
export TSA_EXPECT_GPU=1
if [ -z "$NOTEST" ]; then
  timeout -k 10 900 python -u -m pytest tests -x -v -m gpu --timeout 240 --timeout-method thread ${PYTEST_K:+-k "$PYTEST_K"} \
    > $O/pytest_gpu.log 2>&1
  rc=$?; echo "pytest rc=$rc"; tail -3 $O/pytest_gpu.log; [ $rc -eq 0 ] || exit $rc
fi
if [ -n "$PKGS$HPKGS" ]; then
  TAG=$TAG bash scripts/gpu_ab.sh > $O/ab.out 2>&1; rc=$?; echo "ab rc=$rc"; cat $O/ab.out; [ $rc -eq 0 ] || exit $rc
fi
if [ -z "$NOBENCH" ]; then
  timeout -k 10 600 python bench.py --full --no-profile --record-file "$O/bench_record.json" ${BENCH_ARGS} \
    > $O/bench.json 2> $O/bench.err
  rc=$?; echo "bench rc=$rc"; cut -c1-3000 $O/bench.json; [ $rc -eq 0 ] || { tail -20 $O/bench.err; exit $rc; }
fi
