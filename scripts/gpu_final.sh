#!/bin/bash
# Final-tree GPU call: the PMC passes first (scripts/gpu_profile.sh), stamped on
# the box (tools/pmc_traffic.py writes profiles/pmc_*.json there, keyed by the
# sources' hash) so the bench line that follows reads fresh stamps; then the
# -m gpu suite and the bench line. Rerun tools/pmc_traffic.py <TAG> locally on
# the merged gpurun_out/ to commit the same stamps.
#   TAG=r6k bash scripts/gpu_final.sh       (NOTEST=1 skips the suite)
set -o pipefail
cd "$GRAFT_REPO_ROOT"; TAG=${TAG:-final}; O=gpurun_out/$TAG; mkdir -p $O
export TSA_EXPECT_GPU=1
TAG=$TAG KERNELS=pencil bash scripts/gpu_profile.sh || exit $?
cd "$GRAFT_REPO_ROOT"
python3 tools/pmc_traffic.py $TAG > $O/pmc_traffic.out 2>&1 || { tail -5 $O/pmc_traffic.out; exit 1; }
if [ -z "$NOTEST" ]; then
  timeout -k 10 900 python -u -m pytest tests -x -v -m gpu --timeout 240 --timeout-method thread \
    > $O/pytest_gpu.log 2>&1
  rc=$?; echo "pytest rc=$rc"; tail -3 $O/pytest_gpu.log; [ $rc -eq 0 ] || exit $rc
fi
timeout -k 10 600 python bench.py --full --profile-dir "$O/bench_profile" \
  --record-file "$O/bench_record.json" ${BENCH_ARGS} > $O/bench.json 2> $O/bench.err
rc=$?; echo "bench rc=$rc"; cat $O/bench.json; [ $rc -eq 0 ] || { tail -20 $O/bench.err; exit $rc; }
