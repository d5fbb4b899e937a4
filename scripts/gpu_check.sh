#!/bin/bash
# Round GPU check: gpu tests, smoke, default bench, pointmaze-medium N=1 bench,
# 2-rank gloo rehearsal of the strong-scaling pointmaze bench.  Every GPU step
# has its own time limit; the script stops at the first crash / timeout.
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-bench_out}  # logs of this script
mkdir -p "$OUT"
export TMPDIR=/tmp
echo "== pytest -m gpu"
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 200 --timeout-method thread ${PYTEST_ARGS:-} \
  > $OUT/pytest_gpu.log 2>&1
rc=$?
tail -5 $OUT/pytest_gpu.log
echo "pytest rc=$rc"
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
echo "== smoke"
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 || { tail -20 $OUT/smoke.log; exit 3; }
tail -1 $OUT/smoke.log
echo "== bench"
timeout -k 10 400 python bench.py --full > $OUT/bench.log 2>&1 || { tail -20 $OUT/bench.log; exit 4; }
grep '^{' $OUT/bench.log
timeout -k 10 200 python bench.py --full --workload pointmaze-medium-n1 --steps 3000 > $OUT/bench_n1.log 2>&1 || { tail -20 $OUT/bench_n1.log; exit 5; }
grep '^{' $OUT/bench_n1.log
if [ "${DIST:-1}" = 1 ]; then
  echo "== 2-rank gloo rehearsal"
  timeout -k 10 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 \
    --master-port 29533 bench.py --full --gpus 2 --steps 500 --warmup 20 --dist-backend gloo --workload pointmaze \
    --no-cpu-baseline > $OUT/dist_pointmaze.log 2>&1 || { tail -30 $OUT/dist_pointmaze.log; exit 6; }
  grep '^{' $OUT/dist_pointmaze.log
fi
exit $rc
