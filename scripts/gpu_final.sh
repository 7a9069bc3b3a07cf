#!/bin/bash
# round-end check without the rocprof passes: full GPU suite, smoke, bench.py --full for every BASELINE configuration
LOG=${LOG:-logs}        # output folder, relative to the repository root
export PYTHONDONTWRITEBYTECODE=1
mkdir -p $LOG
timeout 900 python -m pytest tests -q -m gpu -p no:cacheprovider > $LOG/pytest.log 2>&1; echo "pytest exit $?"; tail -2 $LOG/pytest.log
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $LOG/smoke.log 2>&1; echo "smoke exit $?"; tail -1 $LOG/smoke.log
timeout 600 python bench.py --full --steps 20 --warmup 5 > $LOG/bench.log 2> $LOG/bench.err; echo "bench exit $?"; tail -1 $LOG/bench.log | cut -c1-330
for w in cfg1 cfg3 cfg4 cfg5; do
  timeout 500 python bench.py --full --workload $w --steps 10 --warmup 3 > $LOG/bench_$w.log 2> $LOG/bench_$w.err; echo "$w exit $?"; tail -1 $LOG/bench_$w.log | cut -c1-200
done
