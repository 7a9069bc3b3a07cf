#!/bin/bash
LOG=${LOG:-logs}        # output folder, relative to the repository root
export PYTHONDONTWRITEBYTECODE=1
mkdir -p $LOG
timeout 1200 python -m pytest tests -q -m gpu -p no:cacheprovider -s > $LOG/pytest.log 2>&1; echo "pytest exit $?"; grep -E "max\|dlogits\||passed|failed" $LOG/pytest.log | tail -12
timeout 600 python scripts/gpu_cfg3.py > $LOG/cfg3.log 2>&1; echo "cfg3 exit $?"; grep -v amdgpu.ids $LOG/cfg3.log | tail -30
timeout 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29511 bench.py --full --gpus 1 --steps 10 --warmup 3 --no-cpu-baseline > $LOG/bench_torchrun.log 2>&1; echo "torchrun bench exit $?"; tail -1 $LOG/bench_torchrun.log | cut -c1-300
