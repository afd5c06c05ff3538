#!/bin/bash
# VERDICT r05 next-round item 2 wanted the one MI355X of a gpurun box partitioned into 8 logical devices so that RCCL could run with more than one rank.
# The pool refuses every call that would change the partition mode (profiles/r06_rccl_cpx_refusal.log), so this script only READS the partition
# state and, should a box ever show more than one logical device, runs the RCCL legs on them.  Output: $1 (a log file).
set -u
LOG=${1:-gpurun_out/r06_rccl_partition_state.log}; REPO=$PWD
{
echo "== whoami: $(id)"
timeout 60 amd-smi version 2>&1 | head -3
timeout 60 amd-smi partition --current 2>&1 | head -20
timeout 60 amd-smi partition --accelerator 2>&1 | head -40
timeout 60 rocm-smi --showcomputepartition --showmemorypartition 2>&1 | head -20
for f in /sys/class/drm/card*/device/current_compute_partition /sys/class/drm/card*/device/available_compute_partition; do [ -e $f ] && echo "$f: $(cat $f 2>&1)"; done
N=$(timeout 120 python -c 'import torch; print(torch.cuda.device_count())' 2>&1 | tail -1)
echo "== logical devices: $N"
echo "== gfx950 agents: $(timeout 60 rocminfo 2>&1 | grep -c 'Name: *gfx950')"
} > $LOG 2>&1
N=$(grep "== logical devices:" $LOG | awk '{print $4}')
if [ "${N:-1}" -gt 1 ] 2>/dev/null; then
  for W in 2 4 8; do
    [ $W -le $N ] || continue
    echo "== bench.py --gpus $W over RCCL on $N logical devices" >> $LOG
    timeout 900 python -m torch.distributed.run --nnodes=1 --nproc-per-node $W --master-addr 127.0.0.1 --master-port $((29600+W)) bench.py --full --gpus $W --steps 5 --warmup 2 --no-sweep --dist-backend nccl 2>>${LOG%.log}_bench_$W.err | tail -1 > ${LOG%.log}_bench_$W.json
    echo "rc=$? $(head -c 600 ${LOG%.log}_bench_$W.json)" >> $LOG
  done
  echo "== tests/test_sharded_multirank_gpu.py with the RCCL transport on distinct logical devices" >> $LOG
  H2_MULTIRANK_RCCL=1 timeout 1500 python -m pytest tests/test_sharded_multirank_gpu.py -m gpu -x -q >> $LOG 2>&1
else
  echo "== one logical device: no RCCL run with more than one rank is possible on this box" >> $LOG
fi
tail -40 $LOG
