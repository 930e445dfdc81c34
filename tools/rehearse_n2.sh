#!/bin/bash
# The N > 1 code paths on ONE GPU (rates mean nothing): two ranks over gloo sharing the card, then one rank
# with the RCCL all-gather forced.  Usage: tools/rehearse_n2.sh OUT_DIR
# Output: OUT_DIR/rehearsal_n2.json, OUT_DIR/force_sharded.json
set -e
mkdir -p "${1:?usage: tools/rehearse_n2.sh OUT_DIR}"
out=$(cd "$1" && pwd)
cd "$(dirname "$0")/.."
RAGFIN_DIST_BACKEND=gloo RAGFIN_SHARE_GPU=1 timeout -k 10 500 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 \
  --master-addr 127.0.0.1 --master-port 29541 bench.py --gpus 2 --steps 50 --warmup 5 --full > "$out/rehearsal_n2.json" 2> "$out/rehearsal_n2.err"
echo "n2 done"; tail -c 600 "$out/rehearsal_n2.json"; echo
RAGFIN_FORCE_SHARDED=1 timeout -k 10 300 python bench.py --steps 100 --full --no-configs > "$out/force_sharded.json" 2> "$out/force_sharded.err"
echo "force-sharded done"; tail -c 400 "$out/force_sharded.json"; echo
