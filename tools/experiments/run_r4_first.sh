#!/bin/bash
# round 4, first GPU call: probe + the new tests + bench (new legs) + vendor yardstick + slab-chain experiment
cd "$(dirname "$0")/../.."
O=${1:?usage: run_r4_first.sh OUTDIR}
mkdir -p "$O"
export HSA_ENABLE_IPC_MODE_LEGACY=0
( timeout 60 tools/experiments/f16_ovfl_probe ) > $O/r4_probe.log 2>&1
( timeout 900 python -m pytest tests/test_kernels_gpu.py -q -x -k "saturate" ) > $O/r4_t_sat.log 2>&1
( timeout 900 python -m pytest tests/test_frame_parallel_gpu.py -q -s ) > $O/r4_t_fp.log 2>&1
( timeout 1200 python -m pytest tests/test_unet_gpu.py -q -s -k "ddim50_full or i2vgen_properties or config1_properties" ) > $O/r4_t_unet.log 2>&1
( timeout 900 python bench.py --full --steps 10 --warmup 3 --dump-ops $O/r4_ops_40x64.tsv --dump-ops-sim $O/r4_ops_sim_rank0of8.tsv ) > $O/r4_bench.json 2> $O/r4_bench.err
( timeout 600 python tools/vendor_yardstick.py --out $O/r4_vendor_yardstick.tsv ) > $O/r4_vendor.log 2>&1
( timeout 300 python tools/experiments/slab_chain.py ) > $O/r4_slab.log 2>&1
tail -3 $O/r4_probe.log $O/r4_t_sat.log $O/r4_t_fp.log $O/r4_t_unet.log $O/r4_slab.log
tail -c 1500 $O/r4_bench.err
