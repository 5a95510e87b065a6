#!/bin/bash
# Round 6, GPU call 6: TIMING ABLATIONS of conv3x3_slabdma_f16x3_kernel (b0_conv1, b1_conv1) -- side libraries built with -DABL=mask (wrong results, never shipped):
# 1 no epilogue, 2 no MFMAs, 4 no LDS fragment reads, 8 no DMA.  Serial schedule (nothing co-runs), per-kernel HIP-event times.
R=$GRAFT_REPO_ROOT; O=$R/gpurun_out/r06_call6; rm -rf $O; mkdir -p $O; cd $R
NB="--no-cpu-baseline --no-verify --no-pipeline --steps 60 --repeats 2"
run() { tag=$1; shift; timeout 200 python bench.py --full $NB "$@" > $O/$tag.json 2> $O/$tag.err; python -c "
import json
try:
    d=json.load(open('$O/$tag.json')); pk=d['roofline']['per_kernel']
    print('$tag', d.get('ms_per_step'), {k.split('/')[-1]: round(v['avg_us']) for k, v in pk.items() if 'b0_conv' in k or 'b1_conv' in k})
except Exception as e: print('$tag FAILED', e, open('$O/$tag.err').read()[-400:])"; }
run full
for m in 1 2 4 8 6 7 15; do SERL_MI355_LIB=$R/serl_amd/lib/libabl_$m.so run abl_$m; done
run full_again
