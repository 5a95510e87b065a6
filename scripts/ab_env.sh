#!/bin/bash
# GPU box: same-call A/B of one environment switch.  usage: ab_env.sh OUT VAR "v1 v2 ..." ["bench args"] ; prints step time + selected kernel times
R=$GRAFT_REPO_ROOT; O=$R/gpurun_out/$1; mkdir -p $O; cd $R
VAR=$2; VALS=$3; EXTRA=${4:-}
NB="--full --no-cpu-baseline --no-verify --steps 100 --repeats 3 $EXTRA"
for v in $VALS; do
  for m in "--no-pipeline" ""; do
    tag=${VAR}_${v}$(echo $m | tr -d ' -')
    env $VAR=$v python bench.py $NB $m > $O/$tag.json 2> $O/$tag.err
    python - <<PY
import json
try:
    d = json.load(open("$O/$tag.json"))
    pk = d["roofline"]["per_kernel"]
    sel = {k: round(v["avg_us"], 1) for k, v in pk.items() if k in ("conv_init", "conv_igemm/b0_conv0", "conv_igemm/b0_conv1", "conv_igemm/b1_conv1", "conv_igemm/b2_conv1")}
    print("$tag", d["value"], d["ms_per_step"], d["ms_per_step_runs"], d["roofline"]["frac"], sel)
except Exception as e:
    print("$tag FAILED", e)
PY
  done
done
