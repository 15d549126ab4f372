#!/bin/bash
# Round-3 acceptance loop on the GPU box: the whole -m gpu suite, then the driver-style bench line with its --full rows,
# into the directory named by the first argument:  bash tools/r03_check.sh OUT_DIR
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=${1:?usage: tools/r03_check.sh OUT_DIR}
mkdir -p $OUT
cd $R
timeout -k 10 1000 python -m pytest tests -q -m gpu > $OUT/pytest_gpu.log 2>&1
rc=$?; echo "tests rc=$rc"; tail -8 $OUT/pytest_gpu.log
[ $rc -eq 0 ] || exit $rc           # a failed, aborted or hung suite: start nothing more on the GPU
VAH_GEMM_TABLE_DUMP=$OUT/gemm_table.txt timeout -k 10 600 python bench.py --full --steps 20 --warmup 5 > $OUT/bench.json 2> $OUT/bench.err
rc=$?; echo "bench rc=$rc"; [ $rc -eq 0 ] || exit $rc
BENCH_JSON=$OUT/bench.json python - <<'PY'
import json
import os
d=json.loads(open(os.environ['BENCH_JSON']).read().strip().splitlines()[-1])
print(d['value'], d['ms_per_step'], d['roofline']['frac'], d['roofline']['avg_launch_us'], d['config'].get('gemm_candidates_rejected'))
for k,v in d['kernels'].items():
    if k.startswith(('gemm','msda_fused')): print(k, v.get('avg_us'), v.get('frac_of_hbm_peak', v.get('frac_of_mfma_peak')))
PY
