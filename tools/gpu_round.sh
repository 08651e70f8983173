#!/bin/bash
# One GPU-box session: parity tests, microbench, bench lines (eager + graph, --full), rocprof kernel stats. Everything lands in $OUT (default run_out/).
R=$(cd "$(dirname "$0")/.." && pwd)
cd "$R"
OUT=$(mkdir -p "${OUT:-run_out}" && cd "${OUT:-run_out}" && pwd)
export TMPDIR=/tmp
timeout 1200 python -m pytest tests -m gpu -q --no-header -p no:cacheprovider > $OUT/pytest_gpu.log 2>&1
echo "pytest exit $?" >> $OUT/pytest_gpu.log
tail -4 $OUT/pytest_gpu.log
if [ "$1" != "tests" ]; then
timeout 600 python tools/microbench.py 2>&1 | grep -v amdgpu.ids > $OUT/microbench.log
timeout 900 python bench.py --steps 4 --warmup 1 --full 2>/dev/null | tail -1 > $OUT/bench.log
timeout 900 python bench.py --steps 4 --warmup 1 --full --graph --no-cpu-baseline --no-vae --no-encoders 2>/dev/null | tail -1 > $OUT/bench_graph.log
(cd /tmp && timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o bench -- python $R/bench.py --steps 2 --warmup 1 --full --no-cpu-baseline --no-profile --no-vae > $OUT/rocprof.log 2>&1)
ls -R $OUT/prof | head -20 >> $OUT/rocprof.log
cat $OUT/microbench.log
OUT=$OUT python - <<'PY'
import json, os
for f in (os.path.join(os.environ["OUT"], "bench.log"), os.path.join(os.environ["OUT"], "bench_graph.log")):
    try:
        d = json.loads(open(f).read())
        print(f, {k: d[k] for k in ("value", "ms_per_step", "achieved_tflops_per_gpu", "launch", "vae", "sec_per_edit_50_steps", "roofline") if k in d})
    except Exception as e:
        print(f, "unreadable", e)
PY
fi
