#!/bin/bash
# End-of-round check on the GPU box: full bench line, stress configuration, the GPU test suite, smoke.
#     bash tools/final_check.sh OUTDIR
export TMPDIR=/tmp
O=${1:?usage: bash tools/final_check.sh OUTDIR}
mkdir -p "$O"
timeout 900 python bench.py --full > "$O"/bench_line.json 2> "$O"/bench.err; echo "bench rc=$?"
timeout 600 python tools/stress_bench.py "$O"/stress_config5.json > "$O"/stress.log 2>&1; echo "stress rc=$?"
timeout 2400 python -m pytest tests -q -m gpu -x 2>&1 | tail -3
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -2
timeout 600 python tools/gram256_soak.py 100 2>&1 | tail -1
timeout 600 python tools/pool_fwd256_soak.py 120 2>&1 | tail -2
