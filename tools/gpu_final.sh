#!/bin/bash
# round-4 closing evidence: the full -m gpu suite, the default bench line (all fields), the B = 4 line,
# per-call-site step breakdowns, then the rocprofv3 stats / PMC passes (tools/gpu_profile_r4.sh)
set -o pipefail
O=${OUT:-out}/final4; mkdir -p $O
bash tools/gpu_tests.sh || exit 1
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke(); print(\"smoke ok\")" > $O/smoke.log 2>&1 || { tail -5 $O/smoke.log; exit 1; }
tail -1 $O/smoke.log
timeout -k 10 600 python -u bench.py --full > $O/bench_default.log 2>&1 || { tail -5 $O/bench_default.log; exit 1; }
grep -h "^{" $O/bench_default.log | cut -c1-300
timeout -k 10 300 python -u bench.py --full --steps 50 --warmup 10 --no-cpu-baseline --no-other-configs --no-fp32-line --no-psnr --per-gpu-batch 4 > $O/bench4.log 2>&1 || exit 1
grep -h "^{" $O/bench4.log | cut -c1-200
for b in 8 16; do   # the per-GPU shapes of the N = 4 / N = 2 strong-scaling runs
  timeout -k 10 300 python -u bench.py --full --steps 50 --warmup 10 --no-cpu-baseline --no-other-configs --no-fp32-line --no-psnr --per-gpu-batch $b > $O/bench$b.log 2>&1 || exit 1
  grep -h "^{" $O/bench$b.log | cut -c1-200
done
timeout -k 10 200 python -u tools/roles.py 32 > $O/roles32.txt 2>&1 || exit 1
timeout -k 10 200 python -u tools/roles.py 4 > $O/roles4.txt 2>&1 || exit 1
bash tools/gpu_profile_r4.sh
