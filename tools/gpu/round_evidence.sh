# Round evidence on an MI355X:  bash tools/gpu/round_evidence.sh [tag] [part] [out]   (tag defaults to r06; outputs <out>/<tag>_*, out defaults to /tmp/pf_evidence)
# smoke -> full GPU test suite (gradient-parity report lines -> <tag>_parity_report.txt) -> rocprofv3 kernel trace of bench.py
# (stats + steady-state step table with the idle-gap analysis) -> separate PMC passes (FETCH_SIZE / WRITE_SIZE; never combined
# with a trace domain) -> the bench.py --full line (cpu_baseline, hbm_region.unshared) -> one bench line per other configuration of SURVEY 8(d)
# part: all (default) | suite (smoke + tests only) | profiles (everything behind the tests) -- two calls when GPU minutes are short
TAG=${1:-r06}
PART=${2:-all}
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
OUT=$(mkdir -p "${3:-/tmp/pf_evidence}" && cd "${3:-/tmp/pf_evidence}" && pwd)
cd $ROOT
export TMPDIR=/tmp
if [ $PART != profiles ]; then
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -2 | cut -c1-300
rm -f $OUT/${TAG}_parity_report.txt
PF_PARITY_REPORT=$OUT/${TAG}_parity_report.txt timeout 2400 python -m pytest tests -m gpu -q --timeout=900 --tb=line --durations=8 2>&1 | tail -24 | cut -c1-300 > $OUT/${TAG}_pytest_gpu.log
cat $OUT/${TAG}_pytest_gpu.log
fi
[ $PART = suite ] && exit 0
cd /tmp
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_$TAG -o $TAG -- python $ROOT/bench.py --steps 20 --warmup 5 --no_cpu_baseline > $OUT/${TAG}_prof.log 2>&1
cd $ROOT
grep '"metric"' $OUT/${TAG}_prof.log | cut -c1-200
python tools/prof_summary.py $(find /tmp/prof_$TAG -name '*kernel_trace.csv' | head -1) --steps 4 --out $OUT/${TAG}_step_kernels_b256.csv | head -14 | cut -c1-150
cp $(find /tmp/prof_$TAG -name '*kernel_stats.csv' | head -1) $OUT/${TAG}_rocprofv3_stats_b256.csv
cd /tmp
for c in FETCH_SIZE WRITE_SIZE; do
  timeout 600 rocprofv3 --pmc $c --output-format csv -d /tmp/pmc_$c -o p -- python $ROOT/bench.py --steps 2 --warmup 2 --no_cpu_baseline --step_graph 0 > $OUT/${TAG}_pmc_$c.log 2>&1
  f=$(find /tmp/pmc_$c -name '*counter_collection.csv' | head -1)
  python $ROOT/tools/pmc_summary.py $f $c --out $OUT/${TAG}_pmc_$c.csv | head -8 | cut -c1-160
done
# MFMA-busy pass (north_star: "rocprof MFMA-busy"): SQ busy cycles of the matrix pipe beside the SQ / GRBM activity counters, one pass, no
# trace domain; tools/mfma_busy.py turns it into a per-kernel table (derivation and calibration in its docstring)
timeout 600 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVE_CYCLES GRBM_GUI_ACTIVE --output-format csv -d /tmp/pmc_mfma -o p -- python $ROOT/bench.py --steps 2 --warmup 5 --no_cpu_baseline --step_graph 0 > $OUT/${TAG}_pmc_mfma.log 2>&1
f=$(find /tmp/pmc_mfma -name '*counter_collection.csv' | head -1)
python $ROOT/tools/pmc_table.py $f > $OUT/${TAG}_pmc_mfma_busy.csv 2>> $OUT/${TAG}_pmc_mfma.log; head -5 $OUT/${TAG}_pmc_mfma_busy.csv | cut -c1-200
# per-kernel table + the whole-step derivation (busy cycles per dispatch x calls per step of the kernel trace above)
python $ROOT/tools/mfma_busy.py $OUT/${TAG}_pmc_mfma_busy.csv $OUT/${TAG}_step_kernels_b256.csv > $OUT/${TAG}_mfma_busy.txt 2>&1; tail -7 $OUT/${TAG}_mfma_busy.txt | cut -c1-200
cd $ROOT
cp $OUT/${TAG}_pmc_FETCH_SIZE.csv $OUT/${TAG}_pmc_WRITE_SIZE.csv profiles/ 2>/dev/null     # bench.py reads roofline.traffic from profiles/
PF_BENCH_TRACE_STEPS=1 timeout 900 python bench.py --full > $OUT/${TAG}_bench.log 2>&1; grep -v '"metric"' $OUT/${TAG}_bench.log | tail -2 | cut -c1-300; grep '"metric"' $OUT/${TAG}_bench.log | cut -c1-2200
grep '"metric"' $OUT/${TAG}_bench.log > $OUT/${TAG}_bench.json
for c in c2a32 c4 c3 c1; do
  timeout 400 python bench.py --config $c --steps 20 --warmup 5 --no_cpu_baseline > $OUT/${TAG}_bench_$c.json 2> $OUT/${TAG}_bench_$c.err || tail -3 $OUT/${TAG}_bench_$c.err
  python -c "
import json, sys
for ln in open(sys.argv[1]):
    if ln.startswith('{'):
        d = json.loads(ln); print(sys.argv[2], round(d['value']), 'img/s', round(d['ms_per_step'], 2), 'ms/step', d['config'].get('workload', '')[:90])
" $OUT/${TAG}_bench_$c.json $c
done
cd /tmp
# steady-state kernel tables of the other configurations (is any library kernel left in their steps?)
for c in c1 c3; do
  timeout 600 rocprofv3 --kernel-trace --output-format csv -d /tmp/prof_${TAG}_$c -o $c -- python $ROOT/bench.py --config $c --steps 12 --warmup 5 --no_cpu_baseline --step_graph 0 > $OUT/${TAG}_prof_$c.log 2>&1
  marker=k_adam_flat; [ $c = c1 ] && marker=k_momentum_flat
  python $ROOT/tools/prof_summary.py $(find /tmp/prof_${TAG}_$c -name '*kernel_trace.csv' | head -1) --steps 4 --marker $marker --out $OUT/${TAG}_step_kernels_$c.csv | head -12 | cut -c1-150
done
cd $ROOT
# per-layer tables at the benchmarked geometry: every 1x1 forward launch of the roofline region, every backward-filter launch, the
# 3x3 forward / backward-data launches against MIOpen, the dense / few-channel kernels against the libraries they replaced
timeout 600 python tools/gpu/fwd1x1_layers.py > $OUT/${TAG}_fwd1x1_layers.txt 2>/dev/null; tail -2 $OUT/${TAG}_fwd1x1_layers.txt | cut -c1-200
timeout 600 python tools/gpu/wrw_layers.py > $OUT/${TAG}_wrw_layers.txt 2>/dev/null; tail -2 $OUT/${TAG}_wrw_layers.txt | cut -c1-200
timeout 600 python tools/gpu/igemm_bench.py > $OUT/${TAG}_igemm_layers.txt 2>/dev/null; tail -14 $OUT/${TAG}_igemm_layers.txt | cut -c1-200
timeout 600 python tools/gpu/new_kernels_bench.py > $OUT/${TAG}_new_kernels_layers.txt 2>/dev/null; tail -12 $OUT/${TAG}_new_kernels_layers.txt | cut -c1-200
