# run on the GPU box from the repository root: the --full bench line, kernel stats, PMC traffic passes -> OUT (copy the summaries into
# profiles/ afterwards)
# usage:  ATSPEED_COMMIT=<short sha> bash tools/profile_round.sh OUT
set -x
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "${1:?usage: bash tools/profile_round.sh OUT}" && OUT=$(cd "$1" && pwd)
python bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err || exit 1
# the full report of THIS run, where the line's `detail` says it went (the passes below overwrite it)
cp "$ROOT/$(tail -1 $OUT/bench_default.json | python -c 'import json, sys; print(json.load(sys.stdin)["detail"])')" $OUT/bench_detail.json || exit 1
cd /tmp && export TMPDIR=/tmp
# the same command under the kernel trace (sub-passes off: the summary is the headline workload's)
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/stats -- python3 $ROOT/bench.py --full --no-cpu-baseline --aligned-resid-scale '' --single-stream-users 0 --no-configs --no-latency-curve > $OUT/stats.log 2>&1 || exit 1
# HBM-side traffic: FETCH_SIZE and WRITE_SIZE in separate passes, no trace domains next to --pmc
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch -- python3 $ROOT/bench.py --full --steps 2 --warmup 0 --no-cpu-baseline --aligned-resid-scale '' --single-stream-users 0 --no-configs --no-latency-curve > $OUT/pmc_fetch.log 2>&1 || exit 1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_write -- python3 $ROOT/bench.py --full --steps 2 --warmup 0 --no-cpu-baseline --aligned-resid-scale '' --single-stream-users 0 --no-configs --no-latency-curve > $OUT/pmc_write.log 2>&1 || exit 1
cd $ROOT
find $OUT -name "*kernel_stats.csv" | head -3
# keep what is merged back small: the per-dispatch counter CSVs are summarised here, the traces dropped
python tools/pmc_summary.py $OUT $OUT/pmc_traffic.json > $OUT/pmc_summary.log 2>&1
cp $(find $OUT/stats -name "*kernel_stats.csv" | head -1) $OUT/kernel_stats.csv
rm -rf $OUT/stats $OUT/pmc_fetch $OUT/pmc_write
ls -la $OUT
