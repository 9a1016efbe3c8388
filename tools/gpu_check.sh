set -o pipefail
# full GPU suite + the full bench line (the C3 headline, with the pipeline, the C4 point and the CPU baseline)
O=${GA_CHECK_OUT:-check_out}
mkdir -p $O
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 240 --timeout-method thread > $O/gpu_check.log 2>&1 || { tail -40 $O/gpu_check.log; exit 1; }
tail -2 $O/gpu_check.log
timeout -k 10 400 python -u bench.py --full > $O/check_bench.json 2> $O/check_bench.err || { tail -20 $O/check_bench.err; exit 1; }
cat $O/check_bench.json
