set -o pipefail
O=${MLT_OUT_DIR:-validation_out}
mkdir -p "$O"
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread -p no:cacheprovider > "$O"/gputests.log 2>&1 &&
timeout -k 10 120 python -u -c "import __graft_entry__ as g; g.smoke()" > "$O"/smoke.log 2>&1 &&
timeout -k 10 120 python -u bench.py --full > "$O"/bench.log 2>&1 &&
timeout -k 10 180 python -u bench.py --model bert-base --steps 20 --warmup 5 > "$O"/bench_bert.log 2>&1
