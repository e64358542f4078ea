set -o pipefail
cd "$(dirname "$0")/.." && export TMPDIR=/tmp
O=${MLT_OUT_DIR:-validation_out}
mkdir -p "$O"
timeout -k 10 700 python -u -m pytest tests -m gpu -x -v --timeout 150 --timeout-method thread -p no:cacheprovider > "$O"/gputests.log 2>&1 &&
timeout -k 10 120 python -u -c "import __graft_entry__ as g; g.smoke()" > "$O"/smoke.log 2>&1 &&
timeout -k 10 120 python -u bench.py --full --steps 20 --warmup 5 > "$O"/fb_lenet20.log 2>&1 &&
timeout -k 10 120 python -u bench.py --full --batch 4 > "$O"/fb_lenet_b4.log 2>&1 &&
timeout -k 10 200 python -u bench.py --model bert-base --steps 20 --warmup 5 > "$O"/fb_bert.log 2>&1 &&
GEMM_BENCH_TOKENS=65536 timeout -k 10 120 rocprofv3 --kernel-trace --stats --output-format csv -d "$O"/prof_hbl -o hbl -- python3 -u benchmarks/hipblaslt_names.py > "$O"/prof_hbl.log 2>&1
