# Round-end validation on one MI355X: full GPU suite, smoke, driver-protocol benches (the LeNet
# ones with --full: the fp32 engine's figures beside the headline), BERT-base kernel stats.
# Outputs under $MLT_OUT_DIR (default validation_out/).
set -o pipefail
cd "$(dirname "$0")/.." && export TMPDIR=/tmp
O=${MLT_OUT_DIR:-validation_out}
mkdir -p "$O"
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 150 --timeout-method thread -p no:cacheprovider > "$O"/gputests.log 2>&1 &&
timeout -k 10 120 python -u -c "import __graft_entry__ as g; g.smoke()" > "$O"/smoke.log 2>&1 &&
timeout -k 10 120 python -u bench.py --full --steps 20 --warmup 5 > "$O"/fb_lenet20.log 2>&1 &&
timeout -k 10 120 python -u bench.py --full > "$O"/fb_lenet.log 2>&1 &&
timeout -k 10 200 python -u bench.py --model bert-base --steps 20 --warmup 5 > "$O"/fb_bert.log 2>&1 &&
timeout -k 10 200 python -u bench.py --model large --steps 6 --warmup 2 > "$O"/fb_large.log 2>&1 &&
timeout -k 10 200 python -u bench.py --model bert-large --steps 4 --warmup 2 > "$O"/fb_bertlarge.log 2>&1 &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$O"/prof_bert -o bert -- python3 -u bench.py --model bert-base --steps 5 --warmup 2 > "$O"/prof_bert.log 2>&1
