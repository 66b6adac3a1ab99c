#!/bin/bash
# Seven-letter tests after the alphabet-scan change, then the driver's bench command (tools only).
set -o pipefail
# usage: bash tools/hep_round2.sh OUTDIR
out=${1:?usage: bash tools/hep_round2.sh OUTDIR}
cd "$(dirname "$0")/.."; mkdir -p "$out"
timeout -k 10 600 python -u -m pytest tests/test_hepta.py tests/test_duo_raw.py tests/test_gpu_parity.py -x -q --timeout 300 --timeout-method thread > "$out/t.log" 2>&1
rc=$?; tail -3 "$out/t.log"; [ $rc -ne 0 ] && { tail -40 "$out/t.log"; exit $rc; }
timeout -k 10 600 python bench.py --full --gpus 1 --steps 20 --warmup 5 > "$out/bench.json" 2> "$out/bench.err"
rc=$?; [ $rc -ne 0 ] && { tail -20 "$out/bench.err"; exit $rc; }
python -c "import json, sys; d=json.load(open(sys.argv[1])); print(json.dumps(d['summary'])); print(json.dumps(d.get('byte_alphabets'))[:1500])" "$out/bench.json"
