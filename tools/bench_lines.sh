# The round's bench lines for C2 (default auto line), C3 (batch), C5 (slab workload, one GPU), slab 0 of
# C5's 8-way split, and C2 / C3 / C5 with the affine constants (c2a, c3a, c5a),
# taken after tools/pmc_summary.py has stamped profiles/pmc_*.json for this build, so every line's
# roofline carries the counter-derived `achieved` / `frac` (GPU box).  They are --full lines: the
# roofline, the extras of the default line and the CPU baseline are measured only there.
# usage: bash tools/bench_lines.sh OUTDIR   (writes OUTDIR/bench_<cfg>.json and .err)
set -e
out=${1:?usage: bash tools/bench_lines.sh OUTDIR}
mkdir -p "$out"
line() {  # cfg, bench args...
  local cfg=$1; shift
  timeout -k 10 240 python bench.py --full "$@" > "$out/bench_$cfg.json" 2> "$out/bench_$cfg.err"
}
line c2 --steps 10 --warmup 2
line c3 --workload batch --steps 5 --warmup 1
line c5 --workload slab --steps 3 --warmup 1 --cpu-seconds 10
line c5p8 --workload slab --slab-of 8 --steps 3 --warmup 1 --no-cpu-baseline
line c2a --workload pair --params 2,-3,5,2 --steps 10 --warmup 2 --no-extra --no-cpu-baseline
line c5a --workload slab --params 2,-3,5,2 --steps 3 --warmup 1 --no-cpu-baseline
line c3a --workload batch --params 2,-3,5,2 --steps 5 --warmup 1 --no-cpu-baseline
