#!/bin/bash
# every measured artefact of a round in one run: tools/final_runs.sh <tag> <outroot>
#   outroot = the folder the profiling scripts (tools/prof_*.sh, pmc_lut_interp.sh) write their prof_* folders to; this
#   script's own outputs go to <outroot>/<tag>/
tag=${1:-r06}
root=$(cd "$(dirname "$0")/.." && pwd)
outroot=$(mkdir -p "${2:?usage: tools/final_runs.sh <tag> <outroot>}" && cd "$2" && pwd)
out=$outroot/$tag
mkdir -p $out
cd $root
timeout 900 python bench.py --full > $out/bench.json 2> $out/bench.err
{
for a in "--config 1" "--config 3" "--config 4" "--config 4 --warp-fused" "--config 5 --frames 4" "--support 4" "--scale 6" "--scale 8" "--channels 1" "--channels 4" "--input natural"; do
  echo "== bench.py $a"
  timeout 300 python bench.py $a --full --steps 20 --warmup 3 --sustained 2 2>/dev/null | tail -1
done
} > $out/other_configs.txt
timeout 400 python tools/bench_8k.py > $out/8k_blocks_strips.txt 2>&1
timeout 400 python tools/bench_ragged.py > $out/ragged_set5.txt 2>&1
timeout 400 python tools/stamps.py noise natural > $out/phase_breakdown.txt 2>&1
timeout 400 python bench.py --path callsite > $out/callsite.json 2>/dev/null
timeout 400 python bench.py --path classes-torch > $out/classes_torch.json 2>/dev/null
timeout 400 python experiments/probes/probe_warp.py > $out/warp_split.txt 2>&1
timeout 400 python tools/eval_set5.py > $out/set5_table.txt 2>&1
timeout 1500 bash tools/prof_all.sh > $out/prof_all.log 2>&1
# the single LUT pass behind the reference's own signature (lerf_lut_interp_ex): kernel times per (oC, pattern, rotation), LDS kernel and direct kernel
timeout 300 bash tools/prof_lut_interp.sh ${tag}_lut_interp --planes > $out/lut_interp_kernels.txt 2>&1
cp $outroot/prof_${tag}_lut_interp/bench.txt $out/lut_interp_calls.txt
timeout 700 bash tools/pmc_lut_interp.sh ${tag} --quick --kernels lds --iters 3 --no-acc --planes > $out/lut_interp_pmc.txt 2>&1
timeout 300 bash tools/prof_callsite.sh ${tag}_callsite > $out/callsite_profile.txt 2>&1
ls $out
# direct kernels behind the unchanged call sites (FourSimplexInterpFaster x 24, resize): kernel trace of bench.py --path callsite
cd /tmp && export TMPDIR=/tmp
timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $out/callsite_trace -o k -- python3 $root/bench.py --path callsite --steps 5 > /dev/null 2>&1
cd $root
