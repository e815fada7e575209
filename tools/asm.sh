#!/bin/bash
# device assembly of one kernel source + its register summary: tools/asm.sh [out.s] [source]
# source = a file of lerf-pytorch_amd/csrc, with or without its .hip (default lerf_fused.hip: the fused kernels; the other
# instances and lerf_lut_interp.hip give the same table)
out=${1:-/tmp/fused.s}
R=$(cd "$(dirname "$0")/.." && pwd)
src=$(basename "${2:-lerf_fused.hip}" .hip).hip
/opt/rocm/bin/hipcc -O3 -std=c++17 -fno-slp-vectorize --offload-arch=gfx950 -I$R/include -S --cuda-device-only -o $out $R/lerf-pytorch_amd/csrc/$src $EXTRA 2>&1 | grep -v "warning: argument"
python3 - $out <<'PY'
import re,sys
t=open(sys.argv[1]).read()
for m in re.finditer(r'\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_count:\s+(\d+)\n\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)', t):
    n=m.group(1)
    if 'fused' in n or 'lut_interp' in n: print("%-75s sgpr %3s spill %3s vgpr %3s spill %3s scratch %3s" % (n[:75], m.group(3), m.group(4), m.group(5), m.group(6), m.group(2)))
PY
