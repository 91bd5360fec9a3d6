#!/bin/bash
# Registers, spills and scratch of the encode kernels as hipcc allocates them (no GPU needed):
#   bash tools/kernel_resources.sh [extra hipcc flags]
# The assembly is left in $GFY_ASM_OUT (default /tmp/gine_f16.s).
set -e
cd "$(dirname "$0")/../ginfinity_amd/csrc"
OUT=$(mktemp -d)
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math \
  -Wall -Wno-unused-function "$@" --save-temps=obj -c gine_f16.hip -o "$OUT/gine_f16.o"
python3 - "$OUT/gine_f16-hip-amdgcn-amd-amdhsa-gfx950.s" <<'PY'
import re, sys
text = open(sys.argv[1]).read()
meta = text[text.index('amdhsa.kernels:'):]
for block in meta.split('  - .agpr_count:')[1:]:
    name = re.search(r'\.name:\s+(\S+)', block).group(1)
    field = lambda k: re.search(r'\.%s:\s+(\d+)' % k, block).group(1)
    print(f"{name[20:64]:46s} agpr {block.split()[0]:>3s} vgpr {field('vgpr_count'):>3s} "
          f"spilled {field('vgpr_spill_count'):>3s} sgpr {field('sgpr_count'):>3s} "
          f"scratch {field('private_segment_fixed_size')} B")
PY
cp "$OUT/gine_f16-hip-amdgcn-amd-amdhsa-gfx950.s" "${GFY_ASM_OUT:-/tmp/gine_f16.s}"
rm -rf "$OUT"
