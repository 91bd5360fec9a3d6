#!/bin/bash
# Registers, spills and scratch of a file's kernels as hipcc allocates them (no GPU needed):
#   bash tools/kernel_resources.sh [source.hip] [extra hipcc flags]
# The source defaults to gine_f16.hip, the encode kernels; align_kernels.hip gives the aligners'
# table.  The assembly is left in $GFY_ASM_OUT (default /tmp/<source stem>.s).
set -e
cd "$(dirname "$0")/../ginfinity_amd/csrc"
SOURCE=gine_f16.hip
if [[ "${1:-}" == *.hip ]]; then SOURCE="$1"; shift; fi
STEM="${SOURCE%.hip}"
OUT=$(mktemp -d)
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math \
  -Wall -Wno-unused-function "$@" --save-temps=obj -c "$SOURCE" -o "$OUT/$STEM.o"
python3 - "$OUT/$STEM-hip-amdgcn-amd-amdhsa-gfx950.s" <<'PY'
import os, re, sys
text = open(sys.argv[1]).read()
meta = text[text.index('amdhsa.kernels:'):]
names = re.findall(r'\.name:\s+(\S+)', meta)
skip = len(os.path.commonprefix(names)) if len(names) > 1 else 0   # the namespaces the file's kernels share
for block in meta.split('  - .agpr_count:')[1:]:
    name = re.search(r'\.name:\s+(\S+)', block).group(1)
    field = lambda k: re.search(r'\.%s:\s+(\d+)' % k, block).group(1)
    print(f"{name[skip:skip + 44]:46s} agpr {block.split()[0]:>3s} vgpr {field('vgpr_count'):>3s} "
          f"spilled {field('vgpr_spill_count'):>3s} sgpr {field('sgpr_count'):>3s} "
          f"scratch {field('private_segment_fixed_size')} B")
PY
cp "$OUT/$STEM-hip-amdgcn-amd-amdhsa-gfx950.s" "${GFY_ASM_OUT:-/tmp/$STEM.s}"
rm -rf "$OUT"
