#!/bin/bash
# Registers / spills of the pairwise kernels as hipcc allocates them (no GPU needed):
#   bash tools/pairwise_resources.sh [extra hipcc flags]
#   GFY_SOURCE=pairwise_topk.hip bash tools/pairwise_resources.sh     # the top-k kernels
#   GFY_SOURCE=pairwise_topk_ranges.hip bash tools/pairwise_resources.sh   # ... with per-row ranges
#   GFY_SOURCE=pairwise_within.hip bash tools/pairwise_resources.sh   # the radius search (count, fill, order)
#   GFY_SOURCE=align_kernels.hip bash tools/pairwise_resources.sh     # the aligners (no scratch, no barrier)
# Per kernel: registers, spills, scratch, and how many MFMA, LDS-DMA, 16-byte LDS read and barrier
# instructions its code holds (the figures a refactor of the sweep must leave alone).
# The assembly is left in $GFY_ASM_OUT (default /tmp/<source stem>.s, i.e. /tmp/pairwise.s).
set -e
cd "$(dirname "$0")/../ginfinity_amd/csrc"
SOURCE="${GFY_SOURCE:-pairwise.hip}"
STEM="${SOURCE%.hip}"
OUT=$(mktemp -d)
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math \
  -Wall -Wno-unused-function "$@" --save-temps=obj -c "$SOURCE" -o "$OUT/p.o"
python3 - "$OUT/$STEM-hip-amdgcn-amd-amdhsa-gfx950.s" <<'PY'
import re, sys
text = open(sys.argv[1]).read()
meta = text[text.index('amdhsa.kernels:'):]
counted = (('mfma', 'v_mfma'), ('dma', 'global_load_lds'), ('ds128', 'ds_read_b128'),
           ('barrier', 's_barrier'))
for block in meta.split('  - .agpr_count:')[1:]:
    name = re.search(r'\.name:\s+(\S+)', block).group(1)
    field = lambda k: re.search(r'\.%s:\s+(\d+)' % k, block).group(1)
    body = text[text.index('\n%s:' % name):]          # the kernel's instructions
    body = body[:body.index('.Lfunc_end')]
    counts = ' '.join('%s %d' % (label, len(re.findall(r'^\s+%s' % word, body, re.M)))
                      for label, word in counted)
    print(f"{name[:60]:60s} agpr {block.split()[0]:>3s} vgpr {field('vgpr_count'):>3s} "
          f"spilled {field('vgpr_spill_count'):>3s} scratch {field('private_segment_fixed_size')} B "
          f"sgpr {field('sgpr_count'):>3s} {counts}")
PY
cp "$OUT/$STEM-hip-amdgcn-amd-amdhsa-gfx950.s" "${GFY_ASM_OUT:-/tmp/$STEM.s}"
rm -rf "$OUT"
