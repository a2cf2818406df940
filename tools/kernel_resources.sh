#!/bin/bash
# Register / LDS / scratch / occupancy per kernel, from the compiler's own remarks (no GPU needed).
# usage: bash tools/kernel_resources.sh <file-stem> [extra flags]     e.g.  bash tools/kernel_resources.sh blend
cd "$(dirname "$0")/../gscream_amd/csrc" || exit 1
F=$1; shift
# the flags the Makefile compiles this file with: its SRCFLAGS_<file-stem>, read from the Makefile itself (empty for most files)
X=$(make -s --no-print-directory --eval='kernel-resources-flags: ; @echo $(SRCFLAGS_$(F))' kernel-resources-flags F="$F")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 $X "$@" --cuda-device-only -c $F.hip -o /dev/null \
  -Rpass-analysis=kernel-resource-usage 2>&1 | grep -E "Function Name|VGPRs:|AGPRs|ScratchSize|Occupancy|LDS Size|SGPRs:" |
  sed -E 's/.*remark: [^ ]+ //' | paste - - - - - - - | sed -E 's/\[-Rpass-analysis=kernel-resource-usage\]//g; s/ +/ /g'
