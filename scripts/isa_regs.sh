#!/bin/bash
# Registers / scratch / occupancy of chosen kernel instantiations without building the library (hipcc cross-compiles the device
# side of a throw-away translation unit in ~20 s):   bash scripts/isa_regs.sh 'gps::k_fused_level0<4, double, 12, true>(gps::FusedArgs<double, double>)' ...
# The ISA is left in /tmp/isa_regs.s.
# Kernels of a unit's unnamed namespace cannot be instantiated from another unit: --unit compiles the unit itself (device side only)
# and lists its kernels whose names hold one of the words:   bash scripts/isa_regs.sh --unit sampling.hip k_ps_bridge
cd "$(dirname "$0")/../gpslam_amd/csrc" || exit 1
if [ "$1" = "--unit" ]; then
  U=$2; shift 2
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=fast --cuda-device-only -S -o /tmp/isa_regs.s "$U" 2>&1 | grep -v "warning\|^ *[0-9]* *|\|^ *|\|generated\.$" | head -30
  awk '/^_Z[A-Za-z0-9_]*:/{name=$1} /; NumVgprs:/{printf "%s %s\n", name, $0} /; ScratchSize:|; Occupancy:|; LDSByteSize:/{print $0}' /tmp/isa_regs.s | c++filt | sed 's/: *; / /; s/^; //; s/ bytes\/workgroup.*//' | paste - - - - | grep -F -f <(printf '%s\n' "$@") || true
  exit 0
fi
T=_isa_regs_$$.hip
# (api_common.hpp brings every kernel header but level0.hpp, which holds k_fused_level0 and the two k_chunk_*_rows kernels)
printf '#include "api_common.hpp"\n#include "level0.hpp"\n' > $T
for sig in "$@"; do echo "template __global__ void $sig;" >> $T; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=fast --cuda-device-only -S -o /tmp/isa_regs.s $T 2>&1 | grep -v "warning\|^ *[0-9]* *|\|^ *|\|generated\.$" | head -30
rm -f $T
awk '/^_ZN3gps.*:/{name=$1} /; NumVgprs:|; ScratchSize:|; Occupancy:/{printf "%s %s\n", name, $0}' /tmp/isa_regs.s | c++filt | sed 's/(gps::[A-Za-z]*Args<[^)]*)//' | paste - - - | sed 's/[^ ]*ScratchSize/ScratchSize/; s/[^ ]* ; Occupancy/Occupancy/' | grep -F -f <(for sig in "$@"; do echo "$sig" | sed 's/(.*//; s/gps:://'; done) || true
