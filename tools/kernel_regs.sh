#!/bin/bash
# VGPRs / spills / scratch of the FP64 degree-4 MFMA stage kernels for a set of -D flags:  tools/kernel_regs.sh [-DSG_...]
#   tools/kernel_regs.sh xcorr: every kernel of kernels_xcorr.hip, with AGPRs and LDS
#   tools/kernel_regs.sh grad: every kernel of kernels_grad.hip, with AGPRs and (static) LDS; its LDS is dynamic, the plan's
#   tools/kernel_regs.sh gauge: every kernel of kernels_gauge.hip, with AGPRs and LDS (static: four wave-private slabs)
cd "$(dirname "$0")/../seigen_amd/csrc"
if [ "$1" = "gauge" ]; then
  shift
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function "$@" -Rpass-analysis=kernel-resource-usage -c kernels_gauge.hip -o /tmp/kgg_regs_$$.o 2>&1 \
   | grep -E "Function Name|    VGPRs:|AGPRs:|VGPRs Spill|ScratchSize|Occupancy|LDS Size" | sed -e 's/.*remark: *//' -e 's/ \[-Rpass.*//' | paste - - - - - - - \
   | sed -e 's/Function Name: _ZN2sg5gauge//' -e 's/EEvPKT_[^\t]*//'
  rm -f /tmp/kgg_regs_$$.o
  exit 0
fi
if [ "$1" = "grad" ]; then
  shift
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function "$@" -Rpass-analysis=kernel-resource-usage -c kernels_grad.hip -o /tmp/kg_regs_$$.o 2>&1 \
   | grep -E "Function Name|    VGPRs:|AGPRs:|VGPRs Spill|ScratchSize|Occupancy|LDS Size" | sed -e 's/.*remark: *//' -e 's/ \[-Rpass.*//' | paste - - - - - - - \
   | sed -e 's/Function Name: _ZN2sg4grad//' -e 's/EEvPKT_[^\t]*//'
  rm -f /tmp/kg_regs_$$.o
  exit 0
fi
if [ "$1" = "xcorr" ]; then
  shift
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function "$@" -Rpass-analysis=kernel-resource-usage -c kernels_xcorr.hip -o /tmp/kx_regs_$$.o 2>&1 \
   | grep -E "Function Name|    VGPRs:|AGPRs:|VGPRs Spill|ScratchSize|Occupancy|LDS Size" | sed -e 's/.*remark: *//' -e 's/ \[-Rpass.*//' | paste - - - - - - - \
   | sed -e 's/Function Name: _ZN2sg5xcorr[0-9]*//' -e 's/EEvNS0_4ArgsE//' -e 's/EvNS0_4ArgsE//'
  rm -f /tmp/kx_regs_$$.o
  exit 0
fi
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function "$@" -Rpass-analysis=kernel-resource-usage -c kernels_mfma.hip -o /tmp/km_regs_$$.o 2>&1 \
 | grep -E "Function Name|    VGPRs:|VGPR Spill|ScratchSize|Occupancy" | sed -e 's/.*remark: *//' -e 's/ \[-Rpass.*//' | paste - - - - - \
 | grep -E "Id?Li4E" | sed -e 's/Function Name: _ZN2sg12mfma_stage_//' -e 's/EEvNS_9StageArgsE//'
rm -f /tmp/km_regs_$$.o
