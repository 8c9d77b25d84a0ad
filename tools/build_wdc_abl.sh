#!/bin/bash
# ablation builds of the chained W&D kernels (csrc/wd_chain.hip, WDC_ABL), same flags as the production builds:
# tools/bin/libwd_chain{,64,256}_abl<bits>.so for every <bits> given (default 1 4 8). A/B them as library overrides:
#   tools/ab.sh new abl1=MIFX_LIB_WD_CHAIN=tools/bin/libwd_chain_abl1.so,MIFX_LIB_WD_CHAIN64=tools/bin/libwd_chain64_abl1.so,MIFX_LIB_WD_CHAIN256=tools/bin/libwd_chain256_abl1.so -- python -u bench.py
cd "$(dirname "$0")/.." && mkdir -p tools/bin || exit 1
F=$(grep '^// MIFX_HIPCC_FLAGS:' csrc/wd_chain.hip | cut -d: -f2-)
for a in ${@:-1 4 8}; do
  for v in "wd_chain.hip libwd_chain" "wd_chain64.hip libwd_chain64" "wd_chain256.hip libwd_chain256"; do
    set -- $v
    hipcc --offload-arch=gfx950 -O3 -shared -fPIC -Icsrc -DWDC_ABL=$a $F -o tools/bin/$2_abl$a.so csrc/$1 || exit 1
  done
done
