// The register-chained fused Wide&Deep training step (csrc/wd_chain.hip) built for T = 256 examples per workgroup
// iteration: 8 waves x 32 examples (two 16-example column blocks per wave, like the 4-wave T = 128 shape, at two waves
// per SIMD). The large-batch shape: at B = 65536 on 256 workgroups each workgroup runs ONE iteration instead of two,
// so the dependent forward / activation-gradient chains of its 256 examples run once, with both column blocks'
// MFMAs interleaved in each wave, and the per-iteration fixed costs (record fetch, wide gather, loss, the layer
// barriers) are paid once. One iteration per workgroup also means that a layer's weights are dead once the backward
// has passed it: the image is placed in LDS rotated (W2 | W3 | W4 | W5 | W1) and each layer stages its full 256 rows
// of dW operands once, from where the dead weights begin (csrc/wd_chain.hip, "LDS placement"). Same global weight
// image, tile map and gradient slab as the T = 128 library; exported names end in _t256.
//
// MIFX_HIPCC_FLAGS: -fno-honor-nans -fno-honor-infinities -mllvm -amdgpu-kernarg-preload-count=14
#define WDC_T 256
#include "wd_chain.hip"
