// Philox4x32-10 counter-based RNG and the Box-Muller Gaussian shared by the differential-privacy kernels
// (csrc/dp.hip: DP-SGD aggregation and PATE; csrc/wd_general.hip: the noise of the private Wide&Deep step).
// mifx.ops.dp.philox4x32 / gaussian_noise_reference are the host twins (same bits up to the device's logf /
// sincosf). Included inside each translation unit's anonymous namespace.
#pragma once

struct U4 {
  uint32_t x, y, z, w;
};

__device__ __forceinline__ U4 philox(U4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c.x;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c.z;
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
    const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    c = U4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

// uniform in (0, 1]: never 0, so log() is finite
__device__ __forceinline__ float u01(uint32_t v) { return ((float)(v >> 8) + 1.0f) * (1.0f / 16777216.0f); }

__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float& z0, float& z1) {
  const float r = sqrtf(-2.0f * logf(u01(a)));
  float s, c;
  sincosf(6.283185307179586f * u01(b), &s, &c);
  z0 = r * c;
  z1 = r * s;
}
