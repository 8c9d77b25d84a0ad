// Radix keys of csrc/gbdt_sort.hip: the order-preserving unsigned image of a float / double and its inverse, for host
// and device. A negative value has all its bits flipped, a non-negative one its sign bit, so unsigned order of the keys
// is numeric order of the values with -0.0 before +0.0. Every NaN, of any sign or payload, becomes the all-ones key
// (no other value maps there: it would be the bits of a NaN), so NaNs sort last and come back as one positive NaN.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define MIFX_SORT_HD __host__ __device__ inline
#else
#define MIFX_SORT_HD inline
#endif

MIFX_SORT_HD uint64_t mifx_sort_key(double x) {
  uint64_t b;
  memcpy(&b, &x, 8);
  if ((b & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) return ~0ull;
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

MIFX_SORT_HD uint32_t mifx_sort_key(float x) {
  uint32_t b;
  memcpy(&b, &x, 4);
  if ((b & 0x7FFFFFFFu) > 0x7F800000u) return ~0u;
  return (b >> 31) ? ~b : (b | 0x80000000u);
}

MIFX_SORT_HD double mifx_sort_value(uint64_t k) {
  const uint64_t b = (k >> 63) ? (k ^ 0x8000000000000000ull) : ~k;
  double x;
  memcpy(&x, &b, 8);
  return x;
}

// a 32-bit key is the key of a float: its value widened exactly
MIFX_SORT_HD double mifx_sort_value(uint32_t k) {
  const uint32_t b = (k >> 31) ? (k ^ 0x80000000u) : ~k;
  float x;
  memcpy(&x, &b, 4);
  return (double)x;
}
