// exact_div.h -- exact unsigned 32-bit division by a launch constant without a divide: host and device.
//
// gfx950 has no integer divide; a `/` by a value the compiler does not know becomes a float-reciprocal sequence of some 20 VALU instructions
// (four of them quarter-rate multiplies).  Every divisor of the render kernels' pixel bookkeeping (samples per launch, sensor width, rows per
// stripe) is the same for all paths of a launch, so the host forms, once per launch, the multiplier of the Granlund-Montgomery round-up form
// ("Division by invariant integers using multiplication", PLDI 1994, figure 4.1, N = 32):
//   l = ceil(log2 d),  m' = floor(2^32 * (2^l - d) / d) + 1,  sh1 = min(l, 1),  sh2 = max(l - 1, 0)
//   t = mulhi(m', n),  n / d = (t + ((n - t) >> sh1)) >> sh2           for EVERY n < 2^32 and 1 <= d < 2^32
// (t <= n, and t + ((n - t) >> sh1) <= n: nothing overflows).  On the device: a quarter-rate v_mul_hi_u32, a subtract, two shifts and an add.
// Two dwords, so that a record is a kernel argument ColdArgs::Get can read (pt_args.h).  d = 0 gives a record that must not be used.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AMBER_EXACT_DIV_FN __host__ __device__ inline
#else
#define AMBER_EXACT_DIV_FN inline
#endif

struct ExactDiv {
  uint32_t mul;      // m'
  uint32_t shifts;   // sh1 | sh2 << 16
};

AMBER_EXACT_DIV_FN ExactDiv MakeExactDiv(uint32_t d) {
  if (d == 0u) return ExactDiv{0u, 0u};
  uint32_t l = 0;
  while (l < 32u && (static_cast<uint64_t>(1) << l) < d) ++l;
  const uint64_t m = (((static_cast<uint64_t>(1) << l) - d) << 32) / d + 1u;      // (2^l - d) < d <= 2^32 - 1: the product fits 64 bits, m < 2^32
  return ExactDiv{static_cast<uint32_t>(m), (l < 1u ? l : 1u) | ((l > 1u ? l - 1u : 0u) << 16)};
}

// n / d
AMBER_EXACT_DIV_FN uint32_t Quotient(ExactDiv dv, uint32_t n) {
  const uint32_t t = static_cast<uint32_t>((static_cast<uint64_t>(dv.mul) * n) >> 32);
  return (t + ((n - t) >> (dv.shifts & 0xffffu))) >> (dv.shifts >> 16);
}

// n % d, given d again (the record does not hold it)
AMBER_EXACT_DIV_FN uint32_t Remainder(ExactDiv dv, uint32_t d, uint32_t n) { return n - Quotient(dv, n) * d; }
