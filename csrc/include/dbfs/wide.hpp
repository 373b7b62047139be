// Extended-range non-negative values for the betweenness sweeps: m * 2^e with
// m a double and e an int32 -- path counts past 2^1024 and the coefficients
// (1 + delta) / sigma below 2^-1074 that go with them.  One definition for the
// kernels (ms_bc_kernels.hip), the CPU backend and the oracle cpu_betweenness.
//
// Stored form (frexp's): m in [0.5, 1), or m == 0 and e == 0.  A running sum
// (WideSum) is not normalised per term: its m is any double >= 0 and its e the
// largest exponent met so far; wide_normalise brings it to the stored form
// once per row.
//
// Every rounding is the one the plain double operation would make: an operand
// is aligned by an exact power-of-two scaling, the mantissas are added (or
// multiplied, divided) as doubles, and a scaled operand more than 2^1022 below
// the other -- far under half an ulp -- is dropped.  Where every value and
// result is a normal double, wide arithmetic gives the double result bit for
// bit.  The exponent: a count is below (longest row)^depth with depth < 65535,
// so |e| stays below about 2^21.
//
// ldexp and frexp are single FP64 instructions on gfx950 (v_ldexp_f64,
// v_frexp_mant_f64 / v_frexp_exp_i32_f64): no table, no loop.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DBFS_WIDE_FN __host__ __device__ inline
#else
#define DBFS_WIDE_FN inline
#endif

namespace dbfs {

// Bytes of a vertex's record in a wide value matrix: the kMsSources (64)
// mantissas, then their exponents.
constexpr int kWideLanes = 64;
constexpr int64_t kWideRecord = kWideLanes * (sizeof(double) + sizeof(int32_t));  // 768
constexpr int64_t kWideExpOffset = kWideLanes * sizeof(double);                   // 512

// The exponent of a sum that holds nothing yet (and of a zero operand while it
// is aligned): below every real one by far more than 1022, and far enough from
// INT32_MIN that differences and sums of two exponents do not wrap.
constexpr int32_t kWideNoExp = -(int32_t(1) << 29);
constexpr int32_t kWideDrop = 1022;

struct Wide {
  double m;
  int32_t e;
};
using WideSum = Wide;

DBFS_WIDE_FN Wide wide_zero() { return Wide{0.0, 0}; }
DBFS_WIDE_FN Wide wide_one() { return Wide{0.5, 1}; }
DBFS_WIDE_FN WideSum wide_sum_zero() { return WideSum{0.0, kWideNoExp}; }

// m * 2^d, exactly; 0 where d < -1022 (the dropped operand).
DBFS_WIDE_FN double wide_scale(double m, int32_t d) { return d < -kWideDrop ? 0.0 : __builtin_ldexp(m, d); }

// sum += x.  x is a stored value or another running sum; a zero on either
// side, whatever its exponent, leaves the other operand's bits.
DBFS_WIDE_FN void wide_add(WideSum& sum, Wide x) {
  const int32_t se = sum.m == 0.0 ? kWideNoExp : sum.e;
  const int32_t xe = x.m == 0.0 ? kWideNoExp : x.e;
  const int32_t e = se > xe ? se : xe;
  sum.m = wide_scale(sum.m, se - e) + wide_scale(x.m, xe - e);
  sum.e = e;
}

// A running sum (or any m >= 0 with its exponent) in the stored form.
DBFS_WIDE_FN Wide wide_normalise(Wide x) {
  int de = 0;
  const double m = __builtin_frexp(x.m, &de);
  return m == 0.0 ? wide_zero() : Wide{m, x.e + static_cast<int32_t>(de)};
}

DBFS_WIDE_FN Wide wide_from_double(double x) { return wide_normalise(Wide{x, 0}); }

// The value as a double: inf past DBL_MAX, flushed gradually towards 0 below
// 2^-1022 (one rounding of the exact value: m has 53 bits).
DBFS_WIDE_FN double wide_to_double(Wide x) {
  const int32_t e = x.e > 4096 ? 4096 : (x.e < -4096 ? -4096 : x.e);
  return __builtin_ldexp(x.m, e);
}

// delta = sigma * acc as a double (sigma stored, acc a running sum; the value
// is at most n, so it never overflows, and it is flushed gradually towards 0
// when tiny): acc is scaled by 2^sigma.e, exactly, and multiplied by sigma's
// mantissa -- the product the double form rounds.  With wide_coefficient
// below this is written as the double form writes (1 + sigma * acc) / sigma,
// so a compiler that fuses the multiply into the 1 + there (the device's
// does) fuses the same two operations here, and both forms keep the same bits.
DBFS_WIDE_FN double wide_delta(Wide sigma, WideSum acc) {
  return sigma.m * wide_to_double(Wide{acc.m, sigma.e + acc.e});
}

// a / b as a double (the oracle's sigma[v] / sigma[w]); b > 0.
DBFS_WIDE_FN double wide_div_to_double(Wide a, Wide b) {
  return wide_to_double(Wide{a.m / b.m, a.e - b.e});
}

// (1 + delta) / sigma in the stored form; sigma > 0 stored, delta >= 0.
DBFS_WIDE_FN Wide wide_coefficient(double delta, Wide sigma) {
  return wide_normalise(Wide{(1.0 + delta) / sigma.m, -sigma.e});
}

// A vertex's record in a wide matrix: lane s's value.
DBFS_WIDE_FN Wide wide_load(const unsigned char* base, int64_t v, int s) {
  const unsigned char* rec = base + v * kWideRecord;
  return Wide{reinterpret_cast<const double*>(rec)[s], reinterpret_cast<const int32_t*>(rec + kWideExpOffset)[s]};
}
DBFS_WIDE_FN void wide_store(unsigned char* base, int64_t v, int s, Wide x) {
  unsigned char* rec = base + v * kWideRecord;
  reinterpret_cast<double*>(rec)[s] = x.m;
  reinterpret_cast<int32_t*>(rec + kWideExpOffset)[s] = x.e;
}

}  // namespace dbfs
