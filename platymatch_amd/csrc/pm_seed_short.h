// pm_seed_short.h — the table-seeded division WITHOUT its Newton step, and the per-pair predicate that certifies it.  Plain C++
// (no HIP header): pm_common.h includes it for the kernels, tools/microbench/seed_short_host.cpp for the host sweep.
#pragma once
#include <string.h>

#if defined(__HIPCC__)
#define PM_SEED_HD __host__ __device__ __forceinline__
#else
#define PM_SEED_HD static inline
#endif

namespace pm {

// n / d with the table seed r0 = R[s] of div_seeded (pm_common.h) used AS the reciprocal: q = fl(n r0), exact residual, one
// correction — 3 instructions instead of 5.  r0 is good to 2^-51 only, so the corrected quotient sits within about q * 2^-101.7
// of n / d before its rounding, while n / d can lie within q * 2^-107 of a rounding midpoint: NOT correctly rounded in general,
// and nobody has a proof for the chi-square operands either.  It is used only where seed_short_pair_ok below has held for every
// count pair a launch can meet, for that launch's total (seed_cert_kernel, pm_chi2.hip).
PM_SEED_HD double div_seeded_short(double n, double d, double r0) {
    const double q = n * r0;
    const double res = __builtin_fma(-d, q, n);
    return __builtin_fma(res, r0, q);
}

PM_SEED_HD unsigned long long seed_bits(double x) {
    unsigned long long u;
    memcpy(&u, &x, 8);
    return u;
}

// The certificate's predicate for ONE count pair.  Operands exactly as the kernels stage them for two clouds of total T:
// a = fl(ca/T), b = fl(cb/T) or 1e-300 for cb = 0, n = fl(df df), d = fl(a + b); the seed is found as the kernels find it (the
// low dword of fma(d, T, 2^49) is 8 s: seed_offset) in R, where R[i] holds entry r_base + i of R[s] = s ? div(T, s) : 1.  True
// iff the index is s = ca + cb and the short quotient has the bits of div(n, d).  `div` is the reference division: div_pos on the
// device (what fills R and computes every unseeded term there), IEEE n / d on the host.
template <class Div>
PM_SEED_HD bool seed_short_pair_ok(int ca, int cb, double T, const double *R, int r_base, Div div) {
    const double a = (double)ca / T, b = cb ? (double)cb / T : 1e-300;
    const double df = a - b, n = df * df, d = a + b;
    const unsigned int off = (unsigned int)seed_bits(__builtin_fma(d, T, 0x1p49));
    if (off != 8u * (unsigned int)(ca + cb)) return false;
    const double r0 = R[(int)(off >> 3) - r_base];
    return seed_bits(div_seeded_short(n, d, r0)) == seed_bits(div(n, d));
}

}  // namespace pm
