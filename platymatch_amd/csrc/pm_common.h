// pm_common.h — shared device helpers for the gfx950 kernels (wave64, float64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/platymatch_hip.h"
#include "pm_seed_short.h"

#define PM_WAVE 64

// Every arithmetic statement in these kernels is one IEEE rounding: the translation units are
// compiled with -ffp-contract=off and fused operations are written explicitly (__builtin_fma).

namespace pm {

extern thread_local int g_last_hip_error;

inline int launch_status() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        g_last_hip_error = (int)e;
        return PM_ERR_LAUNCH;
    }
    return PM_OK;
}

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ---- deterministic reductions (fixed tree: lane butterfly, then waves in order) ------------------
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, PM_WAVE);
    return v;  // valid in lane 0
}

// Block sum of one double per thread; result valid in thread 0.  `scratch` holds >= blockDim/64 doubles.
__device__ __forceinline__ double block_sum(double v, double *scratch) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    v = wave_sum(v);
    __syncthreads();  // scratch may still be read from a previous call
    if (lane == 0) scratch[wave] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < nw; ++w) r += scratch[w];
    return r;
}

// n / d, correctly rounded, for finite positive d and finite n >= 0 well inside the exponent range (no
// scaling / fix-up needed).  v_rcp_f64 is good to 2^-24.4 on gfx950 (tools/microbench/rcp_accuracy.hip); one
// cubic step r <- r + r*(e + e*e), e = 1 - d*r, leaves a truncation error of e^3 < 2^-73, i.e. the reciprocal
// rounded to nearest in all but ~2^-20 of cases and within 0.5000005 ulp otherwise; the quotient then gets the
// usual exact-residual correction (Markstein).  This is LLVM's AMDGPU f64 division with its two Newton steps
// fused into one (one fma fewer) and without div_scale/div_fixup; it is checked bit for bit against IEEE
// division on 1.3e11 operands, a third of them built to sit within 2^-53 ulp of a rounding midpoint
// (tools/microbench/div_check.hip, also run by the gpu test-suite), and by every chi-square parity test.
__device__ __forceinline__ double div_pos(double n, double d) {
    double r = __builtin_amdgcn_rcp(d);
    const double e = __builtin_fma(-d, r, 1.0);
    const double t = __builtin_fma(e, e, e);
    r = __builtin_fma(r, t, r);
    const double q = n * r;
    const double res = __builtin_fma(-d, q, n);
    return __builtin_fma(res, r, q);
}

// n / d as div_pos, with the reciprocal taken from a table instead of v_rcp_f64: for the chi-square denominators of two clouds
// with ONE common total T.  d = fl(fl(ca/T) + fl(cb/T)) for integer counts ca, cb (a zero cb staged as 1e-300 adds nothing), so
// d = (s/T)(1 + theta) with s = ca + cb and |theta| <= 3 * 2^-53 (two divisions' roundings, each weighted by its share of the sum,
// and the addition's).  r0 = R[s] = fl(T/s) = (T/s)(1 + rho), |rho| <= 2^-53, is therefore a reciprocal of d with relative
// error |1 - d r0| <= 4 * 2^-53 + O(2^-105) < 2^-51.  One Newton step r = r0 + r0 e, e = fl(1 - d r0) (exact up to its own
// rounding of a quantity below 2^-51, i.e. to 2^-104), leaves a truncation error e^2 <= 2^-102 before r's rounding — tighter than
// div_pos's 2^-73 after its cubic step — and the quotient gets the same exact-residual correction.  s = 0 (both counts zero:
// d = 1e-300, n = 1e-600 = 0): R[0] = 1 gives r = 2, q = 0, res = 0, result +0 = 0 / 1e-300.  Checked bit for bit against IEEE
// division over every (ca, cb) with ca + cb < 8 836 for several totals, on the device and on the host
// (tools/microbench/seed_div_check.hip, run by the test-suite both ways).
// The chi-square kernels no longer call it: they divide by div_seeded_short (pm_seed_short.h: the same tail on r0 itself, no
// Newton step), which has no such argument behind it and is therefore CERTIFIED per launch — seed_cert_kernel (pm_chi2.hip)
// evaluates seed_short_pair_ok on the device for every count pair the launch can meet, with the launch's own T, before the cost
// kernel starts; one failing pair and the launch seeds nothing (every term by div_pos, as under PM_CHI2_SEED=0).  div_seeded
// stays as the proven sequence the microbenchmark and its test hold against IEEE division.
__device__ __forceinline__ double div_seeded(double n, double d, double r0) {
    const double e = __builtin_fma(-d, r0, 1.0);
    const double r = __builtin_fma(r0, e, r0);
    const double q = n * r;
    const double res = __builtin_fma(-d, q, n);
    return __builtin_fma(res, r, q);
}

// Byte offset of R[s] for the denominator d above, in ONE instruction: m = fl(d T + 2^49) has an ulp of 1/8, and d T lies within
// s * 2^-51 < 1/16 of the integer s (s < 2^13), so m = 2^49 + s exactly and the low dword of its bit pattern is 8 s.  `magic` is
// 2^49 + base/8 for a table at the (8-byte aligned, < 2^16) address `base`: the low dword is then base + 8 s, the address itself.
__device__ __forceinline__ unsigned int seed_offset(double d, double T, double magic = 0x1p49) {
    return (unsigned int)__double2loint(__builtin_fma(d, T, magic));
}

}  // namespace pm
