// seed_div_check.hip — is the table-seeded float64 division (pm::div_seeded, pm_common.h) still correctly rounded, and is the
// one-instruction table index (pm::seed_offset) exact?  For two clouds with one common total T the chi-square term of the counts
// (ca, cb) is (df * df) / d with a = fl(ca/T), b = fl(cb/T) (1e-300 for cb = 0, as the kernels stage it), df = a - b, d = a + b.
// Exhaustively, for every (ca, cb) with s = ca + cb < 8 836 = 94^2 and every T of the list:
//   index    low dword of the bits of fma(d, T, 2^49) must be 8 s
//   term     R[s] = fl(T/s) (R[0] = 1), e = fma(-d, R, 1), r = fma(R, e, R), q = n r, res = fma(-d, q, n), fma(res, r, q)
//            must have the bits of IEEE n / d
//   recip    r against the correctly rounded 1 / d (reported)
//   control  the same tail with r = R[s], no Newton step (reported; nobody has shown that it fails on this domain)
// One source, two builds:  hipcc -O3 --offload-arch=gfx950 -ffp-contract=off   (runs on the device)
//                          c++ -x c++ -O2 -ffp-contract=off                    (runs on the host, std::fma)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define SD_FN __device__ __forceinline__
#define SD_FMA(a, b, c) __builtin_fma(a, b, c)
#else
#include <cmath>
#define SD_FN static inline
#define SD_FMA(a, b, c) std::fma(a, b, c)
#endif

constexpr int NSEED = 94 * 94;

SD_FN unsigned long long sd_bits(double x) {
    unsigned long long u;
    memcpy(&u, &x, 8);
    return u;
}

// counters: 0 index, 1 term, 2 reciprocal, 3 control
SD_FN void check_pair(int ca, int cb, double T, const double *R, unsigned long long *bad) {
    const double a = (double)ca / T, b = cb ? (double)cb / T : 1e-300;
    const double df = a - b, n = df * df, d = a + b;
    const int s = ca + cb;
    const double m = SD_FMA(d, T, 0x1p49);
    bad[0] += (unsigned int)sd_bits(m) != 8u * (unsigned int)s;
    const double r0 = R[s];                                  // (indexed by the true s: a wrong index is counted, never followed)
    const double e = SD_FMA(-d, r0, 1.0);
    const double r = SD_FMA(r0, e, r0);
    double q = n * r, res = SD_FMA(-d, q, n);
    const double ref = n / d;
    bad[1] += sd_bits(SD_FMA(res, r, q)) != sd_bits(ref);
    bad[2] += sd_bits(r) != sd_bits(1.0 / d);
    q = n * r0, res = SD_FMA(-d, q, n);
    bad[3] += sd_bits(SD_FMA(res, r0, q)) != sd_bits(ref);
}

#if defined(__HIP__)
// pm::div_pos (v_rcp_f64, one cubic step, residual correction): what fills R in the kernel
__device__ __forceinline__ double div_pos(double n, double d) {
    double r = __builtin_amdgcn_rcp(d);
    const double e = __builtin_fma(-d, r, 1.0);
    const double t = __builtin_fma(e, e, e);
    r = __builtin_fma(r, t, r);
    const double q = n * r;
    const double res = __builtin_fma(-d, q, n);
    return __builtin_fma(res, r, q);
}
__global__ void fill(double *R, double T) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < NSEED) R[s] = s ? div_pos(T, (double)s) : 1.0;
}
// one block per ca, its threads stride over cb
__global__ void check(const double *R, double T, unsigned long long *bad) {
    const int ca = blockIdx.x;
    unsigned long long mine[4] = {0, 0, 0, 0};
    for (int cb = threadIdx.x; ca + cb < NSEED; cb += blockDim.x) check_pair(ca, cb, T, R, mine);
    for (int k = 0; k < 4; ++k)
        if (mine[k]) atomicAdd(&bad[k], mine[k]);
}
#define SD_OK(x)                                                           \
    do {                                                                   \
        if ((x) != hipSuccess) {                                           \
            fprintf(stderr, "HIP error at line %d\n", __LINE__);           \
            return 1;                                                      \
        }                                                                  \
    } while (0)
#endif

int main() {
    const int totals[4] = {999, 19999, 49999, 199999};
#if defined(__HIP__)
    double *R;
    unsigned long long *bad;
    SD_OK(hipMalloc(&R, NSEED * sizeof(double)));
    SD_OK(hipMalloc(&bad, 4 * sizeof(unsigned long long)));
#else
    std::vector<double> Rv(NSEED);
    double *R = Rv.data();
#endif
    for (int it = 0; it < 4; ++it) {
        const double T = (double)totals[it];
        unsigned long long h[4] = {0, 0, 0, 0};
#if defined(__HIP__)
        SD_OK(hipMemset(bad, 0, 4 * sizeof(unsigned long long)));
        fill<<<(NSEED + 255) / 256, 256>>>(R, T);
        check<<<NSEED, 256>>>(R, T, bad);
        SD_OK(hipDeviceSynchronize());
        SD_OK(hipMemcpy(h, bad, sizeof(h), hipMemcpyDeviceToHost));
#else
        R[0] = 1.0;
        for (int s = 1; s < NSEED; ++s) R[s] = T / (double)s;
        for (int ca = 0; ca < NSEED; ++ca)
            for (int cb = 0; ca + cb < NSEED; ++cb) check_pair(ca, cb, T, R, h);
#endif
        printf("T %d pairs %llu index_bad %llu term_bad %llu recip_bad %llu control_bad %llu\n", totals[it],
               (unsigned long long)NSEED * (NSEED + 1) / 2, h[0], h[1], h[2], h[3]);
    }
    return 0;
}
