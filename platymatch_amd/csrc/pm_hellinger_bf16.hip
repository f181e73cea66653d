// pm_hellinger_bf16.hip — priced selection from the Hellinger lower bound on the bf16 matrix path: split-bf16, three products.
//
// pm_hellinger.hip's hl_select_kernel answers a solver's row_select(v, k) with v_mfma_f32_32x32x2f32 and is bound by the matrix
// issue rate.  Here every sqrt-descriptor x is split into two bf16 pieces, hi = bf16(x) and lo = bf16(x - hi) (round to nearest
// even, the subtraction exact in float64), and the product of two descriptors is taken as hi.hi + hi.lo + lo.hi with
// v_mfma_f32_32x32x16_bf16: three instructions per 16 bins where the float32 path issues eight, at half the passes each.  The
// semantics are hl_select_kernel's: key = L~ - v_j in float64, L~ = (hA_i + hB_j) - (double)dot in that order, per-row state of
// hA, tau, a count and CAP slots of (dot, column), appends through an LDS atomic, a full buffer cut to its k smallest by
// (key, column) by one wave, the ovf retry protocol, a non-finite price handled as hB := +inf, output (column, BOUND) ascending by
// (key, column), partial lists per split merged by pm_hellinger.hip's hl_select_merge_kernel (launched from here as it is).
// k <= 32 only (the public unary_distance_nearest asks for 32 candidates); k > 32 is an argument error under this precision:
// pm_hellinger_select (float32) serves k up to 64.
// The bounds are valid under their OWN constant PM_HELLINGER_DELTA_BF16X3 (below); their bits differ from the float32 kernels',
// so the "same bits as pm_hellinger_topk / pm_hellinger_list" clause of pm_hellinger_select does NOT carry over: lists of the two
// precisions are both valid, each under its own delta, and are not to be mixed entry by entry.
//
// Layout (hlb_prep_kernel).  Bins are padded with zeros from 360 to 384 = 24 steps of 16: zero operands add exact zeros, the bound
// does not move.  (368 = 23 x 16 would save 4 % of the MFMAs, but 23 is prime: a stage could only be one step or a whole tile;
// 24 leaves the stage shape free and every offset a power-of-two multiple.)  Rows are stored in BLOCKS of 64; a block holds, per
// group of 8 bins g = 0..47, the hi pieces of its 64 rows (64 x 16 bytes) and then the lo pieces (64 x 16 bytes): element
// (row r, bin q, piece p) sits at byte ((q / 8) * 2 + p) * 1024 + r * 16 + (q % 8) * 2 of a block of 98 304 bytes.
//   - a lane's MFMA operand (8 consecutive bins of row lane % 32, bin group lane / 32) is ONE 16-byte LDS read;
//   - the 32 lanes of a half-wave read 512 contiguous bytes, the other half-wave 512 contiguous bytes 2 048 further: every
//     quarter-wave of a ds_read_b128 covers all 64 banks once — conflict-free without padding;
//   - one step (16 bins, both pieces) of a block is 4 096 contiguous bytes: a stage travels global -> registers -> LDS as it lies.
// Rows past the end and non-finite rows are zero rows with h = NaN (moving) / +inf (fixed), as hl_prep_kernel leaves them.
//
// Geometry (hl_select_bf16_kernel).  Against the float32 kernel the MFMA time per tile drops from 46 080 to 24 x 12 x 32 = 9 216
// cycles per wave, the bytes per element stay 4: a 128 x 128 tile with both operands streamed would ask ~21 B/cycle/CU of each
// side.  So a 512-thread workgroup owns a PANEL of 256 moving rows against tiles of 128 fixed rows (half the fixed traffic per
// MFMA), eight waves of 64 x 64 (wave w: row block w % 4, column block w / 4) as four 32 x 32 accumulators.  Budget:
//   - rows per workgroup 256, columns per tile 128, bins per stage 16 (one step), two LDS stages of 16 KB (panel) + 8 KB (tile):
//     three 16-byte copies per thread per stage, loaded before the stage's MFMAs and stored after them, one barrier per stage.
//     (One stage is only ~770 MFMA cycles per SIMD, about what a load from L2 takes: at 12.4 ms for 20 000 x 20 000 x 4, k = 16
//     (profiles/hellinger_select_bf16_20k.txt) the kernel runs far below its MFMA time, and stages waiting for their loads are
//     the SUPPOSED cause — no counter pass was taken.  Loading three stages ahead through four register slots was tried: it
//     spilt to scratch beside the 64 accumulators; a deeper LDS ring has no room beside the rows' state.)
//   - per step and wave 8 ds_read_b128 (2 row halves + 2 column halves, hi and lo) feed 12 MFMAs in the FIXED order hi.hi, hi.lo,
//     lo.hi (each over the four quadrants), bins in index order: an entry's bits depend on nothing else — not on the split, not
//     on the launch geometry.  8 KB of LDS reads per 384 MFMA cycles and wave: 2/3 of the LDS rate at two waves per SIMD (a
//     64 x 32 wave tile would sit at the limit);
//   - state of 256 rows: CAP = 32 for k <= 16 (64 KB), CAP = 48 for k <= 32 (96 KB); with 48 KB of stages and 7 KB of hA, tau,
//     thresholds, counts and ranking scratch: 119 KB / 153 KB of the 160 KB — ONE workgroup per CU, two waves per SIMD, up to 256
//     registers per lane (64 of them accumulators); no scratch (tools/kernel_resources.py);
//   - epilogue: 64 keys per lane per tile would cost ~1/5 of the tile's MFMA time in float64, so a conservative float32 pre-test
//     goes first: an entry is REJECTED only if dot < s_j - t_i in float32, s_j = (hB_j - v_j) lowered and t_i = (tau_i - hA_i)
//     raised by 2^-21 of the operands' magnitudes (+ 1e-30) — four times what the three float32 roundings, the float64 ones and
//     the conversions can amount to (each <= 2^-24 of those magnitudes), so nothing the float64 test would accept is rejected;
//     any NaN in the pre-test passes.  Whatever passes is tested again in float64, by hl_select_kernel's operations, and only
//     that comparison decides.  (Under prices of size 1e6 the pre-test passes nearly everything: correct, not fast.)
//   - workgroups are numbered so that the ~32 that an XCD (32 CUs, one 4 MB L2) holds at a time are 4 panels x 8 column ranges:
//     workgroup L of a launch runs on XCD L % 8, and XCD x takes the work items x * per .. (x + 1) * per - 1 in order, 32
//     consecutive items being such a 4 x 8 group.  The 4 panels (1.5 MB) stay in that L2 and each streamed fixed tile serves four
//     workgroups.  This is a matter of speed only.
//
// Error bound.  PM_HELLINGER_DELTA_BF16X3 bounds |L~ - L| for descriptor rows with sum a, sum b <= 1.  w = 2^-8 (bf16 carries 8
// significant bits), u = 2^-24.  With x = sqrt(a) (correctly rounded in float64; its 2^-53 vanishes below): x = hi + lo + r,
// |x - hi| <= w x, hence |lo| <= w (1 + w) x and |r| <= w |x - hi| <= w^2 x.  xa xb - (ha hb + ha lb + la hb) = la lb + ra xb +
// rb (xa - ra), at most ((1 + w)^2 + 1 + (1 + w^2)) w^2 xa xb <= 3.008 w^2 xa xb; summed over the bins, with sum xa xb <=
// sqrt(sum a sum b) <= 1 (Cauchy-Schwarz): 4.590e-5.  Products of two bf16 values are exact in float32.  ASSUMPTION: an elementary
// addition inside the MFMA errs by at most 2u of the magnitudes it adds (u for a correctly rounded adder; the factor two covers a
// truncating one), whatever the order in which the instruction adds its 16 products to the accumulator.  There are 3 x 360
// products that are not exact zeros, one addition each, and every partial sum is at most sum (ha hb + ha |lb| + |la| hb) <=
// (1 + w)^2 (1 + 2w) <= 1.0158 (+ the accumulated error itself, a factor 1 + 2e-4): 1080 x 2u x 1.016 = 1.308e-4.  The padding
// adds exact zeros.  Together 1.767e-4; pieces below the float32 normal range (< 1.2e-38, truncated or flushed) and the float64
// epilogue (3 x 2^-53) vanish in the slack of the constant below.  Every contract sentence of pm_hellinger_select then holds with
// this delta in place of pm_hellinger_delta.
#include <limits.h>

#include "pm_hellinger.h"

#define PM_HELLINGER_DELTA_BF16X3 1.77e-4

namespace pm {

constexpr int HLB_BLK = HL_BM;                         // rows per block of the layout
constexpr int HLB_STEPS = 24;                          // 16-bin steps per tile (384 bins, 360 of them real)
constexpr int HLB_GROUPS = 2 * HLB_STEPS;              // 8-bin groups
constexpr int HLB_BLK_U4 = HLB_GROUPS * 2 * HLB_BLK;   // 16-byte pieces of a block (6 144)
constexpr int HLB_STEP_U4 = 4 * HLB_BLK;               // 16-byte pieces of one step of a block (256)
constexpr int HLB_PM = 256;                            // moving rows per panel
constexpr int HLB_TN = 128;                            // fixed rows per tile
constexpr int HLB_THREADS = 512;
constexpr int HLB_KMAX = 32;
constexpr int HLB_XP = 4, HLB_XR = 8;                  // panels x column ranges of the group an XCD holds at a time
static_assert(16 * HLB_STEPS >= PM_NBINS && HLB_PM == 4 * HLB_BLK && HLB_TN == 2 * HLB_BLK && HLB_THREADS == 2 * HLB_STEP_U4 &&
                  HLB_XP * HLB_XR == 32,
              "geometry");

typedef __bf16 hlb_bf8 __attribute__((ext_vector_type(8)));
typedef unsigned int hlb_u4 __attribute__((ext_vector_type(4)));      // a 16-byte piece in registers and LDS

// x rounded to bf16 (nearest, ties to even, from the float64 value itself: no double rounding); val: what the 16 bits stand for
__device__ __forceinline__ unsigned int hlb_bf16(double x, double &val) {
    unsigned long long b = (unsigned long long)__double_as_longlong(x);
    b += 0xFFFFFFFFFFFull + ((b >> 45) & 1ull);
    b &= ~((1ull << 45) - 1ull);
    const unsigned int fb = __float_as_uint((float)__longlong_as_double((long long)b)) & 0xffff0000u;
    val = (double)__uint_as_float(fb);
    return fb >> 16;
}

// The split sqrt-descriptors in the layout above + half row sums (bin order, float64, as hl_prep_kernel adds them).  One thread
// per row of the padded cloud (n_pad: a multiple of 64), blockIdx.y = frame.  bad: what h holds for a non-finite / padding row.
__global__ __launch_bounds__(256) void hlb_prep_kernel(const double *__restrict__ sc, size_t frame_stride, int n, int n_pad,
                                                       uint4 *__restrict__ rt, double *__restrict__ h, double bad,
                                                       int32_t *__restrict__ nonfinite1) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pad) return;
    const int f = blockIdx.y, r = i & 63;
    const double *row = sc + (size_t)f * frame_stride + (size_t)i * PM_NBINS;
    uint4 *dst = rt + ((size_t)f * (n_pad / HLB_BLK) + i / HLB_BLK) * HLB_BLK_U4 + r;
    const double inf = __builtin_inf();
    bool ok = i < n;
    double s = 0.0;
    if (ok) {
        for (int q = 0; q < PM_NBINS; ++q) {
            const double x = row[q];
            ok = ok && (x >= 0.0) && (x < inf);
            s += x;
        }
        ok = ok && (s < inf);
    }
    for (int g = 0; g < HLB_GROUPS; ++g) {
        unsigned int hw[4] = {0u, 0u, 0u, 0u}, lw[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int q = 8 * g + t;
            if (ok && q < PM_NBINS) {
                const double x = sqrt(row[q]);
                double hv, lv;
                const unsigned int hb = hlb_bf16(x, hv);
                const unsigned int lb = hlb_bf16(x - hv, lv);
                hw[t >> 1] |= hb << (16 * (t & 1));
                lw[t >> 1] |= lb << (16 * (t & 1));
            }
        }
        dst[(2 * g) * HLB_BLK] = make_uint4(hw[0], hw[1], hw[2], hw[3]);
        dst[(2 * g + 1) * HLB_BLK] = make_uint4(lw[0], lw[1], lw[2], lw[3]);
    }
    h[(size_t)f * n_pad + i] = ok ? 0.5 * s : bad;
    if (!ok && i < n) nonfinite1[0] = 1;
}

// the float32 pre-test's two sides (header): s below hB - v, t above tau - hA, each by 2^-21 of its operands' magnitudes
__device__ __forceinline__ float hlb_below(double hb, double v) {
    if (hb == __builtin_inf()) return __builtin_inff();
    return ((float)(hb - v) - 0x1p-21f * (float)(fabs(hb) + fabs(v))) - 1e-30f;
}
__device__ __forceinline__ float hlb_above(double tau, double ha) {
    if (ha != ha) return -__builtin_inff();          // a non-finite or padding moving row: every entry is rejected at once
    return ((float)(tau - ha) + 0x1p-21f * (float)(fabs(tau) + fabs(ha))) + 1e-30f;
}

struct HlbEntry {      // a lane's entry of the row being ranked
    float dot;
    int col;
    double b, key;
    int rank;
    bool valid;
};

// Ranks by (key, column) of the n <= CAP <= 64 buffered entries of one row, by one wave: rank = number of smaller entries.
// sv: CAP doubles of this wave's scratch; vf: the frame's prices or NULL (buffered columns have finite prices).
template <int CAP>
__device__ __forceinline__ void hlb_rank_row(const float *cd, const int32_t *cc, int n, double ha, const double *__restrict__ hBf,
                                             const double *__restrict__ vf, double *sv, int lane, HlbEntry &e) {
    e.valid = lane < n;
    e.dot = e.valid ? cd[lane] : 0.0f;
    e.col = e.valid ? cc[lane] : INT_MAX;
    e.b = e.valid ? (ha + hBf[e.col]) - (double)e.dot : __builtin_inf();
    e.key = e.valid ? e.b - (vf ? vf[e.col] : 0.0) : __builtin_inf();
    if (lane < CAP) sv[lane] = e.key;
    e.rank = 0;
    hl_wave_sync();
    for (int j = 0; j < n; ++j) {
        const double vj = sv[j];
        const int cj = cc[j];
        e.rank += (vj < e.key || (vj == e.key && cj < e.col)) ? 1 : 0;
    }
    hl_wave_sync();
}

// R = S * F column ranges (frame f = range / S, split sp = range % S), PBn panels from pb0 on; per: work items per XCD.
// out_col / out_val: the final arrays [F][nA][k] when S == 1, the partial lists [F][nA][S][k] otherwise.
template <int CAP>
__global__ __launch_bounds__(HLB_THREADS) void hl_select_bf16_kernel(const uint4 *__restrict__ rAt, const uint4 *__restrict__ rBt,
                                                                  const double *__restrict__ hA, const double *__restrict__ hB,
                                                                  const double *__restrict__ v, int nA, int nB, int CT, int pb0,
                                                                  int PBn, int S, int R, int per, int k,
                                                                  int32_t *__restrict__ out_col, double *__restrict__ out_val) {
    static_assert(CAP <= 64 && CAP >= 16, "a lane ranks one entry");
    __shared__ hlb_u4 A_s[2][4 * HLB_STEP_U4];
    __shared__ hlb_u4 B_s[2][2 * HLB_STEP_U4];
    __shared__ float cd_s[HLB_PM][CAP];
    __shared__ int32_t cc_s[HLB_PM][CAP];
    __shared__ double sv_s[HLB_THREADS / 64][CAP];
    __shared__ double hA_s[HLB_PM], tau_s[HLB_PM];
    __shared__ __attribute__((aligned(16))) float tr_s[HLB_PM];
    __shared__ int cnt_s[HLB_PM];
    __shared__ int ovf_s;

    // the work item of this workgroup (header: XCD x takes items x * per .., 32 consecutive ones are 4 panels x 8 ranges)
    const long item = (long)(blockIdx.x & 7u) * per + (long)(blockIdx.x >> 3);
    const int RG = (R + HLB_XR - 1) / HLB_XR, super = (int)(item >> 5), within = (int)(item & 31);
    const int pl = (super / RG) * HLB_XP + (within & (HLB_XP - 1)), range = (super % RG) * HLB_XR + within / HLB_XP;
    if (pl >= PBn || range >= R) return;          // (the whole workgroup)
    const int pb = pb0 + pl, f = range / S, sp = range % S;

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, rb = w & 3, cb = w >> 2;
    const int t0 = (int)((long)sp * CT / S), t1 = (int)((long)(sp + 1) * CT / S);      // S <= CT: at least one tile
    const double inf = __builtin_inf();
    const double *hBf = hB + (size_t)f * CT * HLB_TN;
    const double *vf = v ? v + (size_t)f * nB : nullptr;
    // this thread's pieces of a stage: two of the panel (blocks tid / 256 and tid / 256 + 2), one of the tile (block tid / 256)
    const hlb_u4 *at = (const hlb_u4 *)rAt + ((size_t)pb * 4 + (tid >> 8)) * HLB_BLK_U4 + (tid & 255);
    const hlb_u4 *bt = (const hlb_u4 *)rBt + ((size_t)f * CT * 2 + (tid >> 8)) * HLB_BLK_U4 + (tid & 255);

    if (tid < HLB_PM) {
        const double ha = hA[(size_t)pb * HLB_PM + tid];                                // (padded: NaN past the cloud's end)
        hA_s[tid] = ha;
        tau_s[tid] = HL_TAU0;
        tr_s[tid] = hlb_above(HL_TAU0, ha);
        cnt_s[tid] = 0;
    }
    if (tid == 0) ovf_s = 0;

    // operand offsets of this lane inside a stage (16-byte pieces): bin group lane / 32, row lane % 32 of the first half
    const int kh = lane >> 5, lo = lane & 31;
    const int aoff = rb * HLB_STEP_U4 + kh * 2 * HLB_BLK + lo, boff = cb * HLB_STEP_U4 + kh * 2 * HLB_BLK + lo;

    hlb_u4 pa0, pa1, pbr;
    const long total = (long)(t1 - t0) * HLB_STEPS;
    pa0 = at[0], pa1 = at[2 * HLB_BLK_U4];
    pbr = bt[(size_t)t0 * 2 * HLB_BLK_U4];
    A_s[0][tid] = pa0, A_s[0][tid + HLB_THREADS] = pa1;
    B_s[0][tid] = pbr;
    __syncthreads();

    hl_f16 acc00, acc01, acc10, acc11;              // (row half, column half) of the wave's 64 x 64
#pragma unroll
    for (int e = 0; e < 16; ++e) acc00[e] = acc01[e] = acc10[e] = acc11[e] = 0.0f;
    for (int tile = t0; tile < t1; ++tile) {
#pragma unroll 1
        for (int c = 0; c < HLB_STEPS; ++c) {
        const int buf = c & 1;
        const bool has_next = (long)(tile - t0) * HLB_STEPS + c + 1 < total;
        if (has_next) {
            const int nc = (c + 1 == HLB_STEPS) ? 0 : c + 1, ntile = (c + 1 == HLB_STEPS) ? tile + 1 : tile;
            pa0 = at[nc * HLB_STEP_U4], pa1 = at[2 * HLB_BLK_U4 + nc * HLB_STEP_U4];
            pbr = bt[(size_t)ntile * 2 * HLB_BLK_U4 + nc * HLB_STEP_U4];
        }
        {
            const hlb_bf8 *Ab = (const hlb_bf8 *)A_s[buf] + aoff, *Bb = (const hlb_bf8 *)B_s[buf] + boff;
            const hlb_bf8 a0h = Ab[0], a1h = Ab[32], b0h = Bb[0], b1h = Bb[32];
            const hlb_bf8 b0l = Bb[HLB_BLK], b1l = Bb[HLB_BLK + 32], a0l = Ab[HLB_BLK], a1l = Ab[HLB_BLK + 32];
            acc00 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0h, b0h, acc00, 0, 0, 0);
            acc01 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0h, b1h, acc01, 0, 0, 0);
            acc10 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1h, b0h, acc10, 0, 0, 0);
            acc11 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1h, b1h, acc11, 0, 0, 0);
            acc00 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0h, b0l, acc00, 0, 0, 0);
            acc01 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0h, b1l, acc01, 0, 0, 0);
            acc10 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1h, b0l, acc10, 0, 0, 0);
            acc11 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1h, b1l, acc11, 0, 0, 0);
            acc00 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0l, b0h, acc00, 0, 0, 0);
            acc01 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0l, b1h, acc01, 0, 0, 0);
            acc10 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1l, b0h, acc10, 0, 0, 0);
            acc11 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1l, b1h, acc11, 0, 0, 0);
        }
        if (has_next) {
            A_s[buf ^ 1][tid] = pa0, A_s[buf ^ 1][tid + HLB_THREADS] = pa1;
            B_s[buf ^ 1][tid] = pbr;
        }
        __syncthreads();
        }
        {   // (after the last stage's barrier: the next tile's first stage already lies in LDS, untouched by what follows)
            // ---- epilogue: this wave's 64 x 64 entries against the rows' thresholds ------------------------------------------------
            const int col0 = tile * HLB_TN + HLB_BLK * cb + lo, col1 = col0 + 32, row0 = HLB_BLK * rb + 4 * kh;
            double hb0 = hBf[col0], hb1 = hBf[col1];                                     // (padded: +inf past the frame's end)
            double v0 = (vf && col0 < nB) ? vf[col0] : 0.0, v1 = (vf && col1 < nB) ? vf[col1] : 0.0;
            if (!(v0 - v0 == 0.0)) hb0 = inf, v0 = 0.0;                                  // a NaN or infinite price: never listed
            if (!(v1 - v1 == 0.0)) hb1 = inf, v1 = 0.0;
            const float s0 = hlb_below(hb0, v0), s1 = hlb_below(hb1, v1);
            unsigned long long pending = 0ull;
#pragma unroll
            for (int q = 0; q < 4; ++q) {          // the float32 pre-test, four consecutive rows of both halves at a time
                const float4 ta = *(const float4 *)&tr_s[row0 + 8 * q], tb = *(const float4 *)&tr_s[row0 + 8 * q + 32];
                const float t0r[4] = {ta.x, ta.y, ta.z, ta.w}, t1r[4] = {tb.x, tb.y, tb.z, tb.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int e = 4 * q + j;
                    if (!(acc00[e] < s0 - t0r[j])) pending |= 1ull << e;
                    if (!(acc01[e] < s1 - t0r[j])) pending |= 1ull << (16 + e);
                    if (!(acc10[e] < s0 - t1r[j])) pending |= 1ull << (32 + e);
                    if (!(acc11[e] < s1 - t1r[j])) pending |= 1ull << (48 + e);
                }
            }
            for (;;) {
                if (pending != 0ull) {
#pragma unroll
                    for (int e = 0; e < 64; ++e) {
                        if (!((pending >> e) & 1ull)) continue;
                        const int q = e >> 4, ee = e & 15, row = row0 + 8 * (ee >> 2) + (ee & 3) + 32 * (q >> 1);
                        float dot = q == 0 ? acc00[ee] : q == 1 ? acc01[ee] : q == 2 ? acc10[ee] : acc11[ee];
                        asm volatile("" : "+v"(dot));          // (opaque: the rare path keeps no 64 values of its own live)
                        // the float64 test decides; tau is read now: a cut may have lowered it since the mask was formed
                        const double key = ((hA_s[row] + ((q & 1) ? hb1 : hb0)) - (double)dot) - ((q & 1) ? v1 : v0);
                        bool done = true;
                        if (key <= tau_s[row]) {
                            const int slot = atomicAdd(&cnt_s[row], 1);
                            if (slot < CAP) {
                                cd_s[row][slot] = dot;
                                cc_s[row][slot] = (q & 1) ? col1 : col0;
                            } else {
                                done = false;
                                ovf_s = 1;
                            }
                        }
                        if (done) pending &= ~(1ull << e);
                        asm volatile("" ::: "memory");
                    }
                }
                __syncthreads();
                if (ovf_s == 0) break;           // (uniform: read between two barriers)
                __syncthreads();
                if (tid == 0) ovf_s = 0;
                for (int r = w; r < HLB_PM; r += HLB_THREADS / 64) {
                    if (__builtin_amdgcn_readfirstlane(cnt_s[r]) < CAP) continue;
                    HlbEntry en;
                    hlb_rank_row<CAP>(cd_s[r], cc_s[r], CAP, hA_s[r], hBf, vf, sv_s[w], lane, en);
                    if (en.valid && en.rank < k) {
                        cd_s[r][en.rank] = en.dot;
                        cc_s[r][en.rank] = en.col;
                        if (en.rank == k - 1) {
                            tau_s[r] = en.key;
                            tr_s[r] = hlb_above(en.key, hA_s[r]);
                        }
                    }
                    if (lane == 0) cnt_s[r] = k;
                    hl_wave_sync();
                }
                __syncthreads();
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) acc00[e] = acc01[e] = acc10[e] = acc11[e] = 0.0f;
        }
    }

    // ---- the rows' lists, ascending by (key, column); the bound is what is written ---------------------------------------------
    for (int r = w; r < HLB_PM; r += HLB_THREADS / 64) {
        const long row = (long)pb * HLB_PM + r;
        if (row >= nA) break;
        const size_t base = (((size_t)f * nA + row) * S + sp) * k;
        const double ha = hA_s[r];
        if (ha != ha) {          // a non-finite moving row
            for (int t = lane; t < k; t += 64) {
                out_col[base + t] = -1;
                out_val[base + t] = ha;
            }
            continue;
        }
        const int n = min(__builtin_amdgcn_readfirstlane(cnt_s[r]), CAP);
        HlbEntry en;
        hlb_rank_row<CAP>(cd_s[r], cc_s[r], n, ha, hBf, vf, sv_s[w], lane, en);
        if (en.valid && en.rank < k) {
            out_col[base + en.rank] = en.col;
            out_val[base + en.rank] = en.b;
        }
        for (int t = min(n, k) + lane; t < k; t += 64) {
            out_col[base + t] = -1;
            out_val[base + t] = inf;
        }
    }
}

// automatic splits: four rounds of one workgroup per CU of a 256-CU device
constexpr HlGeometry HLB_SELECT = {HLB_PM, HLB_TN, HLB_BLK_U4 * sizeof(uint4), true, HLB_KMAX, 1024};

}  // namespace pm

extern "C" size_t pm_hellinger_select_bf16_workspace(int nA, int nB, int n_frames, int k) {
    return pm::hl_layout(pm::HLB_SELECT, nA, nB, n_frames, k).bytes;
}

extern "C" int pm_hellinger_delta_bf16(double *delta1_host) {
    if (!delta1_host) return PM_ERR_INVALID_ARG;
    *delta1_host = PM_HELLINGER_DELTA_BF16X3;
    return PM_OK;
}

extern "C" int pm_hellinger_select_bf16(const double *scA, int nA, const double *scB, int nB, size_t frame_stride, int n_frames,
                                        const double *v, int k, int split, int32_t *out_col, double *out_bound,
                                        int32_t *nonfinite1, void *ws, size_t ws_bytes, void *stream) {
    using namespace pm;
    const HlLayout L = hl_layout(HLB_SELECT, nA, nB, n_frames, k);
    const bool args = scA && scB && out_col && out_bound && nonfinite1;
    if (const int err = hl_check(args, L, nB, n_frames, split, frame_stride, ws, ws_bytes)) return err;
    hipStream_t s = (hipStream_t)stream;
    char *base = (char *)ws;
    uint4 *rA = (uint4 *)(base + L.rA), *rB = (uint4 *)(base + L.rB);
    double *hA = (double *)(base + L.hA), *hB = (double *)(base + L.hB);
    int32_t *pcol = (int32_t *)(base + L.pcol);
    double *pval = (double *)(base + L.pval);
    const long PB = L.PB, CT = L.CT;
    const int S = hl_splits(HLB_SELECT, L, split, n_frames), R = S * n_frames, RG = (R + HLB_XR - 1) / HLB_XR;
    int32_t *oc = S == 1 ? out_col : pcol;
    double *ov = S == 1 ? out_bound : pval;

    hl_clear_flag_kernel<<<1, 1, 0, s>>>(nonfinite1);
    hlb_prep_kernel<<<dim3((unsigned int)((PB * HLB_PM + 255) / 256), 1), 256, 0, s>>>(scA, 0, nA, (int)(PB * HLB_PM), rA, hA,
                                                                                     __builtin_nan(""), nonfinite1);
    hlb_prep_kernel<<<dim3((unsigned int)((CT * HLB_TN + 255) / 256), n_frames), 256, 0, s>>>(scB, frame_stride, nB, (int)(CT * HLB_TN),
                                                                                            rB, hB, __builtin_inf(), nonfinite1);
    // bands of panels (a multiple of HLB_XP each but the last): a launch stays under 2^32 work-items, its item numbers under 2^31
    const long band = std::max((long)HLB_XP, ((0xffffffffL / HLB_THREADS - 8) / (32L * RG)) * HLB_XP);
    for (long b0 = 0; b0 < PB; b0 += band) {
        const long nb = std::min(band, PB - b0), items = (nb + HLB_XP - 1) / HLB_XP * RG * 32, per = (items + 7) / 8;
        const dim3 grid((unsigned int)(per * 8));
        if (k <= 16)
            hl_select_bf16_kernel<32><<<grid, HLB_THREADS, 0, s>>>(rA, rB, hA, hB, v, nA, nB, (int)CT, (int)b0, (int)nb, S, R, (int)per,
                                                                   k, oc, ov);
        else
            hl_select_bf16_kernel<48><<<grid, HLB_THREADS, 0, s>>>(rA, rB, hA, hB, v, nA, nB, (int)CT, (int)b0, (int)nb, S, R, (int)per,
                                                                   k, oc, ov);
    }
    if (S > 1)
        hl_select_merge_kernel<<<dim3((unsigned int)((nA + 3) / 4), n_frames), 256, 0, s>>>(pcol, pval, hA, v, nA, nB, S, k, out_col,
                                                                                           out_bound);
    return launch_status();
}
