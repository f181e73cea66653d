// pm_hellinger.hip — the Hellinger lower bound of the chi-square cost on the matrix cores, fused with a per-row top-K.
//
// For a, b >= 0:  (a-b)^2/(a+b) = (sqrt a - sqrt b)^2 (sqrt a + sqrt b)^2/(a+b) >= (sqrt a - sqrt b)^2,  hence
//     C(i,j) = 0.5 sum_k (a_k-b_k)^2/(a_k+b_k)  >=  L(i,j) = 0.5 (sum a + sum b) - sum_k sqrt(a_k) sqrt(b_k).
// The last sum is a GEMM of the sqrt-descriptors, N x 360 by 360 x M per fixed frame: 2*360 flop per pair where the filter
// build (pm_chi2.hip: filter4_kernel) issues ~5.5 slots per TERM, half of them v_rcp_f32.  Nothing of the N x M product is
// stored: each row keeps its k smallest bounds (k <= 64) and the columns they belong to.
//
// Layout.  hl_prep_kernel writes float32 sqrt-descriptors (sqrt taken in float64, rounded once to float32) in BLOCKS of 64
// rows, bin-major inside a block: element (row r, bin q) of a block sits at  q*64 + ((r + 32 (q & 1)) & 63).  A block is
// 92 160 contiguous bytes, and a 40-bin chunk of it 10 240, so global -> LDS is a straight 16-byte copy (no transposition,
// no LDS write conflicts).  v_mfma_f32_32x32x2f32 wants, from lane l, operand element (row l % 32, bin 2 m + l / 32): with
// the rotation by 32 on odd bins the 64 lanes of one ds_read_b32 touch 64 distinct banks (and each half-wave 32 distinct
// ones), without a padding column.  Rows past the end of a cloud and non-finite rows (a NaN, an infinity, a negative value,
// or a sum that overflows) are zero rows, so the GEMM stays finite; their half row sum h = 0.5 sum is replaced by NaN
// (moving side) or +inf (fixed side) — that value IS the row's flag: a NaN bound never passes a comparison, a +inf bound is
// never listed, and the epilogue needs no masks for ragged edges.
//
// Main kernel (hl_topk_kernel), one 256-thread workgroup per (block of 64 moving rows, column split s, fixed frame):
//   - the block's 64 x 360 sqrt-rows stay in LDS (92 KB) for the whole sweep;
//   - tiles of 64 fixed rows stream through two LDS stages of 40 bins (2 x 10 KB), the next stage travelling through
//     registers while the current one is multiplied: one barrier per stage of 20 MFMAs per wave;
//   - wave w owns the 32 x 32 quadrant (rows 32 (w & 1), columns 32 (w >> 1)): 180 chained v_mfma_f32_32x32x2f32 per tile
//     into 16 accumulation registers, always bins 0..359 in order — an entry's bits do not depend on the launch geometry;
//   - epilogue in registers: L~ = (hA_i + hB_j) - (double)dot against tau_i (LDS), the row's current k-th smallest bound;
//     an entry with L~ <= tau_i (ties kept: the order is by (bound, column)) is appended — (dot, column), 8 bytes — to the
//     row's buffer of HL_CAP = 80 slots.  A full buffer is cut back to its k smallest by (bound, column) by one wave (ranks
//     by counting, 80 x 80 comparisons) and tau_i lowered; lanes whose append found no slot retry after the cut.  After the
//     first tiles appends are rare (~ k ln(M / k) per row), so the sweep runs at the speed of its MFMAs.
//   LDS: 92 160 + 20 480 + 40 960 (buffers) + 2 560 (ranking scratch) + 1 300 = 157 460 B: ONE workgroup per CU, one wave
//   per SIMD — the occupancy this kernel is built for (its 136 registers are not the limit; nothing spills).
//   Measured (profiles/hellinger_*): 22.2 ms for 20 000 x 20 000 x 4 frames, k = 16 — a third of the float32 matrix peak.
// Few row blocks: the fixed rows' tiles are split over S workgroups per (block, frame), each writes its sorted k-list to the
// workspace, hl_select_merge_kernel (without prices) merges the S lists of a row by (bound, column) (one wave per row, a k-round
// tournament over the list heads).  Column sets are disjoint and every list is an exact top-k of its set, so the result is the
// same for any S.
// One ranking (hls_rank_row), one merge and one host side (pm_hellinger.h: workspace layout, split rule, argument check; here:
// hl_prepare, hl_bands) serve every kernel of this file; pm_hellinger_bf16.hip shares the merge and the host helpers.
//
// Error bound.  PM_HELLINGER_DELTA bounds |L~ - L| for descriptor rows with sum a, sum b <= 1, with no assumption about the
// MFMA's internal rounding or summation order: u = 2^-24; each input sqrt is rounded once to float32 (after a correctly
// rounded float64 sqrt: (1 + 2^-53) u), so |ra rb - sqrt a sqrt b| <= (2u + u^2) sqrt a sqrt b, summed: <= 2.0000002 u by
// Cauchy-Schwarz (sum sqrt a sqrt b <= sqrt(sum a sum b) <= 1); each of the 360 multiply-accumulates is charged 2u (product,
// sum) of a partial sum that never exceeds sum ra rb <= 1 + 2u: 720 u (1 + 722 u).  Together 722.04 u = 4.3037e-5; products
// flushed as denormals (< 1.2e-38 each) and the float64 epilogue (3 x 2^-53) vanish in the slack of the constant below.
#include <limits.h>

#include "pm_hellinger.h"

#define PM_HELLINGER_DELTA 4.31e-5

namespace pm {

constexpr int HL_KC = 40;                        // bins per LDS stage
constexpr int HL_NCH = PM_NBINS / HL_KC;         // 9 stages per tile
constexpr int HL_STAGE = HL_KC * HL_BM;          // floats of one stage (640 float4)
constexpr int HL_CAP = 80;                       // candidate slots per row
constexpr int HL_THREADS = 256;
static_assert(HL_KC % 2 == 0 && HL_NCH * HL_KC == PM_NBINS && HL_CAP >= HL_KMAX + 16 && HL_CAP <= 128, "geometry");

__global__ void hl_clear_flag_kernel(int32_t *flag1) { flag1[0] = 0; }

// sqrt-descriptors in the blocked layout + half row sums (bin order, float64, as relaxed_rowsum_kernel adds them).  One thread
// per row of the padded cloud (n_pad: a multiple of 64), blockIdx.y = frame.  bad: what h holds for a non-finite / padding row.
__global__ __launch_bounds__(256) void hl_prep_kernel(const double *__restrict__ sc, size_t frame_stride, int n, int n_pad,
                                                      float *__restrict__ rt, double *__restrict__ h, double bad,
                                                      int32_t *__restrict__ nonfinite1) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pad) return;
    const int f = blockIdx.y, r = i & 63;
    const double *row = sc + (size_t)f * frame_stride + (size_t)i * PM_NBINS;
    float *dst = rt + ((size_t)f * (n_pad / HL_BM) + i / HL_BM) * HL_TILE;
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
    for (int q = 0; q < PM_NBINS; ++q) dst[q * HL_BM + ((r + 32 * (q & 1)) & 63)] = ok ? (float)sqrt(row[q]) : 0.0f;
    h[(size_t)f * n_pad + i] = ok ? 0.5 * s : bad;
    if (!ok && i < n) nonfinite1[0] = 1;
}

template <int NQ>
struct HlsEntries {      // a lane's (at most NQ) entries of the row being ranked
    float dot[NQ];
    int col[NQ];
    double b[NQ], key[NQ];
    int rank[NQ];
    bool valid[NQ];
};

// Ranks by (key, column) of the n <= CAP buffered entries of one row, by one wave: rank = number of smaller entries (columns are
// distinct, so the ranks are a permutation of 0..n-1).  key = bound - v[column]; vf: the frame's prices (buffered columns have
// finite ones) or NULL: key = bound, bit for bit.  sv: CAP doubles of this wave's scratch.
template <int CAP>
__device__ __forceinline__ void hls_rank_row(const float *cd, const int32_t *cc, int n, double ha, const double *__restrict__ hBf,
                                             const double *__restrict__ vf, double *sv, int lane, HlsEntries<(CAP + 63) / 64> &e) {
    constexpr int NQ = (CAP + 63) / 64;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int idx = lane + 64 * q;
        e.valid[q] = idx < n;
        e.dot[q] = e.valid[q] ? cd[idx] : 0.0f;
        e.col[q] = e.valid[q] ? cc[idx] : INT_MAX;
        e.b[q] = e.valid[q] ? (ha + hBf[e.col[q]]) - (double)e.dot[q] : __builtin_inf();
        e.key[q] = e.valid[q] ? e.b[q] - (vf ? vf[e.col[q]] : 0.0) : __builtin_inf();
        if (idx < CAP) sv[idx] = e.key[q];
        e.rank[q] = 0;
    }
    hl_wave_sync();
    for (int j = 0; j < n; ++j) {
        const double vj = sv[j];
        const int cj = cc[j];
#pragma unroll
        for (int q = 0; q < NQ; ++q) e.rank[q] += (vj < e.key[q] || (vj == e.key[q] && cj < e.col[q])) ? 1 : 0;
    }
    hl_wave_sync();
}

// out_col / out_val: the final arrays [F][nA][k] when S == 1, the partial lists [F][nA][S][k] otherwise.
__global__ __launch_bounds__(HL_THREADS) void hl_topk_kernel(const float *__restrict__ rAt, const float *__restrict__ rBt,
                                                             const double *__restrict__ hA, const double *__restrict__ hB, int nA,
                                                             int CT, int rb0, int S, int k, int32_t *__restrict__ out_col,
                                                             double *__restrict__ out_val) {
    __shared__ __attribute__((aligned(16))) float A_s[HL_TILE];
    __shared__ __attribute__((aligned(16))) float B_s[2][HL_STAGE];
    __shared__ float cd_s[HL_BM][HL_CAP];
    __shared__ int32_t cc_s[HL_BM][HL_CAP];
    __shared__ double sv_s[HL_THREADS / 64][HL_CAP];
    __shared__ double hA_s[HL_BM], tau_s[HL_BM];
    __shared__ int cnt_s[HL_BM];
    __shared__ int ovf_s;

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, rh = w & 1, ch = w >> 1;
    const int rb = rb0 + (int)(blockIdx.x / (unsigned int)S), sp = (int)(blockIdx.x % (unsigned int)S), f = blockIdx.y;
    const int t0 = (int)((long)sp * CT / S), t1 = (int)((long)(sp + 1) * CT / S);      // S <= CT: at least one tile
    const double inf = __builtin_inf();
    const double *hBf = hB + (size_t)f * CT * HL_BM;
    const float4 *bt4 = (const float4 *)(rBt + (size_t)f * CT * HL_TILE);

    {   // the row block, straight into LDS
        const float4 *src = (const float4 *)(rAt + (size_t)rb * HL_TILE);
        float4 *dst = (float4 *)A_s;
        for (int i = tid; i < HL_TILE / 4; i += HL_THREADS) dst[i] = src[i];
    }
    if (tid < HL_BM) {
        hA_s[tid] = hA[(size_t)rb * HL_BM + tid];
        tau_s[tid] = inf;
        cnt_s[tid] = 0;
    }
    if (tid == 0) ovf_s = 0;

    // operand offsets of this lane inside a pair of bins (128 floats): bin parity = lane / 32, rotated by 32 on the odd bin
    const int hi = lane >> 5, lo = lane & 31;
    const int aoff = hi * HL_BM + ((32 * rh + lo + 32 * hi) & 63);
    const int boff = hi * HL_BM + ((32 * ch + lo + 32 * hi) & 63);

    float4 p0, p1, p2 = make_float4(0.f, 0.f, 0.f, 0.f);
    {
        const float4 *src = bt4 + (size_t)t0 * (HL_TILE / 4);
        p0 = src[tid];
        p1 = src[tid + 256];
        if (tid < 128) p2 = src[tid + 512];
        float4 *dst = (float4 *)B_s[0];
        dst[tid] = p0;
        dst[tid + 256] = p1;
        if (tid < 128) dst[tid + 512] = p2;
    }
    __syncthreads();

    hl_f16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.0f;
    int tile = t0, c = 0, buf = 0;
    double hb = hBf[(size_t)tile * HL_BM + 32 * ch + lo];
    const long total = (long)(t1 - t0) * HL_NCH;
    for (long st = 0; st < total; ++st) {
        const bool has_next = st + 1 < total;
        const int nc = (c + 1 == HL_NCH) ? 0 : c + 1, ntile = (c + 1 == HL_NCH) ? tile + 1 : tile;
        if (has_next) {
            const float4 *src = bt4 + (size_t)ntile * (HL_TILE / 4) + nc * (HL_STAGE / 4);
            p0 = src[tid];
            p1 = src[tid + 256];
            if (tid < 128) p2 = src[tid + 512];
        }
        const float *Ab = A_s + c * HL_STAGE + aoff, *Bb = B_s[buf] + boff;
#pragma unroll
        for (int m = 0; m < HL_KC / 2; ++m) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ab[m * 128], Bb[m * 128], acc, 0, 0, 0);
        if (has_next) {
            float4 *dst = (float4 *)B_s[buf ^ 1];
            dst[tid] = p0;
            dst[tid + 256] = p1;
            if (tid < 128) dst[tid + 512] = p2;
        }
        if (c == HL_NCH - 1) {
            // ---- epilogue: this wave's 32 x 32 bounds against the rows' thresholds --------------------------------------------
            const int col = tile * HL_BM + 32 * ch + lo;
            unsigned int pending = 0;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int row = 32 * rh + 8 * (v >> 2) + 4 * hi + (v & 3);
                const double val = (hA_s[row] + hb) - (double)acc[v];
                if (val <= tau_s[row] && val != inf) {
                    const int slot = atomicAdd(&cnt_s[row], 1);
                    if (slot < HL_CAP) {
                        cd_s[row][slot] = acc[v];
                        cc_s[row][slot] = col;
                    } else {
                        pending |= 1u << v;
                        ovf_s = 1;
                    }
                }
            }
            __syncthreads();
            while (ovf_s != 0) {         // (uniform: read between two barriers)
                __syncthreads();
                if (tid == 0) ovf_s = 0;
                for (int r = w; r < HL_BM; r += HL_THREADS / 64) {
                    if (__builtin_amdgcn_readfirstlane(cnt_s[r]) < HL_CAP) continue;
                    HlsEntries<2> e;
                    hls_rank_row<HL_CAP>(cd_s[r], cc_s[r], HL_CAP, hA_s[r], hBf, nullptr, sv_s[w], lane, e);
#pragma unroll
                    for (int q = 0; q < 2; ++q)
                        if (e.valid[q] && e.rank[q] < k) {
                            cd_s[r][e.rank[q]] = e.dot[q];
                            cc_s[r][e.rank[q]] = e.col[q];
                            if (e.rank[q] == k - 1) tau_s[r] = e.b[q];
                        }
                    if (lane == 0) cnt_s[r] = k;
                    hl_wave_sync();
                }
                __syncthreads();
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    if (!(pending & (1u << v))) continue;
                    const int row = 32 * rh + 8 * (v >> 2) + 4 * hi + (v & 3);
                    const double val = (hA_s[row] + hb) - (double)acc[v];
                    bool done = true;
                    if (val <= tau_s[row]) {
                        const int slot = atomicAdd(&cnt_s[row], 1);
                        if (slot < HL_CAP) {
                            cd_s[row][slot] = acc[v];
                            cc_s[row][slot] = col;
                        } else {
                            done = false;
                            ovf_s = 1;
                        }
                    }
                    if (done) pending &= ~(1u << v);
                }
                __syncthreads();
            }
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[v] = 0.0f;
            if (has_next) hb = hBf[(size_t)ntile * HL_BM + 32 * ch + lo];
        }
        tile = ntile;
        c = nc;
        buf ^= 1;
        __syncthreads();
    }

    // ---- the rows' lists, ascending by (bound, column) --------------------------------------------------------------------
    for (int r = w; r < HL_BM; r += HL_THREADS / 64) {
        const long row = (long)rb * HL_BM + r;
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
        const int n = min(__builtin_amdgcn_readfirstlane(cnt_s[r]), HL_CAP);
        HlsEntries<2> e;
        hls_rank_row<HL_CAP>(cd_s[r], cc_s[r], n, ha, hBf, nullptr, sv_s[w], lane, e);
#pragma unroll
        for (int q = 0; q < 2; ++q)
            if (e.valid[q] && e.rank[q] < k) {
                out_col[base + e.rank[q]] = e.col[q];
                out_val[base + e.rank[q]] = e.b[q];
            }
        for (int t = min(n, k) + lane; t < k; t += 64) {
            out_col[base + t] = -1;
            out_val[base + t] = inf;
        }
    }
}

// ---- threshold listing: every entry whose bound, reduced by the duals, is at most tau ---------------------------------------
// hl_list_kernel answers the solver's third question (lsap.FilteredMatrix.certificate / threshold_select) without a matrix:
// entry (f, i, j) is listed iff  (L~ - v[f][j]) - u[f][i] <= tau  and  j != skip[f][i],  L~ = (hA_i + hB_j) - (double)dot — the
// same bits hl_topk_kernel reports for the entry (same instruction, same operands, bins 0..359 in order).  There is no per-row
// state, so nothing is resident:
//   - a 256-thread workgroup owns a PANEL of 128 moving rows (two blocks of the layout above) and a range of 128-column tiles
//     of one fixed frame; both operands stream through two LDS stages of HLL_KC = 20 bins: a stage is 2 x (2 blocks x 5 120
//     contiguous bytes) = 20 KB, global -> registers -> LDS as six 16-byte copies per thread, issued before the stage's MFMAs
//     and stored after them: one barrier per stage of 40 MFMAs per wave;
//   - wave w owns the 64 x 64 sub-tile (row block w & 1, column block w >> 1) as FOUR 32 x 32 accumulators: per pair of bins two
//     A reads and two B reads (ds_read_b32, 64 distinct banks each by the odd-bin rotation) feed four independent
//     v_mfma_f32_32x32x2f32 chains — hl_topk_kernel has one chain of 180;
//   - LDS 2 x 20 480 + 2 560 (the panel's hA, u, skip) = 43 520 B: three workgroups per CU; no scratch;
//   - epilogue in registers: 64 entries per lane per tile in float64, a 64-bit mask of the qualifying ones.  Survivors are rare,
//     so a wave whose ballot is empty goes on; otherwise ONE atomicAdd per wave per tile (lane 0, after a wave prefix sum of the
//     lanes' counts) on the frame's 64-bit counter reserves the slots, and each lane writes its entries that fall below cap.
// The column tiles are split over S workgroups per (panel, frame) as in hl_splits; an entry is computed whole by one workgroup,
// so the listed set and its bits do not depend on S.  hl_list_finish_kernel turns the 64-bit counters into count[F] (saturated).
// Measured (profiles/hellinger_list_20k.txt): 20 000 x 20 000 x 4 frames at 16 entries per row, the whole call with its sort by
// (row, column): 11.5 ms against hl_topk_kernel's call at 22.2 ms.
constexpr int HLL_BM = 2 * HL_BM;                 // rows per panel = columns per tile
constexpr int HLL_KC = 20;                        // bins per LDS stage
constexpr int HLL_NCH = PM_NBINS / HLL_KC;        // 18 stages per tile
constexpr int HLL_HALF = HLL_KC * HL_BM;          // floats of one block's part of a stage (320 float4)
constexpr int HLL_STAGE = 2 * HLL_HALF;           // floats of one operand's stage (640 float4)
static_assert(HLL_KC % 2 == 0 && HLL_NCH * HLL_KC == PM_NBINS && HLL_STAGE / 4 == 2 * HL_THREADS + HL_THREADS / 2, "geometry");

__global__ void hl_list_clear_kernel(unsigned long long *cnt, int F, int32_t *flag1) {
    if ((int)threadIdx.x < F) cnt[threadIdx.x] = 0ull;
    if (threadIdx.x == 0) flag1[0] = 0;
}

__global__ void hl_list_finish_kernel(const unsigned long long *cnt, int F, int32_t *count) {
    if ((int)threadIdx.x < F) count[threadIdx.x] = (int32_t)min(cnt[threadIdx.x], (unsigned long long)INT_MAX);
}

__global__ __launch_bounds__(HL_THREADS, 2) void hl_list_kernel(const float *__restrict__ rAt, const float *__restrict__ rBt,
                                                             const double *__restrict__ hA, const double *__restrict__ hB,
                                                             const double *__restrict__ u, const double *__restrict__ v,
                                                             const int32_t *__restrict__ skip, double tau, int nA, int nB, int CT,
                                                             int pb0, int S, int cap, int32_t *__restrict__ out_rc,
                                                             double *__restrict__ out_bound, unsigned long long *__restrict__ cnt) {
    __shared__ __attribute__((aligned(16))) float A_s[2][HLL_STAGE];
    __shared__ __attribute__((aligned(16))) float B_s[2][HLL_STAGE];
    __shared__ double hA_s[HLL_BM], u_s[HLL_BM];
    __shared__ int32_t skip_s[HLL_BM];

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, rh = w & 1, ch = w >> 1;
    const int pb = pb0 + (int)(blockIdx.x / (unsigned int)S), sp = (int)(blockIdx.x % (unsigned int)S), f = blockIdx.y;
    const int t0 = (int)((long)sp * CT / S), t1 = (int)((long)(sp + 1) * CT / S);      // S <= CT: at least one tile
    const double *hBf = hB + (size_t)f * CT * HLL_BM;
    const double *vf = v + (size_t)f * nB;
    const float4 *at4 = (const float4 *)(rAt + (size_t)pb * 2 * HL_TILE);
    const float4 *bt4 = (const float4 *)(rBt + (size_t)f * CT * 2 * HL_TILE);

    if (tid < HLL_BM) {
        const long row = (long)pb * HLL_BM + tid;
        hA_s[tid] = hA[row];                                                            // (padded: NaN past the cloud's end)
        u_s[tid] = row < nA ? u[(size_t)f * nA + row] : 0.0;
        skip_s[tid] = (skip && row < nA) ? skip[(size_t)f * nA + row] : -1;
    }

    // a stage of one operand is 640 float4: 320 of the panel's first block, 320 of its second; this thread copies three of them
    // (the third only in the lower half of the workgroup), from the same offsets of both operands
    int so[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int j = tid + HL_THREADS * q;
        so[q] = (j / (HLL_HALF / 4)) * (HL_TILE / 4) + j % (HLL_HALF / 4);
    }
    const bool third = tid < HL_THREADS / 2;
    // operand offsets of this lane inside a pair of bins (128 floats) of its block, for the two 32-row halves
    const int hi = lane >> 5, lo = lane & 31;
    const int off0 = hi * HL_BM + ((lo + 32 * hi) & 63), off1 = hi * HL_BM + ((32 + lo + 32 * hi) & 63);

    float4 pa0, pa1, pa2 = make_float4(0.f, 0.f, 0.f, 0.f), pb0r, pb1r, pb2r = make_float4(0.f, 0.f, 0.f, 0.f);
    {
        const float4 *sb = bt4 + (size_t)t0 * (2 * HL_TILE / 4);
        pa0 = at4[so[0]], pa1 = at4[so[1]];
        pb0r = sb[so[0]], pb1r = sb[so[1]];
        if (third) pa2 = at4[so[2]], pb2r = sb[so[2]];
        float4 *da = (float4 *)A_s[0], *db = (float4 *)B_s[0];
        da[tid] = pa0, da[tid + HL_THREADS] = pa1;
        db[tid] = pb0r, db[tid + HL_THREADS] = pb1r;
        if (third) da[tid + 2 * HL_THREADS] = pa2, db[tid + 2 * HL_THREADS] = pb2r;
    }
    __syncthreads();

    hl_f16 acc00, acc01, acc10, acc11;              // (row half, column half) of the wave's 64 x 64
#pragma unroll
    for (int e = 0; e < 16; ++e) acc00[e] = acc01[e] = acc10[e] = acc11[e] = 0.0f;
    int tile = t0, c = 0, buf = 0;
    const long total = (long)(t1 - t0) * HLL_NCH;
    for (long st = 0; st < total; ++st) {
        const bool has_next = st + 1 < total;
        const int nc = (c + 1 == HLL_NCH) ? 0 : c + 1, ntile = (c + 1 == HLL_NCH) ? tile + 1 : tile;
        if (has_next) {
            const float4 *sa = at4 + nc * (HLL_HALF / 4);
            const float4 *sb = bt4 + (size_t)ntile * (2 * HL_TILE / 4) + nc * (HLL_HALF / 4);
            pa0 = sa[so[0]], pa1 = sa[so[1]];
            pb0r = sb[so[0]], pb1r = sb[so[1]];
            if (third) pa2 = sa[so[2]], pb2r = sb[so[2]];
        }
        const float *Ab = A_s[buf] + rh * HLL_HALF, *Bb = B_s[buf] + ch * HLL_HALF;
#pragma unroll
        for (int m = 0; m < HLL_KC / 2; ++m) {
            const float a0 = Ab[m * 128 + off0], a1 = Ab[m * 128 + off1], b0 = Bb[m * 128 + off0], b1 = Bb[m * 128 + off1];
            acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc00, 0, 0, 0);
            acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc01, 0, 0, 0);
            acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc10, 0, 0, 0);
            acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc11, 0, 0, 0);
        }
        if (has_next) {
            float4 *da = (float4 *)A_s[buf ^ 1], *db = (float4 *)B_s[buf ^ 1];
            da[tid] = pa0, da[tid + HL_THREADS] = pa1;
            db[tid] = pb0r, db[tid + HL_THREADS] = pb1r;
            if (third) da[tid + 2 * HL_THREADS] = pa2, db[tid + 2 * HL_THREADS] = pb2r;
        }
        if (c == HLL_NCH - 1) {
            // ---- epilogue: this wave's 64 x 64 bounds, reduced by the duals, against tau ------------------------------------------
            const int col0 = tile * HLL_BM + HL_BM * ch + lo, col1 = col0 + 32, row0 = HL_BM * rh + 4 * hi;
            const double hb0 = hBf[col0], hb1 = hBf[col1];                               // (padded: +inf past the frame's end)
            const double v0 = col0 < nB ? vf[col0] : 0.0, v1 = col1 < nB ? vf[col1] : 0.0;
            unsigned long long mask = 0ull;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int r0 = row0 + 8 * (e >> 2) + (e & 3), r1 = r0 + 32;
                const double ha0 = hA_s[r0], ha1 = hA_s[r1], u0 = u_s[r0], u1 = u_s[r1];
                const int s0 = skip_s[r0], s1 = skip_s[r1];
                const double l00 = (ha0 + hb0) - (double)acc00[e], l01 = (ha0 + hb1) - (double)acc01[e];
                const double l10 = (ha1 + hb0) - (double)acc10[e], l11 = (ha1 + hb1) - (double)acc11[e];
                if ((l00 - v0) - u0 <= tau && col0 != s0) mask |= 1ull << e;
                if ((l01 - v1) - u0 <= tau && col1 != s0) mask |= 1ull << (16 + e);
                if ((l10 - v0) - u1 <= tau && col0 != s1) mask |= 1ull << (32 + e);
                if ((l11 - v1) - u1 <= tau && col1 != s1) mask |= 1ull << (48 + e);
                // four rows' values at a time: hoisting all 32 rows' LDS reads would cost the second wave per SIMD
                if ((e & 3) == 3) {
                    asm volatile("" ::: "memory");
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            if (__builtin_amdgcn_ballot_w64(mask != 0ull) != 0ull) {
                const int mine = __popcll(mask);
                int incl = mine;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const int o = __shfl_up(incl, d, PM_WAVE);
                    if (lane >= d) incl += o;
                }
                const int wave_total = __shfl(incl, 63, PM_WAVE);
                unsigned int base_lo = 0, base_hi = 0;
                if (lane == 0) {
                    const unsigned long long b = atomicAdd(&cnt[f], (unsigned long long)wave_total);
                    base_lo = (unsigned int)b, base_hi = (unsigned int)(b >> 32);
                }
                base_lo = __shfl(base_lo, 0, PM_WAVE), base_hi = __shfl(base_hi, 0, PM_WAVE);
                unsigned long long slot = (((unsigned long long)base_hi << 32) | base_lo) + (unsigned long long)(incl - mine);
                int2 *rc = (int2 *)out_rc + (size_t)f * cap;
                double *ob = out_bound + (size_t)f * cap;
                int grow0 = pb * HLL_BM + row0;
                asm volatile("" : "+v"(grow0));          // (not a loop invariant: 32 row numbers would be kept in registers)
#pragma unroll
                for (int e = 0; e < 64; ++e) {
                    if (!((mask >> e) & 1ull)) continue;
                    const int q = e >> 4, ee = e & 15, rl = 8 * (ee >> 2) + (ee & 3) + 32 * (q >> 1);
                    float dot = q == 0 ? acc00[ee] : q == 1 ? acc01[ee] : q == 2 ? acc10[ee] : acc11[ee];
                    // (opaque to the compiler: the bound is formed again here, by the same operations, instead of 64 float64
                    //  values of the test above staying live for this rare path — they would cost the second wave per SIMD)
                    asm volatile("" : "+v"(dot));
                    if (slot < (unsigned long long)cap) {
                        rc[slot] = make_int2(grow0 + rl, (q & 1) ? col1 : col0);
                        ob[slot] = (hA_s[row0 + rl] + ((q & 1) ? hb1 : hb0)) - (double)dot;
                        asm volatile("" ::: "memory");
                    }
                    ++slot;
                }
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) acc00[e] = acc01[e] = acc10[e] = acc11[e] = 0.0f;
        }
        tile = ntile;
        c = nc;
        buf ^= 1;
        __syncthreads();
    }
}

// ---- priced selection: per row the k entries of smallest bound reduced by the column prices ---------------------------------
// hl_select_kernel answers the solver's row_select(v, k): per (frame, moving row) the k columns of smallest
//     key = L~ - v[f][j]   (float64, in that order),   L~ = (hA_i + hB_j) - (double)dot — the bits of the two kernels above,
// ascending by (key, column); what is reported beside the column is the BOUND L~ (the caller re-forms the key by the same
// subtraction).  A column whose price is NaN or +-inf is treated as a non-finite fixed row: its hB becomes +inf, it is never listed.
// With v == NULL (or all prices +0.0) key = L~ bit for bit, and the lists are hl_topk_kernel's.
// Geometry: hl_list_kernel's streamed one (a panel of 128 moving rows against 128-column tiles, both operands through two
// 20-bin LDS stages, four independent MFMA chains per wave, bins 0..359 in order) — nothing of the panel is resident but its
// per-row STATE: hA, tau (the row's current k-th key; DBL_MAX until k entries are known, so a +inf key never passes), a count and
// a buffer of CAP slots of (dot float32, column int32).  Epilogue: 64 keys per lane per tile in float64 against tau into a 64-bit
// mask (as the listing kernel forms its mask); the set bits are appended through an LDS atomic on the row's count.  A full buffer
// is cut to its k smallest by (key, column) by one wave (ranks by counting) and tau lowered; lanes that found no slot retry
// after the cut — the ovf protocol of hl_topk_kernel, one more barrier per tile of 18 stages.  An entry is only ever dropped
// against a tau that k better entries of the row have set, so the final buffer holds the row's exact top-k whatever the order
// of the appends, and the final ranking by (key, column) makes the list deterministic.
// CAP is a template parameter: 32 for k <= 16 (LDS 40 960 of stages + 32 768 of buffers + 3 592 = 77 320 B, 196 registers: two
// workgroups per CU, two waves per SIMD), 80 for k <= 64 (128 008 B, one workgroup per CU); both leave CAP - k >= 16 free slots
// after a cut.  No scratch in either.
// Measured (profiles/hellinger_select_20k.txt): 20 000 x 20 000 x 4 frames, the whole call: 14.9 ms at k = 16, 13.6 ms at k = 8,
// with and without prices, against hl_topk_kernel's call at 22.3 ms.
// Column tiles are split over S workgroups per (panel, frame); each writes its sorted partial list of (column, bound) and
// hl_select_merge_kernel re-forms the keys and merges by (key, column): disjoint column sets, exact partial lists, the same
// subtraction — the result does not depend on S.
// out_col / out_val: the final arrays [F][nA][k] when S == 1, the partial lists [F][nA][S][k] otherwise.
template <int CAP>
__global__ __launch_bounds__(HL_THREADS, 2) void hl_select_kernel(const float *__restrict__ rAt, const float *__restrict__ rBt,
                                                               const double *__restrict__ hA, const double *__restrict__ hB,
                                                               const double *__restrict__ v, int nA, int nB, int CT, int pb0, int S,
                                                               int k, int32_t *__restrict__ out_col, double *__restrict__ out_val) {
    __shared__ __attribute__((aligned(16))) float A_s[2][HLL_STAGE];
    __shared__ __attribute__((aligned(16))) float B_s[2][HLL_STAGE];
    __shared__ float cd_s[HLL_BM][CAP];
    __shared__ int32_t cc_s[HLL_BM][CAP];
    __shared__ double sv_s[HL_THREADS / 64][CAP];
    __shared__ double hA_s[HLL_BM], tau_s[HLL_BM];
    __shared__ int cnt_s[HLL_BM];
    __shared__ int ovf_s;

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, rh = w & 1, ch = w >> 1;
    const int pb = pb0 + (int)(blockIdx.x / (unsigned int)S), sp = (int)(blockIdx.x % (unsigned int)S), f = blockIdx.y;
    const int t0 = (int)((long)sp * CT / S), t1 = (int)((long)(sp + 1) * CT / S);      // S <= CT: at least one tile
    const double inf = __builtin_inf();
    const double *hBf = hB + (size_t)f * CT * HLL_BM;
    const double *vf = v ? v + (size_t)f * nB : nullptr;
    const float4 *at4 = (const float4 *)(rAt + (size_t)pb * 2 * HL_TILE);
    const float4 *bt4 = (const float4 *)(rBt + (size_t)f * CT * 2 * HL_TILE);

    if (tid < HLL_BM) {
        hA_s[tid] = hA[(size_t)pb * HLL_BM + tid];                                      // (padded: NaN past the cloud's end)
        tau_s[tid] = HL_TAU0;
        cnt_s[tid] = 0;
    }
    if (tid == 0) ovf_s = 0;

    // the stage copies, operand offsets and stage loop of hl_list_kernel, written out: moved with that kernel's into one inlined
    // template that calls the epilogue, this kernel compiled to 235 (CAP = 32) and 300 (CAP = 80) registers against 196 and 256
    int so[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int j = tid + HL_THREADS * q;
        so[q] = (j / (HLL_HALF / 4)) * (HL_TILE / 4) + j % (HLL_HALF / 4);
    }
    const bool third = tid < HL_THREADS / 2;
    const int hi = lane >> 5, lo = lane & 31;
    const int off0 = hi * HL_BM + ((lo + 32 * hi) & 63), off1 = hi * HL_BM + ((32 + lo + 32 * hi) & 63);

    float4 pa0, pa1, pa2 = make_float4(0.f, 0.f, 0.f, 0.f), pb0r, pb1r, pb2r = make_float4(0.f, 0.f, 0.f, 0.f);
    {
        const float4 *sb = bt4 + (size_t)t0 * (2 * HL_TILE / 4);
        pa0 = at4[so[0]], pa1 = at4[so[1]];
        pb0r = sb[so[0]], pb1r = sb[so[1]];
        if (third) pa2 = at4[so[2]], pb2r = sb[so[2]];
        float4 *da = (float4 *)A_s[0], *db = (float4 *)B_s[0];
        da[tid] = pa0, da[tid + HL_THREADS] = pa1;
        db[tid] = pb0r, db[tid + HL_THREADS] = pb1r;
        if (third) da[tid + 2 * HL_THREADS] = pa2, db[tid + 2 * HL_THREADS] = pb2r;
    }
    __syncthreads();

    hl_f16 acc00, acc01, acc10, acc11;              // (row half, column half) of the wave's 64 x 64
#pragma unroll
    for (int e = 0; e < 16; ++e) acc00[e] = acc01[e] = acc10[e] = acc11[e] = 0.0f;
    int tile = t0, c = 0, buf = 0;
    const long total = (long)(t1 - t0) * HLL_NCH;
    for (long st = 0; st < total; ++st) {
        const bool has_next = st + 1 < total;
        const int nc = (c + 1 == HLL_NCH) ? 0 : c + 1, ntile = (c + 1 == HLL_NCH) ? tile + 1 : tile;
        if (has_next) {
            const float4 *sa = at4 + nc * (HLL_HALF / 4);
            const float4 *sb = bt4 + (size_t)ntile * (2 * HL_TILE / 4) + nc * (HLL_HALF / 4);
            pa0 = sa[so[0]], pa1 = sa[so[1]];
            pb0r = sb[so[0]], pb1r = sb[so[1]];
            if (third) pa2 = sa[so[2]], pb2r = sb[so[2]];
        }
        const float *Ab = A_s[buf] + rh * HLL_HALF, *Bb = B_s[buf] + ch * HLL_HALF;
#pragma unroll
        for (int m = 0; m < HLL_KC / 2; ++m) {
            const float a0 = Ab[m * 128 + off0], a1 = Ab[m * 128 + off1], b0 = Bb[m * 128 + off0], b1 = Bb[m * 128 + off1];
            acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc00, 0, 0, 0);
            acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc01, 0, 0, 0);
            acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc10, 0, 0, 0);
            acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc11, 0, 0, 0);
        }
        if (has_next) {
            float4 *da = (float4 *)A_s[buf ^ 1], *db = (float4 *)B_s[buf ^ 1];
            da[tid] = pa0, da[tid + HL_THREADS] = pa1;
            db[tid] = pb0r, db[tid + HL_THREADS] = pb1r;
            if (third) da[tid + 2 * HL_THREADS] = pa2, db[tid + 2 * HL_THREADS] = pb2r;
        }
        if (c == HLL_NCH - 1) {
            // ---- epilogue: this wave's 64 x 64 keys against the rows' thresholds -----------------------------------------------
            const int col0 = tile * HLL_BM + HL_BM * ch + lo, col1 = col0 + 32, row0 = HL_BM * rh + 4 * hi;
            double hb0 = hBf[col0], hb1 = hBf[col1];                                     // (padded: +inf past the frame's end)
            double v0 = (vf && col0 < nB) ? vf[col0] : 0.0, v1 = (vf && col1 < nB) ? vf[col1] : 0.0;
            if (!(v0 - v0 == 0.0)) hb0 = inf, v0 = 0.0;                                  // a NaN or infinite price: never listed
            if (!(v1 - v1 == 0.0)) hb1 = inf, v1 = 0.0;
            unsigned long long pending = 0ull;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int r0 = row0 + 8 * (e >> 2) + (e & 3), r1 = r0 + 32;
                const double ha0 = hA_s[r0], ha1 = hA_s[r1], tau0 = tau_s[r0], tau1 = tau_s[r1];
                const double l00 = (ha0 + hb0) - (double)acc00[e], l01 = (ha0 + hb1) - (double)acc01[e];
                const double l10 = (ha1 + hb0) - (double)acc10[e], l11 = (ha1 + hb1) - (double)acc11[e];
                if (l00 - v0 <= tau0) pending |= 1ull << e;
                if (l01 - v1 <= tau0) pending |= 1ull << (16 + e);
                if (l10 - v0 <= tau1) pending |= 1ull << (32 + e);
                if (l11 - v1 <= tau1) pending |= 1ull << (48 + e);
                // four rows' values at a time, as in hl_list_kernel: all 32 rows' LDS reads at once would cost the second wave
                if ((e & 3) == 3) {
                    asm volatile("" ::: "memory");
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            for (;;) {
                if (pending != 0ull) {
#pragma unroll
                    for (int e = 0; e < 64; ++e) {
                        if (!((pending >> e) & 1ull)) continue;
                        const int q = e >> 4, ee = e & 15, row = row0 + 8 * (ee >> 2) + (ee & 3) + 32 * (q >> 1);
                        float dot = q == 0 ? acc00[ee] : q == 1 ? acc01[ee] : q == 2 ? acc10[ee] : acc11[ee];
                        // (opaque to the compiler: the key is formed again here, by the same operations, instead of 64 float64
                        //  values of the test above staying live for this rare path)
                        asm volatile("" : "+v"(dot));
                        const double key = ((hA_s[row] + ((q & 1) ? hb1 : hb0)) - (double)dot) - ((q & 1) ? v1 : v0);
                        bool done = true;
                        if (key <= tau_s[row]) {             // (again: a cut may have lowered tau since the mask was formed)
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
                for (int r = w; r < HLL_BM; r += HL_THREADS / 64) {
                    if (__builtin_amdgcn_readfirstlane(cnt_s[r]) < CAP) continue;
                    HlsEntries<(CAP + 63) / 64> en;
                    hls_rank_row<CAP>(cd_s[r], cc_s[r], CAP, hA_s[r], hBf, vf, sv_s[w], lane, en);
#pragma unroll
                    for (int q = 0; q < (CAP + 63) / 64; ++q)
                        if (en.valid[q] && en.rank[q] < k) {
                            cd_s[r][en.rank[q]] = en.dot[q];
                            cc_s[r][en.rank[q]] = en.col[q];
                            if (en.rank[q] == k - 1) tau_s[r] = en.key[q];
                        }
                    if (lane == 0) cnt_s[r] = k;
                    hl_wave_sync();
                }
                __syncthreads();
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) acc00[e] = acc01[e] = acc10[e] = acc11[e] = 0.0f;
        }
        tile = ntile;
        c = nc;
        buf ^= 1;
        __syncthreads();
    }

    // ---- the rows' lists, ascending by (key, column); the bound is what is written ---------------------------------------------
    for (int r = w; r < HLL_BM; r += HL_THREADS / 64) {
        const long row = (long)pb * HLL_BM + r;
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
        HlsEntries<(CAP + 63) / 64> en;
        hls_rank_row<CAP>(cd_s[r], cc_s[r], n, ha, hBf, vf, sv_s[w], lane, en);
#pragma unroll
        for (int q = 0; q < (CAP + 63) / 64; ++q)
            if (en.valid[q] && en.rank[q] < k) {
                out_col[base + en.rank[q]] = en.col[q];
                out_val[base + en.rank[q]] = en.b[q];
            }
        for (int t = min(n, k) + lane; t < k; t += 64) {
            out_col[base + t] = -1;
            out_val[base + t] = inf;
        }
    }
}

// The merge of all three row-list kernels (here and pm_hellinger_bf16.hip): the S sorted partial lists (column, bound) of one (frame, row) -> its k smallest by (key, column),
// key = bound - v[column] re-formed by the subtraction hl_select_kernel ranked with.  One wave per row; the lane that holds the
// winning head writes it.
__global__ __launch_bounds__(256) void hl_select_merge_kernel(const int32_t *__restrict__ pcol, const double *__restrict__ pval,
                                                              const double *__restrict__ hA, const double *__restrict__ v, int nA,
                                                              int nB, int S, int k, int32_t *__restrict__ out_col,
                                                              double *__restrict__ out_val) {
    const int lane = threadIdx.x & 63, f = blockIdx.y;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nA) return;
    const size_t base = ((size_t)f * nA + row) * S * k, obase = ((size_t)f * nA + row) * k;
    const double *vf = v ? v + (size_t)f * nB : nullptr;
    const double inf = __builtin_inf(), ha = hA[row];
    if (ha != ha) {
        for (int t = lane; t < k; t += 64) {
            out_col[obase + t] = -1;
            out_val[obase + t] = ha;
        }
        return;
    }
    int pos[4], hc[4];
    double hb[4], hk[4];
    auto load = [&](int q) {      // the head of list lane + 64 q at pos[q]: INT_MAX / +inf past its end
        const int l = lane + 64 * q;
        hc[q] = (l < S && pos[q] < k) ? pcol[base + (size_t)l * k + pos[q]] : -1;
        hb[q] = hc[q] >= 0 ? pval[base + (size_t)l * k + pos[q]] : inf;
        hk[q] = hc[q] >= 0 ? hb[q] - (vf ? vf[hc[q]] : 0.0) : inf;
        if (hc[q] < 0) hc[q] = INT_MAX;
    };
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        pos[q] = 0;
        load(q);
    }
    for (int t = 0; t < k; ++t) {
        double bk = hk[0];
        int bc = hc[0];
#pragma unroll
        for (int q = 1; q < 4; ++q)
            if (hk[q] < bk || (hk[q] == bk && hc[q] < bc)) {
                bk = hk[q];
                bc = hc[q];
            }
        double mk = bk;
        int mc = bc;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ok = __shfl_xor(mk, off, PM_WAVE);
            const int oc = __shfl_xor(mc, off, PM_WAVE);
            if (ok < mk || (ok == mk && oc < mc)) {
                mk = ok;
                mc = oc;
            }
        }
        if (mc == INT_MAX) {
            if (lane == 0) {
                out_col[obase + t] = -1;
                out_val[obase + t] = inf;
            }
            continue;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (hc[q] == mc) {          // (columns are distinct: exactly one head of one lane)
                out_col[obase + t] = mc;
                out_val[obase + t] = hb[q];
                ++pos[q];
                load(q);
            }
    }
}

// ---- host side: the three entry points' geometries (pm_hellinger.h), what they run first, and their launches in bands --------
// automatic splits: two workgroups per CU of a 256-CU device for the resident kernel; four such rounds for the selection (a split
// repeats the first tiles' cuts and adds a merge, but a last round that is a quarter full costs more); eight rounds of three per
// CU for the listing (a split costs nothing there — no partial lists, no merge — and short workgroups keep the last round full)
constexpr HlGeometry HL_TOPK = {HL_BM, HL_BM, HL_TILE * sizeof(float), true, HL_KMAX, 512};
constexpr HlGeometry HL_SELECT = {HLL_BM, HLL_BM, HL_TILE * sizeof(float), true, HL_KMAX, 2048};
constexpr HlGeometry HL_LIST = {HLL_BM, HLL_BM, HL_TILE * sizeof(float), false, 0, 6144};

struct HlBuffers {
    float *rA, *rB;
    double *hA, *hB, *pval;
    int32_t *pcol;
    unsigned long long *cnt;
};

// clears the flag (and the listing's counters), then the sqrt-descriptors and half row sums of both clouds into the workspace
static HlBuffers hl_prepare(const HlGeometry &g, const HlLayout &L, void *ws, const double *scA, int nA, const double *scB, int nB,
                            size_t frame_stride, int F, int32_t *nonfinite1, hipStream_t s) {
    char *base = (char *)ws;
    const HlBuffers b = {(float *)(base + L.rA),    (float *)(base + L.rB),     (double *)(base + L.hA),           (double *)(base + L.hB),
                         (double *)(base + L.pval), (int32_t *)(base + L.pcol), (unsigned long long *)(base + L.cnt)};
    const int padA = (int)(L.PB * g.block_rows), padB = (int)(L.CT * g.tile_rows);
    if (g.lists)
        hl_clear_flag_kernel<<<1, 1, 0, s>>>(nonfinite1);
    else
        hl_list_clear_kernel<<<1, 64, 0, s>>>(b.cnt, F, nonfinite1);
    hl_prep_kernel<<<dim3((unsigned int)((padA + 255) / 256), 1), 256, 0, s>>>(scA, 0, nA, padA, b.rA, b.hA, __builtin_nan(""), nonfinite1);
    hl_prep_kernel<<<dim3((unsigned int)((padB + 255) / 256), F), 256, 0, s>>>(scB, frame_stride, nB, padB, b.rB, b.hB, __builtin_inf(),
                                                                              nonfinite1);
    return b;
}

// launch(first block, grid) per band of row blocks: one launch stays under 2^32 work-items, as pm_chi2.hip's launchers cut theirs
template <class Launch>
static void hl_bands(long blocks, int S, int F, Launch launch) {
    const long band = std::max(1L, (0xffffffffL / HL_THREADS) / ((long)S * F));
    for (long b0 = 0; b0 < blocks; b0 += band) launch((int)b0, dim3((unsigned int)(std::min(band, blocks - b0) * S), F));
}

}  // namespace pm

extern "C" size_t pm_hellinger_list_workspace(int nA, int nB, int n_frames) { return pm::hl_layout(pm::HL_LIST, nA, nB, n_frames, 0).bytes; }

extern "C" int pm_hellinger_list(const double *scA, int nA, const double *scB, int nB, size_t frame_stride, int n_frames,
                                 const double *u, const double *v, const int32_t *skip, double tau, int split, int32_t *out_rc,
                                 double *out_bound, int cap, int32_t *count, int32_t *nonfinite1, void *ws, size_t ws_bytes,
                                 void *stream) {
    using namespace pm;
    const HlLayout L = hl_layout(HL_LIST, nA, nB, n_frames, 0);
    const bool args = scA && scB && u && v && out_rc && out_bound && count && nonfinite1 && cap > 0 && tau == tau;
    if (const int err = hl_check(args, L, nB, n_frames, split, frame_stride, ws, ws_bytes)) return err;
    hipStream_t s = (hipStream_t)stream;
    const int S = hl_splits(HL_LIST, L, split, n_frames), CT = (int)L.CT;
    // a +inf bound (a padding or non-finite fixed row) fails the comparison against any finite tau: tau = +inf becomes the largest one
    const double tau_f = std::min(tau, HL_TAU0);

    const HlBuffers b = hl_prepare(HL_LIST, L, ws, scA, nA, scB, nB, frame_stride, n_frames, nonfinite1, s);
    hl_bands(L.PB, S, n_frames, [&](int b0, dim3 grid) {
        hl_list_kernel<<<grid, HL_THREADS, 0, s>>>(b.rA, b.rB, b.hA, b.hB, u, v, skip, tau_f, nA, nB, CT, b0, S, cap, out_rc, out_bound, b.cnt);
    });
    hl_list_finish_kernel<<<1, 64, 0, s>>>(b.cnt, n_frames, count);
    return launch_status();
}

extern "C" size_t pm_hellinger_select_workspace(int nA, int nB, int n_frames, int k) {
    return pm::hl_layout(pm::HL_SELECT, nA, nB, n_frames, k).bytes;
}

extern "C" int pm_hellinger_select(const double *scA, int nA, const double *scB, int nB, size_t frame_stride, int n_frames,
                                   const double *v, int k, int split, int32_t *out_col, double *out_bound, int32_t *nonfinite1,
                                   void *ws, size_t ws_bytes, void *stream) {
    using namespace pm;
    const HlLayout L = hl_layout(HL_SELECT, nA, nB, n_frames, k);
    const bool args = scA && scB && out_col && out_bound && nonfinite1;
    if (const int err = hl_check(args, L, nB, n_frames, split, frame_stride, ws, ws_bytes)) return err;
    hipStream_t s = (hipStream_t)stream;
    const int S = hl_splits(HL_SELECT, L, split, n_frames), CT = (int)L.CT;

    const HlBuffers b = hl_prepare(HL_SELECT, L, ws, scA, nA, scB, nB, frame_stride, n_frames, nonfinite1, s);
    int32_t *oc = S == 1 ? out_col : b.pcol;
    double *ov = S == 1 ? out_bound : b.pval;
    hl_bands(L.PB, S, n_frames, [&](int b0, dim3 grid) {
        if (k <= 16)
            hl_select_kernel<32><<<grid, HL_THREADS, 0, s>>>(b.rA, b.rB, b.hA, b.hB, v, nA, nB, CT, b0, S, k, oc, ov);
        else
            hl_select_kernel<HL_CAP><<<grid, HL_THREADS, 0, s>>>(b.rA, b.rB, b.hA, b.hB, v, nA, nB, CT, b0, S, k, oc, ov);
    });
    if (S > 1)
        hl_select_merge_kernel<<<dim3((unsigned int)((nA + 3) / 4), n_frames), 256, 0, s>>>(b.pcol, b.pval, b.hA, v, nA, nB, S, k, out_col,
                                                                                           out_bound);
    return launch_status();
}

extern "C" size_t pm_hellinger_topk_workspace(int nA, int nB, int n_frames, int k) {
    return pm::hl_layout(pm::HL_TOPK, nA, nB, n_frames, k).bytes;
}

extern "C" int pm_hellinger_delta(double *delta1_host) {
    if (!delta1_host) return PM_ERR_INVALID_ARG;
    *delta1_host = PM_HELLINGER_DELTA;
    return PM_OK;
}

extern "C" int pm_hellinger_topk(const double *scA, int nA, const double *scB, int nB, size_t frame_stride, int n_frames, int k,
                                 int split, int32_t *out_col, double *out_bound, int32_t *nonfinite1, void *ws, size_t ws_bytes,
                                 void *stream) {
    using namespace pm;
    const HlLayout L = hl_layout(HL_TOPK, nA, nB, n_frames, k);
    const bool args = scA && scB && out_col && out_bound && nonfinite1;
    if (const int err = hl_check(args, L, nB, n_frames, split, frame_stride, ws, ws_bytes)) return err;
    hipStream_t s = (hipStream_t)stream;
    const int S = hl_splits(HL_TOPK, L, split, n_frames), CT = (int)L.CT;

    const HlBuffers b = hl_prepare(HL_TOPK, L, ws, scA, nA, scB, nB, frame_stride, n_frames, nonfinite1, s);
    hl_bands(L.PB, S, n_frames, [&](int b0, dim3 grid) {
        hl_topk_kernel<<<grid, HL_THREADS, 0, s>>>(b.rA, b.rB, b.hA, b.hB, nA, CT, b0, S, k, S == 1 ? out_col : b.pcol,
                                                   S == 1 ? out_bound : b.pval);
    });
    if (S > 1)      // (no prices: the keys are the bounds, nB is not read)
        hl_select_merge_kernel<<<dim3((unsigned int)((nA + 3) / 4), n_frames), 256, 0, s>>>(b.pcol, b.pval, b.hA, nullptr, nA, nB, S, k,
                                                                                           out_col, out_bound);
    return launch_status();
}
