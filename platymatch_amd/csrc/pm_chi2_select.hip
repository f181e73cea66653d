// pm_chi2_select.hip — exact rescoring of per-row candidate lists: from a lower bound's lists to the row's proven nearest columns.
//
// pm_hellinger_select (pm_hellinger.hip) answers a solver's row_select(v, k) with a LOWER BOUND of the cost.  What reaches the
// sparse core or a verdict must be the exact chi-square cost with the exact build's bits.  chi2_select_kernel takes the lists as
// they lie — [frame][moving row][kc] columns and bounds — evaluates every candidate exactly, orders each row by exact reduced cost
// and counts how many leading entries are PROVEN to be the row's true smallest: every unlisted column costs at least the last
// listed key minus delta, so an exact key strictly below that threshold cannot be beaten by anything outside the list.
// One launch, no N x M matrix, no temporaries.
//
// Arithmetic (the contract is bits, so nothing here belongs to the matrix cores): per candidate 360 terms
//     b = (b == 0) ? 1e-300 : b;   df = a - b;   T = div_pos(df * df, a + b)
// one rounding each, as chi2_kernel (pm_chi2.hip) forms them.  The 12 terms of a shell stay in registers and go into two running
// sums: natural order p = 0..11 (chi2_kernel's sum: out_cost has pm_chi2_cost's bits) and rolled order p = 6..11, 0..5
// (entries_sym_kernel's sr: out_twin has pm_chi2_entries_sym's out_rolled bits where the frames are the phi permutations of
// frame 1 — a relation this kernel never assumes: the frames are explicit pointers).  Both sums are halved at the end.
//
// Work split.  A UNIT is a pair (frame f, moving row i); lane <-> one candidate of a unit.  The padded list length KC in
// {16, 32, 64} is a template parameter and a wave holds 64 / KC units.  A 256-thread workgroup owns CS_ROWS = 16 consecutive
// moving rows with ALL their frames: the rows are fetched from HBM once per workgroup (a straight 16-byte copy of 46 080
// contiguous bytes into LDS) however many candidates and frames use them — the entry-per-thread route (entries_sym_kernel)
// reads the moving row once per entry.  Units are numbered row-major with the frame fastest and dealt to the waves in order,
// so the units of a wave are the frames of one row (KC = 16, F = 4) or of two neighbouring rows: the lanes of a unit read ONE
// LDS address (a broadcast), and different rows of a wave sit 2 880 B = 16 banks apart: ds_read_b128 without conflicts.
// After the staging barrier the waves never meet again: no barrier in the main loop.
//
// Fixed rows: a gather of kc arbitrary 2 880-byte rows per unit.  Of the two ways to bring them in —
//   (a) a cooperative copy through LDS (8 lanes per 128-byte line, 112-byte row pitch, the next stage in registers), or
//   (b) per-lane 16-byte global loads straight into registers —
// this kernel takes (b).  A lane walks ITS row front to back, 96 contiguous bytes per shell, so every 128-byte line it touches
// is used whole within two consecutive stages whichever way it arrives; (a) would buy fewer, fuller requests per instruction
// at the price of 14 KB of LDS per wave and stage (with the moving rows: one workgroup per CU less), an LDS write and read of
// every byte and a wave-level synchronisation per stage.  With (b) the LDS holds the moving rows alone (three workgroups per
// CU) and the latency is covered by depth instead: a stage is CS_SH = 2 shells = 12 double2 loads per lane (12 KB per wave),
// and the NEXT stage's loads are issued into a second register set before the current stage's 24 divisions start (two register
// sets in ping-pong, the loop unrolled by two: no copies).
// Absent candidates (-1, padded lanes q >= kc, out of range) load row 0 of their frame and are masked afterwards; a wave
// without a single present candidate skips the arithmetic.
//
// Epilogue, inside the wave: key = C - v[f][c] (one float64 subtraction; C when there are no prices), absent lanes +inf with
// column INT_MAX.  Each lane ranks its (key, column) against the KC - 1 others of its unit by cross-lane reads (__shfl; ties of
// equal (key, column) — which lists of distinct columns do not contain — are broken by list position, so the ranks are a
// permutation for any input without NaN keys).  Lanes of rank < k write their slot; absent lanes rank after all present ones
// and so write the -1 / +inf tail.  The threshold T comes from the lane holding list position kc - 1; the proof count is the
// population of a ballot over (present, rank < k, key < T) inside the unit — ranks follow key order, so these are the leading
// entries by construction.  No LDS sort, no atomics but the status word's.
//
// Resources (tools/kernel_resources.py): see DESIGN.md §4.8.  One launch covers up to 2^32 / 256 workgroups of 16 rows
// (268 million rows); beyond that the rows are cut into bands, as the other launchers of this library do.
#include <limits.h>

#include <algorithm>

#include "pm_common.h"

namespace pm {

constexpr int CS_THREADS = 256;
constexpr int CS_ROWS = 16;                            // moving rows per workgroup (46 080 B of LDS)
constexpr int CS_SHELL = 12;                           // bins per (r, theta) shell
constexpr int CS_SH = 2;                               // shells per stage
constexpr int CS_STAGE = CS_SH * CS_SHELL;             // bins per stage (12 double2 per lane)
constexpr int CS_NSTAGE = PM_NBINS / CS_STAGE;         // 15
constexpr int CS_KCMAX = 64;
constexpr double CS_TINY = 1e-300;
static_assert(CS_NSTAGE * CS_STAGE == PM_NBINS && CS_NSTAGE % 2 == 1, "the ping-pong loop: pairs of stages and a last one");

__global__ void cs_clear_status_kernel(int32_t *status1) { status1[0] = 0; }

// Keeps the compiler from moving memory operations across this point.  The ping-pong loop below depends on WHERE the next stage's
// loads are issued: left alone, the compiler folds the preheader's and the loop's loads of one register set into a single load at
// the top of the loop body, directly in front of its use.  (The fixed rows' pointer is not __restrict__ for the same reason: a
// no-alias argument's loads may cross an asm that is not handed the pointer.)
__device__ __forceinline__ void cs_pin() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

// a lane's 24 fixed bins of stage g (its own row)
__device__ __forceinline__ void cs_load_stage(double2 (&B)[CS_STAGE / 2], const double2 *brow, int g) {
    cs_pin();
#pragma unroll
    for (int e = 0; e < CS_STAGE / 2; ++e) B[e] = brow[g * (CS_STAGE / 2) + e];
    cs_pin();
}

// the stage's two shells: 12 terms each, into the natural-order and the rolled-order sum
__device__ __forceinline__ void cs_stage_terms(const double2 (&B)[CS_STAGE / 2], const double *arow, int g, double &sn, double &sr) {
#pragma unroll
    for (int s = 0; s < CS_SH; ++s) {
        double a[CS_SHELL], T[CS_SHELL];
#pragma unroll
        for (int p = 0; p < CS_SHELL; p += 2) {
            const double2 t = *reinterpret_cast<const double2 *>(arow + (g * CS_SH + s) * CS_SHELL + p);
            a[p] = t.x, a[p + 1] = t.y;
        }
#pragma unroll
        for (int p = 0; p < CS_SHELL; ++p) {
            double b = (p & 1) ? B[s * (CS_SHELL / 2) + p / 2].y : B[s * (CS_SHELL / 2) + p / 2].x;
            b = (b == 0.0) ? CS_TINY : b;
            const double df = a[p] - b;
            T[p] = div_pos(df * df, a[p] + b);
        }
#pragma unroll
        for (int p = 0; p < CS_SHELL; ++p) sn = sn + T[p];
#pragma unroll
        for (int p = 0; p < CS_SHELL; ++p) sr = sr + T[(p + 6) % CS_SHELL];
    }
}

template <int KC>
__global__ __launch_bounds__(CS_THREADS, 2) void chi2_select_kernel(const double *__restrict__ scA, int nA, const double *scB,
                                                                 int nB, size_t frame_stride, int F, const double *__restrict__ v,
                                                                 const int32_t *__restrict__ cand_col,
                                                                 const double *__restrict__ cand_bound, int kc, int k, double delta,
                                                                 long row0, int32_t *__restrict__ out_col, double *__restrict__ out_cost,
                                                                 double *__restrict__ out_twin, int32_t *__restrict__ out_proven,
                                                                 int32_t *__restrict__ status1) {
    static_assert(KC == 16 || KC == 32 || KC == 64, "a wave holds 64 / KC units");
    constexpr int UW = 64 / KC;      // units per wave
    __shared__ __attribute__((aligned(16))) double A_s[CS_ROWS * PM_NBINS];

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long r0 = row0 + (long)blockIdx.x * CS_ROWS;                  // (< nA: the launcher's grid)
    const int rows = (int)min((long)CS_ROWS, (long)nA - r0);
    {   // the workgroup's moving rows, straight into LDS
        const double2 *src = reinterpret_cast<const double2 *>(scA + (size_t)r0 * PM_NBINS);
        double2 *dst = reinterpret_cast<double2 *>(A_s);
        for (int e = tid; e < rows * (PM_NBINS / 2); e += CS_THREADS) dst[e] = src[e];
    }
    __syncthreads();

    const int q = lane & (KC - 1), base = lane & ~(KC - 1);              // list position; first lane of the unit
    const int nunits = rows * F;
    const double inf = __builtin_inf();
    const unsigned long long kcmask = kc == 64 ? ~0ull : (1ull << kc) - 1ull;
    for (int u0 = w * UW; u0 < nunits; u0 += (CS_THREADS / 64) * UW) {   // (uniform over the wave)
        const int u = u0 + base / KC;
        const bool unit_ok = u < nunits;
        const int uc = min(u, nunits - 1), rl = uc / F, f = uc - rl * F;
        const size_t unit = (size_t)f * nA + (size_t)(r0 + rl);
        int col = -1;
        double bound = inf;
        if (unit_ok && q < kc) {
            col = cand_col[unit * kc + q];
            bound = cand_bound[unit * kc + q];
        }
        const bool present = (unsigned int)col < (unsigned int)nB;
        const bool bad = col != -1 && !present;
        // the non-finite moving row of pm_hellinger_select: every candidate -1 with a NaN bound
        const bool nanrow = (((__builtin_amdgcn_ballot_w64(col == -1 && bound != bound) >> base) & kcmask) == kcmask) && unit_ok;
        const double *vf = v ? v + (size_t)f * nB : nullptr;

        double sn = 0.0, sr = 0.0;
        if (__builtin_amdgcn_ballot_w64(present) != 0ull) {
            const double2 *brow = reinterpret_cast<const double2 *>(scB + (size_t)f * frame_stride + (size_t)(present ? col : 0) * PM_NBINS);
            const double *arow = A_s + rl * PM_NBINS;
            double2 X[CS_STAGE / 2], Y[CS_STAGE / 2];
            cs_load_stage(X, brow, 0);
#pragma unroll 1
            for (int g = 0; g + 1 < CS_NSTAGE; g += 2) {
                cs_load_stage(Y, brow, g + 1);
                cs_stage_terms(X, arow, g, sn, sr);
                cs_load_stage(X, brow, g + 2);
                cs_stage_terms(Y, arow, g + 1, sn, sr);
            }
            cs_stage_terms(X, arow, CS_NSTAGE - 1, sn, sr);
        }
        const double C = present ? 0.5 * sn : inf, Ct = present ? 0.5 * sr : inf;
        double key = inf, tl = inf;      // tl: this lane's candidate as the LAST of the list -> the unit's threshold
        if (present) {
            const double vc = vf ? vf[col] : 0.0;
            key = vf ? C - vc : C;
            tl = (vf ? bound - vc : bound) - delta;
        } else if (bad) {
            tl = __builtin_nan("");       // (an unusable last candidate proves nothing)
        }
        const int colx = present ? col : INT_MAX;
        int rank = 0;
        for (int j = 0; j < KC; ++j) {
            const double kj = __shfl(key, base + j, PM_WAVE);
            const int cj = __shfl(colx, base + j, PM_WAVE);
            rank += (kj < key || (kj == key && (cj < colx || (cj == colx && j < q)))) ? 1 : 0;
        }
        const double T = __shfl(tl, base + kc - 1, PM_WAVE);
        const unsigned long long below = __builtin_amdgcn_ballot_w64(present && rank < k && key < T);
        if (__builtin_amdgcn_ballot_w64(bad) != 0ull && bad) atomicOr(status1, 2);
        if (!unit_ok) continue;
        if (nanrow) {
            const double nan = __builtin_nan("");
            if (q < k) {
                out_col[unit * k + q] = -1;
                out_cost[unit * k + q] = nan;
                if (out_twin) out_twin[unit * k + q] = nan;
            }
            if (q == 0) {
                out_proven[unit] = 0;
                atomicOr(status1, 1);
            }
            continue;
        }
        if (rank < k) {
            out_col[unit * k + rank] = present ? col : -1;
            out_cost[unit * k + rank] = C;
            if (out_twin) out_twin[unit * k + rank] = Ct;
        }
        if (q == 0) out_proven[unit] = __popcll((below >> base) & (KC == 64 ? ~0ull : (1ull << KC) - 1ull));
    }
}

}  // namespace pm

extern "C" int pm_chi2_select_exact(const double *scA, int nA, const double *scB, int nB, size_t frame_stride, int n_frames,
                                    const double *v, const int32_t *cand_col, const double *cand_bound, int kc, int k, double delta,
                                    int32_t *out_col, double *out_cost, double *out_twin, int32_t *out_proven, int32_t *status1,
                                    void *stream) {
    using namespace pm;
    if (!scA || !scB || !cand_col || !cand_bound || !out_col || !out_cost || !out_proven || !status1 || nA <= 0 || nB <= 0 ||
        n_frames < 1 || n_frames > 4 || kc < 1 || kc > CS_KCMAX || k < 1 || k > kc || !(delta >= 0.0) ||
        (n_frames > 1 && frame_stride < (size_t)nB * PM_NBINS))
        return PM_ERR_INVALID_ARG;
    // descriptor rows are read as 16-byte pieces
    if ((((uintptr_t)scA | (uintptr_t)scB) & 15) != 0 || (n_frames > 1 && (frame_stride & 1) != 0)) return PM_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    cs_clear_status_kernel<<<1, 1, 0, s>>>(status1);
    const long blocks = ((long)nA + CS_ROWS - 1) / CS_ROWS, band = 0xffffffffL / CS_THREADS;      // under 2^32 work-items per launch
    for (long b0 = 0; b0 < blocks; b0 += band) {
        const unsigned int nb = (unsigned int)std::min(band, blocks - b0);
        const long row0 = b0 * CS_ROWS;
#define PM_CS_LAUNCH(KC)                                                                                                            \
    chi2_select_kernel<KC><<<nb, CS_THREADS, 0, s>>>(scA, nA, scB, nB, frame_stride, n_frames, v, cand_col, cand_bound, kc, k, delta, \
                                                     row0, out_col, out_cost, out_twin, out_proven, status1)
        if (kc <= 16)
            PM_CS_LAUNCH(16);
        else if (kc <= 32)
            PM_CS_LAUNCH(32);
        else
            PM_CS_LAUNCH(64);
#undef PM_CS_LAUNCH
    }
    return launch_status();
}
