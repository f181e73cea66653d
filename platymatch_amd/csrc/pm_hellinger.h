// pm_hellinger.h — what pm_hellinger.hip (float32 matrix path) and pm_hellinger_bf16.hip (split-bf16 path) share: the constants of
// the blocked operand layout, the kernels of the first file that the second launches as they are, and the host side that every
// entry point repeats — workspace layout, split rule, argument check.
#pragma once
#include <algorithm>

#include "pm_common.h"

namespace pm {

constexpr int HL_BM = 64;                        // rows per block of the operand layouts (both precisions)
constexpr int HL_TILE = PM_NBINS * HL_BM;        // floats of one 64-row block of the float32 layout
constexpr int HL_KMAX = 64;
constexpr int HL_SMAX = 256;                     // column splits per (row block, frame): what hl_select_merge_kernel merges
constexpr int HL_SPLIT_BLOCKS = 512;             // row blocks x splits never exceeds this (workspace of the partial lists)
constexpr double HL_TAU0 = 1.7976931348623157e308;      // the largest finite double: a +inf key never passes it

typedef float hl_f16 __attribute__((ext_vector_type(16)));

// LDS traffic between the lanes of ONE wave (its operations are processed in order; this keeps the compiler from moving them)
__device__ __forceinline__ void hl_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// defined in pm_hellinger.hip
__global__ void hl_clear_flag_kernel(int32_t *flag1);
__global__ __launch_bounds__(256) void hl_select_merge_kernel(const int32_t *__restrict__ pcol, const double *__restrict__ pval,
                                                              const double *__restrict__ hA, const double *__restrict__ v, int nA,
                                                              int nB, int S, int k, int32_t *__restrict__ out_col,
                                                              double *__restrict__ out_val);

// ---- host side ---------------------------------------------------------------------------------------------------------------
struct HlGeometry {          // what the workspace and the split rule of an entry point depend on
    int block_rows;          // moving rows per workgroup
    int tile_rows;           // fixed rows per tile
    size_t block_bytes;      // bytes of a 64-row block of the operand layout
    bool lists;              // the partial lists of the splits follow the operands (else the listing's counters)
    int kmax;
    long target;             // workgroups of a launch that the automatic split aims at
};

struct HlLayout {
    size_t rA, rB, hA, hB, pcol, pval, cnt, bytes;      // byte offsets (pcol, pval with lists; cnt without); bytes == 0: bad shape
    long PB, CT;                                        // blocks of moving rows, tiles of fixed rows
};

// k is ignored without lists
inline HlLayout hl_layout(const HlGeometry &g, int nA, int nB, int F, int k) {
    HlLayout w = {};
    if (nA <= 0 || nB <= 0 || F < 1 || F > 4 || (g.lists && (k < 1 || k > g.kmax))) return w;
    const size_t PB = ((size_t)nA + g.block_rows - 1) / g.block_rows, CT = ((size_t)nB + g.tile_rows - 1) / g.tile_rows;
    // rows x splits of the partial lists, per frame
    const size_t P = std::min(PB * g.block_rows * HL_SMAX, (size_t)HL_SPLIT_BLOCKS * g.block_rows);
    size_t o = 0;
    w.rA = o, o += align_up(PB * (g.block_rows / HL_BM) * g.block_bytes, 256);
    w.rB = o, o += align_up((size_t)F * CT * (g.tile_rows / HL_BM) * g.block_bytes, 256);
    w.hA = o, o += align_up(PB * g.block_rows * sizeof(double), 256);
    w.hB = o, o += align_up((size_t)F * CT * g.tile_rows * sizeof(double), 256);
    if (g.lists) {
        w.pcol = o, o += align_up((size_t)F * P * k * sizeof(int32_t), 256);
        w.pval = o, o += align_up((size_t)F * P * k * sizeof(double), 256);
    } else {
        w.cnt = o, o += 256;
    }
    w.bytes = o;
    w.PB = (long)PB, w.CT = (long)CT;
    return w;
}

// column splits per (row block, frame): the caller's, or enough for target_workgroups per launch; never more than there are
// tiles, than HL_SMAX, or than the partial lists' workspace of split_rows rows x splits holds (split_rows == 0: no lists, no limit)
inline int hl_splits(int split, long blocks, long tiles, int F, long target_workgroups, long split_rows, int block_rows) {
    long cap = std::min(tiles, (long)HL_SMAX);
    if (split_rows > 0) cap = std::min(cap, std::max(1L, split_rows / block_rows / blocks));
    const long want = split > 0 ? split : (target_workgroups + blocks * F - 1) / (blocks * F);
    return (int)std::max(1L, std::min(want, cap));
}
inline int hl_splits(const HlGeometry &g, const HlLayout &L, int split, int F) {
    return hl_splits(split, L.PB, L.CT, F, g.target, g.lists ? (long)HL_SPLIT_BLOCKS * g.block_rows : 0L, g.block_rows);
}

// the checks of an entry point before anything is enqueued.  pointers: its required pointers are all there; L: hl_layout of its
// arguments (bad shape or k: bytes == 0)
inline int hl_check(bool pointers, const HlLayout &L, int nB, int F, int split, size_t frame_stride, const void *ws, size_t ws_bytes) {
    if (!pointers || L.bytes == 0 || split < 0 || (F > 1 && frame_stride < (size_t)nB * PM_NBINS)) return PM_ERR_INVALID_ARG;
    if (!ws || ((uintptr_t)ws & 15) != 0 || ws_bytes < L.bytes) return PM_ERR_WORKSPACE;
    return PM_OK;
}

}  // namespace pm
