// amgcl_amd — shared device helpers for the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#define WAVE 64

// XCD-aware logical block id (guide cdna_hip_programming.md §1): the command
// processor round-robins workgroups across the 8 XCDs, so blocks with
// blockIdx%8==k run on XCD k.  Remapping gives each XCD one contiguous slice
// of the logical index space: the x-gather bands of neighboring CSR rows
// then land in a single XCD's L2 instead of being replicated in all eight.
// Affects speed only, never correctness.
// MEASURED (kbw384, r02): the swizzle LOST bandwidth on every level
// (L0 4107->3337 GB/s): the natural round-robin dispatch already places
// same-XCD blocks ~8 blocks (~512 rows) apart, inside the stencil's +-n
// x-band, so L2 locality is better WITHOUT the remap.  Off by default,
// kept for A/B (-DAMGCL_SWIZZLE).
__device__ static inline int64_t amg_logical_block() {
#ifdef AMGCL_SWIZZLE
    unsigned g = gridDim.x;
    if ((g & 7u) == 0u)
        return (int64_t)(blockIdx.x & 7u) * (int64_t)(g >> 3) + (blockIdx.x >> 3);
#endif
    return blockIdx.x;
}

// MEASURED (kbw384, r02): nontemporal val/col loads LOST bandwidth badly on
// cache-resident coarse levels (L2-level 3653->2088 GB/s: a 15 MB matrix is
// L2/LLC-resident across V-cycle passes, and the evict-first hint destroys
// that residency) and did not help the streaming fine level either.  Off by
// default, kept for A/B (-DAMGCL_NT).
#ifdef AMGCL_NT
#define AMG_STREAM_LD(p) __builtin_nontemporal_load(p)
#else
#define AMG_STREAM_LD(p) (*(p))
#endif

// Launch geometry for memory-bound grid-stride kernels (guide §6 G11): cap
// at ~8 blocks/CU and grid-stride the rest; rounded to a multiple of 8 so
// the XCD swizzle divides evenly.
static inline int amg_nblocks(int64_t work, int block = 256, int cap = 2048) {
    int64_t b = (work + block - 1) / block;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    if (b > 8) b = (b + 7) & ~(int64_t)7;
    return (int)b;
}

// Sub-wave width of the CSR row kernels by mean row length (lanes per row).
static inline int amg_pick_subw(int64_t nrows, int64_t nnz) {
    double m = nrows ? (double)nnz / (double)nrows : 1.0;
    if (m <= 4) return 2;
    if (m <= 10) return 4;
    if (m <= 24) return 8;
    if (m <= 128) return 16;
    return 32;
}

// One sparse operator as the native solve driver (driver.hip) sees it: CSR
// plus an optional SELL-64 image, padded or compact (see kernels.hip).
// val/sval hold double, or float in the fp32 hierarchy of a mixed-precision
// solve.
struct OpDesc {
    int64_t nrows, nnz;
    const int *ptr;
    const int *col;
    const void *val;
    int subw;        // CSR lanes per row; <= 0: chosen at driver create
    int64_t nslice;  // 0 = no SELL image
    const int64_t *soff;
    const int *scol;
    const void *sval;
    const int *srows;  // optional sigma-sort permutation (slot -> row, < 0 = pad)
    // compact (pad-free) image when smask is set: scol/sval then hold exactly
    // nnz entries, smask one lane mask per slot, moff[nslice + 1] the slices'
    // first masks; soff and srows are unused
    const uint64_t *smask;
    const int64_t *moff;
};

// Which SELL-64 image an operator gets: the compact one when the padding it
// removes outweighs the masks and offsets it adds, in bytes.  slots = padded
// slots (64 x the summed slice widths), nmask = the summed slice widths,
// vbytes = sizeof(value).  The one statement of the rule, for every builder.
static inline bool amg_sell_compact_pays(int64_t slots, int64_t nnz, int64_t nmask,
                                         int64_t nslice, int vbytes) {
    return (slots - nnz) * (4 + vbytes) > 8 * nmask + 8 * (nslice + 1);
}

// Per-level descriptor consumed by amg_driver_create; filled either from
// Python (backend/native.py, torch tensors) or from the torch-free GPU C API
// (capi_gpu.hip, raw device buffers).  backend/native.py keeps a ctypes twin
// and checks it against amg_desc_layout (driver.hip) when it binds.
// The smoother of a level is whichever of ilu_iters, cheb_degree and
// spai1.nrows is nonzero, else the diagonal one in M; a zeroed descriptor
// (what capi_gpu.hip starts from) selects none of the three.
struct LevelDesc {
    OpDesc A;  // A.nrows is the level size (CSR arrays unused when bsize > 0)
    OpDesc P;  // nrows x next->nrows
    OpDesc R;  // next->nrows x nrows
    const double *M;  // diagonal smoother weights (SPAI-0, damped Jacobi)
    double *f;
    double *u;
    double *t;  // workspace (f/u unused at level 0)
    // Chebyshev smoothing (cheb_degree > 0 replaces the diagonal smoother;
    // M then holds the optional D^-1 scaling or null)
    int cheb_degree;
    double cheb_theta;
    double cheb_delta;
    double cheb_sigma1;
    void *cheb_d;  // extra per-level work vector for the recurrence
    // BSR storage of A (bsize > 0)
    int bsize;
    int64_t nbrows;
    const int *bptr;
    const int *bcol;
    const double *bval;
    // SPAI-1 smoothing (spai1.nrows > 0 replaces the diagonal smoother; a
    // zeroed descriptor means "not SPAI-1"): the approximate inverse, CSR
    // with A's pattern, applied as x += spai1 (f - A x).  fp64 only.
    OpDesc spai1;
    // ILU(0) smoothing via damped-Jacobi iterated triangular solves
    // (ilu_iters > 0; the reference's GPU-native ilu_solve.hpp route).
    // ilu_L strictly lower (unit diag implied), ilu_U strictly upper;
    // ilu_dinv is the inverted diagonal of U.
    int ilu_iters;
    double ilu_damping;   // outer relaxation damping
    double ilu_jdamping;  // inner Jacobi damping (0.72)
    OpDesc ilu_L;
    OpDesc ilu_U;
    const double *ilu_dinv;
    double *ilu_y;  // work vectors (level-sized)
    double *ilu_s;
    double *ilu_b;
};
