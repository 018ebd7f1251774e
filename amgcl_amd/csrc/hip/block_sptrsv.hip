// amgcl_amd — exact level-scheduled block (BSR) triangular solve for gfx950.
//
// Block twin of kernels.hip:sptrsv_levels_k, used by the block_ilu0 smoother
// with solve="exact".  The reference reaches the same result for
// static_matrix<double,B,B> values through the serial/level-parallel sweeps
// of amgcl/relaxation/detail/ilu_solve.hpp; here the level schedule over
// BLOCK rows (host: _core.tri_levels on the BSR pattern) is executed by ONE
// cooperative kernel per factor with a grid-wide sync between levels.
//
// In place on z.  Lower: strictly-lower blocks, unit block diagonal.
// Upper: strictly-upper blocks, then the already-inverted diagonal block.
//
// Lane mapping: a block row is owned by a sub-group of G lanes, G the next
// power of two >= B (1,2,4,4,8,8,8,8).  G divides 64, so a sub-group never
// straddles a wavefront and the B partial results of the upper solve can be
// exchanged with width-G shuffles: no scratch vector, no second sync.
// Lane r < B owns scalar row r of the block; lanes >= B touch no memory but
// stay in every loop, so they take part in the shuffles and in every
// grid.sync().
//
// The per-row arithmetic order is that of the host sweep
// (core.cpp:block_ilu0_solve): per stored block t = sum_c M[r][c]*z[c] with c
// ascending, then s -= t; the diagonal multiply sums c ascending from 0.

#include <hip/hip_cooperative_groups.h>
#include <hip/hip_runtime.h>

#include <cstdint>

#define BSPTRSV_BLOCK 256
// The runtime's occupancy answer can be one block per CU above what the
// hardware keeps co-resident for 256-thread blocks; a surplus block would
// never reach the grid barrier.  Stay well inside it: a level-scheduled solve
// gains nothing from more (the barrier cost grows with the block count).
#define BSPTRSV_MAX_PER_CU 4
#define BSPTRSV_MAX_GRID 2048

template <int B>
struct bsptrsv_group {
    static constexpr int value = B <= 1 ? 1 : B <= 2 ? 2 : B <= 4 ? 4 : 8;
};

// z is read by other workgroups after each sync: plain pointer, ordinary
// global loads and stores.
template <int B, bool LOWER>
__global__ void __launch_bounds__(BSPTRSV_BLOCK)
bsr_sptrsv_levels_k(int64_t nlev, const int *__restrict__ lptr,
                    const int *__restrict__ rows, const int *__restrict__ ptr,
                    const int *__restrict__ col, const double *__restrict__ val,
                    const double *__restrict__ dinv, double *z) {
    constexpr int G = bsptrsv_group<B>::value;
    cooperative_groups::grid_group grid = cooperative_groups::this_grid();
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int r = (int)(tid & (G - 1));
    const int64_t sub = tid / G;
    const int64_t nsub = ((int64_t)gridDim.x * blockDim.x) / G;
    const bool owner = r < B;
    for (int64_t lev = 0; lev < nlev; ++lev) {
        const int64_t end = lptr[lev + 1];
        // all G lanes of a sub-group share k, so they loop together
        for (int64_t k = lptr[lev] + sub; k < end; k += nsub) {
            const int64_t i = rows[k];
            double s = 0.0;
            if (owner) {
                s = z[i * B + r];
                for (int j = ptr[i]; j < ptr[i + 1]; ++j) {
                    const double *m = val + ((int64_t)j * B + r) * B;
                    const double *zk = z + (int64_t)col[j] * B;
                    double t = 0.0;
#pragma unroll
                    for (int c = 0; c < B; ++c) t += m[c] * zk[c];
                    s -= t;
                }
            }
            if (LOWER) {
                if (owner) z[i * B + r] = s;
            } else {
                double sc[B];
#pragma unroll
                for (int c = 0; c < B; ++c) sc[c] = G > 1 ? __shfl(s, c, G) : s;
                if (owner) {
                    const double *d = dinv + (i * B + r) * B;
                    double t = 0.0;
#pragma unroll
                    for (int c = 0; c < B; ++c) t += d[c] * sc[c];
                    z[i * B + r] = t;
                }
            }
        }
        grid.sync();
    }
}

// Largest co-resident grid for one instantiation on the current device.
template <int B, bool LOWER>
static int bsptrsv_grid(int *grid_blocks) {
    static int cache[16] = {0};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int)e;
    if (dev >= 0 && dev < 16 && cache[dev]) {
        *grid_blocks = cache[dev];
        return 0;
    }
    int per_cu = 0, ncu = 0;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &per_cu, (const void *)bsr_sptrsv_levels_k<B, LOWER>, BSPTRSV_BLOCK, 0);
    if (e != hipSuccess) return (int)e;
    e = hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return (int)e;
    if (per_cu > BSPTRSV_MAX_PER_CU) per_cu = BSPTRSV_MAX_PER_CU;
    int g = per_cu * ncu;
    if (g < 1) g = 1;
    if (g > BSPTRSV_MAX_GRID) g = BSPTRSV_MAX_GRID;
    if (dev >= 0 && dev < 16) cache[dev] = g;
    *grid_blocks = g;
    return 0;
}

template <int B, bool LOWER>
static int launch_bsr_sptrsv(int64_t nlev, const int *lptr, const int *rows,
                             const int *ptr, const int *col, const double *val,
                             const double *dinv, double *z, int max_blocks,
                             hipStream_t stream) {
    int grid_blocks = 0;
    int rc = bsptrsv_grid<B, LOWER>(&grid_blocks);
    if (rc) return rc;
    if (max_blocks > 0 && max_blocks < grid_blocks) grid_blocks = max_blocks;
    void *args[] = {&nlev, (void *)&lptr, (void *)&rows, (void *)&ptr,
                    (void *)&col, (void *)&val, (void *)&dinv, (void *)&z};
    return (int)hipLaunchCooperativeKernel(
        (const void *)bsr_sptrsv_levels_k<B, LOWER>, dim3(grid_blocks),
        dim3(BSPTRSV_BLOCK), args, 0, stream);
}

#define BSPTRSV_DISPATCH(fn, ...)                                           \
    switch (bsize) {                                                        \
        case 1: return lower ? fn<1, true>(__VA_ARGS__) : fn<1, false>(__VA_ARGS__); \
        case 2: return lower ? fn<2, true>(__VA_ARGS__) : fn<2, false>(__VA_ARGS__); \
        case 3: return lower ? fn<3, true>(__VA_ARGS__) : fn<3, false>(__VA_ARGS__); \
        case 4: return lower ? fn<4, true>(__VA_ARGS__) : fn<4, false>(__VA_ARGS__); \
        case 5: return lower ? fn<5, true>(__VA_ARGS__) : fn<5, false>(__VA_ARGS__); \
        case 6: return lower ? fn<6, true>(__VA_ARGS__) : fn<6, false>(__VA_ARGS__); \
        case 7: return lower ? fn<7, true>(__VA_ARGS__) : fn<7, false>(__VA_ARGS__); \
        case 8: return lower ? fn<8, true>(__VA_ARGS__) : fn<8, false>(__VA_ARGS__); \
        default: return (int)hipErrorInvalidValue;                          \
    }

// z := (I+L)^-1 z (lower != 0) or z := (D+U)^-1 z (lower == 0, dinv = the
// nb*B*B inverted diagonal blocks).  max_blocks > 0 lowers the grid below
// the co-residency bound (never above it); 0 = automatic.
extern "C" int amg_bsr_sptrsv_f64(int64_t nlev, const int *lptr, const int *rows,
                                  int bsize, const int *ptr, const int *col,
                                  const double *val, const double *dinv, double *z,
                                  int lower, int max_blocks, hipStream_t s) {
    BSPTRSV_DISPATCH(launch_bsr_sptrsv, nlev, lptr, rows, ptr, col, val, dinv, z,
                     max_blocks, s)
}

// Launch geometry of one instantiation on the current device: the automatic
// grid (blocks), the workgroup size and the lanes per block row.
extern "C" int amg_bsr_sptrsv_geometry(int bsize, int lower, int *grid_blocks,
                                       int *block_threads, int *group_lanes) {
    if (bsize < 1 || bsize > 8) return (int)hipErrorInvalidValue;
    *block_threads = BSPTRSV_BLOCK;
    *group_lanes = bsize <= 1 ? 1 : bsize <= 2 ? 2 : bsize <= 4 ? 4 : 8;
    BSPTRSV_DISPATCH(bsptrsv_grid, grid_blocks)
}
