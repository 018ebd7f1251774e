// amgcl_amd — hand-written CDNA4 (gfx950) solve-phase kernels.
//
// Replaces the reference's hipSPARSE/rocThrust calls (amgcl/backend/hip.hpp:
// 239-306 SpMV, :486-491 residual, :546-677 vector ops, :532-544 dot,
// :418-446 gather/scatter) with kernels designed for MI355X:
//   - 64-wide wavefronts (sub-wave row groups for CSR SpMV),
//   - memory-bound ops vectorized and grid-stride capped (~2048 blocks),
//   - fused residual and fused diagonal-smoother step (one pass over A),
//   - fused multi-dot reductions (one kernel per CG/BiCGStab dot pair).
//
// Pure HIP: no torch headers; the Python side passes raw device pointers and
// the current torch HIP stream through ctypes (see backend/_hiplib.py).

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <type_traits>

#include "amg_common.h"
#include "amg_kernels.h"

// Every launcher below is written once as a template over the value type
// (launch_*<T>); the extern "C" _f64/_f32 entry points only forward to it.

extern "C" int amg_hip_last_error() { return (int)hipGetLastError(); }

// ---------------------------------------------------------------------------
// CSR SpMV: y = alpha*A*x + beta*y.
// SUBW lanes cooperate on one row (SUBW=1 -> thread per row). The variant is
// chosen by the host from the mean row length. BETA0 avoids reading y.
// ---------------------------------------------------------------------------
template <typename T, int SUBW, bool BETA0>
__global__ void spmv_k(int nrows, const int *__restrict__ ptr,
                       const int *__restrict__ col, const T *__restrict__ val,
                       const T *__restrict__ x, double alpha, double beta,
                       T *__restrict__ y) {
    int64_t tid = amg_logical_block() * blockDim.x + threadIdx.x;
    int lane = (int)(tid & (SUBW - 1));
    int64_t row = tid / SUBW;
    int64_t stride = ((int64_t)gridDim.x * blockDim.x) / SUBW;
    for (; row < nrows; row += stride) {
        double s = 0.0;
        int b = ptr[row], e = ptr[row + 1];
        for (int j = b + lane; j < e; j += SUBW) s += (double)AMG_STREAM_LD(&val[j]) * (double)x[AMG_STREAM_LD(&col[j])];
#pragma unroll
        for (int off = SUBW / 2; off > 0; off >>= 1) s += __shfl_down(s, off, SUBW);
        if (lane == 0) y[row] = (T)(BETA0 ? alpha * s : alpha * s + beta * (double)y[row]);
    }
}

// r = b - A x (fused residual; reference does copy+spmv, hip.hpp:486-491)
template <typename T, int SUBW>
__global__ void residual_k(int nrows, const int *__restrict__ ptr,
                           const int *__restrict__ col, const T *__restrict__ val,
                           const T *__restrict__ rhs, const T *__restrict__ x,
                           T *__restrict__ r) {
    int64_t tid = amg_logical_block() * blockDim.x + threadIdx.x;
    int lane = (int)(tid & (SUBW - 1));
    int64_t row = tid / SUBW;
    int64_t stride = ((int64_t)gridDim.x * blockDim.x) / SUBW;
    for (; row < nrows; row += stride) {
        double s = 0.0;
        int b = ptr[row], e = ptr[row + 1];
        for (int j = b + lane; j < e; j += SUBW) s += (double)AMG_STREAM_LD(&val[j]) * (double)x[AMG_STREAM_LD(&col[j])];
#pragma unroll
        for (int off = SUBW / 2; off > 0; off >>= 1) s += __shfl_down(s, off, SUBW);
        if (lane == 0) r[row] = (T)((double)rhs[row] - s);
    }
}

// t = M ∘ (rhs - A x): the fused SPAI0/Jacobi smoothing step
// (reference: residual + vmul as separate passes, relaxation/spai0.hpp:85-92)
template <typename T, int SUBW>
__global__ void relax_diag_k(int nrows, const int *__restrict__ ptr,
                             const int *__restrict__ col, const T *__restrict__ val,
                             const T *__restrict__ M, const T *__restrict__ rhs,
                             const T *__restrict__ x, T *__restrict__ t) {
    int64_t tid = amg_logical_block() * blockDim.x + threadIdx.x;
    int lane = (int)(tid & (SUBW - 1));
    int64_t row = tid / SUBW;
    int64_t stride = ((int64_t)gridDim.x * blockDim.x) / SUBW;
    for (; row < nrows; row += stride) {
        double s = 0.0;
        int b = ptr[row], e = ptr[row + 1];
        for (int j = b + lane; j < e; j += SUBW) s += (double)AMG_STREAM_LD(&val[j]) * (double)x[AMG_STREAM_LD(&col[j])];
#pragma unroll
        for (int off = SUBW / 2; off > 0; off >>= 1) s += __shfl_down(s, off, SUBW);
        if (lane == 0) t[row] = (T)((double)M[row] * ((double)rhs[row] - s));
    }
}

// The one place a runtime sub-wave width becomes a template argument:
// launch(std::integral_constant<int, SW>) for the widths the row kernels are
// instantiated for, hipErrorInvalidValue for any other.  subw <= 0 picks the
// width from the mean row length.
template <typename F>
static int by_subw(int subw, int64_t nrows, int64_t nnz, F launch) {
    if (subw <= 0) subw = amg_pick_subw(nrows, nnz);
#define CASE(SW)                                     \
    case SW:                                         \
        launch(std::integral_constant<int, SW>{});   \
        break;
    switch (subw) {
        CASE(1) CASE(2) CASE(4) CASE(8) CASE(16) CASE(32) CASE(64)
        default: return (int)hipErrorInvalidValue;
    }
#undef CASE
    return (int)hipGetLastError();
}

template <typename T>
static int launch_spmv(int64_t nrows, int64_t nnz, const int *ptr, const int *col,
                       const T *val, const T *x, double alpha, double beta, T *y,
                       int subw, hipStream_t stream) {
    return by_subw(subw, nrows, nnz, [&](auto sw) {
        constexpr int SW = decltype(sw)::value;
        const int grid = amg_nblocks(nrows * SW);
        if (beta == 0.0)
            spmv_k<T, SW, true><<<grid, 256, 0, stream>>>(nrows, ptr, col, val, x, alpha, beta, y);
        else
            spmv_k<T, SW, false><<<grid, 256, 0, stream>>>(nrows, ptr, col, val, x, alpha, beta, y);
    });
}

template <typename T>
static int launch_residual(int64_t nrows, int64_t nnz, const int *ptr, const int *col,
                           const T *val, const T *rhs, const T *x, T *r, int subw,
                           hipStream_t stream) {
    return by_subw(subw, nrows, nnz, [&](auto sw) {
        constexpr int SW = decltype(sw)::value;
        residual_k<T, SW><<<amg_nblocks(nrows * SW), 256, 0, stream>>>(nrows, ptr, col, val,
                                                                      rhs, x, r);
    });
}

template <typename T>
static int launch_relax_diag(int64_t nrows, int64_t nnz, const int *ptr, const int *col,
                             const T *val, const T *M, const T *rhs, const T *x, T *t,
                             int subw, hipStream_t stream) {
    return by_subw(subw, nrows, nnz, [&](auto sw) {
        constexpr int SW = decltype(sw)::value;
        relax_diag_k<T, SW><<<amg_nblocks(nrows * SW), 256, 0, stream>>>(nrows, ptr, col,
                                                                        val, M, rhs, x, t);
    });
}

extern "C" int amg_spmv_f64(int64_t nrows, int64_t nnz, const int *ptr, const int *col,
                            const double *val, const double *x, double alpha,
                            double beta, double *y, int subw, hipStream_t stream) {
    return launch_spmv(nrows, nnz, ptr, col, val, x, alpha, beta, y, subw, stream);
}
extern "C" int amg_spmv_f32(int64_t nrows, int64_t nnz, const int *ptr, const int *col,
                            const float *val, const float *x, double alpha, double beta,
                            float *y, int subw, hipStream_t stream) {
    return launch_spmv(nrows, nnz, ptr, col, val, x, alpha, beta, y, subw, stream);
}

extern "C" int amg_residual_f64(int64_t nrows, int64_t nnz, const int *ptr, const int *col,
                                const double *val, const double *rhs, const double *x,
                                double *r, int subw, hipStream_t stream) {
    return launch_residual(nrows, nnz, ptr, col, val, rhs, x, r, subw, stream);
}
extern "C" int amg_residual_f32(int64_t nrows, int64_t nnz, const int *ptr, const int *col,
                                const float *val, const float *rhs, const float *x,
                                float *r, int subw, hipStream_t stream) {
    return launch_residual(nrows, nnz, ptr, col, val, rhs, x, r, subw, stream);
}

extern "C" int amg_relax_diag_f64(int64_t nrows, int64_t nnz, const int *ptr,
                                  const int *col, const double *val, const double *M,
                                  const double *rhs, const double *x, double *t,
                                  int subw, hipStream_t stream) {
    return launch_relax_diag(nrows, nnz, ptr, col, val, M, rhs, x, t, subw, stream);
}
extern "C" int amg_relax_diag_f32(int64_t nrows, int64_t nnz, const int *ptr,
                                  const int *col, const float *val, const float *M,
                                  const float *rhs, const float *x, float *t, int subw,
                                  hipStream_t stream) {
    return launch_relax_diag(nrows, nnz, ptr, col, val, M, rhs, x, t, subw, stream);
}

// ---------------------------------------------------------------------------
// SELL-64 (sliced ELLPACK, slice = one 64-wide wavefront) kernels.
//
// CSR sub-wavefront mapping is fine for the 7-nnz fine level (cross-row
// gather coalescing), but on AMG coarse levels (mean 30-70 nnz/row) the
// lanes of a sub-wave walk ONE row's column list, so every x-gather hits a
// different cache line (measured: level-1 SpMV 2.0 TB/s vs 4.3 at level 0).
// SELL-64 is the wave-native layout: lane = row, slices stored column-major,
// so val/col stream perfectly coalesced AND the 64 lanes gather the i-th
// (sorted) neighbor of 64 *consecutive* rows — addresses that are themselves
// nearly consecutive for locality-ordered matrices.  Padding rows carry
// col = 0 / val = 0 (contribute nothing).  Conceptual twin of the
// reference's hybrid-ELL GPU format (amgcl/backend/vexcl_static_matrix.hpp
// csr2ell_kernel :450), redesigned for 64-wide CDNA4 wavefronts.
// ---------------------------------------------------------------------------
// srows: optional sigma-sort row permutation (slot -> row id; < 0 = pad
// slot).  Sorting rows by length inside sigma-sized windows cuts the slice
// padding of ragged coarse levels; the permutation stays within a window,
// so the scattered x/rhs/y accesses remain L2-local.
//
// COMPACT: the pad-free image.  Same mapping (slice = 64 consecutive rows,
// lane = row, slot i = the row's i-th CSR entry) but a slot stores only the
// lanes whose row is longer than i, packed in lane order, and one 64-bit lane
// mask per slot says which lanes those are.  moff[s] .. moff[s+1] index the
// slice's masks (its width w may be 0); the slice's entries start at the CSR
// ptr[64 s], so the image holds exactly nnz entries.  A lane's products are
// summed in slot order as in the padded kernel; only the trailing 0 * x[0]
// terms of the padding are gone.  The slice index is made wave-uniform, so
// masks and the running entry offset stay in scalar registers; the masks of
// SELLC_U slots are fetched ahead of the loads that depend on them.
#define SELLC_U 4
template <typename T, int MODE, bool COMPACT>  // 0: y=aAx+by  1: r=rhs-Ax  2: xn=x+M(rhs-Ax)
__global__ void sell_k(int64_t nrows, int64_t nslice,
                       const int64_t *__restrict__ soff,  // COMPACT: moff
                       const int *__restrict__ col,
                       const T *__restrict__ val, const int *__restrict__ srows,
                       const uint64_t *__restrict__ smask, const int *__restrict__ ptr,
                       const T *__restrict__ x,
                       double alpha, double beta, const T *__restrict__ rhs,
                       const T *__restrict__ M, T *__restrict__ y) {
    const int wpb = blockDim.x / WAVE;
    int wid = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
    if (COMPACT) wid = __builtin_amdgcn_readfirstlane(wid);
    int64_t s = (int64_t)blockIdx.x * wpb + wid;
    int64_t sstride = (int64_t)gridDim.x * wpb;
    for (; s < nslice; s += sstride) {
        double acc = 0.0;
        if (COMPACT) {
            const int64_t mbeg = soff[s];
            const int w = (int)(soff[s + 1] - mbeg);
            int64_t off = ptr[s * WAVE];
            for (int i = 0; i < w; i += SELLC_U) {
                uint64_t m[SELLC_U];
                int c[SELLC_U];
                T v[SELLC_U];
#pragma unroll
                for (int k = 0; k < SELLC_U; ++k) m[k] = i + k < w ? smask[mbeg + i + k] : 0;
#pragma unroll
                for (int k = 0; k < SELLC_U; ++k) {
                    c[k] = 0;
                    v[k] = (T)0;
                    if ((m[k] >> lane) & 1) {
                        // entries of this slot below this lane: the mbcnt pair
                        const int64_t j = off + __builtin_amdgcn_mbcnt_hi(
                            (unsigned)(m[k] >> 32),
                            __builtin_amdgcn_mbcnt_lo((unsigned)m[k], 0u));
                        c[k] = col[j];
                        v[k] = val[j];
                    }
                    off += __popcll(m[k]);
                }
                // gathers of all SELLC_U slots in flight before the first sum;
                // an inactive lane adds 0 * 0
                T xv[SELLC_U];
#pragma unroll
                for (int k = 0; k < SELLC_U; ++k) {
                    xv[k] = (T)0;
                    if ((m[k] >> lane) & 1) xv[k] = x[c[k]];
                }
#pragma unroll
                for (int k = 0; k < SELLC_U; ++k) acc += (double)v[k] * (double)xv[k];
            }
        } else {
            int64_t beg = soff[s], end = soff[s + 1];
            for (int64_t j = beg + lane; j < end; j += WAVE)
                acc += (double)val[j] * (double)x[col[j]];
        }
        int64_t row = (!COMPACT && srows) ? (int64_t)srows[s * WAVE + lane] : s * WAVE + lane;
        if (row >= 0 && row < nrows) {
            if (MODE == 0)
                y[row] = (T)(beta == 0.0 ? alpha * acc
                                         : alpha * acc + beta * (double)y[row]);
            else if (MODE == 1)
                y[row] = (T)((double)rhs[row] - acc);
            else
                y[row] = (T)((double)x[row] +
                             (double)M[row] * ((double)rhs[row] - acc));
        }
    }
}

template <typename T, int MODE>
static int launch_sell(int64_t nrows, int64_t nslice, const int64_t *soff, const int *col,
                       const T *val, const int *srows, const T *x, double alpha,
                       double beta, const T *rhs, const T *M, T *y, hipStream_t stream) {
    sell_k<T, MODE, false><<<amg_nblocks(nslice * WAVE), 256, 0, stream>>>(
        nrows, nslice, soff, col, val, srows, nullptr, nullptr, x, alpha, beta, rhs, M, y);
    return (int)hipGetLastError();
}

template <typename T, int MODE>
static int launch_sellc(int64_t nrows, int64_t nslice, const int64_t *moff,
                        const uint64_t *smask, const int *ptr, const int *col,
                        const T *val, const T *x, double alpha, double beta, const T *rhs,
                        const T *M, T *y, hipStream_t stream) {
    sell_k<T, MODE, true><<<amg_nblocks(nslice * WAVE), 256, 0, stream>>>(
        nrows, nslice, moff, col, val, nullptr, smask, ptr, x, alpha, beta, rhs, M, y);
    return (int)hipGetLastError();
}

extern "C" int amg_sell_spmv_f64(int64_t nrows, int64_t nslice, const int64_t *soff,
                                 const int *col, const double *val, const int *srows,
                                 const double *x, double alpha, double beta, double *y,
                                 hipStream_t stream) {
    return launch_sell<double, 0>(nrows, nslice, soff, col, val, srows, x, alpha, beta,
                                  nullptr, nullptr, y, stream);
}
extern "C" int amg_sell_spmv_f32(int64_t nrows, int64_t nslice, const int64_t *soff,
                                 const int *col, const float *val, const int *srows,
                                 const float *x, double alpha, double beta, float *y,
                                 hipStream_t stream) {
    return launch_sell<float, 0>(nrows, nslice, soff, col, val, srows, x, alpha, beta,
                                 nullptr, nullptr, y, stream);
}

extern "C" int amg_sell_residual_f64(int64_t nrows, int64_t nslice, const int64_t *soff,
                                     const int *col, const double *val, const int *srows,
                                     const double *rhs, const double *x, double *r,
                                     hipStream_t stream) {
    return launch_sell<double, 1>(nrows, nslice, soff, col, val, srows, x, 0.0, 0.0, rhs,
                                  nullptr, r, stream);
}
extern "C" int amg_sell_residual_f32(int64_t nrows, int64_t nslice, const int64_t *soff,
                                     const int *col, const float *val, const int *srows,
                                     const float *rhs, const float *x, float *r,
                                     hipStream_t stream) {
    return launch_sell<float, 1>(nrows, nslice, soff, col, val, srows, x, 0.0, 0.0, rhs,
                                 nullptr, r, stream);
}

extern "C" int amg_sell_relax_f64(int64_t nrows, int64_t nslice, const int64_t *soff,
                                  const int *col, const double *val, const int *srows,
                                  const double *M, const double *rhs, const double *x,
                                  double *xn, hipStream_t stream) {
    return launch_sell<double, 2>(nrows, nslice, soff, col, val, srows, x, 0.0, 0.0, rhs,
                                  M, xn, stream);
}
extern "C" int amg_sell_relax_f32(int64_t nrows, int64_t nslice, const int64_t *soff,
                                  const int *col, const float *val, const int *srows,
                                  const float *M, const float *rhs, const float *x,
                                  float *xn, hipStream_t stream) {
    return launch_sell<float, 2>(nrows, nslice, soff, col, val, srows, x, 0.0, 0.0, rhs,
                                 M, xn, stream);
}

// CSR -> SELL-64 fill: one wave per slice, iterating the element index i so
// every store of a wave is fully coalesced (lane-major); the CSR reads are
// gathers of 64 rows' i-th entries, which land close together for sorted
// matrices (setup-time cost matters: the fine level alone is ~11 GB).
template <typename T>
__global__ void sell_fill_k(int64_t nrows, int64_t nslice, const int *__restrict__ ptr,
                            const int *__restrict__ col, const T *__restrict__ val,
                            const int64_t *__restrict__ soff,
                            const int *__restrict__ srows, int *__restrict__ scol,
                            T *__restrict__ sval) {
    const int wpb = blockDim.x / WAVE;
    int wid = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
    int64_t s = (int64_t)blockIdx.x * wpb + wid;
    int64_t sstride = (int64_t)gridDim.x * wpb;
    for (; s < nslice; s += sstride) {
        int64_t row = srows ? (int64_t)srows[s * WAVE + lane] : s * WAVE + lane;
        int b = 0, len = 0;
        if (row >= 0 && row < nrows) {
            b = ptr[row];
            len = ptr[row + 1] - b;
        }
        int64_t beg = soff[s];
        int w = (int)((soff[s + 1] - beg) / WAVE);
        for (int i = 0; i < w; ++i) {
            int64_t dst = beg + (int64_t)i * WAVE + lane;
            if (i < len) {
                scol[dst] = col[b + i];
                sval[dst] = val[b + i];
            } else {  // padding written here so the host can use empty buffers
                scol[dst] = 0;
                sval[dst] = (T)0;
            }
        }
    }
}

template <typename T>
static int launch_sell_fill(int64_t nrows, int64_t nslice, const int *ptr, const int *col,
                            const T *val, const int64_t *soff, const int *srows,
                            int *scol, T *sval, hipStream_t stream) {
    sell_fill_k<T><<<amg_nblocks(nslice * WAVE), 256, 0, stream>>>(
        nrows, nslice, ptr, col, val, soff, srows, scol, sval);
    return (int)hipGetLastError();
}

extern "C" int amg_sell_fill_f64(int64_t nrows, int64_t nslice, const int *ptr,
                                 const int *col, const double *val,
                                 const int64_t *soff, const int *srows, int *scol,
                                 double *sval, hipStream_t stream) {
    return launch_sell_fill(nrows, nslice, ptr, col, val, soff, srows, scol, sval, stream);
}
extern "C" int amg_sell_fill_f32(int64_t nrows, int64_t nslice, const int *ptr,
                                 const int *col, const float *val,
                                 const int64_t *soff, const int *srows, int *scol,
                                 float *sval, hipStream_t stream) {
    return launch_sell_fill(nrows, nslice, ptr, col, val, soff, srows, scol, sval, stream);
}

// Compact-image twins of the entry points above (no sigma permutation: that
// form exists only to cut padding).
#define AMG_SELLC_ENTRIES(T, SFX)                                                          \
    extern "C" int amg_sellc_spmv_##SFX(int64_t nrows, int64_t nslice, const int64_t *moff, \
                                        const uint64_t *smask, const int *ptr,             \
                                        const int *col, const T *val, const T *x,          \
                                        double alpha, double beta, T *y,                   \
                                        hipStream_t stream) {                              \
        return launch_sellc<T, 0>(nrows, nslice, moff, smask, ptr, col, val, x, alpha,     \
                                  beta, nullptr, nullptr, y, stream);                      \
    }                                                                                      \
    extern "C" int amg_sellc_residual_##SFX(int64_t nrows, int64_t nslice,                 \
                                            const int64_t *moff, const uint64_t *smask,    \
                                            const int *ptr, const int *col, const T *val,  \
                                            const T *rhs, const T *x, T *r,                \
                                            hipStream_t stream) {                          \
        return launch_sellc<T, 1>(nrows, nslice, moff, smask, ptr, col, val, x, 0.0, 0.0,  \
                                  rhs, nullptr, r, stream);                                \
    }                                                                                      \
    extern "C" int amg_sellc_relax_##SFX(int64_t nrows, int64_t nslice,                    \
                                         const int64_t *moff, const uint64_t *smask,       \
                                         const int *ptr, const int *col, const T *val,     \
                                         const T *M, const T *rhs, const T *x, T *xn,      \
                                         hipStream_t stream) {                             \
        return launch_sellc<T, 2>(nrows, nslice, moff, smask, ptr, col, val, x, 0.0, 0.0,  \
                                  rhs, M, xn, stream);                                     \
    }                                                                                      \
    extern "C" int amg_sellc_fill_##SFX(int64_t nrows, int64_t nslice, const int *ptr,     \
                                        const int *col, const T *val, const int64_t *moff, \
                                        uint64_t *smask, int *scol, T *sval,               \
                                        hipStream_t stream) {                              \
        sellc_fill_k<T><<<amg_nblocks(nslice * WAVE), 256, 0, stream>>>(                   \
            nrows, nslice, ptr, col, val, moff, smask, scol, sval);                        \
        return (int)hipGetLastError();                                                     \
    }

// CSR -> compact SELL-64 fill, one wave per slice like sell_fill_k.  Slot i's
// mask is the ballot of i < len; lane 0 stores it, the active lanes store
// their entry at the slice's running offset plus their rank in the mask.
// moff must give each slice its longest row's length as width.
template <typename T>
__global__ void sellc_fill_k(int64_t nrows, int64_t nslice, const int *__restrict__ ptr,
                             const int *__restrict__ col, const T *__restrict__ val,
                             const int64_t *__restrict__ moff,
                             uint64_t *__restrict__ smask, int *__restrict__ scol,
                             T *__restrict__ sval) {
    const int wpb = blockDim.x / WAVE;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const int lane = threadIdx.x & (WAVE - 1);
    int64_t s = (int64_t)blockIdx.x * wpb + wid;
    int64_t sstride = (int64_t)gridDim.x * wpb;
    for (; s < nslice; s += sstride) {
        const int64_t row = s * WAVE + lane;
        int b = 0, len = 0;
        if (row < nrows) {
            b = ptr[row];
            len = ptr[row + 1] - b;
        }
        const int64_t mbeg = moff[s];
        const int w = (int)(moff[s + 1] - mbeg);
        int64_t off = ptr[s * WAVE];
        for (int i = 0; i < w; ++i) {
            const uint64_t m = __ballot(i < len);
            if (lane == 0) smask[mbeg + i] = m;
            if (i < len) {
                const int64_t j = off + __builtin_amdgcn_mbcnt_hi(
                    (unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                scol[j] = col[b + i];
                sval[j] = val[b + i];
            }
            off += __popcll(m);
        }
    }
}

AMG_SELLC_ENTRIES(double, f64)
AMG_SELLC_ENTRIES(float, f32)
#undef AMG_SELLC_ENTRIES

// Which image an operator gets (amg_sell_compact_pays, amg_common.h), for the
// Python builder.
extern "C" int amg_sell_compact_rule(int64_t slots, int64_t nnz, int64_t nmask,
                                     int64_t nslice, int vbytes) {
    return amg_sell_compact_pays(slots, nnz, nmask, nslice, vbytes) ? 1 : 0;
}

// ---------------------------------------------------------------------------
// Exact sparse triangular solve (level-scheduled), for ILU0 smoothing.
//
// The reference's exact GPU ILU0 uses the vendor SpSV machinery
// (amgcl/relaxation/rocsparse_ilu0.hpp:225-300, hipsparseSpSV).  Here the
// level schedule (rows grouped by dependency depth, computed on the host by
// _core.tri_levels) is executed by ONE cooperative kernel that loops over
// levels with a grid-wide sync between them — no per-level launch storm
// (a 512^3 ILU0 has ~1500 levels) and no vendor analysis object.
// In-place on z: lower solve uses the strictly-lower unit-diagonal factor,
// upper solve the strictly-upper factor with the inverted diagonal.
// ---------------------------------------------------------------------------
#include <hip/hip_cooperative_groups.h>

template <typename T, bool LOWER>
__global__ void sptrsv_levels_k(int64_t nlev, const int *__restrict__ lptr,
                                const int *__restrict__ rows,
                                const int *__restrict__ mp,
                                const int *__restrict__ mc,
                                const T *__restrict__ mv,
                                const T *__restrict__ dinv, T *__restrict__ z) {
    cooperative_groups::grid_group grid = cooperative_groups::this_grid();
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
    for (int64_t lev = 0; lev < nlev; ++lev) {
        for (int64_t r = lptr[lev] + tid; r < lptr[lev + 1]; r += nthreads) {
            int row = rows[r];
            double s = (double)z[row];
            for (int j = mp[row]; j < mp[row + 1]; ++j)
                s -= (double)mv[j] * (double)z[mc[j]];
            z[row] = LOWER ? (T)s : (T)((double)dinv[row] * s);
        }
        grid.sync();
    }
}

template <typename T, bool LOWER>
static int launch_sptrsv(int64_t nlev, const int *lptr, const int *rows,
                         const int *mp, const int *mc, const T *mv,
                         const T *dinv, T *z, hipStream_t stream) {
    static int grid_blocks = 0;
    const int block = 256;
    if (!grid_blocks) {
        int per_cu = 0, ncu = 0;
        hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(
            &per_cu, (const void *)sptrsv_levels_k<T, LOWER>, block, 0);
        if (e != hipSuccess) return (int)e;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, 0) != hipSuccess) return -1;
        ncu = prop.multiProcessorCount;
        grid_blocks = per_cu * ncu;
        if (grid_blocks < 1) grid_blocks = 1;
        if (grid_blocks > 2048) grid_blocks = 2048;
    }
    void *args[] = {&nlev, (void *)&lptr, (void *)&rows, (void *)&mp,
                    (void *)&mc, (void *)&mv, (void *)&dinv, (void *)&z};
    return (int)hipLaunchCooperativeKernel((const void *)sptrsv_levels_k<T, LOWER>,
                                           dim3(grid_blocks), dim3(block), args, 0,
                                           stream);
}

extern "C" int amg_sptrsv_f64(int64_t nlev, const int *lptr, const int *rows,
                              const int *mp, const int *mc, const double *mv,
                              const double *dinv, double *z, int lower,
                              hipStream_t stream) {
    return lower ? launch_sptrsv<double, true>(nlev, lptr, rows, mp, mc, mv, dinv, z,
                                               stream)
                 : launch_sptrsv<double, false>(nlev, lptr, rows, mp, mc, mv, dinv, z,
                                                stream);
}

extern "C" int amg_coop_supported() {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeCooperativeLaunch, 0) !=
        hipSuccess)
        return 0;
    return v;
}

// ---------------------------------------------------------------------------
// Vector primitives (memory-bound, grid-stride; guide App. B elementwise)
// ---------------------------------------------------------------------------
template <typename T>
__global__ void axpby_k(int64_t n, double a, const T *__restrict__ x, double b,
                        T *__restrict__ y) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    if (b == 0.0)
        for (; i < n; i += stride) y[i] = (T)(a * (double)x[i]);
    else
        for (; i < n; i += stride) y[i] = (T)(a * (double)x[i] + b * (double)y[i]);
}

template <typename T>
__global__ void axpbypcz_k(int64_t n, double a, const T *__restrict__ x, double b,
                           const T *__restrict__ y, double c, T *__restrict__ z) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    if (c == 0.0)
        for (; i < n; i += stride) z[i] = (T)(a * (double)x[i] + b * (double)y[i]);
    else
        for (; i < n; i += stride) z[i] = (T)(a * (double)x[i] + b * (double)y[i] + c * (double)z[i]);
}

// z = a*(m∘x) + b*z
template <typename T>
__global__ void vmul_k(int64_t n, double a, const T *__restrict__ m,
                       const T *__restrict__ x, double b, T *__restrict__ z) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    if (b == 0.0)
        for (; i < n; i += stride) z[i] = (T)(a * (double)m[i] * (double)x[i]);
    else
        for (; i < n; i += stride) z[i] = (T)(a * (double)m[i] * (double)x[i] + b * (double)z[i]);
}

template <typename T>
__global__ void fill_k(int64_t n, double v, T *__restrict__ x) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) x[i] = (T)v;
}

template <typename T>
static int launch_axpby(int64_t n, double a, const T *x, double b, T *y,
                        hipStream_t stream) {
    axpby_k<T><<<amg_nblocks(n), 256, 0, stream>>>(n, a, x, b, y);
    return (int)hipGetLastError();
}

template <typename T>
static int launch_axpbypcz(int64_t n, double a, const T *x, double b, const T *y,
                           double c, T *z, hipStream_t stream) {
    axpbypcz_k<T><<<amg_nblocks(n), 256, 0, stream>>>(n, a, x, b, y, c, z);
    return (int)hipGetLastError();
}

template <typename T>
static int launch_vmul(int64_t n, double a, const T *m, const T *x, double b, T *z,
                       hipStream_t stream) {
    vmul_k<T><<<amg_nblocks(n), 256, 0, stream>>>(n, a, m, x, b, z);
    return (int)hipGetLastError();
}

template <typename T>
static int launch_fill(int64_t n, double v, T *x, hipStream_t stream) {
    fill_k<T><<<amg_nblocks(n), 256, 0, stream>>>(n, v, x);
    return (int)hipGetLastError();
}

extern "C" int amg_axpby_f64(int64_t n, double a, const double *x, double b, double *y,
                             hipStream_t stream) {
    return launch_axpby(n, a, x, b, y, stream);
}
extern "C" int amg_axpby_f32(int64_t n, double a, const float *x, double b, float *y,
                             hipStream_t stream) {
    return launch_axpby(n, a, x, b, y, stream);
}

extern "C" int amg_axpbypcz_f64(int64_t n, double a, const double *x, double b,
                                const double *y, double c, double *z, hipStream_t stream) {
    return launch_axpbypcz(n, a, x, b, y, c, z, stream);
}
extern "C" int amg_axpbypcz_f32(int64_t n, double a, const float *x, double b,
                                const float *y, double c, float *z, hipStream_t stream) {
    return launch_axpbypcz(n, a, x, b, y, c, z, stream);
}

extern "C" int amg_vmul_f64(int64_t n, double a, const double *m, const double *x,
                            double b, double *z, hipStream_t stream) {
    return launch_vmul(n, a, m, x, b, z, stream);
}
extern "C" int amg_vmul_f32(int64_t n, double a, const float *m, const float *x, double b,
                            float *z, hipStream_t stream) {
    return launch_vmul(n, a, m, x, b, z, stream);
}

extern "C" int amg_fill_f64(int64_t n, double v, double *x, hipStream_t stream) {
    return launch_fill(n, v, x, stream);
}
extern "C" int amg_fill_f32(int64_t n, double v, float *x, hipStream_t stream) {
    return launch_fill(n, v, x, stream);
}

// ---------------------------------------------------------------------------
// Reductions. Per-thread grid-stride accumulate -> wave shfl reduce -> one
// atomicAdd per wave (fp64 global atomics are device-scope on CDNA4,
// guide §6 G12). Host zeroes `out` (cheap fill kernel) before the launch.
// amg_dot2 fuses two inner products into one pass (batch the
// CG dots into one reduction).
// ---------------------------------------------------------------------------
template <typename T>
__global__ void dot_k(int64_t n, const T *__restrict__ x, const T *__restrict__ y,
                      double *__restrict__ out) {
    __shared__ double lds[4];  // 256 threads = 4 waves
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    double s = 0.0;
    for (; i < n; i += stride) s += (double)x[i] * (double)y[i];
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) s += __shfl_down(s, off, WAVE);
    int wid = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
    if (lane == 0) lds[wid] = s;
    __syncthreads();
    if (threadIdx.x == 0)
        atomicAdd(out, lds[0] + lds[1] + lds[2] + lds[3]);
}

template <typename T>
__global__ void dot2_k(int64_t n, const T *__restrict__ x1, const T *__restrict__ y1,
                       const T *__restrict__ x2, const T *__restrict__ y2,
                       double *__restrict__ out) {
    __shared__ double lds[8];
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    double s1 = 0.0, s2 = 0.0;
    for (; i < n; i += stride) {
        s1 += (double)x1[i] * (double)y1[i];
        s2 += (double)x2[i] * (double)y2[i];
    }
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        s1 += __shfl_down(s1, off, WAVE);
        s2 += __shfl_down(s2, off, WAVE);
    }
    int wid = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
    if (lane == 0) {
        lds[wid] = s1;
        lds[wid + 4] = s2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(out, lds[0] + lds[1] + lds[2] + lds[3]);
        atomicAdd(out + 1, lds[4] + lds[5] + lds[6] + lds[7]);
    }
}

template <typename T>
static int launch_dot(int64_t n, const T *x, const T *y, double *out, hipStream_t stream) {
    fill_k<double><<<1, 64, 0, stream>>>(1, 0.0, out);
    dot_k<T><<<amg_nblocks(n, 256, 2048), 256, 0, stream>>>(n, x, y, out);
    return (int)hipGetLastError();
}

extern "C" int amg_dot_f64(int64_t n, const double *x, const double *y, double *out,
                           hipStream_t stream) {
    return launch_dot(n, x, y, out, stream);
}
extern "C" int amg_dot_f32(int64_t n, const float *x, const float *y, double *out,
                           hipStream_t stream) {
    return launch_dot(n, x, y, out, stream);
}

extern "C" int amg_dot2_f64(int64_t n, const double *x1, const double *y1,
                            const double *x2, const double *y2, double *out,
                            hipStream_t stream) {
    fill_k<double><<<1, 64, 0, stream>>>(2, 0.0, out);
    dot2_k<double><<<amg_nblocks(n, 256, 2048), 256, 0, stream>>>(n, x1, y1, x2, y2, out);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------
// gather/scatter by index list — halo pack/unpack for the distributed layer
// (reference: thrust::gather/scatter, backend/hip.hpp:418-446)
// ---------------------------------------------------------------------------
template <typename T>
__global__ void gather_k(int64_t n, const T *__restrict__ x,
                         const int *__restrict__ idx, T *__restrict__ buf) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) buf[i] = x[idx[i]];
}

template <typename T>
__global__ void scatter_k(int64_t n, const T *__restrict__ buf,
                          const int *__restrict__ idx, T *__restrict__ x) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) x[idx[i]] = buf[i];
}

template <typename T>
static int launch_gather(int64_t n, const T *x, const int *idx, T *buf,
                         hipStream_t stream) {
    gather_k<T><<<amg_nblocks(n), 256, 0, stream>>>(n, x, idx, buf);
    return (int)hipGetLastError();
}

template <typename T>
static int launch_scatter(int64_t n, const T *buf, const int *idx, T *x,
                          hipStream_t stream) {
    scatter_k<T><<<amg_nblocks(n), 256, 0, stream>>>(n, buf, idx, x);
    return (int)hipGetLastError();
}

extern "C" int amg_gather_f64(int64_t n, const double *x, const int *idx, double *buf,
                              hipStream_t stream) {
    return launch_gather(n, x, idx, buf, stream);
}
extern "C" int amg_gather_f32(int64_t n, const float *x, const int *idx, float *buf,
                              hipStream_t stream) {
    return launch_gather(n, x, idx, buf, stream);
}

extern "C" int amg_scatter_f64(int64_t n, const double *buf, const int *idx, double *x,
                               hipStream_t stream) {
    return launch_scatter(n, buf, idx, x, stream);
}
extern "C" int amg_scatter_f32(int64_t n, const float *buf, const int *idx, float *x,
                               hipStream_t stream) {
    return launch_scatter(n, buf, idx, x, stream);
}

// ---------------------------------------------------------------------------
// Dense GEMV for the device-resident coarse solve: u = Ainv * f.
// Ainv is ncoarse x ncoarse row-major fp64 (<= ~3000). One wave per row,
// coalesced row reads, shfl reduce. Memory-bound on Ainv (~72 MB at 3000).
// ---------------------------------------------------------------------------
template <typename T>
__global__ void gemv_k(int n, const T *__restrict__ a, const T *__restrict__ f,
                       T *__restrict__ u) {
    int64_t wid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    int lane = threadIdx.x & (WAVE - 1);
    int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / WAVE;
    for (int64_t row = wid; row < n; row += nwaves) {
        const T *arow = a + row * n;
        double s = 0.0;
        for (int j = lane; j < n; j += WAVE) s += (double)arow[j] * (double)f[j];
#pragma unroll
        for (int off = WAVE / 2; off > 0; off >>= 1) s += __shfl_down(s, off, WAVE);
        if (lane == 0) u[row] = (T)s;
    }
}

template <typename T>
static int launch_gemv(int64_t n, const T *a, const T *f, T *u, hipStream_t stream) {
    gemv_k<T><<<amg_nblocks(n * WAVE), 256, 0, stream>>>((int)n, a, f, u);
    return (int)hipGetLastError();
}

extern "C" int amg_gemv_f64(int64_t n, const double *a, const double *f, double *u,
                            hipStream_t stream) {
    return launch_gemv(n, a, f, u, stream);
}
extern "C" int amg_gemv_f32(int64_t n, const float *a, const float *f, float *u,
                            hipStream_t stream) {
    return launch_gemv(n, a, f, u, stream);
}

// precision casts (mixed-precision boundary)
__global__ void cast_d2s_k(int64_t n, const double *__restrict__ src, float *__restrict__ dst) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) dst[i] = (float)src[i];
}
__global__ void cast_s2d_k(int64_t n, const float *__restrict__ src, double *__restrict__ dst) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) dst[i] = (double)src[i];
}
extern "C" int amg_cast_d2s(int64_t n, const double *src, float *dst, hipStream_t s) {
    cast_d2s_k<<<amg_nblocks(n), 256, 0, s>>>(n, src, dst);
    return (int)hipGetLastError();
}
extern "C" int amg_cast_s2d(int64_t n, const float *src, double *dst, hipStream_t s) {
    cast_s2d_k<<<amg_nblocks(n), 256, 0, s>>>(n, src, dst);
    return (int)hipGetLastError();
}


// ---------------------------------------------------------------------------
// Multicolor Gauss-Seidel sweep: rows listed in `rows` share a color
// (mutually independent), so the in-place update is race-free.
// x[i] = (b[i] - sum_{j != i} a_ij x_j) / a_ii
// ---------------------------------------------------------------------------
__global__ void gs_color_k(int64_t nlist, const int *__restrict__ rows,
                           const int *__restrict__ ptr, const int *__restrict__ col,
                           const double *__restrict__ val, const double *__restrict__ b,
                           double *__restrict__ x) {
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; t < nlist; t += stride) {
        int i = rows[t];
        double s = b[i], d = 1.0;
        for (int j = ptr[i]; j < ptr[i + 1]; ++j) {
            int c = col[j];
            double v = val[j];
            if (c == i) d = v;
            else s -= v * x[c];
        }
        x[i] = s / d;
    }
}

extern "C" int amg_gs_color_f64(int64_t nlist, const int *rows, const int *ptr,
                                const int *col, const double *val, const double *b,
                                double *x, hipStream_t stream) {
    gs_color_k<<<amg_nblocks(nlist), 256, 0, stream>>>(nlist, rows, ptr, col, val, b, x);
    return (int)hipGetLastError();
}


// ---------------------------------------------------------------------------
// Fused CG tail: x += alpha p ; r -= alpha q ; out[0] += ||r_new||^2
// (saves one full pass over r and a separate reduction per iteration)
// ---------------------------------------------------------------------------
__global__ void cg_tail_k(int64_t n, double alpha, const double *__restrict__ p,
                          const double *__restrict__ q, double *__restrict__ x,
                          double *__restrict__ r, double *__restrict__ out) {
    __shared__ double lds[4];
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    double s = 0.0;
    for (; i < n; i += stride) {
        x[i] += alpha * p[i];
        double rn = r[i] - alpha * q[i];
        r[i] = rn;
        s += rn * rn;
    }
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) s += __shfl_down(s, off, WAVE);
    int wid = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
    if (lane == 0) lds[wid] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out, lds[0] + lds[1] + lds[2] + lds[3]);
}

extern "C" int amg_cg_tail_f64(int64_t n, double alpha, const double *p, const double *q,
                               double *x, double *r, double *out, hipStream_t stream) {
    fill_k<double><<<1, 64, 0, stream>>>(1, 0.0, out);
    cg_tail_k<<<amg_nblocks(n, 256, 2048), 256, 0, stream>>>(n, alpha, p, q, x, r, out);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------
// complex128 solve kernels (parity: amgcl/value_type/complex.hpp — the
// reference instantiates its backends over std::complex; here the HIP
// backend gets hand-written double2 kernels; setup stays on the host's
// complex engine and levels move per level, the reference's own layout).
// Scalars (alpha/beta) arrive as (re, im) double pairs; inner products are
// adjoint (conj on the first argument), accumulated per-part via fp64
// device atomics.
// ---------------------------------------------------------------------------
struct c128 {
    double re, im;
};
__device__ static inline c128 cmul(c128 a, c128 b) {
    return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}
__device__ static inline c128 cmulc(c128 a, c128 b) {  // conj(a) * b
    return {a.re * b.re + a.im * b.im, a.re * b.im - a.im * b.re};
}
__device__ static inline c128 cadd(c128 a, c128 b) { return {a.re + b.re, a.im + b.im}; }
__device__ static inline c128 csub(c128 a, c128 b) { return {a.re - b.re, a.im - b.im}; }

template <int SUBW, int MODE>  // 0: y=aAx+by  1: r=rhs-Ax  2: t=M(rhs-Ax)
__global__ void cspmv_k(int64_t nrows, const int *__restrict__ ptr,
                        const int *__restrict__ col, const c128 *__restrict__ val,
                        const c128 *__restrict__ x, c128 alpha, c128 beta,
                        const c128 *__restrict__ rhs, const c128 *__restrict__ M,
                        c128 *__restrict__ y) {
    int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int lane = (int)(tid & (SUBW - 1));
    int64_t row = tid / SUBW;
    int64_t stride = ((int64_t)gridDim.x * blockDim.x) / SUBW;
    for (; row < nrows; row += stride) {
        c128 s = {0.0, 0.0};
        int b = ptr[row], e = ptr[row + 1];
        for (int j = b + lane; j < e; j += SUBW) s = cadd(s, cmul(val[j], x[col[j]]));
#pragma unroll
        for (int off = SUBW / 2; off > 0; off >>= 1) {
            s.re += __shfl_down(s.re, off, SUBW);
            s.im += __shfl_down(s.im, off, SUBW);
        }
        if (lane == 0) {
            if (MODE == 0) {
                c128 out = cmul(alpha, s);
                if (beta.re != 0.0 || beta.im != 0.0)
                    out = cadd(out, cmul(beta, y[row]));
                y[row] = out;
            } else if (MODE == 1) {
                y[row] = csub(rhs[row], s);
            } else {
                y[row] = cmul(M[row], csub(rhs[row], s));
            }
        }
    }
}

template <int MODE>
static int cspmv_dispatch(int64_t nrows, int64_t nnz, const int *ptr, const int *col,
                          const void *val, const void *x, c128 a, c128 b,
                          const void *rhs, const void *M, void *y, int subw,
                          hipStream_t stream) {
    return by_subw(subw, nrows, nnz, [&](auto sw) {
        constexpr int SW = decltype(sw)::value;
        cspmv_k<SW, MODE><<<amg_nblocks(nrows * SW), 256, 0, stream>>>(
            nrows, ptr, col, (const c128 *)val, (const c128 *)x, a, b, (const c128 *)rhs,
            (const c128 *)M, (c128 *)y);
    });
}

extern "C" int amg_spmv_c128(int64_t nrows, int64_t nnz, const int *ptr, const int *col,
                             const void *val, const void *x, double ar, double ai,
                             double br, double bi, void *y, int subw,
                             hipStream_t stream) {
    return cspmv_dispatch<0>(nrows, nnz, ptr, col, val, x, {ar, ai}, {br, bi}, nullptr,
                             nullptr, y, subw, stream);
}
extern "C" int amg_residual_c128(int64_t nrows, int64_t nnz, const int *ptr,
                                 const int *col, const void *val, const void *rhs,
                                 const void *x, void *r, int subw, hipStream_t stream) {
    return cspmv_dispatch<1>(nrows, nnz, ptr, col, val, x, {0, 0}, {0, 0}, rhs, nullptr,
                             r, subw, stream);
}
extern "C" int amg_relax_diag_c128(int64_t nrows, int64_t nnz, const int *ptr,
                                   const int *col, const void *val, const void *M,
                                   const void *rhs, const void *x, void *t, int subw,
                                   hipStream_t stream) {
    return cspmv_dispatch<2>(nrows, nnz, ptr, col, val, x, {0, 0}, {0, 0}, rhs, M, t,
                             subw, stream);
}

template <int MODE>  // 0: y=ax+by  1: z=ax+by+cz  2: z=a(m.x)+bz
__global__ void cvec_k(int64_t n, c128 a, const c128 *__restrict__ x, c128 b,
                       const c128 *__restrict__ yv, c128 c, const c128 *__restrict__ m,
                       c128 *__restrict__ z) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        if (MODE == 0) {
            c128 out = cmul(a, x[i]);
            if (b.re != 0.0 || b.im != 0.0) out = cadd(out, cmul(b, z[i]));
            z[i] = out;
        } else if (MODE == 1) {
            c128 out = cadd(cmul(a, x[i]), cmul(b, yv[i]));
            if (c.re != 0.0 || c.im != 0.0) out = cadd(out, cmul(c, z[i]));
            z[i] = out;
        } else {
            c128 out = cmul(a, cmul(m[i], x[i]));
            if (b.re != 0.0 || b.im != 0.0) out = cadd(out, cmul(b, z[i]));
            z[i] = out;
        }
    }
}

extern "C" int amg_axpby_c128(int64_t n, double ar, double ai, const void *x,
                              double br, double bi, void *y, hipStream_t stream) {
    cvec_k<0><<<amg_nblocks(n), 256, 0, stream>>>(n, {ar, ai}, (const c128 *)x, {br, bi},
                                              nullptr, {0, 0}, nullptr, (c128 *)y);
    return (int)hipGetLastError();
}
extern "C" int amg_axpbypcz_c128(int64_t n, double ar, double ai, const void *x,
                                 double br, double bi, const void *y, double cr,
                                 double ci, void *z, hipStream_t stream) {
    cvec_k<1><<<amg_nblocks(n), 256, 0, stream>>>(n, {ar, ai}, (const c128 *)x, {br, bi},
                                              (const c128 *)y, {cr, ci}, nullptr,
                                              (c128 *)z);
    return (int)hipGetLastError();
}
extern "C" int amg_vmul_c128(int64_t n, double ar, double ai, const void *m,
                             const void *x, double br, double bi, void *z,
                             hipStream_t stream) {
    cvec_k<2><<<amg_nblocks(n), 256, 0, stream>>>(n, {ar, ai}, (const c128 *)x, {br, bi},
                                              nullptr, {0, 0}, (const c128 *)m,
                                              (c128 *)z);
    return (int)hipGetLastError();
}

// adjoint inner product: out[0:2] += sum conj(x)*y (host zeroes out first)
__global__ void cdot_k(int64_t n, const c128 *__restrict__ x,
                       const c128 *__restrict__ y, double *__restrict__ out) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    c128 s = {0.0, 0.0};
    for (; i < n; i += stride) s = cadd(s, cmulc(x[i], y[i]));
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        s.re += __shfl_down(s.re, off, WAVE);
        s.im += __shfl_down(s.im, off, WAVE);
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        atomicAdd(&out[0], s.re);
        atomicAdd(&out[1], s.im);
    }
}

extern "C" int amg_dot_c128(int64_t n, const void *x, const void *y, double *out,
                            hipStream_t stream) {
    cdot_k<<<amg_nblocks(n, 256, 2048), 256, 0, stream>>>(n, (const c128 *)x,
                                                      (const c128 *)y, out);
    return (int)hipGetLastError();
}

// y = Inv * f (dense row-major n x n, complex)
__global__ void cgemv_k(int64_t n, const c128 *__restrict__ inv,
                        const c128 *__restrict__ f, c128 *__restrict__ y) {
    int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    int lane = threadIdx.x & (WAVE - 1);
    int64_t stride = ((int64_t)gridDim.x * blockDim.x) / WAVE;
    for (; row < n; row += stride) {
        c128 s = {0.0, 0.0};
        const c128 *r = inv + row * n;
        for (int64_t j = lane; j < n; j += WAVE) s = cadd(s, cmul(r[j], f[j]));
#pragma unroll
        for (int off = WAVE / 2; off > 0; off >>= 1) {
            s.re += __shfl_down(s.re, off, WAVE);
            s.im += __shfl_down(s.im, off, WAVE);
        }
        if (lane == 0) y[row] = s;
    }
}

extern "C" int amg_gemv_c128(int64_t n, const void *inv, const void *f, void *y,
                             hipStream_t stream) {
    cgemv_k<<<amg_nblocks(n * WAVE), 256, 0, stream>>>(n, (const c128 *)inv,
                                                   (const c128 *)f, (c128 *)y);
    return (int)hipGetLastError();
}

__global__ void cfill_k(int64_t n, c128 v, c128 *__restrict__ x) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) x[i] = v;
}

extern "C" int amg_fill_c128(int64_t n, double vr, double vi, void *x,
                             hipStream_t stream) {
    cfill_k<<<amg_nblocks(n), 256, 0, stream>>>(n, {vr, vi}, (c128 *)x);
    return (int)hipGetLastError();
}
