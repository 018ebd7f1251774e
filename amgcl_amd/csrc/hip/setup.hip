// amgcl_amd — device-side AMG setup engine (gfx950).
//
// The reference always assembles the AMG hierarchy on the host
// (docs/design.rst:20-38) and pays a full H2D transfer per level
// (amgcl/backend/hip.hpp:382-409). On MI355X the host is the bottleneck
// (GPU-box containers are CPU-quota'd), so this file implements the whole
// smoothed-aggregation setup on the GPU:
//   - diagonal + strong-connection mask   (plain_aggregates.hpp:136 semantics)
//   - parallel MIS(2) aggregation with provisional 2nd-ring claiming
//     (identical algorithm to the host engine in csrc/core/core.cpp, which
//     mirrors the reference's distributed pmis; deterministic hash keys)
//   - smoothed prolongation P             (smoothed_aggregation.hpp:157-232)
//   - CSR transpose (R = P^T)
//   - SpGEMM with per-wave LDS hash accumulators (Galerkin triple product,
//     coarsening/detail/galerkin.hpp:42)
//   - SPAI-0 / damped-Jacobi smoother weights on device
//   - SPAI-1 approximate inverse (per-row normal equations + Cholesky)
//   - inclusive i32 scan
//
// All kernels are deterministic except SpGEMM value accumulation order
// (LDS atomicAdd), which is a reduction-order nondeterminism identical in
// kind to the reference's OpenMP inner products.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "amg_kernels.h"

#define WAVE 64

static inline int nblk(int64_t work, int block = 256, int cap = 4096) {
    int64_t b = (work + block - 1) / block;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

// Bitonic sort of an LDS (key,val) table with LANES cooperating threads.
// Empty slots must hold key = INT_MAX (sorted to the tail). SLOTS power of 2.
template <int LANES, int SLOTS>
__device__ __forceinline__ void lds_bitonic(int *k, double *v, int lane) {
    for (int size = 2; size <= SLOTS; size <<= 1) {
        for (int strd = size >> 1; strd > 0; strd >>= 1) {
            __builtin_amdgcn_s_waitcnt(0);
            __builtin_amdgcn_wave_barrier();
            for (int t = lane; t < SLOTS / 2; t += LANES) {
                int i = ((t / strd) * strd * 2) + (t % strd);
                int j = i + strd;
                bool up = ((i & size) == 0);
                int ki = k[i], kj = k[j];
                if ((ki > kj) == up) {
                    k[i] = kj;
                    k[j] = ki;
                    double tv = v[i];
                    v[i] = v[j];
                    v[j] = tv;
                }
            }
        }
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ uint64_t agg_key_d(int i) {
    uint32_t x = (uint32_t)i;
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return ((uint64_t)x << 32) | (uint32_t)i;
}

// ---------------------------------------------------------------------------
// diagonal + strong mask + smoother weights
// ---------------------------------------------------------------------------
// One-pass-over-A setup kernels use 4 lanes per row (coalesced col/val
// loads, like the solve-phase spmv/residual kernels): the thread-per-row
// version measured only ~450 GB/s on 512^3 where subwarp rows reach multi-TB/s.
#define SETUP_SW 4

__global__ void diag_k(int64_t n, const int *__restrict__ ptr, const int *__restrict__ col,
                       const double *__restrict__ val, double *__restrict__ d) {
    int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int lane = (int)(tid & (SETUP_SW - 1));
    int64_t i = tid / SETUP_SW;
    int64_t stride = ((int64_t)gridDim.x * blockDim.x) / SETUP_SW;
    for (; i < n; i += stride) {
        double v = 0.0;
        for (int j = ptr[i] + lane; j < ptr[i + 1]; j += SETUP_SW)
            if (col[j] == (int)i) v = val[j];
#pragma unroll
        for (int off = SETUP_SW / 2; off > 0; off >>= 1)
            v += __shfl_down(v, off, SETUP_SW);
        if (lane == 0) d[i] = v;
    }
}

__global__ void strong_k(int64_t n, const int *__restrict__ ptr, const int *__restrict__ col,
                         const double *__restrict__ val, const double *__restrict__ d,
                         double eps2, uint8_t *__restrict__ S) {
    int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int lane = (int)(tid & (SETUP_SW - 1));
    int64_t i = tid / SETUP_SW;
    int64_t stride = ((int64_t)gridDim.x * blockDim.x) / SETUP_SW;
    for (; i < n; i += stride) {
        double edi = eps2 * d[i];
        for (int j = ptr[i] + lane; j < ptr[i + 1]; j += SETUP_SW) {
            int c = col[j];
            double v = val[j];
            S[j] = (c != (int)i) && (edi * d[c] < v * v);
        }
    }
}

__global__ void spai0_k(int64_t n, const int *__restrict__ ptr, const int *__restrict__ col,
                        const double *__restrict__ val, double *__restrict__ m) {
    int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int lane = (int)(tid & (SETUP_SW - 1));
    int64_t i = tid / SETUP_SW;
    int64_t stride = ((int64_t)gridDim.x * blockDim.x) / SETUP_SW;
    for (; i < n; i += stride) {
        double num = 0.0, den = 0.0;
        for (int j = ptr[i] + lane; j < ptr[i + 1]; j += SETUP_SW) {
            double v = val[j];
            den += v * v;
            if (col[j] == (int)i) num = v;
        }
#pragma unroll
        for (int off = SETUP_SW / 2; off > 0; off >>= 1) {
            den += __shfl_down(den, off, SETUP_SW);
            num += __shfl_down(num, off, SETUP_SW);
        }
        if (lane == 0) m[i] = den > 0.0 ? num / den : 0.0;
    }
}

extern "C" int amg_setup_diag(int64_t n, const int *ptr, const int *col, const double *val,
                              double *d, hipStream_t s) {
    diag_k<<<nblk(n * SETUP_SW), 256, 0, s>>>(n, ptr, col, val, d);
    return (int)hipGetLastError();
}
extern "C" int amg_setup_strong(int64_t n, const int *ptr, const int *col, const double *val,
                                const double *d, double eps2, uint8_t *S, hipStream_t s) {
    strong_k<<<nblk(n * SETUP_SW), 256, 0, s>>>(n, ptr, col, val, d, eps2, S);
    return (int)hipGetLastError();
}
extern "C" int amg_setup_spai0(int64_t n, const int *ptr, const int *col, const double *val,
                               double *m, hipStream_t s) {
    spai0_k<<<nblk(n * SETUP_SW), 256, 0, s>>>(n, ptr, col, val, m);
    return (int)hipGetLastError();
}

// Gershgorin spectral-radius bound: max_i sum_j |a_ij| (optionally scaled by
// 1/|a_ii|), for the Chebyshev smoother (amgcl/backend/builtin.hpp:781).
__global__ void gersh_k(int64_t n, const int *__restrict__ ptr, const int *__restrict__ col,
                        const double *__restrict__ val, int scale, double *__restrict__ out) {
    __shared__ double lds[4];
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    double m = 0.0;
    for (; i < n; i += stride) {
        double s = 0.0, dia = 1.0;
        for (int j = ptr[i]; j < ptr[i + 1]; ++j) {
            s += fabs(val[j]);
            if (col[j] == (int)i) dia = fabs(val[j]);
        }
        if (scale && dia > 0.0) s /= dia;
        if (s > m) m = s;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        double o = __shfl_down(m, off, 64);
        if (o > m) m = o;
    }
    int wid = threadIdx.x / 64, lane = threadIdx.x & 63;
    if (lane == 0) lds[wid] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        double bm = fmax(fmax(lds[0], lds[1]), fmax(lds[2], lds[3]));
        // device-scope atomic max on double via CAS
        unsigned long long *o = (unsigned long long *)out;
        unsigned long long cur = *o;
        while (__longlong_as_double((long long)cur) < bm) {
            unsigned long long next = (unsigned long long)__double_as_longlong(bm);
            unsigned long long old = atomicCAS(o, cur, next);
            if (old == cur) break;
            cur = old;
        }
    }
}

extern "C" int amg_gershgorin(int64_t n, const int *ptr, const int *col, const double *val,
                              int scale, double *out, hipStream_t s) {
    hipMemsetAsync(out, 0, sizeof(double), s);
    gersh_k<<<nblk(n, 256, 1024), 256, 0, s>>>(n, ptr, col, val, scale, out);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------
// SPAI-1 smoother setup (amgcl/relaxation/spai1.hpp:82-120)
// ---------------------------------------------------------------------------
// M has A's pattern, so only its values are produced.  With I = {c_0 < ... <
// c_{k-1}} the pattern of row i, row i of M minimises ||e_i^T - m^T A(I,:)||
// over the ROWS of A in I (the reference's QR problem).  Its normal equations
//   G m = rhs,   G[a][b] = <A(c_a,:), A(c_b,:)>,   rhs[a] = A(c_a, i)
// need only CSR rows of A (no transpose) and are solved by Cholesky.  Rows of
// A must have sorted columns: the sparse dots are two-pointer merges and rhs
// is a binary search.
//
// Two tiers by row length k: up to SPAI1_SHORT one wave per row with G in
// LDS; longer rows come through a worklist, one block per row with G in a
// global workspace slot.
//
// A pivot <= k * 2^-52 * G[c][c] (G's original diagonal entry) cannot be told
// from zero, since that is the bound on the rounding error of the computed
// pivot; such a row reports row+1 through atomicMax on *flag and its output
// is unspecified.
//
// The pivot test is only as sharp as sqrt and division are.  The library is
// built with -ffast-math, under which gfx950's f64 division is a Newton-
// refined reciprocal with one residual correction and f64 sqrt keeps its full
// refinement: both stay within an ulp, which the bound above allows for.

#define SPAI1_SHORT 32                // longest row of the wave-per-row tier
#define SPAI1_LD (SPAI1_SHORT + 1)    // LDS leading dimension, padded: lanes a
                                      // reading G[a][j] fall on banks 2(a+j) % 64
#define SPAI1_WPB 4                   // waves (rows in flight) per block
#define SPAI1_EPS 2.220446049250313e-16  // 2^-52

// Orders one wave's LDS traffic: the LDS serves a wave's accesses in issue
// order, so what is left to prevent is the compiler moving them.
__device__ __forceinline__ void spai1_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// <A(r,:), A(s,:)> for the rows stored at [i, ie) and [j, je)
__device__ __forceinline__ double spai1_row_dot(const int *__restrict__ col,
                                                const double *__restrict__ val, int i,
                                                int ie, int j, int je) {
    double s = 0.0;
    if (i == j) {
        for (; i < ie; ++i) s += val[i] * val[i];
        return s;
    }
    while (i < ie && j < je) {
        int ci = col[i], cj = col[j];
        if (ci == cj) s += val[i] * val[j];
        i += (ci <= cj);
        j += (cj <= ci);
    }
    return s;
}

// A(r, c) for the row stored at [lo, hi), 0 if absent
__device__ __forceinline__ double spai1_entry(const int *__restrict__ col,
                                              const double *__restrict__ val, int lo,
                                              int hi, int c) {
    const int end = hi;
    while (lo < hi) {
        int mid = lo + ((hi - lo) >> 1);
        if (col[mid] < c) lo = mid + 1; else hi = mid;
    }
    return (lo < end && col[lo] == c) ? val[lo] : 0.0;
}

// p in [0, k(k+1)/2) -> (a <= b) with p = b(b+1)/2 + a
__device__ __forceinline__ void spai1_pair(int64_t p, int *a, int *b) {
    int64_t t = (int64_t)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
    while (t * (t + 1) / 2 > p) --t;
    while ((t + 1) * (t + 2) / 2 <= p) ++t;
    *b = (int)t;
    *a = (int)(p - t * (t + 1) / 2);
}

// Short tier: rows with 1 <= k <= SPAI1_SHORT, one wave per row.
__global__ __launch_bounds__(64 * SPAI1_WPB) void spai1_short_k(
    int64_t n, const int *__restrict__ ptr, const int *__restrict__ col,
    const double *__restrict__ val, double *__restrict__ mval, int *__restrict__ flag) {
    __shared__ double Gs[SPAI1_WPB][SPAI1_SHORT * SPAI1_LD];
    __shared__ int pbs[SPAI1_WPB][SPAI1_SHORT], pes[SPAI1_WPB][SPAI1_SHORT];
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    double *G = Gs[w];
    int *pb = pbs[w], *pe = pes[w];
    const int64_t stride = (int64_t)gridDim.x * SPAI1_WPB;
    for (int64_t row = (int64_t)blockIdx.x * SPAI1_WPB + w; row < n; row += stride) {
        const int b0 = ptr[row];
        const int k = ptr[row + 1] - b0;
        if (k < 1 || k > SPAI1_SHORT) continue;  // wave-uniform
        spai1_wave_sync();                       // the previous row is done with the LDS
        // extents of the pattern's rows; lane a keeps rhs[a] (later y, then m)
        double ra = 0.0;
        if (lane < k) {
            int c = col[b0 + lane];
            int cb = ptr[c], ce = ptr[c + 1];
            pb[lane] = cb;
            pe[lane] = ce;
            ra = spai1_entry(col, val, cb, ce, (int)row);
        }
        spai1_wave_sync();
        // G: the a <= b pairs over the 64 lanes, mirrored
        const int np = k * (k + 1) / 2;
        for (int p = lane; p < np; p += WAVE) {
            int a, b;
            spai1_pair(p, &a, &b);
            double s = spai1_row_dot(col, val, pb[a], pe[a], pb[b], pe[b]);
            G[a * SPAI1_LD + b] = s;
            G[b * SPAI1_LD + a] = s;
        }
        spai1_wave_sync();
        // Cholesky G = L L^T, left-looking; lane a owns row a, L overwrites
        // the lower triangle
        const double d0 = lane < k ? G[lane * SPAI1_LD + lane] : 1.0;
        bool singular = false;
        for (int c = 0; c < k; ++c) {
            double s = 0.0;
            if (lane >= c && lane < k) {
                s = G[lane * SPAI1_LD + c];
                for (int j = 0; j < c; ++j) s -= G[lane * SPAI1_LD + j] * G[c * SPAI1_LD + j];
            }
            const double piv = __shfl(s, c, WAVE);
            const double dc = __shfl(d0, c, WAVE);
            if (piv <= (double)k * SPAI1_EPS * dc) {
                singular = true;
                break;
            }
            const double l = __builtin_sqrt(piv);
            if (lane == c) G[c * SPAI1_LD + c] = l;
            else if (lane > c && lane < k) G[lane * SPAI1_LD + c] = s / l;
            spai1_wave_sync();
        }
        if (singular) {
            if (lane == 0) atomicMax(flag, (int)row + 1);
            continue;
        }
        // L y = rhs, then L^T m = y, on the lanes' registers
        for (int c = 0; c < k; ++c) {
            const double yc = __shfl(ra, c, WAVE) / G[c * SPAI1_LD + c];
            if (lane == c) ra = yc;
            else if (lane > c && lane < k) ra -= G[lane * SPAI1_LD + c] * yc;
        }
        for (int c = k - 1; c >= 0; --c) {
            const double mc = __shfl(ra, c, WAVE) / G[c * SPAI1_LD + c];
            if (lane == c) ra = mc;
            else if (lane < c) ra -= G[c * SPAI1_LD + lane] * mc;
        }
        if (lane < k) mval[b0 + lane] = ra;
    }
}

// Long tier: worklist rows (k > SPAI1_SHORT), one block per workspace slot.
// A slot holds kmax*(kmax+2) doubles: the k x k upper factor U (G = U^T U,
// row-major, so that the threads' reads along a row of U coalesce) and the
// two solve vectors.
__global__ __launch_bounds__(256) void spai1_long_k(
    int64_t nlong, const int *__restrict__ list, const int *__restrict__ ptr,
    const int *__restrict__ col, const double *__restrict__ val,
    double *__restrict__ mval, int *__restrict__ flag, int kmax, double *work) {
    __shared__ double sh[2];  // pivot of the column at hand, G's original diagonal entry
    const int tid = threadIdx.x;
    double *U = work + (int64_t)blockIdx.x * kmax * (kmax + 2);
    double *r = U + (int64_t)kmax * kmax;
    double *y = r + kmax;
    for (int64_t w = blockIdx.x; w < nlong; w += gridDim.x) {
        const int row = list[w];
        const int b0 = ptr[row];
        const int64_t k = ptr[row + 1] - b0;
        if (k < 1 || k > kmax) {  // block-uniform; a worklist/kmax mismatch
            if (tid == 0) atomicMax(flag, row + 1);
            continue;
        }
        const int *I = col + b0;
        __syncthreads();  // the previous row is done with the slot
        for (int a = tid; a < k; a += 256) {
            int c = I[a];
            r[a] = spai1_entry(col, val, ptr[c], ptr[c + 1], row);
        }
        const int64_t np = k * (k + 1) / 2;
        for (int64_t p = tid; p < np; p += 256) {
            int a, b;
            spai1_pair(p, &a, &b);
            int ca = I[a], cb = I[b];
            U[a * k + b] = spai1_row_dot(col, val, ptr[ca], ptr[ca + 1], ptr[cb], ptr[cb + 1]);
        }
        __syncthreads();
        // column c of the factorisation fills row c of U
        bool singular = false;
        for (int64_t c = 0; c < k; ++c) {
            for (int64_t a = c + tid; a < k; a += 256) {
                double s = U[c * k + a];
                for (int64_t j = 0; j < c; ++j) s -= U[j * k + a] * U[j * k + c];
                if (a == c) {
                    sh[0] = s;
                    sh[1] = U[c * k + c];
                }
                U[c * k + a] = s;
            }
            __syncthreads();
            const double piv = sh[0], dc = sh[1];
            if (piv <= (double)k * SPAI1_EPS * dc) {  // block-uniform
                singular = true;
                break;
            }
            const double l = __builtin_sqrt(piv);
            for (int64_t a = c + tid; a < k; a += 256)
                U[c * k + a] = (a == c) ? l : U[c * k + a] / l;
            __syncthreads();
        }
        if (singular) {
            if (tid == 0) atomicMax(flag, row + 1);
            continue;
        }
        // U^T y = rhs, column by column
        for (int64_t c = 0; c < k; ++c) {
            const double yc = r[c] / U[c * k + c];
            if (tid == 0) y[c] = yc;
            for (int64_t a = c + 1 + tid; a < k; a += 256) r[a] -= U[c * k + a] * yc;
            __syncthreads();
        }
        // U m = y, column by column from the last
        for (int64_t c = k - 1; c >= 0; --c) {
            const double mc = y[c] / U[c * k + c];
            if (tid == 0) mval[b0 + c] = mc;
            for (int64_t j = tid; j < c; j += 256) y[j] -= U[j * k + c] * mc;
            __syncthreads();
        }
    }
}

extern "C" int amg_spai1_short_max(void) { return SPAI1_SHORT; }

// longrows/nlong: the rows longer than amg_spai1_short_max(); kmax: the
// longest of them; work: slots * kmax*(kmax+2) doubles.  *flag is cleared
// here and holds row+1 of a singular row afterwards (0: none).
extern "C" int amg_setup_spai1(int64_t n, const int *ptr, const int *col, const double *val,
                               double *mval, int *flag, int64_t nlong, const int *longrows,
                               int kmax, int slots, double *work, hipStream_t s) {
    hipError_t rc = hipMemsetAsync(flag, 0, sizeof(int), s);
    if (rc != hipSuccess) return (int)rc;
    if (n > 0)
        spai1_short_k<<<nblk(n, SPAI1_WPB), 64 * SPAI1_WPB, 0, s>>>(n, ptr, col, val, mval,
                                                                   flag);
    if (nlong > 0) {
        if (!longrows || !work || slots < 1 || kmax <= SPAI1_SHORT)
            return (int)hipErrorInvalidValue;
        int grid = (int)(nlong < slots ? nlong : slots);
        spai1_long_k<<<grid, 256, 0, s>>>(nlong, longrows, ptr, col, val, mval, flag, kmax,
                                          work);
    }
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------
// inclusive scan (i32), hierarchical
// ---------------------------------------------------------------------------
#define SCAN_BLOCK 1024  // threads; each block scans SCAN_BLOCK elements

__global__ void scan_block_k(int64_t n, const int *__restrict__ in, int *__restrict__ out,
                             int *__restrict__ sums) {
    __shared__ int lds[SCAN_BLOCK];
    int64_t base = (int64_t)blockIdx.x * SCAN_BLOCK;
    int t = threadIdx.x;
    lds[t] = (base + t < n) ? in[base + t] : 0;
    __syncthreads();
    // Hillis-Steele
    for (int off = 1; off < SCAN_BLOCK; off <<= 1) {
        int v = (t >= off) ? lds[t - off] : 0;
        __syncthreads();
        lds[t] += v;
        __syncthreads();
    }
    if (base + t < n) out[base + t] = lds[t];
    if (t == SCAN_BLOCK - 1 && sums) sums[blockIdx.x] = lds[t];
}

__global__ void scan_add_k(int64_t n, int *__restrict__ out, const int *__restrict__ sums) {
    int64_t base = (int64_t)blockIdx.x * SCAN_BLOCK;
    int t = threadIdx.x;
    if (blockIdx.x > 0 && base + t < n) out[base + t] += sums[blockIdx.x - 1];
}

static int scan_i32_device(int *a, int64_t n, hipStream_t s) {
    if (n <= 0) return 0;
    int64_t nblocks = (n + SCAN_BLOCK - 1) / SCAN_BLOCK;
    if (nblocks == 1) {
        scan_block_k<<<1, SCAN_BLOCK, 0, s>>>(n, a, a, nullptr);
        return (int)hipGetLastError();
    }
    int *sums = nullptr;
    int rc = (int)hipMallocAsync((void **)&sums, nblocks * sizeof(int), s);
    if (rc) return rc;
    scan_block_k<<<nblocks, SCAN_BLOCK, 0, s>>>(n, a, a, sums);
    rc = scan_i32_device(sums, nblocks, s);
    if (rc) return rc;
    scan_add_k<<<nblocks, SCAN_BLOCK, 0, s>>>(n, a, sums);
    hipFreeAsync(sums, s);
    return (int)hipGetLastError();
}

extern "C" int amg_scan_i32(int *a, int64_t n, hipStream_t s) {
    return scan_i32_device(a, n, s);
}

// ---------------------------------------------------------------------------
// aggregation rounds (device twin of core.cpp:aggregates_parallel)
// id: -1 undef, -2 removed, >=0 root-node index; prov: provisional flag
// ---------------------------------------------------------------------------
__global__ void agg_init_k(int64_t n, const int *__restrict__ ptr, const uint8_t *__restrict__ S,
                           int *__restrict__ id) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        int st = -2;
        for (int j = ptr[i]; j < ptr[i + 1]; ++j)
            if (S[j]) { st = -1; break; }
        id[i] = st;
    }
}

// m1 needs to be valid for every node within distance 1 of an UNDEF node.
// `near` marks those nodes (set during the previous round's passes or the
// init pass); everything else keeps m1 = 0 without re-reading its row.
// Frontier lists: after the first rounds, the active set (UNDEF nodes and
// their strong 1-ring) shrinks monotonically, so the round kernels iterate
// a compacted index list instead of re-scanning all n nodes (the host
// engine's sparse branch, on the device).  list == nullptr -> full range.
#define AGG_FOREACH(i)                                                              int64_t _t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;                    int64_t _stride = (int64_t)gridDim.x * blockDim.x;                              for (; _t < nwork; _t += _stride)                                                   if (int64_t i = (list ? (int64_t)list[_t] : _t); true)

__global__ void agg_clear_near_k(int64_t nwork, const int *__restrict__ list,
                                 uint8_t *__restrict__ near) {
    AGG_FOREACH(i) near[i] = 0;
}

// scan-based compaction (flag -> inclusive scan -> scatter): a single
// global counter costs ~10 ns per atomic even wave-aggregated (measured
// 21 ms for a 134M-node frontier); three stream passes cost ~2 ms.
// flags are indexed by LIST POSITION t, not node id.
__global__ void agg_flag_k(int64_t nwork, const int *__restrict__ list,
                           const uint8_t *__restrict__ near, int *__restrict__ flags) {
    AGG_FOREACH(i) flags[_t] = near[i] ? 1 : 0;
}

__global__ void agg_scatter_list_k(int64_t nwork, const int *__restrict__ list,
                                   const uint8_t *__restrict__ near,
                                   const int *__restrict__ flags_scanned,
                                   int *__restrict__ out) {
    AGG_FOREACH(i) if (near[i]) out[flags_scanned[_t] - 1] = (int)i;
}

__global__ void agg_m1_k(int64_t nwork, const int *__restrict__ list,
                         const int *__restrict__ ptr, const int *__restrict__ col,
                         const uint8_t *__restrict__ S, const int *__restrict__ id,
                         const uint8_t *__restrict__ near, uint64_t *__restrict__ m1) {
    AGG_FOREACH(i) {
        if (!near[i]) {
            m1[i] = 0;
            continue;
        }
        uint64_t m = (id[i] == -1) ? agg_key_d((int)i) : 0;
        for (int j = ptr[i]; j < ptr[i + 1]; ++j) {
            if (!S[j]) continue;
            int c = col[j];
            if (id[c] == -1) {
                uint64_t k = agg_key_d(c);
                if (k > m) m = k;
            }
        }
        m1[i] = m;
    }
}

// near[i] = i is UNDEF or has an UNDEF strong neighbor
__global__ void agg_near_k(int64_t nwork, const int *__restrict__ list,
                           const int *__restrict__ ptr, const int *__restrict__ col,
                           const uint8_t *__restrict__ S, const int *__restrict__ id,
                           uint8_t *__restrict__ near) {
    AGG_FOREACH(i) {
        if (id[i] == -1) {
            near[i] = 1;
            for (int j = ptr[i]; j < ptr[i + 1]; ++j)
                if (S[j]) near[col[j]] = 1;
        }
    }
}

__global__ void agg_roots_k(int64_t nwork, const int *__restrict__ list,
                            const int *__restrict__ ptr, const int *__restrict__ col,
                            const uint8_t *__restrict__ S, int *__restrict__ id,
                            const uint64_t *__restrict__ m1, uint8_t *__restrict__ newroot) {
    AGG_FOREACH(i) {
        newroot[i] = 0;
        if (id[i] != -1) continue;
        uint64_t key = agg_key_d((int)i);
        uint64_t m2 = m1[i];
        for (int j = ptr[i]; j < ptr[i + 1] && m2 <= key; ++j) {
            if (!S[j]) continue;
            uint64_t v = m1[col[j]];
            if (v > m2) m2 = v;
        }
        if (m2 == key) {
            id[i] = (int)i;
            newroot[i] = 1;
        }
    }
}

__global__ void agg_claim_k(int64_t nwork, const int *__restrict__ list,
                            const int *__restrict__ ptr, const int *__restrict__ col,
                            const uint8_t *__restrict__ S, int *__restrict__ id,
                            uint8_t *__restrict__ prov, const uint8_t *__restrict__ newroot) {
    AGG_FOREACH(i) {
        if (!newroot[i]) continue;
        for (int j = ptr[i]; j < ptr[i + 1]; ++j) {
            int c = col[j];
            if (!S[j]) continue;
            if (id[c] == -1 || prov[c]) {
                id[c] = (int)i;
                prov[c] = 0;
            }
        }
    }
}

// Two-phase adoption: the mark pass reads the stable post-claim state and
// records each node's choice; the commit pass applies it. A single fused
// pass would race (a neighbor turning provisional concurrently could be
// mistaken for a firm member, making the result timing-dependent).
__global__ void agg_adopt_mark_k(int64_t nwork, const int *__restrict__ list,
                                 const int *__restrict__ ptr,
                                 const int *__restrict__ col, const uint8_t *__restrict__ S,
                                 const int *__restrict__ id, const uint8_t *__restrict__ prov,
                                 int *__restrict__ choice) {
    AGG_FOREACH(i) {
        if (id[i] != -1) continue;
        uint64_t best = 0;
        int root = -1;
        for (int j = ptr[i]; j < ptr[i + 1]; ++j) {
            int c = col[j];
            if (!S[j] || c == (int)i) continue;
            if (id[c] >= 0 && !prov[c]) {
                uint64_t k = agg_key_d(id[c]);
                if (k > best) { best = k; root = id[c]; }
            }
        }
        choice[i] = root;
    }
}

__global__ void agg_adopt_commit_k(int64_t nwork, const int *__restrict__ list,
                                   int *__restrict__ id,
                                   uint8_t *__restrict__ prov,
                                   const int *__restrict__ choice,
                                   int *__restrict__ remaining) {
    int my_remaining = 0;
    AGG_FOREACH(i) {
        if (id[i] != -1) continue;
        int root = choice[i];
        if (root >= 0) {
            id[i] = root;
            prov[i] = 1;
        } else {
            ++my_remaining;
        }
    }
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1)
        my_remaining += __shfl_down(my_remaining, off, WAVE);
    if ((threadIdx.x & (WAVE - 1)) == 0 && my_remaining)
        atomicAdd(remaining, my_remaining);
}

__global__ void agg_mark_roots_k(int64_t n, const int *__restrict__ id, int *__restrict__ mark) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) mark[i] = (id[i] == (int)i) ? 1 : 0;
}

__global__ void agg_relabel_k(int64_t n, int *__restrict__ id, const int *__restrict__ mark) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride)
        if (id[i] >= 0) id[i] = mark[id[i]] - 1;
}

extern "C" int amg_agg_init(int64_t n, const int *ptr, const uint8_t *S, int *id, hipStream_t s) {
    agg_init_k<<<nblk(n), 256, 0, s>>>(n, ptr, S, id);
    return (int)hipGetLastError();
}
static int agg_round_impl(int64_t nwork, const int *list, const int *ptr,
                          const int *col, const uint8_t *S, int *id, uint8_t *prov,
                          uint64_t *m1, uint8_t *newroot, uint8_t *near,
                          int *remaining, hipStream_t s) {
    if (list)
        agg_clear_near_k<<<nblk(nwork), 256, 0, s>>>(nwork, list, near);
    else
        (void)hipMemsetAsync(near, 0, nwork, s);
    agg_near_k<<<nblk(nwork), 256, 0, s>>>(nwork, list, ptr, col, S, id, near);
    agg_m1_k<<<nblk(nwork), 256, 0, s>>>(nwork, list, ptr, col, S, id, near, m1);
    agg_roots_k<<<nblk(nwork), 256, 0, s>>>(nwork, list, ptr, col, S, id, m1, newroot);
    agg_claim_k<<<nblk(nwork), 256, 0, s>>>(nwork, list, ptr, col, S, id, prov, newroot);
    // reuse the m1 buffer as the choice array (i32 fits in the u64 slots)
    agg_adopt_mark_k<<<nblk(nwork), 256, 0, s>>>(nwork, list, ptr, col, S, id, prov,
                                                 (int *)m1);
    agg_adopt_commit_k<<<nblk(nwork), 256, 0, s>>>(nwork, list, id, prov, (int *)m1,
                                                   remaining);
    return (int)hipGetLastError();
}

extern "C" int amg_agg_round(int64_t n, const int *ptr, const int *col, const uint8_t *S,
                             int *id, uint8_t *prov, uint64_t *m1, uint8_t *newroot,
                             uint8_t *near, int *remaining, hipStream_t s) {
    return agg_round_impl(n, nullptr, ptr, col, S, id, prov, m1, newroot, near,
                          remaining, s);
}
// whole MIS round loop driven from C: one ctypes call per level instead of
// one per round (the Python round loop cost ~11 ms/round of host gaps at
// 134M rows — launch latency + torch op dispatch + .item() round-trips).
// Convergence is polled with a pinned-memory readback every `sync_stride`
// rounds. Returns hipError, or 9999 if max_rounds was exhausted.
// lists: caller-provided scratch of 3n ints — two ping-pong frontier lists
// plus a flag/scan buffer; nullptr disables frontier compaction.
extern "C" int amg_agg_run(int64_t n, const int *ptr, const int *col, const uint8_t *S,
                           int *id, uint8_t *prov, uint64_t *m1, uint8_t *newroot,
                           uint8_t *near, int *remaining, int sync_stride,
                           int max_rounds, int *rounds_out, int *lists,
                           hipStream_t s) {
    int *h_rem = nullptr;
    hipError_t e = hipHostMalloc((void **)&h_rem, 2 * sizeof(int),
                                 hipHostMallocDefault);
    if (e != hipSuccess) return (int)e;
    int *L[2] = {lists, lists ? lists + n : nullptr};
    int cur = -1;          // -1: full range; 0/1: active list index
    int64_t nwork = n;
    int64_t last_rem = n;  // UNDEF count at the last poll
    int first_cround = -1;
    int rc = 0;
    bool done = false;
    int round = 0;
    for (; round < max_rounds; ++round) {
        e = hipMemsetAsync(remaining, 0, sizeof(int), s);
        if (e != hipSuccess) { rc = (int)e; break; }
        const int *list = cur < 0 ? nullptr : L[cur];
        // refresh near first (it defines the next frontier superset)
        if (list)
            agg_clear_near_k<<<nblk(nwork), 256, 0, s>>>(nwork, list, near);
        else
            (void)hipMemsetAsync(near, 0, n, s);
        agg_near_k<<<nblk(nwork), 256, 0, s>>>(nwork, list, ptr, col, S, id, near);
        // compact the frontier once the UNDEF count is small (the active
        // set shrinks monotonically), then refresh every 4th round: later
        // rounds stop re-scanning all n nodes
        if (lists && last_rem * 4 < n &&
            (first_cround < 0 || (round - first_cround) % 4 == 0)) {
            int nxt = cur < 0 ? 0 : 1 - cur;
            int *F = lists + 2 * n;  // flags/scan scratch (n ints)
            agg_flag_k<<<nblk(nwork), 256, 0, s>>>(nwork, list, near, F);
            rc = scan_i32_device(F, nwork, s);
            if (rc) break;
            agg_scatter_list_k<<<nblk(nwork), 256, 0, s>>>(nwork, list, near, F,
                                                           L[nxt]);
            e = hipMemcpyAsync(h_rem + 1, F + (nwork - 1), sizeof(int),
                               hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) { rc = (int)e; break; }
            if (h_rem[1] > 0 && h_rem[1] < nwork) {
                cur = nxt;
                nwork = h_rem[1];
            }
            if (first_cround < 0) first_cround = round;
        }
        const int *list2 = cur < 0 ? nullptr : L[cur];
        agg_m1_k<<<nblk(nwork), 256, 0, s>>>(nwork, list2, ptr, col, S, id, near, m1);
        agg_roots_k<<<nblk(nwork), 256, 0, s>>>(nwork, list2, ptr, col, S, id, m1,
                                                newroot);
        agg_claim_k<<<nblk(nwork), 256, 0, s>>>(nwork, list2, ptr, col, S, id, prov,
                                                newroot);
        agg_adopt_mark_k<<<nblk(nwork), 256, 0, s>>>(nwork, list2, ptr, col, S, id,
                                                     prov, (int *)m1);
        agg_adopt_commit_k<<<nblk(nwork), 256, 0, s>>>(nwork, list2, id, prov,
                                                       (int *)m1, remaining);
        rc = (int)hipGetLastError();
        if (rc) break;
        if (round % sync_stride == sync_stride - 1 || round > 8) {
            e = hipMemcpyAsync(h_rem, remaining, sizeof(int), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) { rc = (int)e; break; }
            if (*h_rem == 0) { done = true; break; }
            last_rem = *h_rem;
        }
    }
    (void)hipHostFree(h_rem);
    if (rc) return rc;
    if (!done) return 9999;
    if (rounds_out) *rounds_out = round + 1;
    return 0;
}

extern "C" int amg_agg_renumber(int64_t n, int *id, int *mark, hipStream_t s) {
    agg_mark_roots_k<<<nblk(n), 256, 0, s>>>(n, id, mark);
    int rc = scan_i32_device(mark, n, s);
    if (rc) return rc;
    agg_relabel_k<<<nblk(n), 256, 0, s>>>(n, id, mark);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------
// smoothed prolongation P = (I - omega Df^-1 Af) P_tent, fused
// (device twin of core.cpp:smoothed_prolongation). 8 lanes per row with a
// 64-slot LDS hash keyed by aggregate id (the original thread-per-row local
// dedup array spilled to scratch and ran at <500 GB/s). Rows with more than
// PROW_MAX distinct aggregates raise `overflow` -> host fallback.
// ---------------------------------------------------------------------------
#define PROW_MAX 56
#define PSLOTS 64
#define PMASK (PSLOTS - 1)
#define PGRP 8

__global__ void psmooth_count_k(int64_t n, const int *__restrict__ ptr,
                                const int *__restrict__ col, const uint8_t *__restrict__ S,
                                const int *__restrict__ id, int *__restrict__ cnt,
                                int *__restrict__ overflow) {
    __shared__ int keys[32][PSLOTS];
    int gid = threadIdx.x / PGRP;
    int lane = threadIdx.x & (PGRP - 1);
    int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / PGRP;
    int64_t stride = ((int64_t)gridDim.x * blockDim.x) / PGRP;
    int *tk = keys[gid];
    for (; i < n; i += stride) {
        for (int t = lane; t < PSLOTS; t += PGRP) tk[t] = -1;
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_wave_barrier();
        int inserted = 0;
        bool ovf = false;
        for (int j = ptr[i] + lane; j < ptr[i + 1] && !ovf; j += PGRP) {
            int c = col[j];
            if (c != (int)i && !S[j]) continue;
            int a = id[c];
            if (a < 0) continue;
            uint32_t h = ((uint32_t)a * 2654435761u) & PMASK;
            int probes = 0;
            while (true) {
                int old = atomicCAS(&tk[h], -1, a);
                if (old == -1) { ++inserted; break; }
                if (old == a) break;
                h = (h + 1) & PMASK;
                if (++probes >= PSLOTS) { ovf = true; break; }  // table full
            }
        }
        if (ovf) atomicAdd(overflow, 1);
#pragma unroll
        for (int off = PGRP / 2; off > 0; off >>= 1)
            inserted += __shfl_down(inserted, off, PGRP);
        if (lane == 0) {
            if (inserted > PROW_MAX) atomicAdd(overflow, 1);
            cnt[i] = inserted;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

__global__ void psmooth_fill_k(int64_t n, const int *__restrict__ ptr,
                               const int *__restrict__ col, const double *__restrict__ val,
                               const uint8_t *__restrict__ S, const int *__restrict__ id,
                               double omega, const int *__restrict__ pptr,
                               int *__restrict__ pcol, double *__restrict__ pval) {
    __shared__ int keys[32][PSLOTS];
    __shared__ double vals[32][PSLOTS];
    int gid = threadIdx.x / PGRP;
    int lane = threadIdx.x & (PGRP - 1);
    int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / PGRP;
    int64_t stride = ((int64_t)gridDim.x * blockDim.x) / PGRP;
    int *tk = keys[gid];
    double *tv = vals[gid];
    for (; i < n; i += stride) {
        for (int t = lane; t < PSLOTS; t += PGRP) {
            tk[t] = -1;
            tv[t] = 0.0;
        }
        // filtered diagonal: original diagonal plus weak off-diagonal values
        double dia = 0.0;
        for (int j = ptr[i] + lane; j < ptr[i + 1]; j += PGRP)
            if (col[j] == (int)i || !S[j]) dia += val[j];
#pragma unroll
        for (int off = PGRP / 2; off > 0; off >>= 1)
            dia += __shfl_down(dia, off, PGRP);
        dia = __shfl(dia, (threadIdx.x & ~(PGRP - 1)) & 63, 64);
        if (dia != 0.0) dia = -omega / dia;
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_wave_barrier();
        for (int j = ptr[i] + lane; j < ptr[i + 1]; j += PGRP) {
            int c = col[j];
            if (c != (int)i && !S[j]) continue;
            int a = id[c];
            if (a < 0) continue;
            double v = (c == (int)i) ? (1.0 - omega) : dia * val[j];
            uint32_t h = ((uint32_t)a * 2654435761u) & PMASK;
            while (true) {
                int old = atomicCAS(&tk[h], -1, a);
                if (old == -1 || old == a) {
                    atomicAdd(&tv[h], v);
                    break;
                }
                h = (h + 1) & PMASK;
            }
        }
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_wave_barrier();
        // unsorted compaction (P columns need no ordering downstream: the
        // transpose and SpGEMM consumers are order-free, and host downloads
        // canonicalize; a per-row bitonic here measured 2x the kernel cost)
        int mine = 0;
        for (int t = lane; t < PSLOTS; t += PGRP)
            if (tk[t] != -1) ++mine;
        int off = mine;
#pragma unroll
        for (int d = 1; d < PGRP; d <<= 1) {
            int v = __shfl_up(off, d, PGRP);
            if (lane >= d) off += v;
        }
        off -= mine;
        int base = (i == 0) ? 0 : pptr[i - 1];
        int h2 = base + off;
        for (int t = lane; t < PSLOTS; t += PGRP)
            if (tk[t] != -1) {
                pcol[h2] = tk[t];
                pval[h2] = tv[t];
                ++h2;
            }
        __builtin_amdgcn_wave_barrier();
    }
}

// tentative (piecewise-constant) prolongation for non-smoothed aggregation
__global__ void ptent_count_k(int64_t n, const int *__restrict__ id, int *__restrict__ cnt) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) cnt[i] = id[i] >= 0 ? 1 : 0;
}

__global__ void ptent_fill_k(int64_t n, const int *__restrict__ id, const int *__restrict__ pptr,
                             int *__restrict__ pcol, double *__restrict__ pval) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        if (id[i] < 0) continue;
        int base = (i == 0) ? 0 : pptr[i - 1];
        pcol[base] = id[i];
        pval[base] = 1.0;
    }
}

extern "C" int amg_psmooth_count(int64_t n, const int *ptr, const int *col, const uint8_t *S,
                                 const int *id, int *cnt, int *overflow, hipStream_t s) {
    psmooth_count_k<<<nblk(n * PGRP), 256, 0, s>>>(n, ptr, col, S, id, cnt, overflow);
    return (int)hipGetLastError();
}
extern "C" int amg_psmooth_fill(int64_t n, const int *ptr, const int *col, const double *val,
                                const uint8_t *S, const int *id, double omega,
                                const int *pptr_scanned, int *pcol, double *pval,
                                hipStream_t s) {
    psmooth_fill_k<<<nblk(n * PGRP), 256, 0, s>>>(n, ptr, col, val, S, id, omega,
                                                  pptr_scanned, pcol, pval);
    return (int)hipGetLastError();
}
extern "C" int amg_ptent_count(int64_t n, const int *id, int *cnt, hipStream_t s) {
    ptent_count_k<<<nblk(n), 256, 0, s>>>(n, id, cnt);
    return (int)hipGetLastError();
}
extern "C" int amg_ptent_fill(int64_t n, const int *id, const int *pptr_scanned, int *pcol,
                              double *pval, hipStream_t s) {
    ptent_fill_k<<<nblk(n), 256, 0, s>>>(n, id, pptr_scanned, pcol, pval);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------
// transpose
// ---------------------------------------------------------------------------
__global__ void tcount_k(int64_t nnz, const int *__restrict__ col, int *__restrict__ tcnt) {
    int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; j < nnz; j += stride) atomicAdd(&tcnt[col[j]], 1);
}

__global__ void tscatter_k(int64_t n, const int *__restrict__ ptr, const int *__restrict__ col,
                           const double *__restrict__ val, int *__restrict__ cursor,
                           int *__restrict__ tcol, double *__restrict__ tval) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        for (int j = ptr[i]; j < ptr[i + 1]; ++j) {
            int c = col[j];
            int h = atomicAdd(&cursor[c], 1);
            tcol[h] = (int)i;
            tval[h] = val[j];
        }
    }
}

// per-row insertion sort (short rows); ptr_scanned is the inclusive scan,
// row i spans [ptr[i-1], ptr[i])
__global__ void sort_rows_k(int64_t n, const int *__restrict__ ptr_scanned,
                            int *__restrict__ col, double *__restrict__ val) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        int b = (i == 0) ? 0 : ptr_scanned[i - 1];
        int e = ptr_scanned[i];
        for (int k = b + 1; k < e; ++k) {
            int ck = col[k];
            double vk = val[k];
            int m = k;
            while (m > b && col[m - 1] > ck) {
                col[m] = col[m - 1];
                val[m] = val[m - 1];
                --m;
            }
            col[m] = ck;
            val[m] = vk;
        }
    }
}

extern "C" int amg_transpose_count(int64_t nnz, const int *col, int *tcnt, hipStream_t s) {
    tcount_k<<<nblk(nnz), 256, 0, s>>>(nnz, col, tcnt);
    return (int)hipGetLastError();
}
extern "C" int amg_transpose_scatter(int64_t n, const int *ptr, const int *col,
                                     const double *val, int *cursor, int *tcol, double *tval,
                                     hipStream_t s) {
    tscatter_k<<<nblk(n), 256, 0, s>>>(n, ptr, col, val, cursor, tcol, tval);
    return (int)hipGetLastError();
}
extern "C" int amg_sort_rows(int64_t n, const int *ptr_scanned, int *col, double *val,
                             hipStream_t s) {
    sort_rows_k<<<nblk(n), 256, 0, s>>>(n, ptr_scanned, col, val);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------
// SpGEMM: wave-per-row with LDS hash accumulators.
// Count pass: 512-slot key table per wave (4 waves/block -> 8 KiB LDS).
// Fill pass: 512-slot key+value tables per wave (24 KiB LDS per block).
// Rows with more than ~448 distinct output columns set `overflow`; the host
// falls back to the CPU spgemm for that product (never triggered by the
// Poisson/SA chain, whose rows stay < 100).
// ---------------------------------------------------------------------------
#define HSLOTS 512
#define HMASK (HSLOTS - 1)
// small-row bin: 8 lanes per row, 128-slot tables (rows with ub <= SGSMALL)
#define SGRP 8
#define SSLOTS 128
#define SSMASK (SSLOTS - 1)
#define SGSMALL 96

// per-row product upper bound (for binning)
__global__ void spgemm_ub_k(int64_t an, const int *__restrict__ aptr,
                            const int *__restrict__ acol, const int *__restrict__ bptr,
                            int *__restrict__ ub) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < an; i += stride) {
        int u = 0;
        for (int ja = aptr[i]; ja < aptr[i + 1]; ++ja) {
            int ca = acol[ja];
            u += bptr[ca + 1] - bptr[ca];
        }
        ub[i] = u;
    }
}

// Small-bin rows work in chunks of SGRP A entries: each lane of the 8-lane
// group stages ONE A entry (its B-row begin and length, loaded in parallel).
// The count pass, whose result does not depend on insertion order, then
// flattens the chunk's products: a width-8 scan gives the product prefix and
// the lanes stride the products t = lane, lane+8, ...  Everything stays in
// registers; all shuffles sit in group-uniform control flow.
__device__ __forceinline__ int sg_scan(int x, int lane) {
#pragma unroll
    for (int d = 1; d < SGRP; d <<= 1) {
        int v = __shfl_up(x, d, SGRP);
        if (lane >= d) x += v;
    }
    return x;  // inclusive
}

// entry holding product t of the chunk: the number of inclusive prefixes
// <= t (empty B rows repeat a prefix and are stepped over); `e` receives
// that entry's exclusive prefix. t >= p[SGRP-1] clamps to the last lane.
__device__ __forceinline__ int sg_find(const int (&p)[SGRP], int t, int &e) {
    int ja = 0;
    e = 0;
#pragma unroll
    for (int k = 0; k < SGRP - 1; ++k)
        if (p[k] <= t) {
            ja = k + 1;
            e = p[k];
        }
    return ja;
}

// templated on the LDS table size, tiered by ub: the dominant fine-level
// A*P rows have <= 24 candidates, where a 32-slot table quarters the
// init/extract traffic of the 128-slot one (measured: the init dominates
// 5:1 for 24-candidate rows)
template <int SLOTS>
__global__ void spgemm_count_small_k(int64_t an, const int *__restrict__ aptr,
                                     const int *__restrict__ acol,
                                     const int *__restrict__ bptr,
                                     const int *__restrict__ bcol,
                                     const int *__restrict__ ub, int *__restrict__ cnt,
                                     int ub_lo, int ub_hi) {
    __shared__ int keys[32][SLOTS];  // 32 groups of 8 lanes (256 threads)
    constexpr int MASK = SLOTS - 1;
    int gid = threadIdx.x / SGRP;
    int lane = threadIdx.x & (SGRP - 1);
    int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / SGRP;
    int64_t stride = ((int64_t)gridDim.x * blockDim.x) / SGRP;
    int *tk = keys[gid];
    for (; row < an; row += stride) {
        int u = ub[row];
        if (u <= ub_lo || u > ub_hi) continue;
        for (int t = lane; t < SLOTS; t += SGRP) tk[t] = -1;
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_wave_barrier();
        int inserted = 0;
        const int aend = aptr[row + 1];
        for (int j0 = aptr[row]; j0 < aend; j0 += SGRP) {
            int j = j0 + lane;
            int bb = 0, bl = 0;
            if (j < aend) {
                int ca = acol[j];
                bb = bptr[ca];
                bl = bptr[ca + 1] - bb;
            }
            int inc = sg_scan(bl, lane);
            int p[SGRP];
#pragma unroll
            for (int k = 0; k < SGRP; ++k) p[k] = __shfl(inc, k, SGRP);
            const int tot = p[SGRP - 1];
            for (int t0 = 0; t0 < tot; t0 += SGRP) {
                int t = t0 + lane, e;
                int ja = sg_find(p, t, e);
                int bj = __shfl(bb, ja, SGRP);
                if (t < tot) {
                    int key = bcol[bj + (t - e)];
                    uint32_t h = ((uint32_t)key * 2654435761u) & MASK;
                    while (true) {
                        int old = atomicCAS(&tk[h], -1, key);
                        if (old == -1) { ++inserted; break; }
                        if (old == key) break;
                        h = (h + 1) & MASK;
                    }
                }
            }
        }
#pragma unroll
        for (int off = SGRP / 2; off > 0; off >>= 1)
            inserted += __shfl_down(inserted, off, SGRP);
        if (lane == 0) cnt[row] = inserted;
        __builtin_amdgcn_wave_barrier();
    }
}

// Small-bin fill, templated on the LDS table size and tiered by the exact
// output length (a 64-slot table suffices for len <= 48 rows and halves the
// init/extraction work of the dominant fine-level A*P product).
template <int SLOTS>
__global__ void spgemm_fill_small_k(int64_t an, const int *__restrict__ aptr,
                                    const int *__restrict__ acol,
                                    const double *__restrict__ aval,
                                    const int *__restrict__ bptr,
                                    const int *__restrict__ bcol,
                                    const double *__restrict__ bval,
                                    const int *__restrict__ ub,
                                    const int *__restrict__ cptr_scanned,
                                    int *__restrict__ ccol, double *__restrict__ cval,
                                    int do_sort, int len_lo, int len_hi) {
    __shared__ int keys[32][SLOTS];
    __shared__ double vals[32][SLOTS];
    constexpr int SMASK_S = SLOTS - 1;
    int gid = threadIdx.x / SGRP;
    int lane = threadIdx.x & (SGRP - 1);
    int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / SGRP;
    int64_t stride = ((int64_t)gridDim.x * blockDim.x) / SGRP;
    int *tk = keys[gid];
    double *tv = vals[gid];
    for (; row < an; row += stride) {
        if (ub[row] > SGSMALL) continue;
        int base = (row == 0) ? 0 : cptr_scanned[row - 1];
        int len = cptr_scanned[row] - base;
        if (len <= len_lo || len > len_hi) continue;
        for (int t = lane; t < SLOTS; t += SGRP) {
            tk[t] = -1;
            tv[t] = 0.0;
        }
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_wave_barrier();
        const int aend = aptr[row + 1];
        for (int j0 = aptr[row]; j0 < aend; j0 += SGRP) {
            int j = j0 + lane;
            int bb = 0, bl = 0;
            double va = 0.0;
            if (j < aend) {
                int ca = acol[j];
                va = aval[j];
                bb = bptr[ca];
                bl = bptr[ca + 1] - bb;
            }
            // The entries are staged in parallel, but inserted one after the
            // other with the lanes striding one B row, as before: the slot a
            // key lands in, and with it the order of an unsorted row and the
            // order of every sum, depend on which products share an
            // instruction, and results must not move with this change.
            const int nj = min(SGRP, aend - j0);
            for (int k = 0; k < nj; ++k) {
                const int bk = __shfl(bb, k, SGRP);
                const int ek = bk + __shfl(bl, k, SGRP);
                const double vk = __shfl(va, k, SGRP);
                for (int jb = bk + lane; jb < ek; jb += SGRP) {
                    int key = bcol[jb];
                    double v = vk * bval[jb];
                    uint32_t h = ((uint32_t)key * 2654435761u) & SMASK_S;
                    while (true) {
                        int old = atomicCAS(&tk[h], -1, key);
                        if (old == -1 || old == key) {
                            atomicAdd(&tv[h], v);
                            break;
                        }
                        h = (h + 1) & SMASK_S;
                    }
                }
            }
        }
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_wave_barrier();
        if (do_sort) {
            // sorted extraction: empties to +inf, bitonic, write the prefix
            for (int t = lane; t < SLOTS; t += SGRP)
                if (tk[t] == -1) tk[t] = 0x7fffffff;
            lds_bitonic<SGRP, SLOTS>(tk, tv, lane);
            for (int t = lane; t < len; t += SGRP) {
                ccol[base + t] = tk[t];
                cval[base + t] = tv[t];
            }
        } else {
            // unsorted compaction (intermediate products: order irrelevant);
            // per-lane local count -> exclusive shfl prefix -> direct writes
            int mine = 0;
            for (int t = lane; t < SLOTS; t += SGRP)
                if (tk[t] != -1) ++mine;
            int off = mine;
#pragma unroll
            for (int d = 1; d < SGRP; d <<= 1) {
                int v = __shfl_up(off, d, SGRP);
                if (lane >= d) off += v;
            }
            off -= mine;  // exclusive prefix within the group
            int h = base + off;
            for (int t = lane; t < SLOTS; t += SGRP)
                if (tk[t] != -1) {
                    ccol[h] = tk[t];
                    cval[h] = tv[t];
                    ++h;
                }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// Big rows: wave per row, with the (ja, jb) product space FLATTENED across
// the 64 lanes via an LDS prefix of B-row lengths (short B rows would leave
// most lanes idle under the naive per-A-entry split). A rows longer than
// BIGROW raise `overflow` -> host fallback.
#define BIGROW 256

__device__ __forceinline__ int pfx_find(const int *pfx, int len, int t) {
    // largest ja with pfx[ja] <= t  (pfx[0] = 0, ascending)
    int lo = 0, hi = len;  // invariant: pfx[lo] <= t < pfx[hi+? ]
    while (hi - lo > 1) {
        int mid = (lo + hi) >> 1;
        if (pfx[mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

// inclusive wave scan of the staged B-row lengths
__device__ __forceinline__ int wave_scan(int x, int lane) {
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        int v = __shfl_up(x, d, WAVE);
        if (lane >= d) x += v;
    }
    return x;
}

// Count pass, wave per row, templated on the LDS table size. The exact
// output length is unknown before counting, so rows tier by the product
// upper bound: distinct keys <= ub, so any row with ub < SLOTS is safe in
// the smaller table. (ub_lo, ub_hi] selects this launch's tier.
// Big-row worklist: rows with ub > SGSMALL (the wave-per-row tiers).
// Measured: letting the big-tier kernels scan-and-skip ALL rows wave-per-row
// costs ~33 ms per fine-level product where only 0.03% of rows qualify.
// Built by flag -> scan -> scatter (no global-atomic counter); the count
// lives in device memory so the launches need no host sync.
__global__ void spg_bigflag_k(int64_t an, const int *__restrict__ ub,
                              int *__restrict__ flags) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < an; i += stride) flags[i] = ub[i] > SGSMALL ? 1 : 0;
}

__global__ void spg_bigscatter_k(int64_t an, const int *__restrict__ ub,
                                 const int *__restrict__ flags_scanned,
                                 int *__restrict__ list, int *__restrict__ nbig) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < an; i += stride) {
        if (ub[i] > SGSMALL) list[flags_scanned[i] - 1] = (int)i;
        if (i == an - 1) *nbig = flags_scanned[i];
    }
}

template <int SLOTS>
__global__ void spgemm_count_k(int64_t an, const int *__restrict__ biglist,
                               const int *__restrict__ nbig,
                               const int *__restrict__ aptr,
                               const int *__restrict__ acol, const int *__restrict__ bptr,
                               const int *__restrict__ bcol, const int *__restrict__ ub,
                               int *__restrict__ cnt, int *__restrict__ overflow,
                               int ub_lo, int ub_hi) {
    __shared__ int keys[4][SLOTS];
    __shared__ int pfx[4][BIGROW + 1];
    __shared__ int bbeg[4][BIGROW];
    constexpr int SMASK = SLOTS - 1;
    int wid = threadIdx.x / WAVE;
    int lane = threadIdx.x & (WAVE - 1);
    int64_t idx = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    int64_t stride = ((int64_t)gridDim.x * blockDim.x) / WAVE;
    const int64_t nwork = *nbig;
    int *tk = keys[wid];

    for (; idx < nwork; idx += stride) {
        int64_t row = biglist[idx];
        int total = ub[row];
        if (total <= ub_lo || total > ub_hi) continue;
        int ab = aptr[row], alen = aptr[row + 1] - ab;
        for (int t = lane; t < SLOTS; t += WAVE) tk[t] = -1;
        const bool huge = alen > BIGROW;
        if (!huge) {
            // product-space prefix: every lane stages its own A entries,
            // wave scan per 64-wide chunk, running total carried across
            int acc = 0;
            for (int j0 = 0; j0 < alen; j0 += WAVE) {
                int j = j0 + lane;
                int bb = 0, bl = 0;
                if (j < alen) {
                    int ca = acol[ab + j];
                    bb = bptr[ca];
                    bl = bptr[ca + 1] - bb;
                }
                int inc = wave_scan(bl, lane);
                if (j < alen) {
                    pfx[wid][j] = acc + inc - bl;
                    bbeg[wid][j] = bb;
                }
                acc += __shfl(inc, WAVE - 1, WAVE);
            }
            if (lane == 0) pfx[wid][alen] = acc;
        }
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_wave_barrier();
        int inserted = 0;
        bool ovf = false;
        if (huge) {
            // rare very-long A rows (big coarse aggregates): iterate A
            // entries serially, the wave splits each B row — no LDS staging
            for (int j = 0; j < alen && !ovf; ++j) {
                int ca = acol[ab + j];
                for (int jb = bptr[ca] + lane; jb < bptr[ca + 1] && !ovf;
                     jb += WAVE) {
                    int key = bcol[jb];
                    uint32_t h = ((uint32_t)key * 2654435761u) & SMASK;
                    int probes = 0;
                    while (true) {
                        int old = atomicCAS(&tk[h], -1, key);
                        if (old == -1) { ++inserted; break; }
                        if (old == key) break;
                        h = (h + 1) & SMASK;
                        if (++probes >= SLOTS) { ovf = true; break; }
                    }
                }
            }
        } else {
        for (int t = lane; t < total && !ovf; t += WAVE) {
            int ja = pfx_find(pfx[wid], alen, t);
            int key = bcol[bbeg[wid][ja] + (t - pfx[wid][ja])];
            uint32_t h = ((uint32_t)key * 2654435761u) & SMASK;
            int probes = 0;
            while (true) {
                int old = atomicCAS(&tk[h], -1, key);
                if (old == -1) { ++inserted; break; }
                if (old == key) break;
                h = (h + 1) & SMASK;
                if (++probes >= SLOTS) { ovf = true; break; }
            }
        }
        }
        if (ovf && lane == 0) atomicAdd(overflow, 1);
#pragma unroll
        for (int off = WAVE / 2; off > 0; off >>= 1)
            inserted += __shfl_down(inserted, off, WAVE);
        if (lane == 0) cnt[row] = inserted;
        __builtin_amdgcn_wave_barrier();
    }
}

// Fill pass, wave per row, templated on the LDS table size. The count pass
// already fixed each row's exact output length, so rows are tiered by it:
// len <= MIDLEN rows use a 128-slot table (4x cheaper init + extraction,
// ~2x LDS occupancy) and only genuinely wide rows pay for 512 slots.
// (len_lo, len_hi] selects this launch's tier.
#define MIDLEN 96

template <int SLOTS>
__global__ void spgemm_fill_k(int64_t an, const int *__restrict__ biglist,
                              const int *__restrict__ nbig,
                              const int *__restrict__ aptr,
                              const int *__restrict__ acol, const double *__restrict__ aval,
                              const int *__restrict__ bptr, const int *__restrict__ bcol,
                              const double *__restrict__ bval, const int *__restrict__ ub,
                              const int *__restrict__ cptr_scanned, int *__restrict__ ccol,
                              double *__restrict__ cval, int do_sort, int len_lo,
                              int len_hi) {
    __shared__ int keys[4][SLOTS];
    __shared__ double vals[4][SLOTS];
    __shared__ int pfx[4][BIGROW + 1];
    __shared__ int bbeg[4][BIGROW];
    __shared__ double av[4][BIGROW];
    constexpr int SMASK = SLOTS - 1;
    int wid = threadIdx.x / WAVE;
    int lane = threadIdx.x & (WAVE - 1);
    int64_t idx = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    int64_t stride = ((int64_t)gridDim.x * blockDim.x) / WAVE;
    const int64_t nwork = *nbig;
    int *tk = keys[wid];
    double *tv = vals[wid];

    for (; idx < nwork; idx += stride) {
        int64_t row = biglist[idx];
        int total = ub[row];
        if (total <= SGSMALL) continue;
        int ab = aptr[row], alen = aptr[row + 1] - ab;
        int base = (row == 0) ? 0 : cptr_scanned[row - 1];
        int len = cptr_scanned[row] - base;
        if (len <= len_lo || len > len_hi) continue;
        const bool huge = alen > BIGROW;
        for (int t = lane; t < SLOTS; t += WAVE) {
            tk[t] = -1;
            tv[t] = 0.0;
        }
        if (!huge) {
            int acc = 0;
            for (int j0 = 0; j0 < alen; j0 += WAVE) {
                int j = j0 + lane;
                int bb = 0, bl = 0;
                if (j < alen) {
                    int ca = acol[ab + j];
                    av[wid][j] = aval[ab + j];
                    bb = bptr[ca];
                    bl = bptr[ca + 1] - bb;
                }
                int inc = wave_scan(bl, lane);
                if (j < alen) {
                    pfx[wid][j] = acc + inc - bl;
                    bbeg[wid][j] = bb;
                }
                acc += __shfl(inc, WAVE - 1, WAVE);
            }
            if (lane == 0) pfx[wid][alen] = acc;
        }
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_wave_barrier();
        if (huge) {
            for (int j = 0; j < alen; ++j) {
                int ca = acol[ab + j];
                double va = aval[ab + j];
                for (int jb = bptr[ca] + lane; jb < bptr[ca + 1]; jb += WAVE) {
                    int key = bcol[jb];
                    double v = va * bval[jb];
                    uint32_t h = ((uint32_t)key * 2654435761u) & SMASK;
                    while (true) {
                        int old = atomicCAS(&tk[h], -1, key);
                        if (old == -1 || old == key) {
                            atomicAdd(&tv[h], v);
                            break;
                        }
                        h = (h + 1) & SMASK;
                    }
                }
            }
        } else {
        for (int t = lane; t < total; t += WAVE) {
            int ja = pfx_find(pfx[wid], alen, t);
            int jb = bbeg[wid][ja] + (t - pfx[wid][ja]);
            int key = bcol[jb];
            double v = av[wid][ja] * bval[jb];
            uint32_t h = ((uint32_t)key * 2654435761u) & SMASK;
            while (true) {
                int old = atomicCAS(&tk[h], -1, key);
                if (old == -1 || old == key) {
                    atomicAdd(&tv[h], v);
                    break;
                }
                h = (h + 1) & SMASK;
            }
        }
        }
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_wave_barrier();
        if (do_sort) {
            for (int t = lane; t < SLOTS; t += WAVE)
                if (tk[t] == -1) tk[t] = 0x7fffffff;
            lds_bitonic<WAVE, SLOTS>(tk, tv, lane);
            for (int t = lane; t < len; t += WAVE) {
                ccol[base + t] = tk[t];
                cval[base + t] = tv[t];
            }
        } else {
            int mine = 0;
            for (int t = lane; t < SLOTS; t += WAVE)
                if (tk[t] != -1) ++mine;
            int off = mine;
#pragma unroll
            for (int d = 1; d < WAVE; d <<= 1) {
                int v = __shfl_up(off, d, WAVE);
                if (lane >= d) off += v;
            }
            off -= mine;
            int h = base + off;
            for (int t = lane; t < SLOTS; t += WAVE)
                if (tk[t] != -1) {
                    ccol[h] = tk[t];
                    cval[h] = tv[t];
                    ++h;
                }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// ---------------------------------------------------------------------------
// 7-point Poisson fixture generated directly in device memory (same
// semantics as the host generator / reference tests/sample_problem.hpp:11).
// ---------------------------------------------------------------------------
// Row-strip form: rows [row_beg, row_end) with GLOBAL columns — the
// distributed fixture (one strip per rank, reference
// examples/mpi/mpi_solver.cpp assemble_poisson3d shape).  Global column ids
// stay int32, so the GLOBAL problem may reach 2^31 unknowns (~1290^3) even
// though one GPU holds only its strip.
__global__ void poisson_cnt_k(int64_t n, int64_t nz, int64_t row_beg, int64_t row_end,
                              int *__restrict__ cnt) {
    int64_t idx = row_beg + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; idx < row_end; idx += stride) {
        int64_t i = idx % n, j = (idx / n) % n, k = idx / (n * n);
        cnt[idx - row_beg] =
            1 + (k > 0) + (j > 0) + (i > 0) + (i + 1 < n) + (j + 1 < n) + (k + 1 < nz);
    }
}

__global__ void poisson_fill_k(int64_t n, int64_t nz, int64_t row_beg, int64_t row_end,
                               const int *__restrict__ ptr_scanned,
                               int *__restrict__ col, double *__restrict__ val) {
    int64_t idx = row_beg + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; idx < row_end; idx += stride) {
        int64_t i = idx % n, j = (idx / n) % n, k = idx / (n * n);
        int64_t loc = idx - row_beg;
        int h = (loc == 0) ? 0 : ptr_scanned[loc - 1];
        if (k > 0)      { col[h] = (int)(idx - n * n); val[h] = -1.0; ++h; }
        if (j > 0)      { col[h] = (int)(idx - n);     val[h] = -1.0; ++h; }
        if (i > 0)      { col[h] = (int)(idx - 1);     val[h] = -1.0; ++h; }
        col[h] = (int)idx; val[h] = 6.0; ++h;
        if (i + 1 < n)  { col[h] = (int)(idx + 1);     val[h] = -1.0; ++h; }
        if (j + 1 < n)  { col[h] = (int)(idx + n);     val[h] = -1.0; ++h; }
        if (k + 1 < nz) { col[h] = (int)(idx + n * n); val[h] = -1.0; ++h; }
    }
}

extern "C" int amg_poisson_cnt(int64_t n, int64_t nz, int64_t row_beg, int64_t row_end,
                               int *cnt, hipStream_t s) {
    poisson_cnt_k<<<nblk(row_end - row_beg), 256, 0, s>>>(n, nz, row_beg, row_end, cnt);
    return (int)hipGetLastError();
}
extern "C" int amg_poisson_fill(int64_t n, int64_t nz, int64_t row_beg, int64_t row_end,
                                const int *ptr_scanned, int *col, double *val,
                                hipStream_t s) {
    poisson_fill_k<<<nblk(row_end - row_beg), 256, 0, s>>>(n, nz, row_beg, row_end,
                                                           ptr_scanned, col, val);
    return (int)hipGetLastError();
}

// bigscratch: caller scratch of (2*an + 1) ints — flags/scan buffer,
// the big-row list, and its device-side count (kernels read the count from
// device memory, so no host sync is needed to size the launches).
extern "C" int amg_spgemm_count(int64_t an, const int *aptr, const int *acol, const int *bptr,
                                const int *bcol, int *ub, int *cnt, int *overflow,
                                int *bigscratch, hipStream_t s) {
    int *flags = bigscratch;
    int *biglist = bigscratch + an;
    int *nbig = bigscratch + 2 * an;
    spgemm_ub_k<<<nblk(an), 256, 0, s>>>(an, aptr, acol, bptr, ub);
    spg_bigflag_k<<<nblk(an), 256, 0, s>>>(an, ub, flags);
    int rc = scan_i32_device(flags, an, s);
    if (rc) return rc;
    spg_bigscatter_k<<<nblk(an), 256, 0, s>>>(an, ub, flags, biglist, nbig);
    // single count pass: a 32-slot count tier measured WORSE (the count is
    // candidate-probing-bound, not table-init-bound, and the second sweep
    // costs a full pass) — the small table only pays in the FILL
    spgemm_count_small_k<SSLOTS><<<nblk(an * SGRP), 256, 0, s>>>(
        an, aptr, acol, bptr, bcol, ub, cnt, 0, SGSMALL);
    spgemm_count_k<HSLOTS><<<nblk(an * WAVE), 256, 0, s>>>(
        an, biglist, nbig, aptr, acol, bptr, bcol, ub, cnt, overflow, SGSMALL, 1 << 30);
    return (int)hipGetLastError();
}
extern "C" int amg_spgemm_fill(int64_t an, const int *aptr, const int *acol, const double *aval,
                               const int *bptr, const int *bcol, const double *bval,
                               const int *ub, const int *cptr_scanned, int *ccol,
                               double *cval, int do_sort, const int *bigscratch,
                               hipStream_t s) {
    const int *biglist = bigscratch + an;
    const int *nbig = bigscratch + 2 * an;
    spgemm_fill_small_k<32><<<nblk(an * SGRP), 256, 0, s>>>(an, aptr, acol, aval, bptr,
                                                            bcol, bval, ub, cptr_scanned,
                                                            ccol, cval, do_sort, 0, 20);
    spgemm_fill_small_k<64><<<nblk(an * SGRP), 256, 0, s>>>(an, aptr, acol, aval, bptr,
                                                            bcol, bval, ub, cptr_scanned,
                                                            ccol, cval, do_sort, 20, 48);
    spgemm_fill_small_k<SSLOTS><<<nblk(an * SGRP), 256, 0, s>>>(an, aptr, acol, aval, bptr,
                                                                bcol, bval, ub, cptr_scanned,
                                                                ccol, cval, do_sort, 48,
                                                                1 << 30);
    // wave-per-row tiers by exact output length, over the big-row list only
    spgemm_fill_k<128><<<nblk(an * WAVE), 256, 0, s>>>(
        an, biglist, nbig, aptr, acol, aval, bptr, bcol, bval, ub, cptr_scanned, ccol,
        cval, do_sort, 0, MIDLEN);
    spgemm_fill_k<HSLOTS><<<nblk(an * WAVE), 256, 0, s>>>(
        an, biglist, nbig, aptr, acol, aval, bptr, bcol, bval, ub, cptr_scanned, ccol,
        cval, do_sort, MIDLEN, 1 << 30);
    return (int)hipGetLastError();
}
