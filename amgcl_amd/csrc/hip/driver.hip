// amgcl_amd — native solve driver (gfx950).
//
// Runs the entire AMG-preconditioned Krylov solve (V/W-cycle + CG/BiCGStab
// loop) in C++: one ctypes call per solve, no Python between kernels.
// This is the runtime counterpart of the reference's compiled solve templates
// (amgcl/amg.hpp:514-553 cycle; amgcl/solver/cg.hpp:152-204;
// amgcl/solver/bicgstab.hpp:176-240), specialized for the HIP backend with
// diagonal (SPAI0 / damped-Jacobi), Chebyshev, ILU(0) and SPAI-1 smoothers.
//
// Per-level relaxation uses a pointer-swapping fused kernel
//   x_new = x + M ∘ (rhs - A x)
// so the separate axpby pass of the generic path disappears.
//
// Launchers from the other .hip files come from amg_kernels.h.  Each entry
// point is enter_driver -> body -> finish(), so every return of a body, an
// error included, leaves through the same stream hand-back.

#include <hip/hip_runtime.h>

#include "amg_common.h"
#include "amg_kernels.h"

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <type_traits>
#include <utility>
#include <vector>

// Value-type dispatch for the templated cycle (fp64, or the fp32 hierarchy of
// mixed precision): name<T>(args...) calls amg_name_f64 or amg_name_f32 from
// amg_kernels.h.  BSR is fp64-only (block_value + mixed precision is rejected
// upstream); its call sites refuse T = float themselves.
#define AMG_BY_TYPE(name)                                 \
    template <typename T, typename... Args>               \
    static inline int name(Args... args) {                \
        if constexpr (std::is_same_v<T, double>)          \
            return amg_##name##_f64(args...);             \
        else                                              \
            return amg_##name##_f32(args...);             \
    }
AMG_BY_TYPE(spmv)
AMG_BY_TYPE(residual)
AMG_BY_TYPE(gemv)
AMG_BY_TYPE(sell_spmv)
AMG_BY_TYPE(sell_residual)
AMG_BY_TYPE(sell_relax)
AMG_BY_TYPE(sellc_spmv)
AMG_BY_TYPE(sellc_residual)
AMG_BY_TYPE(sellc_relax)
AMG_BY_TYPE(axpby)
AMG_BY_TYPE(vmul)
AMG_BY_TYPE(fill)
#undef AMG_BY_TYPE

// x_new = x + M ∘ (rhs - A x), written to a separate buffer (pointer swap)
template <int SUBW, typename T>
__global__ void relax_swap_k(int64_t nrows, const int *__restrict__ ptr,
                             const int *__restrict__ col, const T *__restrict__ val,
                             const T *__restrict__ M, const T *__restrict__ rhs,
                             const T *__restrict__ x, T *__restrict__ xn) {
    int64_t tid = amg_logical_block() * blockDim.x + threadIdx.x;
    int lane = (int)(tid & (SUBW - 1));
    int64_t row = tid / SUBW;
    int64_t stride = ((int64_t)gridDim.x * blockDim.x) / SUBW;
    for (; row < nrows; row += stride) {
        T s = (T)0;
        int b = ptr[row], e = ptr[row + 1];
        for (int j = b + lane; j < e; j += SUBW)
            s += AMG_STREAM_LD(&val[j]) * x[AMG_STREAM_LD(&col[j])];
#pragma unroll
        for (int off = SUBW / 2; off > 0; off >>= 1) s += __shfl_down(s, off, SUBW);
        if (lane == 0) xn[row] = x[row] + M[row] * (rhs[row] - s);
    }
}

// first pre-smooth of a cycle starts from u = 0: x_new = M ∘ rhs (no A pass)
template <typename T>
__global__ void relax_zero_k(int64_t n, const T *__restrict__ M,
                             const T *__restrict__ rhs, T *__restrict__ xn) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) xn[i] = M[i] * rhs[i];
}

struct GraphEntry {
    const double *rhs;
    double *x;
    double *xswap;
    hipGraphExec_t exec;
};

struct Driver {
    std::vector<LevelDesc> lv;
    const void *coarse_inv;  // dense n x n (may be null -> smooth coarsest)
    int64_t ncoarse;
    int npre, npost, ncycle, pre_cycles;
    hipStream_t stream;
    double *dotbuf_d;  // 2 doubles
    double *dotbuf_h;  // pinned host, 2 doubles
    // hipGraph cache for the V-cycle: the cycle is a fixed kernel sequence
    // over fixed pointers, so one capture per (rhs, x, x_swap) triple turns
    // the whole preconditioner application (dozens of launches, the coarse
    // tail being pure launch overhead) into a single graph launch.
    std::vector<GraphEntry> graphs;
    bool use_graphs;
    // The solve runs on an internal non-blocking stream, event-chained to the
    // caller's (torch) stream at entry/exit.  The torch default stream is the
    // HIP *legacy* stream, which hipStreamBeginCapture cannot capture
    // (hipErrorStreamCaptureUnsupported, measured r02); an owned stream both
    // enables graph capture and decouples the solve from torch's stream.
    hipStream_t ext_stream;  // caller's stream (ordering boundary only)
    hipEvent_t ev_in, ev_out;
    // mixed precision: the cycle runs fp32 on the (fp32) LevelDescs while the
    // Krylov loop keeps the fp64 fine operator below + f32 cast buffers
    int f32;
    OpDesc a64;
    float *cb_r, *cb_x, *cb_s;  // level-0-sized cast buffers (f32 mode)
};

#define CHK(x)                          \
    do {                                \
        int _rc = (x);                  \
        if (_rc) return _rc;            \
    } while (0)

// y = alpha op x + beta y and r = rhs - op x, through the operator's SELL
// image when it has one (compact if smask is set, else padded), else CSR:
// the only place that choice is made
template <typename T>
static int op_spmv(Driver *D, const OpDesc &op, const T *x, double alpha, double beta,
                   T *y) {
    if (op.nslice && op.smask)
        return sellc_spmv<T>(op.nrows, op.nslice, op.moff, op.smask, op.ptr, op.scol,
                             (const T *)op.sval, x, alpha, beta, y, D->stream);
    if (op.nslice)
        return sell_spmv<T>(op.nrows, op.nslice, op.soff, op.scol, (const T *)op.sval,
                            op.srows, x, alpha, beta, y, D->stream);
    return spmv<T>(op.nrows, op.nnz, op.ptr, op.col, (const T *)op.val, x, alpha, beta, y,
                   op.subw, D->stream);
}

template <typename T>
static int op_residual(Driver *D, const OpDesc &op, const T *rhs, const T *x, T *r) {
    if (op.nslice && op.smask)
        return sellc_residual<T>(op.nrows, op.nslice, op.moff, op.smask, op.ptr, op.scol,
                                 (const T *)op.sval, rhs, x, r, D->stream);
    if (op.nslice)
        return sell_residual<T>(op.nrows, op.nslice, op.soff, op.scol,
                                (const T *)op.sval, op.srows, rhs, x, r, D->stream);
    return residual<T>(op.nrows, op.nnz, op.ptr, op.col, (const T *)op.val, rhs, x, r,
                       op.subw, D->stream);
}

// residual through whichever storage this level's A carries (BSR, else L.A)
template <typename T>
static int level_residual(Driver *D, const LevelDesc &L, const T *rhs, const T *x,
                          T *r) {
    if (!L.bsize) return op_residual<T>(D, L.A, rhs, x, r);
    if constexpr (std::is_same_v<T, double>)
        return amg_bsr_residual_f64(L.nbrows, L.bsize, L.bptr, L.bcol, L.bval, rhs, x, r,
                                    D->stream);
    else
        return (int)hipErrorInvalidValue;
}

// Chebyshev polynomial smoothing, in place on x (driver twin of
// relaxation/chebyshev.py _polynomial; scratch r provided by the caller,
// d lives in the level)
template <typename T>
static int cheb_apply(Driver *D, const LevelDesc &L, const T *rhs, T *x, T *r) {
    T *d = (T *)L.cheb_d;
    CHK(level_residual<T>(D, L, rhs, x, r));
    if (L.M) CHK(vmul<T>(L.A.nrows, 1.0, (const T *)L.M, r, 0.0, r, D->stream));
    double rho = 1.0 / L.cheb_sigma1;
    CHK(axpby<T>(L.A.nrows, 1.0 / L.cheb_theta, r, 0.0, d, D->stream));
    for (int k = 0; k < L.cheb_degree; ++k) {
        CHK(axpby<T>(L.A.nrows, 1.0, d, 1.0, x, D->stream));
        CHK(level_residual<T>(D, L, rhs, x, r));
        if (L.M) CHK(vmul<T>(L.A.nrows, 1.0, (const T *)L.M, r, 0.0, r, D->stream));
        double rho_next = 1.0 / (2.0 * L.cheb_sigma1 - rho);
        CHK(axpby<T>(L.A.nrows, 2.0 * rho_next / L.cheb_delta, r, rho_next * rho, d,
                     D->stream));
        rho = rho_next;
    }
    return 0;
}

// ILU(0) smoothing step, in place on x (driver twin of relaxation/ilu0.py
// _solve_jacobi; parity: amgcl/relaxation/detail/ilu_solve.hpp:44-124):
//   t = rhs - A x;  t <- (LU)^{-1} t by damped-Jacobi iterated triangular
//   solves;  x += damping * t.   fp64 only (ILU + mixed is not offered).
template <typename T>
static int ilu_apply(Driver *D, const LevelDesc &L, const T *rhs, T *x, T *t) {
    return (int)hipErrorInvalidValue;  // specialized for double below
}

template <>
int ilu_apply<double>(Driver *D, const LevelDesc &L, const double *rhs, double *x,
                      double *t) {
    const int64_t n = L.A.nrows;
    hipStream_t st = D->stream;
    double *y = L.ilu_y, *s = L.ilu_s, *b = L.ilu_b;
    const double om = L.ilu_jdamping;
    CHK(level_residual<double>(D, L, rhs, x, t));
    // lower: (I + L) y = t
    CHK(hipMemcpyAsync(y, t, n * sizeof(double), hipMemcpyDeviceToDevice, st));
    for (int it = 0; it < L.ilu_iters; ++it) {
        CHK(op_spmv<double>(D, L.ilu_L, y, -1.0, 0.0, s));
        CHK(amg_axpby_f64(n, 1.0, t, 1.0, s, st));
        CHK(amg_axpby_f64(n, om, s, 1.0 - om, y, st));
    }
    // upper: (D + U) z = y  ->  z = Dinv (y - U z), z kept in y
    CHK(hipMemcpyAsync(b, y, n * sizeof(double), hipMemcpyDeviceToDevice, st));
    CHK(amg_vmul_f64(n, 1.0, L.ilu_dinv, b, 0.0, y, st));
    for (int it = 0; it < L.ilu_iters; ++it) {
        CHK(op_spmv<double>(D, L.ilu_U, y, -1.0, 0.0, s));
        CHK(amg_axpby_f64(n, 1.0, b, 1.0, s, st));
        CHK(amg_vmul_f64(n, 1.0, L.ilu_dinv, s, 0.0, s, st));
        CHK(amg_axpby_f64(n, om, s, 1.0 - om, y, st));
    }
    CHK(amg_axpby_f64(n, L.ilu_damping, y, 1.0, x, st));
    return 0;
}

// SPAI-1 smoothing step, in place on x (driver twin of relaxation/spai0.py
// Spai1._step; parity: amgcl/relaxation/spai1.hpp:126-134):
//   t = rhs - A x;  x += M t,  M = L.spai1.   fp64 only (SPAI-1 + mixed is
// not offered).  From a zero guess (t null) it is x = M rhs, one kernel.
template <typename T>
static int spai1_apply(Driver *D, const LevelDesc &L, const T *rhs, T *x, T *t) {
    return (int)hipErrorInvalidValue;  // specialized for double below
}

template <>
int spai1_apply<double>(Driver *D, const LevelDesc &L, const double *rhs, double *x,
                        double *t) {
    if (!t) return op_spmv<double>(D, L.spai1, rhs, 1.0, 0.0, x);
    CHK(level_residual<double>(D, L, rhs, x, t));
    return op_spmv<double>(D, L.spai1, t, 1.0, 1.0, x);
}

template <typename T>
static int relax_swap(Driver *D, const LevelDesc &L, const T *rhs, T **x, T **xn) {
    if (L.spai1.nrows > 0) {  // in place, no pointer swap
        CHK(spai1_apply<T>(D, L, rhs, *x, *xn));
        return 0;
    }
    if (L.ilu_iters) {  // in place, no pointer swap
        CHK(ilu_apply<T>(D, L, rhs, *x, *xn));
        return 0;
    }
    if (L.cheb_degree) {  // in place, no pointer swap
        CHK(cheb_apply<T>(D, L, rhs, *x, *xn));
        return 0;
    }
    if (L.bsize) {
        // xn = M o (rhs - A x); xn += x; swap
        if constexpr (std::is_same_v<T, double>)
            CHK(amg_bsr_relax_f64(L.nbrows, L.bsize, L.bptr, L.bcol, L.bval, L.M, rhs,
                                  *x, *xn, D->stream));
        else
            return (int)hipErrorInvalidValue;
        CHK(axpby<T>(L.A.nrows, 1.0, *x, 1.0, *xn, D->stream));
        std::swap(*x, *xn);
        return 0;
    }
    const OpDesc &A = L.A;
    const T *M = (const T *)L.M;
    if (A.nslice) {
        if (A.smask)
            CHK(sellc_relax<T>(A.nrows, A.nslice, A.moff, A.smask, A.ptr, A.scol,
                               (const T *)A.sval, M, rhs, *x, *xn, D->stream));
        else
            CHK(sell_relax<T>(A.nrows, A.nslice, A.soff, A.scol, (const T *)A.sval,
                              A.srows, M, rhs, *x, *xn, D->stream));
        std::swap(*x, *xn);
        return 0;
    }
    int grid = amg_nblocks(A.nrows * A.subw);
    const T *val = (const T *)A.val;
#define RCASE(SW)                                                                       \
    case SW:                                                                            \
        relax_swap_k<SW, T><<<grid, 256, 0, D->stream>>>(A.nrows, A.ptr, A.col, val, M, \
                                                         rhs, *x, *xn);                 \
        break;
    switch (A.subw) {
        RCASE(1) RCASE(2) RCASE(4) RCASE(8) RCASE(16) RCASE(32) RCASE(64)
        default: return hipErrorInvalidValue;
    }
#undef RCASE
    std::swap(*x, *xn);
    return (int)hipGetLastError();
}

// one multigrid cycle; *u_io holds the iterate buffer (may be swapped),
// uses L.t as the swap partner / residual scratch
template <typename T>
static int cycle(Driver *D, int li, const T *f, T **u_io, T **scratch, bool u_is_zero) {
    LevelDesc &L = D->lv[li];
    const bool coarsest = (li + 1 == (int)D->lv.size());

    // relax_zero writes into the swap buffer and swaps, so zero-guess and
    // general smooths have identical pointer parity (no copy-back needed)
    auto relax_zero = [&](LevelDesc &LL, const T *ff, T **u2, T **sc) -> int {
        // in place like its general form, so neither swaps
        if (LL.spai1.nrows > 0) return spai1_apply<T>(D, LL, ff, *u2, (T *)nullptr);
        if (LL.cheb_degree || LL.bsize || LL.ilu_iters) {
            // no fused zero-guess form for these smoothers: clear + general
            CHK(fill<T>(LL.A.nrows, 0.0, *u2, D->stream));
            return relax_swap<T>(D, LL, ff, u2, sc);
        }
        relax_zero_k<T><<<amg_nblocks(LL.A.nrows), 256, 0, D->stream>>>(
            LL.A.nrows, (const T *)LL.M, ff, *sc);
        std::swap(*u2, *sc);
        return 0;
    };

    if (coarsest) {
        if (D->coarse_inv) {
            CHK(gemv<T>(L.A.nrows, (const T *)D->coarse_inv, f, *u_io, D->stream));
        } else {
            for (int i = 0; i < D->npre + D->npost; ++i) {
                if (u_is_zero && i == 0) {
                    CHK(relax_zero(L, f, u_io, scratch));
                    continue;
                }
                CHK(relax_swap<T>(D, L, f, u_io, scratch));
            }
        }
        return (int)hipGetLastError();
    }

    LevelDesc &N = D->lv[li + 1];
    for (int i = 0; i < D->npre; ++i) {
        if (u_is_zero && i == 0) {
            CHK(relax_zero(L, f, u_io, scratch));
            continue;
        }
        CHK(relax_swap<T>(D, L, f, u_io, scratch));
    }
    // t = f - A u ; f_next = R t
    CHK(level_residual<T>(D, L, f, *u_io, *scratch));
    CHK(op_spmv<T>(D, L.R, *scratch, 1.0, 0.0, (T *)N.f));
    T *nu = (T *)N.u;
    T *nscratch = (T *)N.t;
    for (int c = 0; c < D->ncycle; ++c) {
        CHK(cycle<T>(D, li + 1, (const T *)N.f, &nu, &nscratch, c == 0));
        // after the first sub-cycle the iterate is nonzero
    }
    // u += P u_next
    CHK(op_spmv<T>(D, L.P, nu, 1.0, 1.0, *u_io));
    for (int i = 0; i < D->npost; ++i)
        CHK(relax_swap<T>(D, L, f, u_io, scratch));
    return (int)hipGetLastError();
}

// fp64 in/out preconditioner application; in f32 mode the V-cycle runs on the
// fp32 hierarchy between two cast kernels (backend/detail/mixing.hpp shape)
static int precond_apply(Driver *D, const double *rhs, double *x, double *x_swap) {
    const int64_t n = D->lv[0].A.nrows;
    if (D->f32) {
        CHK(amg_cast_d2s(n, rhs, D->cb_r, D->stream));
        float *u = D->cb_x;
        float *scratch = D->cb_s;
        for (int c = 0; c < D->pre_cycles; ++c)
            CHK(cycle<float>(D, 0, D->cb_r, &u, &scratch, c == 0));
        CHK(amg_cast_s2d(n, u, x, D->stream));
        return 0;
    }
    double *u = x;
    double *scratch = x_swap;
    for (int c = 0; c < D->pre_cycles; ++c)
        CHK(cycle<double>(D, 0, rhs, &u, &scratch, c == 0));
    if (u != x)
        CHK(hipMemcpyAsync(x, u, n * sizeof(double), hipMemcpyDeviceToDevice, D->stream));
    return 0;
}

// Graph-cached preconditioner application.  The per-cycle launch sequence is
// deterministic (the relax pointer-swap count is fixed), so a capture is
// valid for every later call with the same buffer triple.  Falls back to the
// direct path if capture fails (e.g. nested capture) or AMGCL_NO_GRAPH=1.
static int precond_apply_graphed(Driver *D, const double *rhs, double *x,
                                 double *x_swap) {
    if (!D->use_graphs) return precond_apply(D, rhs, x, x_swap);
    for (const GraphEntry &g : D->graphs)
        if (g.rhs == rhs && g.x == x && g.xswap == x_swap)
            return (int)hipGraphLaunch(g.exec, D->stream);
    if (D->graphs.size() >= 8) return precond_apply(D, rhs, x, x_swap);
    if (hipStreamBeginCapture(D->stream, hipStreamCaptureModeThreadLocal) !=
        hipSuccess)
        return precond_apply(D, rhs, x, x_swap);
    int rc = precond_apply(D, rhs, x, x_swap);
    hipGraph_t graph;
    hipError_t ec = hipStreamEndCapture(D->stream, &graph);
    if (rc) return rc;
    if (ec != hipSuccess) return (int)ec;
    hipGraphExec_t exec;
    ec = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ec != hipSuccess) {
        // capture succeeded but instantiation failed: run directly
        (void)hipGetLastError();
        D->use_graphs = false;
        return precond_apply(D, rhs, x, x_swap);
    }
    D->graphs.push_back({rhs, x, x_swap, exec});
    return (int)hipGraphLaunch(exec, D->stream);
}

// order the internal stream after the caller's stream (entry) and the
// caller's stream after the internal one (exit)
static int enter_driver(Driver *D) {
    if (D->stream == D->ext_stream) return 0;
    CHK((int)hipEventRecord(D->ev_in, D->ext_stream));
    CHK((int)hipStreamWaitEvent(D->stream, D->ev_in, 0));
    return 0;
}
static int leave_driver(Driver *D) {
    if (D->stream == D->ext_stream) return 0;
    CHK((int)hipEventRecord(D->ev_out, D->stream));
    CHK((int)hipStreamWaitEvent(D->ext_stream, D->ev_out, 0));
    return 0;
}

static int read_dots(Driver *D, int n, double *out) {
    CHK(hipMemcpyAsync(D->dotbuf_h, D->dotbuf_d, n * sizeof(double),
                       hipMemcpyDeviceToHost, D->stream));
    CHK(hipStreamSynchronize(D->stream));
    for (int i = 0; i < n; ++i) out[i] = D->dotbuf_h[i];
    return 0;
}

extern "C" void *amg_driver_create(const LevelDesc *levels, int nlevels,
                                   const void *coarse_inv, int64_t ncoarse, int npre,
                                   int npost, int ncycle, int pre_cycles, int f32,
                                   const OpDesc *a64, hipStream_t stream) {
    if (f32 && !a64) return nullptr;
    Driver *D = new Driver();
    D->lv.assign(levels, levels + nlevels);
    if (a64) D->a64 = *a64;
    // settle every automatic CSR width once (relax_swap switches on it)
    auto settle = [](OpDesc &op) {
        if (op.subw <= 0) op.subw = amg_pick_subw(op.nrows, op.nnz);
    };
    settle(D->a64);
    for (LevelDesc &L : D->lv)
        for (OpDesc *op : {&L.A, &L.P, &L.R, &L.spai1, &L.ilu_L, &L.ilu_U}) settle(*op);
    D->coarse_inv = coarse_inv;
    D->ncoarse = ncoarse;
    D->npre = npre;
    D->npost = npost;
    D->ncycle = ncycle;
    D->pre_cycles = pre_cycles;
    D->stream = stream;
    D->f32 = f32;
    D->cb_r = D->cb_x = D->cb_s = nullptr;
    const char *ng = getenv("AMGCL_NO_GRAPH");
    D->use_graphs = !(ng && ng[0] && ng[0] != '0');
    D->ext_stream = stream;
    D->ev_in = D->ev_out = nullptr;
    hipStream_t st_int = nullptr;
    if (hipStreamCreateWithFlags(&st_int, hipStreamNonBlocking) == hipSuccess &&
        hipEventCreateWithFlags(&D->ev_in, hipEventDisableTiming) == hipSuccess &&
        hipEventCreateWithFlags(&D->ev_out, hipEventDisableTiming) == hipSuccess) {
        D->stream = st_int;  // all driver work goes to the internal stream
    } else {
        if (st_int) (void)hipStreamDestroy(st_int);
        D->use_graphs = false;  // legacy stream cannot be captured
    }
    bool ok = hipMalloc((void **)&D->dotbuf_d, 2 * sizeof(double)) == hipSuccess &&
              hipHostMalloc((void **)&D->dotbuf_h, 2 * sizeof(double)) == hipSuccess;
    if (ok && f32) {
        int64_t n = D->lv[0].A.nrows;
        ok = hipMalloc((void **)&D->cb_r, n * sizeof(float)) == hipSuccess &&
             hipMalloc((void **)&D->cb_x, n * sizeof(float)) == hipSuccess &&
             hipMalloc((void **)&D->cb_s, n * sizeof(float)) == hipSuccess;
    }
    if (!ok) {
        delete D;
        return nullptr;
    }
    return D;
}

extern "C" void amg_driver_destroy(void *h) {
    Driver *D = (Driver *)h;
    if (!D) return;
    (void)hipFree(D->dotbuf_d);
    (void)hipHostFree(D->dotbuf_h);
    for (GraphEntry &g : D->graphs) (void)hipGraphExecDestroy(g.exec);
    if (D->stream != D->ext_stream) (void)hipStreamDestroy(D->stream);
    if (D->ev_in) (void)hipEventDestroy(D->ev_in);
    if (D->ev_out) (void)hipEventDestroy(D->ev_out);
    if (D->cb_r) (void)hipFree(D->cb_r);
    if (D->cb_x) (void)hipFree(D->cb_x);
    if (D->cb_s) (void)hipFree(D->cb_s);
    delete D;
}

// OpDesc / LevelDesc layout as compiled, for the ctypes twins (backend/
// native.py) to check themselves against when they bind: both sizes, then
// the offset of every OpDesc member and of every top-level LevelDesc member
// in declaration order.  Writes at most cap entries, returns the full count.
extern "C" int amg_desc_layout(int64_t *out, int cap) {
#define OP(m) offsetof(OpDesc, m)
#define LV(m) offsetof(LevelDesc, m)
    const size_t v[] = {
        sizeof(OpDesc), sizeof(LevelDesc),
        OP(nrows), OP(nnz), OP(ptr), OP(col), OP(val), OP(subw), OP(nslice), OP(soff), OP(scol),
        OP(sval), OP(srows), OP(smask), OP(moff),
        LV(A), LV(P), LV(R), LV(M), LV(f), LV(u), LV(t), LV(cheb_degree), LV(cheb_theta),
        LV(cheb_delta), LV(cheb_sigma1), LV(cheb_d), LV(bsize), LV(nbrows), LV(bptr), LV(bcol),
        LV(bval), LV(spai1), LV(ilu_iters), LV(ilu_damping), LV(ilu_jdamping), LV(ilu_L), LV(ilu_U),
        LV(ilu_dinv), LV(ilu_y), LV(ilu_s), LV(ilu_b)};
#undef OP
#undef LV
    const int count = (int)(sizeof v / sizeof v[0]);
    for (int i = 0; i < count && i < cap; ++i) out[i] = (int64_t)v[i];
    return count;
}

// The single exit of every entry point once enter_driver has succeeded; rc
// is what the body returned (0, a failed launch, a BiCGStab breakdown).  The
// caller's stream is always ordered after the internal one, and a solve also
// waits for the internal stream, so no kernel is left running on the caller's
// buffers behind an error return.  The body's code comes first.
static int finish(Driver *D, int rc, bool sync) {
    int rc_leave = leave_driver(D);
    int rc_sync = sync ? (int)hipStreamSynchronize(D->stream) : 0;
    return rc ? rc : rc_leave ? rc_leave : rc_sync;
}

// standalone preconditioner application (used by the distributed layer:
// the Krylov loop stays in Python for halo exchange, but each local V-cycle
// runs natively)
extern "C" int amg_driver_precond(void *h, const double *rhs, double *x, double *x_swap) {
    Driver *D = (Driver *)h;
    CHK(enter_driver(D));
    return finish(D, precond_apply_graphed(D, rhs, x, x_swap), /*sync=*/false);
}

// The fp64 fine operator the Krylov loops iterate with: level 0's A, or in
// mixed mode the fp64 copy (level 0 then describes the fp32 operator the
// cycle runs on, which has no BSR form)
struct FineOp {
    Driver *D;
    OpDesc op;
    const LevelDesc *bsr;  // level 0 when it stores A as BSR, else null
    explicit FineOp(Driver *D)
        : D(D), op(D->f32 ? D->a64 : D->lv[0].A),
          bsr(!D->f32 && D->lv[0].bsize ? &D->lv[0] : nullptr) {}
    // y = alpha A x + beta y, storage precedence as in level_residual
    int spmv(const double *x, double alpha, double beta, double *y) const {
        if (bsr)
            return amg_bsr_spmv_f64(bsr->nbrows, bsr->bsize, bsr->bptr, bsr->bcol,
                                    bsr->bval, x, alpha, beta, y, D->stream);
        return op_spmv<double>(D, op, x, alpha, beta, y);
    }
    int residual(const double *rhs, const double *x, double *r) const {
        return bsr ? level_residual<double>(D, *bsr, rhs, x, r)
                   : op_residual<double>(D, op, rhs, x, r);
    }
};

struct Krylov {
    double norm_rhs, eps, res;  // ||rhs||, absolute target, current ||r||
};

// Shared entry of the Krylov loops: ||rhs||, eps, r = rhs - A x (copied to
// r_copy if given: BiCGStab's shadow residual) and ||r||.  A zero rhs is
// solved by x = 0: res = eps = 0 then keeps the caller's loop from starting.
static int krylov_begin(Driver *D, const FineOp &A, const double *rhs, double *x,
                        double *r, double *r_copy, double tol, double abstol,
                        Krylov *k) {
    const int64_t n = A.op.nrows;
    hipStream_t st = D->stream;
    double dot;
    CHK(amg_dot_f64(n, rhs, rhs, D->dotbuf_d, st));
    CHK(read_dots(D, 1, &dot));
    k->norm_rhs = sqrt(dot);
    k->eps = k->res = 0.0;
    if (k->norm_rhs == 0.0) return amg_fill_f64(n, 0.0, x, st);
    k->eps = tol * k->norm_rhs > abstol ? tol * k->norm_rhs : abstol;
    CHK(A.residual(rhs, x, r));
    if (r_copy)
        CHK(hipMemcpyAsync(r_copy, r, n * sizeof(double), hipMemcpyDeviceToDevice, st));
    CHK(amg_dot_f64(n, r, r, D->dotbuf_d, st));
    CHK(read_dots(D, 1, &dot));
    k->res = sqrt(dot);
    return 0;
}

// shared tail: iteration count and relative residual (0 for a zero rhs)
static int krylov_end(const Krylov &k, int64_t iter, int64_t *iters_out,
                      double *resid_out) {
    *iters_out = iter;
    *resid_out = k.norm_rhs == 0.0 ? 0.0 : k.res / k.norm_rhs;
    return 0;
}

// Preconditioned CG (parity: amgcl/solver/cg.hpp:152-204).
// Work vectors r,s,p,q + s_swap provided by the caller (device, n doubles).
static int cg_solve(Driver *D, const double *rhs, double *x, double *r, double *s,
                    double *p, double *q, double *s_swap, double tol, double abstol,
                    int maxiter, int64_t *iters_out, double *resid_out) {
    const FineOp A(D);
    const int64_t n = A.op.nrows;
    hipStream_t st = D->stream;
    double dots[2];
    Krylov k;
    CHK(krylov_begin(D, A, rhs, x, r, nullptr, tol, abstol, &k));

    double rho1 = 0.0, rho2 = 0.0;
    int64_t iter = 0;
    while (k.res > k.eps && iter < maxiter) {
        CHK(precond_apply_graphed(D, r, s, s_swap));
        rho2 = rho1;
        CHK(amg_dot_f64(n, r, s, D->dotbuf_d, st));
        CHK(read_dots(D, 1, dots));
        rho1 = dots[0];
        if (iter == 0) {
            CHK(hipMemcpyAsync(p, s, n * sizeof(double), hipMemcpyDeviceToDevice, st));
        } else {
            CHK(amg_axpby_f64(n, 1.0, s, rho1 / rho2, p, st));
        }
        CHK(A.spmv(p, 1.0, 0.0, q));
        CHK(amg_dot_f64(n, q, p, D->dotbuf_d, st));
        CHK(read_dots(D, 1, dots));
        double alpha = rho1 / dots[0];
        // fused x/r update + residual norm (single pass over x,r,p,q)
        CHK(amg_cg_tail_f64(n, alpha, p, q, x, r, D->dotbuf_d, st));
        CHK(read_dots(D, 1, dots));
        k.res = sqrt(dots[0]);
        ++iter;
    }
    return krylov_end(k, iter, iters_out, resid_out);
}

extern "C" int amg_driver_cg(void *h, const double *rhs, double *x, double *r, double *s,
                             double *p, double *q, double *s_swap, double tol,
                             double abstol, int maxiter, int64_t *iters_out,
                             double *resid_out) {
    Driver *D = (Driver *)h;
    CHK(enter_driver(D));
    return finish(D, cg_solve(D, rhs, x, r, s, p, q, s_swap, tol, abstol, maxiter,
                              iters_out, resid_out), /*sync=*/true);
}

// Preconditioned BiCGStab, right-preconditioned
// (parity: amgcl/solver/bicgstab.hpp:176-240).
// work: r,p,v,s2,t2,rh,T,T_swap (device, n doubles each); -2 = breakdown
static int bicgstab_solve(Driver *D, const double *rhs, double *x, double *r, double *p,
                          double *v, double *s2, double *t2, double *rh, double *T,
                          double *T_swap, double tol, double abstol, int maxiter,
                          int64_t *iters_out, double *resid_out) {
    const FineOp A(D);
    const int64_t n = A.op.nrows;
    hipStream_t st = D->stream;
    double dots[2];
    Krylov k;
    CHK(krylov_begin(D, A, rhs, x, r, rh, tol, abstol, &k));

    double rho1 = 0.0, rho2 = 0.0, alpha = 0.0, omega = 0.0;
    int64_t iter = 0;
    bool first = true;
    while (k.res > k.eps && iter < maxiter) {
        rho2 = rho1;
        CHK(amg_dot_f64(n, r, rh, D->dotbuf_d, st));
        CHK(read_dots(D, 1, dots));
        rho1 = dots[0];
        if (first) {
            CHK(hipMemcpyAsync(p, r, n * sizeof(double), hipMemcpyDeviceToDevice, st));
            first = false;
        } else {
            if (rho2 == 0.0 || omega == 0.0) return -2;
            double beta = (rho1 * alpha) / (rho2 * omega);
            CHK(amg_axpbypcz_f64(n, 1.0, r, -beta * omega, v, beta, p, st));
        }
        // v = A (M^-1 p);  T = M^-1 p
        CHK(precond_apply_graphed(D, p, T, T_swap));
        CHK(A.spmv(T, 1.0, 0.0, v));
        CHK(amg_dot_f64(n, rh, v, D->dotbuf_d, st));
        CHK(read_dots(D, 1, dots));
        alpha = rho1 / dots[0];
        CHK(amg_axpby_f64(n, alpha, T, 1.0, x, st));
        CHK(amg_axpbypcz_f64(n, 1.0, r, -alpha, v, 0.0, s2, st));
        CHK(amg_dot_f64(n, s2, s2, D->dotbuf_d, st));
        CHK(read_dots(D, 1, dots));
        k.res = sqrt(dots[0]);
        if (k.res > k.eps) {
            CHK(precond_apply_graphed(D, s2, T, T_swap));
            CHK(A.spmv(T, 1.0, 0.0, t2));
            CHK(amg_dot2_f64(n, t2, s2, t2, t2, D->dotbuf_d, st));
            CHK(read_dots(D, 2, dots));
            omega = dots[0] / dots[1];
            if (omega == 0.0) return -2;
            CHK(amg_axpby_f64(n, omega, T, 1.0, x, st));
            CHK(amg_axpbypcz_f64(n, 1.0, s2, -omega, t2, 0.0, r, st));
            CHK(amg_dot_f64(n, r, r, D->dotbuf_d, st));
            CHK(read_dots(D, 1, dots));
            k.res = sqrt(dots[0]);
        }
        ++iter;
    }
    return krylov_end(k, iter, iters_out, resid_out);
}

extern "C" int amg_driver_bicgstab(void *h, const double *rhs, double *x, double *r,
                                   double *p, double *v, double *s2, double *t2,
                                   double *rh, double *T, double *T_swap, double tol,
                                   double abstol, int maxiter, int64_t *iters_out,
                                   double *resid_out) {
    Driver *D = (Driver *)h;
    CHK(enter_driver(D));
    return finish(D, bicgstab_solve(D, rhs, x, r, p, v, s2, t2, rh, T, T_swap, tol,
                                    abstol, maxiter, iters_out, resid_out),
                  /*sync=*/true);
}
