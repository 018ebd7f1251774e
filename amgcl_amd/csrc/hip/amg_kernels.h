// amgcl_amd — the extern "C" functions one .hip file calls from another.
//
// Included by the files that define these functions as well as by the files
// that call them, so a declaration that disagrees with its definition is a
// compile error.  Functions reached only through ctypes are not listed.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

struct OpDesc;  // amg_common.h
struct LevelDesc;

extern "C" {

// ---- kernels.hip: CSR / SELL-64 / vector launchers used by the solve driver
int amg_spmv_f64(int64_t nrows, int64_t nnz, const int *ptr, const int *col,
                 const double *val, const double *x, double alpha, double beta,
                 double *y, int subw, hipStream_t stream);
int amg_spmv_f32(int64_t nrows, int64_t nnz, const int *ptr, const int *col,
                 const float *val, const float *x, double alpha, double beta, float *y,
                 int subw, hipStream_t stream);
int amg_residual_f64(int64_t nrows, int64_t nnz, const int *ptr, const int *col,
                     const double *val, const double *rhs, const double *x, double *r,
                     int subw, hipStream_t stream);
int amg_residual_f32(int64_t nrows, int64_t nnz, const int *ptr, const int *col,
                     const float *val, const float *rhs, const float *x, float *r,
                     int subw, hipStream_t stream);
int amg_sell_spmv_f64(int64_t nrows, int64_t nslice, const int64_t *soff, const int *col,
                      const double *val, const int *srows, const double *x, double alpha,
                      double beta, double *y, hipStream_t stream);
int amg_sell_spmv_f32(int64_t nrows, int64_t nslice, const int64_t *soff, const int *col,
                      const float *val, const int *srows, const float *x, double alpha,
                      double beta, float *y, hipStream_t stream);
int amg_sell_residual_f64(int64_t nrows, int64_t nslice, const int64_t *soff,
                          const int *col, const double *val, const int *srows,
                          const double *rhs, const double *x, double *r,
                          hipStream_t stream);
int amg_sell_residual_f32(int64_t nrows, int64_t nslice, const int64_t *soff,
                          const int *col, const float *val, const int *srows,
                          const float *rhs, const float *x, float *r,
                          hipStream_t stream);
int amg_sell_relax_f64(int64_t nrows, int64_t nslice, const int64_t *soff, const int *col,
                       const double *val, const int *srows, const double *M,
                       const double *rhs, const double *x, double *xn,
                       hipStream_t stream);
int amg_sell_relax_f32(int64_t nrows, int64_t nslice, const int64_t *soff, const int *col,
                       const float *val, const int *srows, const float *M,
                       const float *rhs, const float *x, float *xn, hipStream_t stream);
int amg_sell_fill_f64(int64_t nrows, int64_t nslice, const int *ptr, const int *col,
                      const double *val, const int64_t *soff, const int *srows, int *scol,
                      double *sval, hipStream_t stream);
// compact SELL-64 image (moff, smask, the CSR ptr, then the nnz-long scol/sval)
int amg_sellc_spmv_f64(int64_t nrows, int64_t nslice, const int64_t *moff,
                       const uint64_t *smask, const int *ptr, const int *col,
                       const double *val, const double *x, double alpha, double beta,
                       double *y, hipStream_t stream);
int amg_sellc_spmv_f32(int64_t nrows, int64_t nslice, const int64_t *moff,
                       const uint64_t *smask, const int *ptr, const int *col,
                       const float *val, const float *x, double alpha, double beta,
                       float *y, hipStream_t stream);
int amg_sellc_residual_f64(int64_t nrows, int64_t nslice, const int64_t *moff,
                           const uint64_t *smask, const int *ptr, const int *col,
                           const double *val, const double *rhs, const double *x,
                           double *r, hipStream_t stream);
int amg_sellc_residual_f32(int64_t nrows, int64_t nslice, const int64_t *moff,
                           const uint64_t *smask, const int *ptr, const int *col,
                           const float *val, const float *rhs, const float *x, float *r,
                           hipStream_t stream);
int amg_sellc_relax_f64(int64_t nrows, int64_t nslice, const int64_t *moff,
                        const uint64_t *smask, const int *ptr, const int *col,
                        const double *val, const double *M, const double *rhs,
                        const double *x, double *xn, hipStream_t stream);
int amg_sellc_relax_f32(int64_t nrows, int64_t nslice, const int64_t *moff,
                        const uint64_t *smask, const int *ptr, const int *col,
                        const float *val, const float *M, const float *rhs,
                        const float *x, float *xn, hipStream_t stream);
int amg_sellc_fill_f64(int64_t nrows, int64_t nslice, const int *ptr, const int *col,
                       const double *val, const int64_t *moff, uint64_t *smask,
                       int *scol, double *sval, hipStream_t stream);
int amg_sellc_fill_f32(int64_t nrows, int64_t nslice, const int *ptr, const int *col,
                       const float *val, const int64_t *moff, uint64_t *smask, int *scol,
                       float *sval, hipStream_t stream);
int amg_sell_compact_rule(int64_t slots, int64_t nnz, int64_t nmask, int64_t nslice,
                          int vbytes);
int amg_axpby_f64(int64_t n, double a, const double *x, double b, double *y,
                  hipStream_t stream);
int amg_axpby_f32(int64_t n, double a, const float *x, double b, float *y,
                  hipStream_t stream);
int amg_axpbypcz_f64(int64_t n, double a, const double *x, double b, const double *y,
                     double c, double *z, hipStream_t stream);
int amg_vmul_f64(int64_t n, double a, const double *m, const double *x, double b,
                 double *z, hipStream_t stream);
int amg_vmul_f32(int64_t n, double a, const float *m, const float *x, double b, float *z,
                 hipStream_t stream);
int amg_fill_f64(int64_t n, double v, double *x, hipStream_t stream);
int amg_fill_f32(int64_t n, double v, float *x, hipStream_t stream);
int amg_dot_f64(int64_t n, const double *x, const double *y, double *out,
                hipStream_t stream);
int amg_dot2_f64(int64_t n, const double *x1, const double *y1, const double *x2,
                 const double *y2, double *out, hipStream_t stream);
int amg_gemv_f64(int64_t n, const double *a, const double *f, double *u,
                 hipStream_t stream);
int amg_gemv_f32(int64_t n, const float *a, const float *f, float *u, hipStream_t stream);
int amg_cg_tail_f64(int64_t n, double alpha, const double *p, const double *q, double *x,
                    double *r, double *out, hipStream_t stream);
int amg_cast_d2s(int64_t n, const double *src, float *dst, hipStream_t stream);
int amg_cast_s2d(int64_t n, const float *src, double *dst, hipStream_t stream);

// ---- block.hip: BSR launchers (fp64 only)
int amg_bsr_spmv_f64(int64_t nbrows, int bsize, const int *ptr, const int *col,
                     const double *val, const double *x, double alpha, double beta,
                     double *y, hipStream_t stream);
int amg_bsr_residual_f64(int64_t nbrows, int bsize, const int *ptr, const int *col,
                         const double *val, const double *rhs, const double *x,
                         double *r, hipStream_t stream);
int amg_bsr_relax_f64(int64_t nbrows, int bsize, const int *ptr, const int *col,
                      const double *val, const double *M, const double *rhs,
                      const double *x, double *t, hipStream_t stream);

// ---- setup.hip: device setup engine used by the torch-free C API
int amg_setup_diag(int64_t n, const int *ptr, const int *col, const double *val,
                   double *d, hipStream_t s);
int amg_setup_strong(int64_t n, const int *ptr, const int *col, const double *val,
                     const double *d, double eps2, uint8_t *S, hipStream_t s);
int amg_setup_spai0(int64_t n, const int *ptr, const int *col, const double *val,
                    double *m, hipStream_t s);
int amg_spai1_short_max(void);
int amg_setup_spai1(int64_t n, const int *ptr, const int *col, const double *val,
                    double *mval, int *flag, int64_t nlong, const int *longrows, int kmax,
                    int slots, double *work, hipStream_t s);
int amg_scan_i32(int *a, int64_t n, hipStream_t s);
int amg_agg_init(int64_t n, const int *ptr, const uint8_t *S, int *id, hipStream_t s);
int amg_agg_run(int64_t n, const int *ptr, const int *col, const uint8_t *S, int *id,
                uint8_t *prov, uint64_t *m1, uint8_t *newroot, uint8_t *near,
                int *remaining, int sync_stride, int max_rounds, int *rounds_out,
                int *lists, hipStream_t s);
int amg_agg_renumber(int64_t n, int *id, int *mark, hipStream_t s);
int amg_psmooth_count(int64_t n, const int *ptr, const int *col, const uint8_t *S,
                      const int *id, int *cnt, int *overflow, hipStream_t s);
int amg_psmooth_fill(int64_t n, const int *ptr, const int *col, const double *val,
                     const uint8_t *S, const int *id, double omega,
                     const int *pptr_scanned, int *pcol, double *pval, hipStream_t s);
int amg_transpose_count(int64_t nnz, const int *col, int *tcnt, hipStream_t s);
int amg_transpose_scatter(int64_t n, const int *ptr, const int *col, const double *val,
                          int *cursor, int *tcol, double *tval, hipStream_t s);
int amg_spgemm_count(int64_t an, const int *aptr, const int *acol, const int *bptr,
                     const int *bcol, int *ub, int *cnt, int *overflow, int *bigscratch,
                     hipStream_t s);
int amg_spgemm_fill(int64_t an, const int *aptr, const int *acol, const double *aval,
                    const int *bptr, const int *bcol, const double *bval, const int *ub,
                    const int *cptr_scanned, int *ccol, double *cval, int do_sort,
                    const int *bigscratch, hipStream_t s);

// ---- driver.hip: native solve driver entry points
void *amg_driver_create(const LevelDesc *levels, int nlevels, const void *coarse_inv,
                        int64_t ncoarse, int npre, int npost, int ncycle, int pre_cycles,
                        int f32, const OpDesc *a64, hipStream_t stream);
void amg_driver_destroy(void *h);
int amg_driver_precond(void *h, const double *rhs, double *x, double *x_swap);
int amg_driver_cg(void *h, const double *rhs, double *x, double *r, double *s, double *p,
                  double *q, double *s_swap, double tol, double abstol, int maxiter,
                  int64_t *iters_out, double *resid_out);
int amg_driver_bicgstab(void *h, const double *rhs, double *x, double *r, double *p,
                        double *v, double *s2, double *t2, double *rh, double *T,
                        double *T_swap, double tol, double abstol, int maxiter,
                        int64_t *iters_out, double *resid_out);

}  // extern "C"
