/*
 * amgcore_hip -- MI355X (gfx950) native replacement for the solve-phase
 * boundary of PyAMG: the `pyamg.amg_core` relaxation kernels, scipy's
 * csr/bsr matvec at the reference's call sites, and a device-resident
 * multigrid hierarchy that runs multilevel_solver.solve() entirely in HBM.
 *
 * C ABI only: plain pointers, ints and doubles; no C++/torch types.  fp64
 * values (section 1 also float32, complex64, complex128), int32 indices (the
 * reference instantiates `int` indices only, pyamg/amg_core/amg_core.i:108).  Every function returns 0 on success or a
 * negative AMG_E* code; amg_last_error() gives the message.  Nothing here
 * falls back to the CPU: without a usable HIP device every compute entry
 * point fails with AMG_ENODEV.
 *
 * Section 1 mirrors the reference's SWIG table one-to-one (each (T*, int size)
 * pair of the C++ prototype is kept, so a binding can forward numpy arrays
 * unchanged).  All reference paths are relative to /root/reference.
 */
#ifndef AMGCORE_HIP_H
#define AMGCORE_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define AMG_OK        0
#define AMG_EINVAL   -1   /* bad argument / inconsistent sizes */
#define AMG_ENODEV   -2   /* no HIP device / HIP runtime error */
#define AMG_ENOMEM   -3
#define AMG_ESTATE   -4   /* hierarchy not finalised, level missing, ... */
#define AMG_ENOTIMPL -5

const char *amg_last_error(void);
int amg_device_count(void);
/* "gfx950:..." of the selected device, or "" */
const char *amg_device_name(int device);
/* device allocations the library made and still holds, over the whole process (buffers handed to the caller, such as
 * amg_dev_alloc's, are not counted): back at its earlier value once everything built since has been destroyed */
long amg_dev_live_buffers(void);

/* ------------------------------------------------------------------------ */
/* 1. amg_core drop-ins.  HOST pointers (numpy buffers), results written in  */
/*    place exactly like the reference; x (and temp / z) are mutated.        */
/*    Arithmetic per row is the reference's (same left-to-right sums, no     */
/*    FMA contraction); sequential sweeps are executed by dependency-level   */
/*    scheduling, which reproduces the sequential iterates bit for bit.      */
/* ------------------------------------------------------------------------ */

/* Sweep ranges.  Every sweeping entry visits `for (i = start; i != stop; i += step)` over rows, block rows,
 * positions of Id or subdomains: step may be negative, start == stop is an empty sweep that touches nothing,
 * and AMG_EINVAL (with every array untouched) answers step == 0, a range that never reaches stop, one that
 * leaves the matrix, and an Id entry outside it.  jacobi_ne alone loops `for (i = start; i < stop; i += step)`
 * and takes a positive step only.
 * temp and z are the caller's, read and written back:
 *  - jacobi and block_jacobi copy x into temp on the swept (block) rows only, read temp on every column of a
 *    swept row, so also the caller's values outside the sweep, and write x on the swept rows;
 *  - bsr_jacobi copies the prefix temp[0 .. |stop - start| * blocksize) = x[...] from index 0 whatever start
 *    is, reads the caller's temp beyond it, and takes a step >= 1 only (the reference's copy loop does not
 *    end for a negative one);
 *  - jacobi_ne zeroes temp on the swept rows, accumulates every swept row's update onto temp, onto the
 *    caller's values on columns outside the sweep, then adds temp to x on the swept rows;
 *  - gauss_seidel_nr keeps z = b - A x up to date: z is the residual going in and coming out. */

/* pyamg/amg_core/relaxation.h:33-62, called from pyamg/relaxation/relaxation.py:349 */
int amgcore_gauss_seidel_f64(const int Ap[], int Ap_size, const int Aj[], int Aj_size,
                             const double Ax[], int Ax_size, double x[], int x_size,
                             const double b[], int b_size,
                             int row_start, int row_stop, int row_step);
/* relaxation.h:89-173, relaxation.py:353 */
int amgcore_bsr_gauss_seidel_f64(const int Ap[], int Ap_size, const int Aj[], int Aj_size,
                                 const double Ax[], int Ax_size, double x[], int x_size,
                                 const double b[], int b_size,
                                 int row_start, int row_stop, int row_step, int blocksize);
/* relaxation.h:201-239, relaxation.py:416 */
int amgcore_jacobi_f64(const int Ap[], int Ap_size, const int Aj[], int Aj_size,
                       const double Ax[], int Ax_size, double x[], int x_size,
                       const double b[], int b_size, double temp[], int temp_size,
                       int row_start, int row_stop, int row_step,
                       const double omega[], int omega_size);
/* relaxation.h:267-360, relaxation.py:425 */
int amgcore_bsr_jacobi_f64(const int Ap[], int Ap_size, const int Aj[], int Aj_size,
                           const double Ax[], int Ax_size, double x[], int x_size,
                           const double b[], int b_size, double temp[], int temp_size,
                           int row_start, int row_stop, int row_step, int blocksize,
                           const double omega[], int omega_size);
/* relaxation.h:394-426, relaxation.py:739 */
int amgcore_gauss_seidel_indexed_f64(const int Ap[], int Ap_size, const int Aj[], int Aj_size,
                                     const double Ax[], int Ax_size, double x[], int x_size,
                                     const double b[], int b_size, const int Id[], int Id_size,
                                     int row_start, int row_stop, int row_step);
/* relaxation.h:465-496, relaxation.py:818 */
int amgcore_jacobi_ne_f64(const int Ap[], int Ap_size, const int Aj[], int Aj_size,
                          const double Ax[], int Ax_size, double x[], int x_size,
                          const double b[], int b_size, const double Tx[], int Tx_size,
                          double temp[], int temp_size,
                          int row_start, int row_stop, int row_step,
                          const double omega[], int omega_size);
/* relaxation.h:935-1007, relaxation.py:272-277: one sweep of multiplicative overlapping Schwarz over
 * the subdomains row_start, row_start+row_step, ... (Sj/Sp sorted index lists, Tx/Tp their inverted
 * diagonal blocks, row-major) */
int amgcore_overlapping_schwarz_csr_f64(const int Ap[], int Ap_size, const int Aj[], int Aj_size,
                                        const double Ax[], int Ax_size, double x[], int x_size,
                                        const double b[], int b_size, const double Tx[], int Tx_size,
                                        const int Tp[], int Tp_size, const int Sj[], int Sj_size,
                                        const int Sp[], int Sp_size, int nsdomains, int nrows,
                                        int row_start, int row_stop, int row_step);
/* relaxation.h:529-561, relaxation.py:907 */
int amgcore_gauss_seidel_ne_f64(const int Ap[], int Ap_size, const int Aj[], int Aj_size,
                                const double Ax[], int Ax_size, double x[], int x_size,
                                const double b[], int b_size,
                                int row_start, int row_stop, int row_step,
                                const double Tx[], int Tx_size, double omega);
/* relaxation.h:594-631, relaxation.py:995 (A in CSC) */
int amgcore_gauss_seidel_nr_f64(const int Ap[], int Ap_size, const int Aj[], int Aj_size,
                                const double Ax[], int Ax_size, double x[], int x_size,
                                double z[], int z_size,
                                int col_start, int col_stop, int col_step,
                                const double Tx[], int Tx_size, double omega);
/* relaxation.h:661-728, relaxation.py:503 */
int amgcore_block_jacobi_f64(const int Ap[], int Ap_size, const int Aj[], int Aj_size,
                             const double Ax[], int Ax_size, double x[], int x_size,
                             const double b[], int b_size, const double Tx[], int Tx_size,
                             double temp[], int temp_size,
                             int row_start, int row_stop, int row_step,
                             const double omega[], int omega_size, int blocksize);
/* relaxation.h:755-810, relaxation.py:588 */
int amgcore_block_gauss_seidel_f64(const int Ap[], int Ap_size, const int Aj[], int Aj_size,
                                   const double Ax[], int Ax_size, double x[], int x_size,
                                   const double b[], int b_size, const double Tx[], int Tx_size,
                                   int row_start, int row_stop, int row_step, int blocksize);

/* scipy.sparse._sparsetools.csr_matvec / bsr_matvec (third party) as used by
 * `A * x` at pyamg/multilevel.py:496,498,544; pyamg/util/linalg.py:112;
 * pyamg/relaxation/relaxation.py:661,666.  y is ACCUMULATED into, as scipy does. */
int amgcore_csr_matvec_f64(int n_row, int n_col, const int Ap[], const int Aj[],
                           const double Ax[], const double x[], double y[]);
int amgcore_bsr_matvec_f64(int n_brow, int n_bcol, int R, int C, const int Ap[], const int Aj[],
                           const double Ax[], const double x[], double y[]);

/* pyamg/amg_core/evolution_strength.h (called by pyamg/strength.py:658-662, 781-782, 802-803).  float64 only: the
 * measure they serve is real by the time they run.  Each is the reference's loop, operation for operation:
 * incomplete_mat_mult_csr (:675-699): Sx[ptr] = <A[row, :], B[:, col]> on the pattern of S, A and S sorted CSR,
 *   B sorted CSC; every sum starts from 0.0, takes its products in index order, multiply and add round separately.
 * apply_distance_filter (:135-167): per row, threshold = epsilon * min(off-diagonal values, from DBL_MAX); the
 *   diagonal becomes 1.0, off-diagonal values >= threshold 0.0.  apply_absolute_distance_filter (:60-83): threshold
 *   = epsilon.
 * min_blocks (:212-237): Tx[i] = smallest non-zero value of block i (blocksize values), DBL_MAX when it has none. */
int amgcore_incomplete_mat_mult_csr_f64(const int Ap[], int Ap_size, const int Aj[], int Aj_size, const double Ax[], int Ax_size,
                                        const int Bp[], int Bp_size, const int Bj[], int Bj_size, const double Bx[], int Bx_size,
                                        const int Sp[], int Sp_size, const int Sj[], int Sj_size, double Sx[], int Sx_size,
                                        int num_rows);
int amgcore_apply_distance_filter_f64(int n_row, double epsilon, const int Sp[], int Sp_size, const int Sj[], int Sj_size,
                                      double Sx[], int Sx_size);
int amgcore_apply_absolute_distance_filter_f64(int n_row, double epsilon, const int Sp[], int Sp_size, const int Sj[],
                                               int Sj_size, double Sx[], int Sx_size);
int amgcore_min_blocks_f64(int n_blocks, int blocksize, const double Sx[], int Sx_size, double Tx[], int Tx_size);

/* pyamg/amg_core/smoothed_aggregation.h, the three helpers of energy_prolongation_smoother (smooth.py:21-64, 283-457;
 * util/utils.py:1617-1707; csrc/energy.hip).  float64 only.  One lane owns one scalar of the output and adds that
 * scalar's products in the order the reference's loops reach them, multiply and add rounded separately, no atomics.
 * incomplete_mat_mult_bsr (:797-869): Sx += A * B on the block pattern of S.  A: n_brow block rows of brow_A x bcol_A
 *   blocks; B: Bp_size - 1 block rows of bcol_A x bcol_B blocks; S: brow_A x bcol_B blocks in n_bcol block columns.
 *   Rows of A, B and S in any order.  An entry of S takes jj ascending through row i of A, kk ascending through row
 *   Aj[jj] of B, the block product's inner index ascending.  A row of S that stores a column twice is reproduced as
 *   the reference has it: the later slot receives everything, the earlier slot keeps what it held.
 * satisfy_constraints_helper (:556-605): x = conj(B_c) (ColsPerBlock * NullDim values per block column), y = U * B_c
 *   (RowsPerBlock * NullDim per block row), z = BtBinv (NullDim^2 per block row); every block of S loses
 *   y_i * (z_i * x_j^T), both products from 0.0 with the inner index ascending.
 * calc_BtB (:656-734): b = the products of the candidates' columns (BsqCols = NullDim (NullDim + 1) / 2 per row of
 *   B_c); x[i] = B_i^T B_i over the scalar columns of block row i of S in stored order, from 0.0.
 * Bad offsets, columns outside the matrix, null arrays and arrays shorter than the block sizes ask for are
 * AMG_EINVAL before any launch. */
int amgcore_incomplete_mat_mult_bsr_f64(const int Ap[], int Ap_size, const int Aj[], int Aj_size, const double Ax[], int Ax_size,
                                        const int Bp[], int Bp_size, const int Bj[], int Bj_size, const double Bx[], int Bx_size,
                                        const int Sp[], int Sp_size, const int Sj[], int Sj_size, double Sx[], int Sx_size,
                                        int n_brow, int n_bcol, int brow_A, int bcol_A, int bcol_B);
int amgcore_satisfy_constraints_helper_f64(int RowsPerBlock, int ColsPerBlock, int num_block_rows, int NullDim, const double x[],
                                           int x_size, const double y[], int y_size, const double z[], int z_size, const int Sp[],
                                           int Sp_size, const int Sj[], int Sj_size, double Sx[], int Sx_size);
int amgcore_calc_BtB_f64(int NullDim, int Nnodes, int ColsPerBlock, const double b[], int b_size, int BsqCols, double x[], int x_size,
                         const int Sp[], int Sp_size, const int Sj[], int Sj_size);
/* truncate_rows_csr (smoothed_aggregation.h:898-960), float64 only, in place: every row longer than k is permuted by the
 * reference's quicksort on magnitudes (middle element to the left as pivot, strict <, column indices carried along) and
 * its first len - k entries are set to 0.0, so that among equal magnitudes the reference's choice survives.  One lane
 * per row, an explicit stack of at most 32 ranges, no per-row buffer: rows of any length. */
int amgcore_truncate_rows_csr_f64(int n_row, int k, const int Sp[], int Sp_size, int Sj[], int Sj_size, double Sx[], int Sx_size);
/* The row-parallel stages of the classical setup (amg_core/ruge_stuben.h, csrc/classical.hip), float64
 * only, one lane per row walking it in stored order:
 * classical_strength_of_connection (:46-93): Sp, Sj[:nnz], Sx[:nnz] as the reference leaves them (count, exclusive scan,
 *   stable fill).  The row maximum starts at DBL_MIN and a NaN never replaces it; the threshold is theta * max, the test >=;
 *   every stored diagonal entry is kept at its own position.  Rows in any order, duplicates allowed.
 * maximum_row_value (:110-130): x[i] = max(DBL_MIN, |a| over row i).
 * rs_direct_interpolation_pass1 (:497-516): Bp, the last offset being the number of entries of the prolongator.
 * rs_direct_interpolation_pass2 (:520-595): Bj (renumbered by the exclusive scan of splitting) and Bx; sums from +0.0 in
 *   stored order, plain divisions, only sum_strong_pos == 0 special-cased, non-finite weights stored as they come.  Bp has
 *   to be what pass 1 returns for the same S and splitting.
 * Offsets that do not start at 0 or decrease, a column outside the matrix, a splitting value other than 0 and 1 and arrays
 * shorter than the offsets ask for are AMG_EINVAL before any launch. */
int amgcore_classical_strength_of_connection_f64(int n_row, double theta, const int Ap[], int Ap_size, const int Aj[], int Aj_size,
                                                 const double Ax[], int Ax_size, int Sp[], int Sp_size, int Sj[], int Sj_size, double Sx[],
                                                 int Sx_size);
int amgcore_maximum_row_value_f64(int n_row, double x[], int x_size, const int Ap[], int Ap_size, const int Aj[], int Aj_size,
                                  const double Ax[], int Ax_size);
int amgcore_rs_direct_interpolation_pass1_f64(int n_nodes, const int Sp[], int Sp_size, const int Sj[], int Sj_size, const int splitting[],
                                              int splitting_size, int Bp[], int Bp_size);
int amgcore_rs_direct_interpolation_pass2_f64(int n_nodes, const int Ap[], int Ap_size, const int Aj[], int Aj_size, const double Ax[],
                                              int Ax_size, const int Sp[], int Sp_size, const int Sj[], int Sj_size, const double Sx[],
                                              int Sx_size, const int splitting[], int splitting_size, const int Bp[], int Bp_size, int Bj[],
                                              int Bj_size, double Bx[], int Bx_size);
/* pyamg/util/linalg.py:17-53 norm(x) (2-norm) */
int amgcore_norm2_f64(const double x[], long n, double *result);

/* The same thirteen entries for the reference's other value types (amg_core.i:139-144): suffix _f32
 * (float), _c64 (complex<float>) and _c128 (complex<double>), with the argument lists of the _f64
 * entries.  Complex values are interleaved (re, im) pairs, numpy's layout; every *_size counts
 * elements of the value type.  F is the real type of the value type: the omega of gauss_seidel_ne /
 * gauss_seidel_nr.  Rounding follows the reference's compiled kernels bit for bit. */
typedef struct { float re, im; } amg_c64;
typedef struct { double re, im; } amg_c128;

#define AMGCORE_TYPED_ENTRIES(SUF, T, F)                                                                       \
int amgcore_gauss_seidel_##SUF(const int Ap[], int Ap_size, const int Aj[], int Aj_size, const T Ax[],         \
                               int Ax_size, T x[], int x_size, const T b[], int b_size,                       \
                               int row_start, int row_stop, int row_step);                                    \
int amgcore_bsr_gauss_seidel_##SUF(const int Ap[], int Ap_size, const int Aj[], int Aj_size, const T Ax[],     \
                                   int Ax_size, T x[], int x_size, const T b[], int b_size,                   \
                                   int row_start, int row_stop, int row_step, int blocksize);                 \
int amgcore_jacobi_##SUF(const int Ap[], int Ap_size, const int Aj[], int Aj_size, const T Ax[], int Ax_size,  \
                         T x[], int x_size, const T b[], int b_size, T temp[], int temp_size,                 \
                         int row_start, int row_stop, int row_step, const T omega[], int omega_size);         \
int amgcore_bsr_jacobi_##SUF(const int Ap[], int Ap_size, const int Aj[], int Aj_size, const T Ax[],           \
                             int Ax_size, T x[], int x_size, const T b[], int b_size, T temp[],               \
                             int temp_size, int row_start, int row_stop, int row_step, int blocksize,         \
                             const T omega[], int omega_size);                                                \
int amgcore_gauss_seidel_indexed_##SUF(const int Ap[], int Ap_size, const int Aj[], int Aj_size,               \
                                       const T Ax[], int Ax_size, T x[], int x_size, const T b[],             \
                                       int b_size, const int Id[], int Id_size,                               \
                                       int row_start, int row_stop, int row_step);                            \
int amgcore_jacobi_ne_##SUF(const int Ap[], int Ap_size, const int Aj[], int Aj_size, const T Ax[],            \
                            int Ax_size, T x[], int x_size, const T b[], int b_size, const T Tx[],            \
                            int Tx_size, T temp[], int temp_size, int row_start, int row_stop,                \
                            int row_step, const T omega[], int omega_size);                                   \
int amgcore_overlapping_schwarz_csr_##SUF(const int Ap[], int Ap_size, const int Aj[], int Aj_size,            \
                                          const T Ax[], int Ax_size, T x[], int x_size, const T b[],          \
                                          int b_size, const T Tx[], int Tx_size, const int Tp[],              \
                                          int Tp_size, const int Sj[], int Sj_size, const int Sp[],           \
                                          int Sp_size, int nsdomains, int nrows,                              \
                                          int row_start, int row_stop, int row_step);                         \
int amgcore_gauss_seidel_ne_##SUF(const int Ap[], int Ap_size, const int Aj[], int Aj_size, const T Ax[],      \
                                  int Ax_size, T x[], int x_size, const T b[], int b_size,                    \
                                  int row_start, int row_stop, int row_step, const T Tx[], int Tx_size,       \
                                  F omega);                                                                   \
int amgcore_gauss_seidel_nr_##SUF(const int Ap[], int Ap_size, const int Aj[], int Aj_size, const T Ax[],      \
                                  int Ax_size, T x[], int x_size, T z[], int z_size,                          \
                                  int col_start, int col_stop, int col_step, const T Tx[], int Tx_size,       \
                                  F omega);                                                                   \
int amgcore_block_jacobi_##SUF(const int Ap[], int Ap_size, const int Aj[], int Aj_size, const T Ax[],         \
                               int Ax_size, T x[], int x_size, const T b[], int b_size, const T Tx[],         \
                               int Tx_size, T temp[], int temp_size, int row_start, int row_stop,             \
                               int row_step, const T omega[], int omega_size, int blocksize);                 \
int amgcore_block_gauss_seidel_##SUF(const int Ap[], int Ap_size, const int Aj[], int Aj_size, const T Ax[],   \
                                     int Ax_size, T x[], int x_size, const T b[], int b_size, const T Tx[],   \
                                     int Tx_size, int row_start, int row_stop, int row_step, int blocksize);  \
int amgcore_csr_matvec_##SUF(int n_row, int n_col, const int Ap[], const int Aj[], const T Ax[],               \
                             const T x[], T y[]);                                                             \
int amgcore_bsr_matvec_##SUF(int n_brow, int n_bcol, int R, int C, const int Ap[], const int Aj[],             \
                             const T Ax[], const T x[], T y[]);

AMGCORE_TYPED_ENTRIES(f32, float, float)
AMGCORE_TYPED_ENTRIES(c64, amg_c64, float)
AMGCORE_TYPED_ENTRIES(c128, amg_c128, double)

/* ------------------------------------------------------------------------ */
/* 2. Device-resident hierarchy: multilevel_solver.solve()/__solve()         */
/*    (pyamg/multilevel.py:316-548) with A_l, P_l, R_l, smoother constants   */
/*    and all work vectors in HBM.                                           */
/* ------------------------------------------------------------------------ */
typedef struct amg_hier amg_hier;

enum { AMG_FMT_CSR = 0, AMG_FMT_BSR = 1 };
enum { AMG_MAT_A = 0, AMG_MAT_P = 1, AMG_MAT_R = 2 };
enum { AMG_PRE = 0, AMG_POST = 1 };
enum { AMG_CYCLE_V = 0, AMG_CYCLE_W = 1, AMG_CYCLE_F = 2, AMG_CYCLE_AMLI = 3 };
enum { AMG_SWEEP_FORWARD = 0, AMG_SWEEP_BACKWARD = 1, AMG_SWEEP_SYMMETRIC = 2 };
/* smoother kinds = the relaxation.py entry points a smoothing.py closure calls */
enum { AMG_SM_NONE = 0, AMG_SM_JACOBI = 1, AMG_SM_GAUSS_SEIDEL = 2, AMG_SM_SOR = 3,
       AMG_SM_POLYNOMIAL = 4, AMG_SM_BLOCK_JACOBI = 5, AMG_SM_BLOCK_GAUSS_SEIDEL = 6,
       AMG_SM_GAUSS_SEIDEL_INDEXED = 7, AMG_SM_SCHWARZ = 8, AMG_SM_GAUSS_SEIDEL_NE = 9,
       AMG_SM_GAUSS_SEIDEL_NR = 10, AMG_SM_JACOBI_NE = 11 };

typedef struct {
    int kind;            /* AMG_SM_* */
    int iterations;      /* >= 1 */
    int sweep;           /* AMG_SWEEP_* (gauss_seidel, sor, block_gauss_seidel, indexed) */
    double omega;        /* jacobi / block_jacobi: omega already divided by rho; sor: omega */
    int ncoef;           /* polynomial: Horner coefficients (chebyshev: -coeffs[:-1]) */
    const double *coef;  /* host pointer, copied */
    int blocksize;       /* block_jacobi / block_gauss_seidel */
    const double *Dinv;  /* host pointer, (n/bs)*bs*bs row-major inverse diagonal blocks, copied;
                            normal-equation kinds: n entries 1/diag(A A^H) (ne, jacobi_ne) or 1/diag(A^H A) (nr) */
    const int *indices;  /* gauss_seidel_indexed: row order (host pointer, copied) */
    int nindices;
    /* schwarz (relaxation.py:172-278; level A must be CSR or BSR(1,1)): sorted subdomain index lists
     * Sj[Sp[d]..Sp[d+1]) and their inverted diagonal blocks Tx[Tp[d]..Tp[d+1]), row-major
     * (relaxation.schwarz_parameters); host pointers, copied */
    const int *Sj, *Sp, *Tp;
    const double *Tx;
    int nsdomains;
} amg_smoother_desc;

#define AMG_SM_CALLBACK 100
/* A relaxation supplied by the caller (the device-resident Krylov smoothers, pyamg/relaxation/smoothing.py:481-509):
 * called inside the cycle with DEVICE pointers to the level's iterate and right-hand side; it enqueues its work on
 * amg_hier_stream(h) (amg_hier_apply, amg_dev_*) and returns 0, or non-zero to abort the solve. */
typedef int (*amg_relax_callback)(void *user, int level, double *x_dev, const double *b_dev);
/* A coarse solver supplied by the caller (multilevel.py:642-692: Krylov names, callables): HOST vectors of the
 * coarsest level's size; x is zero on entry. */
typedef int (*amg_coarse_callback)(void *user, int n, const double *b_host, double *x_host);

/* flags for amg_hier_solve */
#define AMG_SOLVE_X0_ZERO        1  /* caller guarantees x is all zeros on entry */
#define AMG_SOLVE_NO_EARLY_STOP  2  /* run exactly maxiter cycles; residual norms stay on
                                       the device until the end (no per-iteration sync) */
#define AMG_SOLVE_DEVICE_VECTORS 4  /* b and x are DEVICE pointers */

amg_hier *amg_hier_create(int nlevels, int device);
void amg_hier_destroy(amg_hier *h);

/* Copy one operator of level `lvl` into HBM.  fmt/R/C describe the scipy
 * container (csr_matrix, or bsr_matrix with blocksize (R,C)); nrows/ncols are
 * scalar dimensions; Ax has nnz (CSR) or nblocks*R*C (BSR, blocks row-major)
 * entries.  Pointers are host pointers unless on_device != 0, in which case
 * they are device pointers (CSR / BSR(1,1) only); the arrays are copied either way. */
int amg_hier_set_matrix(amg_hier *h, int lvl, int which, int fmt, int nrows, int ncols,
                        int R, int C, const int *Ap, const int *Aj, const double *Ax,
                        int on_device);
int amg_hier_set_smoother(amg_hier *h, int lvl, int which, const amg_smoother_desc *d);
/* Block smoothers act on A re-blocked to their own blocksize
 * (pyamg/relaxation/relaxation.py:471,563: A = A.tobsr(blocksize=(bs,bs))).  When
 * level A is not already BSR(bs,bs), pass that re-blocked copy here AFTER
 * amg_hier_set_smoother; which = AMG_PRE / AMG_POST, or 2 for the coarse smoother. */
int amg_hier_set_block_matrix(amg_hier *h, int lvl, int which, int nbrows, int bs, const int *Ap,
                              const int *Aj, const double *Ax);
/* Normal-equation smoothers (relaxation.py:744-997; level A must be CSR or BSR(1,1)) work on other
 * layouts of A, passed AFTER amg_hier_set_smoother: slot 0 = A by columns (the CSC arrays: indptr over
 * columns, row indices ascending, values) for gauss_seidel_nr and jacobi_ne; slot 1 = A by rows with
 * sorted column indices, needed by gauss_seidel_nr only when the level's A has unsorted rows. */
int amg_hier_set_aux_matrix(amg_hier *h, int lvl, int which, int slot, int nmajor, int nminor,
                            const int *Ap, const int *Aj, const double *Ax);
/* coarse_grid_solver('pinv'/'pinv2'/'lu'/'cholesky'/'splu'): a dense n x n
 * row-major operator M with x = M b (multilevel.py:608-641) */
int amg_hier_set_coarse_dense(amg_hier *h, const double *M, int n);
/* coarse_grid_solver(<relaxation name>) (multilevel.py:662-680): x = 0, then the smoother */
int amg_hier_set_coarse_smoother(amg_hier *h, const amg_smoother_desc *d);
int amg_hier_set_callback_smoother(amg_hier *h, int lvl, int which, amg_relax_callback cb, void *user);
int amg_hier_set_coarse_callback(amg_hier *h, amg_coarse_callback cb, void *user);
/* y = M x for a stored operator on DEVICE vectors, enqueued on the hierarchy's stream (which = AMG_MAT_A/P/R);
 * amg_hier_apply_aux: the auxiliary operator of a smoother slot (amg_hier_set_aux_matrix: A by columns = A^T by rows) */
int amg_hier_apply(amg_hier *h, int lvl, int which, const double *x_dev, double *y_dev);
int amg_hier_apply_aux(amg_hier *h, int lvl, int which, int slot, const double *x_dev, double *y_dev);
/* device scratch of the hierarchy for the amg_dev_* reductions: AMG_DEV_SCRATCH doubles -- AMG_DEV_PARTIALS partial sums
 * of the first stage, then 8 result slots.  amg_dev_dot_host / amg_dev_norm_host put their result in
 * scratch[AMG_DEV_HOST_SLOT]; the slots before it are the hierarchy's own (AMLI step lengths, the solve's norms). */
#define AMG_DEV_PARTIALS  1024
#define AMG_DEV_SCRATCH   (AMG_DEV_PARTIALS + 8)
#define AMG_DEV_HOST_SLOT (AMG_DEV_PARTIALS + 6)
double *amg_hier_scratch(amg_hier *h);
/* allocate work vectors, build Gauss-Seidel level schedules */
int amg_hier_finalize(amg_hier *h);
/* After amg_hier_finalize: free the CSR arrays of operators whose stencil / sliced form serves every application the
 * hierarchy's cycles make of them (A_l under polynomial / Jacobi smoothers from a complete stencil form; A_l (l >= 1),
 * P_l, R_l under polynomial smoothers from a complete sliced form).  Lossless forms: same bits.  Returns the bytes
 * freed (0 for partitioned hierarchies).  Afterwards a smoother that needs the arrays cannot be attached (AMG_ESTATE). */
long amg_hier_release_sources(amg_hier *h);

/* multilevel_solver.solve(b, x0, tol, maxiter, cycle) with accel=None
 * (multilevel.py:316-471).  x holds x0 on entry and the solution on exit;
 * residuals must have room for maxiter+1 doubles; *nres = number written. */
int amg_hier_solve(amg_hier *h, const double *b, double *x, double tol, int maxiter, int cycle,
                   double *residuals, int *nres, int flags);
/* multilevel_solver.solve(b, x0, tol, maxiter, cycle, accel='cg'): conjugate gradients
 * (pyamg/krylov/_cg.py:84-179) preconditioned by one cycle from a zero guess
 * (aspreconditioner, multilevel.py:306-314), all vectors resident.  residuals (room for
 * maxiter+1) receives the preconditioner-norm history sqrt(<r,Mr>); *info = 0, or -1 when
 * an indefinite operator / preconditioner stops the iteration as in the reference. */
int amg_hier_pcg(amg_hier *h, const double *b, double *x, double tol, int maxiter, int cycle,
                 double *residuals, int *nres, int *info, int flags);
/* one multilevel_solver.__solve(0, x, b, cycle) (multilevel.py:473-548) on
 * host (flags=0) or device (AMG_SOLVE_DEVICE_VECTORS) vectors */
int amg_hier_cycle(amg_hier *h, const double *b, double *x, int cycle, int flags);
/* levels[lvl].presmoother(A, x, b) / postsmoother on host vectors */
int amg_hier_relax(amg_hier *h, int lvl, int which, const double *b, double *x);
/* read-only view of what a smoother over square blocks will run (the counterpart of amg_mat_gs_info; which = 0 / 1 for
 * the level's smoothers, 2 for the coarse smoother): fills out[0 .. min(nout, 12)) and returns the number written,
 * AMG_ESTATE when the smoother has no block schedule (block_gauss_seidel, and gauss_seidel / sor on a BSR level, after
 * amg_hier_finalize) or no block operator (block_jacobi, jacobi on a BSR level).  Fields: 0 dependency levels (0 for
 * the Jacobi kinds), 1 block size, 2 dataflow form built, 3 its blocks per lane (8 or 5), 4 its lanes per scalar row,
 * 5 its block rows per chunk, 6 its chunks, 7 its slot rows (3 .. 7: 0 without the form), 8 the level-ordered copy
 * of the streamed levels is held, 9 slices of the sliced form (the schedule's level-cut one, or the operator's for the
 * Jacobi kinds; 0: none), 10 block rows scheduled (the operator's block rows for the Jacobi kinds), 11 the longest
 * off-diagonal block count the dataflow form's builder counted (0 where it was not run or declined before counting) */
#define AMG_BLOCK_INFO_FIELDS 12
int amg_hier_block_info(amg_hier *h, int lvl, int which, int *out, int nout);
/* y = M x for a stored operator (host vectors) */
int amg_hier_matvec(amg_hier *h, int lvl, int which, const double *x, double *y);

/* bookkeeping for measurement */
/* algorithmic bytes of one cycle per SURVEY.md section 8(d) */
double amg_hier_cycle_bytes(amg_hier *h, int cycle);
/* storage form level lvl's A is applied from: 0 CSR, 1 offset-pattern, 2 stencil, 3 sliced (SELL-64-sigma) */
int amg_hier_operator_form(amg_hier *h, int lvl);
/* Value index for a level whose A is in stencil form and holds at most 255 distinct values (constant-coefficient
 * stencils): one-byte codes into a dictionary instead of the 8-byte values; the products use the same doubles, so
 * results are bit-identical.  r3: built automatically when the operator is set (amg_set_value_index(0) or
 * AMG_VALUE_INDEX=0 turns that off; an operator whose values do not compress keeps them).  This entry toggles one
 * level: on > 0 builds/enables it and returns the number of distinct values (0: not applicable, < 0: error);
 * on == 0 returns to the plain values; on < 0 queries (distinct values when in use, else 0). */
int amg_hier_value_index(amg_hier *h, int lvl, int on);
void amg_set_value_index(int on);       /* process-wide default for operators set afterwards */
int amg_value_index_enabled(void);
/* Fused level-0 smoother chains: when level 0's A is the coded 7-point stencil of a box grid
 * whose couplings stay inside the box, the hierarchy is not partitioned and both smoothers are Chebyshev of degree 2
 * (two coefficients, one iteration), the pre-smoother and the restriction's residual run as one tiled sweep, and the
 * post-smoother and the next residual norm's residual as another.  Same bits as the separate passes.
 * amg_set_level0_fusion(0) selects the separate passes (process-wide; tests); amg_hier_level0_fused says whether a
 * finalised hierarchy takes the fused path now (1) or not (0). */
void amg_set_level0_fusion(int on);
int amg_hier_level0_fused(amg_hier *h);
/* r12: a setup-time scan flags the planes of that box on which every column's code word equals the one on the plane
 * below; on those planes the chains keep the word in a register instead of loading it (the first plane of a z chunk
 * always loads).  Same bits.  amg_set_level0_plane_reuse(0) makes every plane load (process-wide; tests, default 1);
 * amg_hier_level0_plane_reuse returns the number of flagged planes, 0 when the chains are not taken or the switch is off. */
void amg_set_level0_plane_reuse(int on);
int amg_hier_level0_plane_reuse(amg_hier *h);
/* The row sums of the chains with a leading residual take a slot a row does not store (code 255) as a stored +0.0 and
 * drop the per-slot compare and selects: the sum starts at +0.0 and is never -0.0, so adding (+0.0) * operand keeps its
 * bits for every finite operand.  (The chain without a leading residual keeps the selects: it is not bound by them.)
 * An Inf or NaN next to an absent slot (a diverged iterate) spreads one row further than under the selects.
 * amg_set_level0_zero_slots(0) runs the select form (process-wide; tests and A/Bs, default 1); drops captured graphs. */
void amg_set_level0_zero_slots(int on);
/* Setup-side (replaces the host sweeps behind pyamg/aggregation/aggregation.py:313-320 `relaxation_as_linear_operator(
 * ('gauss_seidel', ...), A, 0) * B`, i.e. amg_core gauss_seidel of relaxation.h:34-62 on A x = 0): nsweeps Gauss-Seidel
 * sweeps over level lvl's operator in its own row order, from the CSR arrays in HBM; dirs[k] != 0 = descending rows;
 * b == NULL means a zero right-hand side; x (host) is updated in place; bit-identical to the sequential loop.
 * AMG_ENOTIMPL: a row of more than 8 entries, or the CSR arrays are not on the device -- keep the host sweep. */
int amg_hier_gs_natural(amg_hier *h, int lvl, double *x, const double *b, const unsigned char *dirs, int nsweeps);

/* bytes of one r = b - A x on level lvl: moved = 0 the CSR figure of SURVEY.md 8(d), 1 what the form in use streams */
double amg_hier_operator_bytes(amg_hier *h, int lvl, int moved);
/* bytes one solve() iteration needs as this library runs it: offset-pattern operators without
 * their column indices, and one level-0 application less when the outer residual is kept */
double amg_hier_cycle_bytes_moved(amg_hier *h, int cycle);
/* device time of the timed part of the last amg_hier_solve, ms (hipEvents on the solve stream) */
double amg_hier_last_solve_ms(amg_hier *h);
long amg_hier_device_bytes(amg_hier *h);
/* the hipStream_t the hierarchy launches on, as void* */
void *amg_hier_stream(amg_hier *h);
/* raw device access to level work vectors for a caller that stays on the device */
double *amg_hier_dev_x(amg_hier *h);
double *amg_hier_dev_b(amg_hier *h);

/* Stand-alone device SpMV benchmark hook: y = A x on a stored operator,
 * `reps` back-to-back launches timed with hipEvents on the hierarchy stream;
 * returns average ms per launch in *ms. */
int amg_hier_time_spmv(amg_hier *h, int lvl, int which, int mode, int reps, double *ms);
/* same for one application of a stored smoother (which = AMG_PRE / AMG_POST / 2 = coarse smoother)
 * to the level's resident vectors */
int amg_hier_time_relax(amg_hier *h, int lvl, int which, int reps, double *ms);

/* ------------------------------------------------------------------------ */
/* 3. Device-pointer API: one operator in HBM + the vector kernels on        */
/*    caller-owned DEVICE vectors and stream (hipStream_t as void*).  The    */
/*    row-partitioned multi-GPU cycle (pyamg_amd/distributed.py) is built    */
/*    from these; halos move through torch.distributed (RCCL).               */
/* ------------------------------------------------------------------------ */
typedef struct amg_mat amg_mat;
/* copies a host CSR into HBM (local rows of a partitioned operator; column indices local) */
amg_mat *amg_mat_create(int device, int nrows, int ncols, const int *Ap, const int *Aj, const double *Ax);
void amg_mat_destroy(amg_mat *m);
long amg_mat_nnz(amg_mat *m);
/* rows per workgroup of the CSR stream kernels for this operator (fixed at creation; amg_set_tile_target) */
int amg_mat_rows_per_block(amg_mat *m);
/* fraction of the entries stored with 16-bit column codes (amg_set_index16 before creation); 0 = none kept */
double amg_mat_index16_fraction(amg_mat *m);
/* storage form the operator is applied from: 0 CSR, 1 offset-pattern, 2 stencil */
int amg_mat_form(amg_mat *m);
/* one csr_stream launch.  mode: 0 out=Mx  1 out+=Mx  2 out=b-Mx  3 out=b-Mx,out2=c0*out
 * 4 out=c0*b+Mx  5 out=v2+(c0*b+Mx)  6 Jacobi (CSR rounding)  7 Jacobi (BSR(1,1) rounding);
 * xg is the gathered vector (owned entries followed by the halo) */
int amg_mat_apply(amg_mat *m, int mode, const double *xg, const double *b, const double *v2, double *out,
                  double *out2, double c0, double gscale, void *stream);   /* products are a_ij*(gscale*xg_j); 0 = 1 */
/* the same launch over rows [row_lo, row_hi) only (interior rows first, boundary rows after the halo arrived) */
int amg_mat_apply_rows(amg_mat *m, int mode, int row_lo, int row_hi, const double *xg, const double *b,
                       const double *v2, double *out, double *out2, double c0, double gscale, void *stream);
/* Gauss-Seidel over the operator's own rows (order NULL: 0..nrows-1, else an index list as for
 * gauss_seidel_indexed); columns >= nrows (halo) stay frozen: GS inside a rank, Jacobi across */
int amg_mat_build_gs(amg_mat *m, const int *order, int norder);
int amg_mat_gs_levels(amg_mat *m);
/* read-only view of the schedule amg_mat_build_gs made (the counterpart of amg_mat_form): fills out[0 .. min(nout, 12))
 * and returns the number written, AMG_ESTATE without a schedule.  Fields: 0 dependency levels, 1 chained launches,
 * 2 levels inside chains, 3 long-row chains (gs_chainl*), 4 LDS hand-off copy of the short-row chains (gs_chain2),
 * 5 its slots per row (4 / 8 / 12; 0 when it was not attempted), 6 ring codes of the long-row chains (gs_chainl2),
 * 7 dataflow form built, 8 its lanes per row, 9 its chunks, 10 the default (amg_set_gs_flow(1)) sweeps it,
 * 11 the level-ordered copy of the other paths is still held */
#define AMG_GS_INFO_FIELDS 12
int amg_mat_gs_info(amg_mat *m, int *out, int nout);
int amg_mat_gs_sweep(amg_mat *m, double *x, const double *b, int reverse, int bsr1, void *stream);
/* a whole sequence of directional sweeps (seq[k] != 0: backward) as the in-cycle smoothers issue them: the
 * dataflow form runs up to four of them per launch */
int amg_mat_gs_sweeps(amg_mat *m, double *x, const double *b, const unsigned char *seq, int nseq, int bsr1, void *stream);
int amg_dev_scale(double *out, const double *in, double c, long n, void *stream);
int amg_dev_axpy(double *x, const double *h, long n, void *stream);
int amg_dev_axpy_scaled(double *x, const double *r, double c, long n, void *stream);   /* x += c*r */
/* result_dev[0] = ||x||_2 / <x, y> by the fixed-order two-stage reduction; scratch: AMG_DEV_PARTIALS doubles that the
 * first stage overwrites; result_dev: any other device double (n == 0 gives 0.0) */
int amg_dev_norm2(const double *x, long n, double *scratch, double *result_dev, void *stream);
int amg_dev_dot(const double *x, const double *y, long n, double *scratch, double *result_dev, void *stream);
int amg_dev_dense_apply(const double *Mt, const double *b, double *x, int n, void *stream);
int amg_dev_gather(double *out, const double *in, const int *idx, long n, void *stream);
/* device-resident vectors for the Krylov methods around the cycle: allocation, copies (kind 0 H2D, 1 D2H, 2 D2D),
 * BLAS-1 updates, and reductions that return ONE scalar to the host */
double *amg_dev_alloc(long n);
void amg_dev_free(double *p);
int amg_dev_copy(double *dst, const double *src, long n, int kind, void *stream);
int amg_dev_fill(double *x, double v, long n, void *stream);
int amg_dev_axmy(double *w, const double *v, double a, long n, void *stream);          /* w -= a v */
int amg_dev_scale_add(double *p, double beta, const double *z, long n, void *stream);  /* p = beta p + z */
int amg_dev_sub(double *out, const double *a, const double *b, long n, void *stream);  /* out = a - b */
int amg_dev_divide(double *w, double a, long n, void *stream);                          /* w /= a */
int amg_dev_dot_host(const double *x, const double *y, long n, double *scratch, double *result, void *stream);
int amg_dev_norm_host(const double *x, long n, double *scratch, double *result, void *stream);

/* ------------------------------------------------------------------------ */
/* 4. Row-partitioned hierarchies: one process per GPU of a node, every level */
/*    cut into contiguous row blocks, halos pushed GPU-to-GPU over xGMI, one   */
/*    8-byte all-reduce per residual norm.  The reference   */
/*    has no distributed path; the arithmetic contract is the single-GPU cycle  */
/*    (pyamg/multilevel.py:316-548): every row keeps its stored summation order.*/
/* ------------------------------------------------------------------------ */
typedef struct amg_comm amg_comm;
/* transport 0 = "peer": arenas in fine-grained HBM mapped into every rank through HIP IPC; a hand-off is a kernel
 * that stores into the consumer's arena plus a system-scope flag, the consumer polls the flag from a one-wave kernel
 * with a wall-clock budget -- all on the hierarchy's stream, capturable in a hipGraph.
 * transport 1 = "rccl": grouped ncclSend / ncclRecv and ncclAllReduce on the same stream (librccl dlopen-ed). */
amg_comm *amg_comm_create(int rank, int world, int device, int transport);
void amg_comm_destroy(amg_comm *c);
/* declare an exchange plan: counts[dst * world + src] doubles travel from src to dst per exchange (identical matrix
 * on every rank).  Returns the channel id (>= 0). */
int amg_comm_add_channel(amg_comm *c, const int *counts);
/* fix the layout and allocate; peer transport: handle_out[64] = this rank's IPC handle, to be all-gathered */
int amg_comm_commit(amg_comm *c, unsigned char *handle_out);
/* peer transport: map the other ranks' arenas; handles = world x 64 bytes in rank order */
int amg_comm_connect(amg_comm *c, const unsigned char *handles);
/* rccl transport: rank 0 draws a 128-byte unique id (libpath NULL: "librccl.so"), every rank joins with it */
int amg_comm_rccl_unique_id(const char *libpath, unsigned char *id_out);
int amg_comm_rccl_init(amg_comm *c, const char *libpath, const unsigned char *id);
/* stand-alone use on device pointers: dst_halo <- the peers' entries (v[send_idx[k]] on their side, send_idx NULL =
 * identity); *result = sqrt(sum over ranks of *partial), added in rank order */
int amg_comm_exchange(amg_comm *c, int channel, const double *v, const int *send_idx, double *dst_halo, void *stream);
int amg_comm_allreduce_sqrt(amg_comm *c, int channel, const double *partial, double *result, void *stream);
/* peer transport: non-zero (with an error message) if some wait ran out of its budget */
int amg_comm_check(amg_comm *c);
/* Attach a communicator BEFORE the operators are set: level operators are then the rank's rows with columns
 * renumbered [owned | halo]; reduce_channel = a channel with count 1 between every pair of ranks (itself included). */
int amg_hier_set_comm(amg_hier *h, amg_comm *comm, int reduce_channel);
int amg_hier_set_partition(amg_hier *h, int lvl, int n_own, int n_halo, int channel, const int *send_idx, int i0, int i1);
int amg_hier_set_gather(amg_hier *h, int lvl, int channel, int rows);
int amg_hier_set_coarse_gather(amg_hier *h, int channel, int lo);
int amg_hier_comm_check(amg_hier *h);

/* Setup-time helper (hierarchy construction, not the cycle): Arnoldi iteration on
 * M = diag(dinv) * A_lvl (dinv NULL: M = A_lvl) as in pyamg/util/linalg.py:173-279, used for
 * the spectral-radius estimates behind omega and the Chebyshev bounds.  H is
 * (maxiter+1) x maxiter row-major on the host; the basis stays on the device. */
int amg_arnoldi(amg_hier *h, int lvl, const double *dinv, const double *v0, int maxiter,
                double breakdown_tol, double *H, int *steps, int *breakdown);
/* v = V[:, :m] @ coef (restart vector); v is a host buffer of length n */
int amg_arnoldi_combine(amg_hier *h, const double *coef, int m, double *v);
void amg_arnoldi_free(amg_hier *h);

/* replay each iteration (cycle + residual norm) from a hipGraph once its launch sequence has
 * been seen (default on; env AMG_HIP_GRAPHS=0 disables).  Speed only: same kernels, same order. */
void amg_hier_use_graphs(amg_hier *h, int on);
/* on (default): amg_hier_solve keeps the residual vector b - A x it forms for the convergence test
 * (multilevel.py:461) and a polynomial pre-smoother on level 0 starts from it instead of forming
 * the same b - A x again (relaxation.py:655).  Same bits either way; off restores the two passes. */
void amg_hier_keep_residual(amg_hier *h, int on);

/* tuning knobs (speed only): 0 = scalar loads, 1 = 16-byte loads in the CSR stream kernel;
 * XCD chunk: consecutive row blocks given to one XCD (0 = round-robin dispatch order) */
void amg_set_stream_variant(int v);
/* 1 (default): the CSR stream kernel runs as persistent workgroups that prefetch the next row block's row pointers,
 * entries and epilogue operands while they gather for the current one; 0: one row block per workgroup.  Same bits. */
void amg_set_stream_pipe(int on);
void amg_set_xcd_chunk(int c);
/* 1 (default): operators in offset-pattern form map row blocks to XCDs periodically in the slowest
 * grid axis, so one XCD's L2 serves a row's neighbours in the planes above and below; 0: chunked */
void amg_set_xcd_period(int on);
/* 1 (default): operators whose rows are subsets of one stencil of <= 32 offsets are applied from
 * the stencil form (padded values + row masks, no indices); 0: from the pattern / CSR forms */
void amg_set_stencil_form(int on);
/* stencil form: two consecutive rows per lane, every streamed operand a 16-byte access (half the vector-memory
 * instructions for the same bytes): 1 (default) for launches of 30 M rows and more with stencils of up to 7 offsets
 * (where it is measured faster), 2 always, 0 never (one row per lane).  Same bits. */
void amg_set_stencil_pairs(int on);
/* operators without grid structure (Galerkin operators, restriction): 1 (default) whole-operator applications run from
 * the sliced form (rows sorted by length in windows of 256 -- restrictions 64 --, slices of 64 rows stored entry-major: one lane per row,
 * no row pointer, no LDS); 0: from CSR.  Same bits. */
void amg_set_sell_form(int on);
/* the sliced form's column indices as 16-bit window codes (two per word, 16 window origins per slice; slices whose
 * columns need more windows keep their 32-bit indices): 1 (default) built with the form and read by the kernel,
 * 0: 32-bit indices.  10 B per stored entry instead of 12; same columns, same order, same bits. */
void amg_set_sell_index16(int on);
/* runs of narrow Gauss-Seidel dependency levels are swept by one workgroup in one launch: 2 (default) the sweep runs
 * in level-order numbering, new values are handed from level to level through LDS and everything else is requested
 * two levels ahead; 1 operands gathered back from L2 after each barrier (also what index lists and partitioned
 * levels use); 0: one launch per level.  Same bits. */
void amg_set_gs_chain(int on);
/* levels too wide for a chain, one launch each: 1 (default) the launch's workgroups get their entry ranges in the kernel
 * arguments (gs_level_kernel: two memory round trips per launch), 0 the general stream kernel (three) */
void amg_set_gs_level_hint(int on);
/* Gauss-Seidel sweeps (pyamg/amg_core/relaxation.h:34-62, :90-173 with 1x1 blocks) as ONE persistent launch per
 * smoother application ("dataflow" form, csrc/gsflow.hip): rows wait for their own operands instead of for a
 * dependency level.  1 (default): schedules whose levels would otherwise be launches of their own or long-row chains
 * (3-D operators, coarse levels of smoothed-aggregation hierarchies); 2: every schedule the form exists for; 0: never
 * (level launches and chained sweeps).  Read when a schedule is built and when it is swept.  Same bits. */
void amg_set_gs_flow(int mode);
/* look-ahead of the dataflow sweep in dependency levels (resident waves = look-ahead x average chunks per level);
 * 0: the default (4) */
void amg_set_gs_flow_lookahead(int levels);
/* host-synchronous: nonzero when a wave of a dataflow sweep gave up waiting (4 s budget) since the last call -- the
 * iterates of that sweep are then unusable.  amg_hier_solve checks it before it returns. */
int amg_gs_flow_status(void);
/* A of a BSR(bs,bs) level can be applied straight from its blocks (8 B per entry + 4 B per block) instead
 * of from the CSR expansion (12 B per entry); same summation order, same bits.  0: never, 1 (default):
 * for blocks of 3x3 and larger (where it is measured faster), 2: always */
void amg_set_bsr_spmv(int on);
/* 1: operators uploaded from now on also get 16-bit column codes (row blocks whose columns fit 16
 * windows of 4096) and the stream kernel reads those; 0 (default): always the 32-bit indices.
 * Lossless; off by default because the measured gain is within +-8 % per operator */
void amg_set_index16(int on);
/* products per workgroup aimed at when choosing rows per workgroup (default 2048 = one LDS tile) */
void amg_set_tile_target(int t);

/* ---- setup on the device: Galerkin products -------------------------------------------------------------------
 * Ac = (R * A) * P with scipy's csr_matmat arithmetic and output order (what pyamg/aggregation/aggregation.py:425-426
 * computes as R * A * P): per output row the products accumulate in the order (entry of the left row, entry of the
 * right row), columns come out in reverse first-touch order, exact zeros are dropped -- bit-identical to scipy.
 * A is level `level` of a hierarchy handle that already holds it in HBM as CSR (the handle behind the setup-time
 * spectral-radius estimate); R, P are host CSR arrays with 64-bit row pointers.  Cp receives n_coarse + 1 offsets;
 * amg_galerkin_fetch copies the Cp[n_coarse] columns / values to the host and releases the product.
 * A fetch of a product with entries into null arrays is AMG_EINVAL and releases it all the same.
 * AMG_EINVAL (nothing left allocated) when the operator is not held as CSR or the device tables would not fit: a row
 * that outgrows the tables in LDS and has more than 2^22 products (the memory guard of csrc/spgemm.hip). */
typedef struct amg_galerkin amg_galerkin;
int amg_hier_galerkin(amg_hier *h, int level, int n_coarse, const int64_t *Rp, const int *Rj, const double *Rx,
                      const int64_t *Pp, const int *Pj, const double *Px, int64_t *Cp, amg_galerkin **out);
int amg_galerkin_fetch(amg_galerkin *g, int *Cj, double *Cx);
/* C = A * B for host CSR operands through the same kernels (n_row x n_inner times n_inner x n_col).
 * Every product entry of this section requires of its RIGHT-hand operands (B here; A and P of a Galerkin product) that a
 * row holds each column once: the lanes of a group take the entries of a right-hand row side by side and two entries
 * with one column would lose a product.  Left-hand rows may repeat columns, and no operand needs sorted rows.  The
 * callers in the package hand operators they did not build to the host product when they hold duplicates. */
int amg_csr_matmat_device(int n_row, int n_inner, int n_col, const int64_t *Ap, const int *Aj, const double *Ax,
                          const int64_t *Bp, const int *Bj, const double *Bx, int64_t *Cp, amg_galerkin **out);
/* The same products for complex128 operands (values as interleaved (real, imaginary) pairs of doubles), scipy's complex
 * csr_matmat bit for bit: each product is (ar br - ai bi, ar bi + ai br) without contraction, every output entry
 * accumulates from zero in traversal order, part by part, and is dropped only when BOTH parts are zero of either sign
 * (an entry whose real part cancels exactly keeps its zero as computed).  Device tables hold 2048 entries per wave
 * (24 bytes each) where the float64 ones hold 4096; the overflow tiers are the same and end in AMG_EINVAL.
 * amg_csr_matmat_device_c128: C = A * B.  amg_galerkin_device_c128: (R * A) * P from three host CSR operands
 * (R n_coarse x n_fine, A n_fine x n_fine, P n_fine x n_coarse); R * A never leaves HBM.  Both fill Cp and leave the
 * product in *out; amg_galerkin_fetch_c128 copies its columns and values to the host and releases it (the float64
 * fetch refuses a complex product and the other way round). */
int amg_csr_matmat_device_c128(int n_row, int n_inner, int n_col, const int64_t *Ap, const int *Aj, const void *Ax,
                               const int64_t *Bp, const int *Bj, const void *Bx, int64_t *Cp, amg_galerkin **out);
int amg_galerkin_device_c128(int n_fine, int n_coarse, const int64_t *Rp, const int *Rj, const void *Rx,
                             const int64_t *Ap, const int *Aj, const void *Ax,
                             const int64_t *Pp, const int *Pj, const void *Px, int64_t *Cp, amg_galerkin **out);
int amg_galerkin_fetch_c128(amg_galerkin *g, int *Cj, void *Cx);
/* What the calling thread's most recent product (one A * B of the entries above; of a Galerkin product the last one
 * that ran) did, as AMG_SPGEMM_ROUTE_FIELDS ints; the first min(n, AMG_SPGEMM_ROUTE_FIELDS) are copied to out and the
 * number of fields is returned:
 *   0  value type: 0 float64, 1 complex128
 *   1  lanes per output row first tried (8, 16, 32 or 64; 0 for a product without rows)
 *   2  lanes per output row that produced the result (1: one thread per row; 0: no kernel ran to the end)
 *   3  where the tables lived: 0 no kernel (a product without rows), 1 LDS, 2 HBM, a table per wave, 3 HBM, a table per
 *      thread, 4 refused (AMG_EINVAL: the caller's host product)
 *   4  table entries per row (per thread: of the first tier; refused: what the longest row's products would have needed)
 *   5  workgroups of the launches that produced the result (per thread: of the first tier)
 *   6  rows redone in the second tier of the per-thread tables */
#define AMG_SPGEMM_ROUTE_FIELDS 7
int amg_spgemm_last_route(int *out, int n);

/* Evolution strength of connection (pyamg/strength.py:433-816) for a real operator and ONE candidate vector, every
 * stage in HBM (csrc/strength.hip).  A: n x n CSR on the host with sorted rows, no duplicates and
 * no stored zeros (64-bit offsets); b: the candidate; rho: the spectral-radius estimate of Dinv A; k = 1, 2, 4, ...
 * (AMG_ENOTIMPL otherwise); symmetrize: 0.5 (S + S^T) before the unit diagonal.  On return Cp (n + 1 offsets) is
 * filled and *out holds the measure; amg_strength_fetch copies its columns and values (Cp[n] each) to the host and
 * releases it.  Same bits and stored order as the reference's sequence given the same rho.  times_ms (or NULL)
 * receives the milliseconds of the upload [0] and of the stages [1]. */
typedef struct amg_strength amg_strength;
int amg_evolution_strength_device(int n, const int64_t *Ap, const int *Aj, const double *Ax, const double *b, double rho,
                                  double epsilon, int k, int symmetrize, int64_t *Cp, amg_strength **out, double *times_ms);
int amg_strength_fetch(amg_strength *s, int *Cj, double *Cx);

/* CG energy minimisation of a tentative prolongator (smooth.py:283-457) for a real operator, the whole iteration in HBM
 * (csrc/energy.hip).  A: n_brow x n_brow blocks of R x R (BSR on the host).  Sp/Sj: the fixed
 * pattern, n_brow x n_bcol blocks of R x Cc, rows sorted and unique (AMG_EINVAL otherwise).  Tx: the tentative
 * prolongator's values on that pattern; Bc: the coarse candidates (n_bcol * Cc rows of ND values); BtBinv: ND x ND per
 * block row; Dinv: one weight per scalar row.  Up to maxiter iterations; stops when <R, Z> < tol or R holds no
 * non-zero.  *out then holds the result: amg_energy_fetch copies its values (on the pattern) to the host and releases
 * it.  *iterations (or NULL): finished iterations.  trace (or NULL, else 2 * maxiter doubles): <R, Z> and <P, AP> of
 * every started iteration.  times_ms (or NULL): milliseconds of the upload [0] and of the iterations [1]. */
typedef struct amg_energy amg_energy;
int amg_energy_smooth_device(int n_brow, int n_bcol, int R, int Cc, int ND, const int *Ap, const int *Aj, const double *Ax,
                             const int *Sp, const int *Sj, const double *Tx, const double *Bc, const double *BtBinv,
                             const double *Dinv, int maxiter, double tol, amg_energy **out, int *iterations, double *trace,
                             double *times_ms);
/* The same iteration with the root-node rules (smooth.py:1129-1146 and :443-445).  root_row:
 * n_bcol entries, the block row of column j's root node; the roots must be distinct and in range, R == Cc, and the
 * pattern's row at each root must hold exactly one block, column j (AMG_EINVAL otherwise, before any launch).  Bf (or
 * NULL: no initial fit): the fine candidates, n_brow * R rows of ND values; with it T <- T - (T B_c - B_f) BtBinv B_c^T
 * runs on the pattern first.  The root blocks of T are set to the identity after the fit and after every
 * T += alpha P; R, Z, P and AP are not masked.  Result handle and amg_energy_fetch as above. */
int amg_energy_smooth_rootnode_device(int n_brow, int n_bcol, int R, int Cc, int ND, const int *Ap, const int *Aj, const double *Ax,
                                      const int *Sp, const int *Sj, const double *Tx, const double *Bc, const double *BtBinv,
                                      const double *Dinv, const int *root_row, const double *Bf, int maxiter, double tol,
                                      amg_energy **out, int *iterations, double *trace, double *times_ms);
int amg_energy_fetch(amg_energy *h, double *Tx);

/* The parallel C/F splittings of the classical setup (csrc/split.hip); graphs are CSR on the host
 * with 32-bit offsets from 0 and columns inside the graph (AMG_EINVAL otherwise, before any launch).
 *
 * amg_mis_device: Luby's maximal independent set run to completion (amg_core/graph.h:90-156, max_iters == -1) on the
 * graph as handed in.  x: one state per vertex; entries other than `active` keep their value, an active vertex next to
 * a C entry becomes F, the others are decided by (y, index), the larger index winning a tie.  On a structurally
 * symmetric graph the result equals the reference's sweeps.  *rounds (or NULL): rounds run.
 *
 * amg_cljp_device: the CLJP selection loop (amg_core/ruge_stuben.h:373-478) on the start weights weight0 (the random
 * or colour weights plus the in-degree, computed on the host).  T = S^T.  splitting: 1 = C, 0 = F.  *passes (or
 * NULL): passes run.
 *
 * times_ms (or NULL): milliseconds of the upload [0], of the rounds or passes [1] and of the download [2]. */
int amg_mis_device(int n, const int *Ap, const int *Aj, const double *y, int active, int C, int F, int *x, int *rounds,
                   double *times_ms);
int amg_cljp_device(int n, const int *Sp, const int *Sj, const int *Tp, const int *Tj, const double *weight0, int *splitting,
                    int *passes, double *times_ms);

/* The distance-k independent set and the MIS(2) aggregation (csrc/misagg.hip); graphs as above.
 *
 * amg_mis_k_device: maximal_independent_set_k_parallel (amg_core/graph.h:501-589) on the graph as handed in, which need
 * not be symmetric: x (n ints, written) is 1 for the members and 0 for the others after at most max_iters rounds (-1:
 * until no vertex is active).  k >= 1; y: n finite weights, the larger index winning a tie.  AMG_ESTATE when more than
 * n rounds leave work (weights at or below -1, on which the reference does not end either).
 *
 * amg_mis_aggregation_device: the aggregation of section 8l on a structurally symmetric graph (the caller's check): the
 * set with k = 2, its members with an off-diagonal entry as roots, numbered in ascending order, and the two attachment
 * rounds.  agg (n ints): the aggregate of every vertex, -1 for a vertex without off-diagonal entries; cpts (room for n
 * ints): the *n_agg roots, ascending.
 *
 * *rounds (or NULL): rounds of the set.  times_ms (or NULL): milliseconds of the upload [0], of everything that runs in
 * HBM [1] and of the download [2]. */
int amg_mis_k_device(int n, const int *Ap, const int *Aj, int k, const double *y, int max_iters, int *x, int *rounds, double *times_ms);
int amg_mis_aggregation_device(int n, const int *Ap, const int *Aj, const double *y, int *agg, int *cpts, int *n_agg, int *rounds,
                               double *times_ms);

/* The smoothed-aggregation stages around the aggregation (csrc/prolong.hip), real float64; matrices
 * are CSR on the host with 32-bit offsets from 0 and columns inside the matrix (AMG_EINVAL otherwise, before any launch).
 *
 * amg_symmetric_strength_device: symmetric_strength_of_connection of an n x n operator whose rows may be unsorted, hold
 * a column more than once, lack a diagonal entry or be empty.  d_i: the sum of row i's diagonal entries in stored order;
 * an entry is kept when it is on the diagonal or a*a >= ((theta*theta) * |d_i|) * |d_j|; the kept entries, in stored
 * order, become magnitudes divided by the row's largest one (by 1 where that is 0).  Sp (n + 1 offsets) is filled and
 * *out holds the columns and values; amg_symmetric_strength_fetch copies them (Sp[n] each) and releases the result, also
 * when it fails.
 *
 * amg_fit_candidates_device: the tentative prolongator of fit_candidates (amg_core/smoothed_aggregation.h:323-452).
 * Tp, Tj: AggOp (n_fine x n_coarse, at most one entry per row; a node without one is unaggregated); B: n_fine blocks of
 * K1 x K2 candidates, row-major.  Per aggregate, modified Gram-Schmidt over the K1 rows of each of its members in
 * ascending node order, every norm and dot product a sequential sum from zero, the threshold tol * norm taken before the
 * orthogonalisation.  Tx (Tp[n_fine] blocks of K1 x K2, block k that of the node whose entry is number k of AggOp) and R
 * (n_coarse blocks of K2 x K2) are written.
 *
 * amg_jacobi_prolongation_device: P = T, then `degree` times P <- P - W * P with W_ik = (S_ik * dinv_i) * w, the
 * products by the routes of amg_csr_matmat_device, the difference with the entry order and the dropped zeros of scipy's
 * csr_minus_csr.  S: n x n; T: n x n_coarse, no column twice in a row (AMG_EINVAL); dinv: n
 * values.  AMG_ENOTIMPL where a product route refuses.  Pp (n + 1 offsets) is filled and *out holds the columns and
 * values for amg_jacobi_prolongation_fetch (Pp[n] each), which releases the result, also when it fails.
 *
 * times_ms (or NULL, three doubles): milliseconds of the upload [0] and of everything that runs in HBM [1], written by
 * the stage entry, and of the download [2], written by amg_fit_candidates_device itself and by the two fetch entries. */
typedef struct amg_prolong amg_prolong;
int amg_symmetric_strength_device(int n, const int *Ap, const int *Aj, const double *Ax, double theta, int *Sp, amg_prolong **out,
                                  double *times_ms);
int amg_symmetric_strength_fetch(amg_prolong *h, int *Sj, double *Sx, double *times_ms);
int amg_fit_candidates_device(int n_fine, int n_coarse, int K1, int K2, const int *Tp, const int *Tj, const double *B, double tol,
                              double *Tx, double *R, double *times_ms);
int amg_jacobi_prolongation_device(int n, int n_coarse, const int *Sp, const int *Sj, const double *Sx, const double *dinv, double w,
                                   int degree, const int *Tp, const int *Tj, const double *Tx, int *Pp, amg_prolong **out,
                                   double *times_ms);
int amg_jacobi_prolongation_fetch(amg_prolong *h, int *Pj, double *Px, double *times_ms);

/* One level of the classical setup in HBM from one upload of A (csrc/classical.hip): classical
 * strength with theta, the strength graph without its diagonal with its transpose's pattern and the in-degrees, the start
 * weights, the splitting (kind 0: PMIS, Luby's rounds on S + S^T with double(in-degree) + r; kind 1: CLJP, r then + 1.0 per
 * dependent), and direct interpolation on S's pattern with the values the strength stage wrote.  A: n x n CSR on the host,
 * n > 0; r: n start values in [0, 1) from the host.  reversed != 0: interpolation walks every row of S from its last
 * entry to its first, sums and entries of P alike (the order in which the host route meets S when the rows of A are not
 * sorted); A's rows are walked as stored either way.  On return *out holds the result, sizes[0] the entries of S, sizes[1]
 * the entries of P, *rounds (or NULL) the rounds or passes of the splitting.  amg_classical_level_fetch copies splitting (n),
 * Pp (n + 1), Pj and Px (sizes[1] each, Pj in coarse numbering) and, where Sp is not NULL, Sp (n + 1), Sj and Sx (sizes[0]
 * each, Sx as |S| with every row divided by its largest entry) to the host and releases the result, also when it fails.
 * times_ms (or NULL): milliseconds of the upload [0], strength [1], graph and weights [2], splitting [3] and interpolation
 * [4]; the fetch writes the same five and its own time [5]. */
typedef struct amg_classical amg_classical;
int amg_classical_level_device(int n, const int *Ap, const int *Aj, const double *Ax, double theta, int kind, int reversed,
                               const double *r, amg_classical **out, long *sizes, int *rounds, double *times_ms);
int amg_classical_level_fetch(amg_classical *h, int *splitting, int *Pp, int *Pj, double *Px, int *Sp, int *Sj, double *Sx,
                              double *times_ms);
/* The same level with the interpolation chosen: interpolation 0 is direct interpolation (amg_classical_level_device is this
 * entry with 0, 0), 1 is extended+i (below) on the pattern of S in the order the strength stage stored it, whatever
 * `reversed` says, truncated to max_per_row entries per row where that is > 0.  With extended+i a column stored twice in a
 * row of A is AMG_EINVAL before any launch.  The result is fetched with amg_classical_level_fetch. */
int amg_classical_level_build(int n, const int *Ap, const int *Aj, const double *Ax, double theta, int kind, int reversed,
                              const double *r, int interpolation, int max_per_row, amg_classical **out, long *sizes, int *rounds,
                              double *times_ms);

/* R = P^T for a float64 CSR matrix P (n_row x n_col, host arrays, 32-bit offsets) with the bits and the order of scipy's
 * P.T.tocsr() (csr_tocsc, DESIGN.md section 8k, csrc/transpose.hip): row c of R holds the entries of column c of P in the
 * order in which a walk over P's stored arrays meets them -- ascending row of P, and within a row of P the stored order.
 * A column stored twice in a row stays two entries in that order; nothing is summed, dropped or sorted by value; values
 * are copied bit for bit; an empty column gives repeated offsets; the rows of P may be stored in any order.  On return
 * Rp (n_col + 1 offsets) is filled and *out holds the columns and values; amg_csr_transpose_fetch copies them (Rp[n_col]
 * each) to the host and releases the result, also when it fails or is handed NULL arrays.  Offsets that do not start at
 * 0 or decrease and a column outside [0, n_col) are AMG_EINVAL before any launch, with Rp untouched.  Without rows or
 * without entries the result is empty and nothing is launched.
 * amg_transpose_last_route: what the calling thread's most recent transpose (this entry or a chain level) did, as
 * AMG_TRANSPOSE_ROUTE_FIELDS ints: [0] 1 where kernels ran, [1] the rows of R ordered by one lane each (at most 32
 * entries, empty rows included), [2] by one wave with the row in LDS (at most 2048), [3] by one workgroup on the row's
 * keys in HBM (longer).  Returns the number of fields. */
typedef struct amg_transpose amg_transpose;
int amg_csr_transpose_device(int n_row, int n_col, const int *Pp, const int *Pj, const double *Px, int *Rp, amg_transpose **out);
int amg_csr_transpose_fetch(amg_transpose *h, int *Rj, double *Rx);
#define AMG_TRANSPOSE_ROUTE_FIELDS 4
int amg_transpose_last_route(int *out, int n);

/* A chain of classical levels that stays in HBM: one upload of A_0, then per level one call that
 * builds it and one that downloads what the host hierarchy keeps.
 *
 * amg_classical_chain_begin validates A_0 (n x n, n > 0, as amg_classical_level_build does, and no column twice in a
 * row) and uploads it as the chain's resident operator.  reversed: as in amg_classical_level_device.
 *
 * amg_classical_chain_level builds the level of the resident operator exactly as amg_classical_level_build does
 * (theta, kind, r: n start values from the host, interpolation, max_per_row), then R = P^T by the transpose above,
 * R * A and A_c = (R * A) * P by the routes of amg_csr_matmat_device; R * A is released.  sizes (5 longs): the entries
 * of S [0], P [1], R [2] and A_c [3] and the coarse size [4].  flags (AMG_CHAIN_FLAG_FIELDS ints): [0] 1 where every
 * row of A_c is strictly ascending, [1] 1 where every value of A_c is finite -- both from one pass over A_c in HBM --
 * [2] and [3] the tables (field 3 of amg_spgemm_last_route) of R * A and of (R * A) * P, [4 .. 7] the fields of
 * amg_transpose_last_route.  *rounds (or NULL): the rounds or passes of the splitting.  times_ms (or NULL, AMG_CHAIN_STAGES
 * doubles): upload [0] (A_0 with the first level, r with every level), strength [1], graph and weights [2], splitting
 * [3], interpolation [4], transpose [5], the two products and the pass over A_c [6]; the fetch writes the same seven and
 * its own time [7].  Returns 0, or AMG_CHAIN_PRODUCT_REFUSED where a product was refused (a row of more than 2^22
 * products on a level too large for per-thread tables, or 2^31 entries or more): the level then holds its splitting, P
 * and S only, sizes[3] is 0 and flags[0], flags[1] are 0.  A non-finite value of A_c is no error of this level: it is
 * reported in flags[1] and the caller decides about the next one.  Any other return is an error and leaves the chain
 * without a level, its resident operator as it was.
 *
 * amg_classical_chain_fetch copies the level just built to the host: splitting (n), Pp (n + 1), Pj, Px (sizes[1]), Rp
 * (sizes[4] + 1), Rj, Rx (sizes[2]), Cp (sizes[4] + 1), Cj, Cx (sizes[3]) and, where Sp is not NULL, Sp, Sj, Sx as
 * amg_classical_level_fetch does.  It then makes A_c the resident operator (the next level runs with reversed = 0 where
 * flags[0] was 1, with 1 otherwise) and releases the level's other buffers.  Rp NULL: R is not copied; Cp NULL: A_c is not
 * copied (it becomes the resident operator all the same).  After AMG_CHAIN_PRODUCT_REFUSED the R and C
 * arrays are not read (NULL will do) and the chain is left without an operator: the caller forms the coarse operator on
 * the host and begins another chain.  A failing fetch, one with a NULL splitting or Pp included, releases the level and keeps the
 * operator the chain had.
 *
 * amg_classical_chain_free releases the chain with everything it holds (NULL: nothing). */
typedef struct amg_classical_chain amg_classical_chain;
#define AMG_CHAIN_FLAG_FIELDS 8
#define AMG_CHAIN_STAGES 8
#define AMG_CHAIN_PRODUCT_REFUSED 1
int amg_classical_chain_begin(int n, const int *Ap, const int *Aj, const double *Ax, int reversed, amg_classical_chain **out);
int amg_classical_chain_level(amg_classical_chain *chain, double theta, int kind, const double *r, int interpolation, int max_per_row,
                              long *sizes, int *flags, int *rounds, double *times_ms);
int amg_classical_chain_fetch(amg_classical_chain *chain, int *splitting, int *Pp, int *Pj, double *Px, int *Rp, int *Rj, double *Rx,
                              int *Cp, int *Cj, double *Cx, int *Sp, int *Sj, double *Sx, double *times_ms);
void amg_classical_chain_free(amg_classical_chain *chain);

/* A chain of MIS(2) smoothed-aggregation levels that stays in HBM (csrc/prolong.hip): one upload
 * of A_0 and of its one candidate B_0, then per level one call that builds it and one that downloads what the host
 * hierarchy keeps.  Real float64, scalar unknowns, one candidate.
 *
 * amg_sa_chain_begin validates A_0 (n x n, n > 0, no column twice in a row: AMG_EINVAL; a value that is not finite:
 * AMG_ENOTIMPL) and uploads it with B (n values) as the chain's resident operator and candidate.
 *
 * amg_sa_chain_level builds the level of the resident operator (n: its rows as the caller has them, the length of y,
 * dinv and B; another size is AMG_EINVAL before anything is read): symmetric strength with theta on the operator as it is
 * stored (strength_mode AMG_SA_STRENGTH_CSR: amg_symmetric_strength_device's; _SQUARED: the same on the values a*a, one
 * rounding, what the host makes of a BSR operator with 1 x 1 blocks; _ONES: the whole pattern in stored order with every
 * value 1.0, the host's answer for such an operator with theta == 0); a check that the pattern of S is structurally
 * symmetric (AMG_EINVAL "expected a structurally symmetric pattern" otherwise); MIS(2) aggregation on y (n finite
 * weights); AggOp from the aggregate of every vertex; the tentative prolongator T and the coarse candidate B_c with tol;
 * the rows of the operator sorted by column, where they are not sorted already; `degree` Jacobi steps P <- P - W P with
 * W_ik = (A_ik * dinv_i) * w on the sorted operator; R = P^T; R * A and A_c = (R * A) * P on the sorted operator; one
 * pass over A_c for its facts.  B (or NULL): n values that replace the resident candidate first.
 * sizes (5 longs): the entries of S [0], T [1], P [2] and A_c [3] and the coarse size [4].  flags
 * (AMG_SA_CHAIN_FLAG_FIELDS ints): [0] 1 where every row of A_c is strictly ascending, [1] 1 where every value of A_c
 * is finite, [2] 1 where the pattern of S is symmetric, [3] why the level stopped after the aggregation or in the
 * smoothing (0: it did not, AMG_SA_NO_AGGREGATE: MIS(2) found no aggregate, AMG_SA_SMOOTHING_REFUSED: a product of the
 * smoothing was refused), [4] and [5] the tables of R * A and of (R * A) * P, [6 .. 9] the fields of
 * amg_transpose_last_route.  *rounds (or NULL): the rounds of the independent set.  times_ms (or NULL,
 * AMG_SA_CHAIN_STAGES doubles): upload [0], strength [1], symmetry check, aggregation and AggOp [2], tentative
 * prolongator [3], row sort [4] (exactly 0 where the rows were sorted already), smoothing [5], transpose [6], the two products and the pass over A_c [7]; the fetch
 * writes the same eight and its own time [8].  Returns 0, or AMG_CHAIN_PRODUCT_REFUSED where a Galerkin product was
 * refused: the level then holds P and B_c (and S, the aggregates and T for a caller that keeps them).  A second call
 * before the fetch is AMG_ESTATE.  Any other return is an error and leaves the chain without a level, its resident
 * operator and candidate as they were.
 *
 * amg_sa_chain_fetch copies the level to the host: Pp (n + 1), Pj, Px (sizes[2]), Rp (sizes[4] + 1), Rj, Rx (sizes[2]),
 * Cp (sizes[4] + 1), Cj, Cx (sizes[3]), Bc (sizes[4]) and, where they are not NULL, Sp (n + 1), Sj, Sx (sizes[0]), agg
 * (n, -1: no aggregate) and Tx (sizes[1]).  A_c (in the order of the product) and B_c then become the resident operator
 * and candidate.  With Rp or Cp NULL a built level is fetched like one
 * whose product was refused: its caller forms the coarse operator itself.  After AMG_CHAIN_PRODUCT_REFUSED the R and C arrays are not read; after a level that stopped
 * (flags[3]) only Sp, Sj, Sx are, and they are required; either way the chain is left without an operator.  A failing
 * fetch releases the level and keeps the operator the chain had.
 *
 * amg_sa_chain_free releases the chain with everything it holds (NULL: nothing). */
typedef struct amg_sa_chain amg_sa_chain;
#define AMG_SA_CHAIN_FLAG_FIELDS 10
#define AMG_SA_CHAIN_STAGES 9
#define AMG_SA_STRENGTH_CSR 0
#define AMG_SA_STRENGTH_SQUARED 1
#define AMG_SA_STRENGTH_ONES 2
#define AMG_SA_NO_AGGREGATE 1
#define AMG_SA_SMOOTHING_REFUSED 2
int amg_sa_chain_begin(int n, const int *Ap, const int *Aj, const double *Ax, const double *B, amg_sa_chain **out);
int amg_sa_chain_level(amg_sa_chain *chain, int n, double theta, int strength_mode, const double *y, const double *dinv, double w, int degree,
                       const double *B, double tol, long *sizes, int *flags, int *rounds, double *times_ms);
int amg_sa_chain_fetch(amg_sa_chain *chain, int *Pp, int *Pj, double *Px, int *Rp, int *Rj, double *Rx, int *Cp, int *Cj, double *Cx,
                       double *Bc, int *Sp, int *Sj, double *Sx, int *agg, double *Tx, double *times_ms);
void amg_sa_chain_free(amg_sa_chain *chain);

/* Extended+i (distance-two) interpolation (csrc/classical.hip) from a float64 CSR operator A, the
 * pattern of a strength matrix S of A's shape and a C/F splitting (1 = C, 0 = F), all on the host with 32-bit offsets;
 * rows in any stored order.  An F row interpolates from C_hat, its strong C neighbours and those of its strong F
 * neighbours, with the sign-filtered row sums of section 8j; every sum in the order stated there, so the result has the
 * bits of the host route (amgsetup_extended_interpolation_*).  max_per_row > 0: rows of more finite entries keep the
 * max_per_row of largest magnitude (ties: the smaller column), rescaled to the row sum; 0: no truncation.  On return Pp
 * (n + 1 offsets) is filled and *out holds the columns (coarse numbering, ascending per row) and values;
 * amg_extended_interpolation_fetch copies them (Pp[n] each) to the host and releases the result, also when it fails.
 * Offsets that do not start at 0 or decrease, a column outside the matrix, a column stored twice in a row of A or S,
 * a splitting value other than 0 and 1 and a negative max_per_row are AMG_EINVAL before any launch, with Pp untouched.
 * times_ms (or NULL): milliseconds of the upload [0] and of the stages [1]. */
typedef struct amg_interpolation amg_interpolation;
int amg_extended_interpolation_device(int n, const int *Ap, const int *Aj, const double *Ax, const int *Sp, const int *Sj,
                                      const int *splitting, int max_per_row, int *Pp, amg_interpolation **out, double *times_ms);
int amg_extended_interpolation_fetch(amg_interpolation *h, int *Pj, double *Px);

/* ------------------------------------------------------------------------ */
/* 5. Resident hierarchies of other value types: the cycle of section 2      */
/*    (multilevel.py:316-556) for a hierarchy whose A_l, P_l, R_l hold       */
/*    complex128 values.  Eager launches on plain CSR / BSR forms.           */
/* ------------------------------------------------------------------------ */
/* Value types of a hierarchy.  Only AMG_VALUE_C128 is implemented; the others return AMG_ENOTIMPL.
 * complex128 values are pairs of doubles (real, imaginary), like amg_c128 and numpy's complex128. */
#define AMG_VALUE_F64  0
#define AMG_VALUE_F32  1
#define AMG_VALUE_C64  2
#define AMG_VALUE_C128 3

typedef struct amg_hierx amg_hierx;

/* kind: the amg_smoother_desc kinds 0 (none), 1 (jacobi), 2 (gauss_seidel), 3 (sor), 4 (polynomial),
 * 5 (block_jacobi), 6 (block_gauss_seidel); any other kind returns AMG_ENOTIMPL.  omega and Dinv hold values
 * of the hierarchy's type (jacobi's omega as type_prep makes it; sor's omega must be real), the polynomial
 * coefficients are doubles. */
typedef struct {
    int kind;
    int iterations;
    int sweep;                 /* AMG_SWEEP_* */
    const void *omega;         /* one value */
    int ncoef;
    const double *coef;
    int blocksize;
    const void *Dinv;          /* n/blocksize blocks of blocksize^2 values, row-major */
} amg_smoother_desc_x;

/* A coarse solver supplied by the caller, with HOST vectors of the hierarchy's type; x is zero on entry. */
typedef int (*amg_coarse_callback_x)(void *user, int n, const void *b_host, void *x_host);

/* *out receives the handle; AMG_ENOTIMPL (and *out = NULL) for value types other than AMG_VALUE_C128 */
int amg_hierx_create(int value_type, int nlevels, int device, amg_hierx **out);
void amg_hierx_destroy(amg_hierx *h);
/* as amg_hier_set_matrix (HOST arrays, copied); A must be square (BSR: square blocks) */
int amg_hierx_set_matrix(amg_hierx *h, int lvl, int which, int fmt, int nrows, int ncols, int R, int C,
                         const int *Ap, const int *Aj, const void *Ax);
/* which = AMG_PRE / AMG_POST, or 2 for the coarse solver of the last level */
int amg_hierx_set_smoother(amg_hierx *h, int lvl, int which, const amg_smoother_desc_x *d);
/* as amg_hier_set_block_matrix: A re-blocked for a block smoother, passed after amg_hierx_set_smoother */
int amg_hierx_set_block_matrix(amg_hierx *h, int lvl, int which, int nbrows, int bs, const int *Ap,
                               const int *Aj, const void *Ax);
/* coarse solve = the dense n x n operator M (row-major), applied with sequential row sums */
int amg_hierx_set_coarse_dense(amg_hierx *h, const void *M, int n);
int amg_hierx_set_coarse_callback(amg_hierx *h, amg_coarse_callback_x fn, void *user);
/* builds the schedules and work vectors and seals the handle: setters called after it return AMG_ESTATE, and
 * calling it again returns 0 without doing anything.  One coarse solver per handle. */
int amg_hierx_finalize(amg_hierx *h);
/* amg_hier_solve for HOST vectors of the hierarchy's type; flags AMG_SOLVE_X0_ZERO, AMG_SOLVE_NO_EARLY_STOP;
 * residuals (maxiter + 1 doubles) receive the residual norms, *nres their count */
int amg_hierx_solve(amg_hierx *h, const void *b, void *x, double tol, int maxiter, int cycle, double *residuals,
                    int *nres, int flags);
/* one cycle of x for the right-hand side b; AMG_SOLVE_X0_ZERO: start from zero.  HOST vectors, or with
 * AMG_SOLVE_DEVICE_VECTORS device vectors: copied in and out on the hierarchy's stream, without synchronising */
int amg_hierx_cycle(amg_hierx *h, const void *b, void *x, int cycle, int flags);
long amg_hierx_device_bytes(amg_hierx *h);
double amg_hierx_last_solve_ms(amg_hierx *h);

/* ---- device-resident vectors for the Krylov methods that wrap the cycle (pyamg_amd/krylov_c128.py): vectors of
 * the hierarchy's value type live in HBM; only scalars cross PCIe.  All work is ordered on amg_hierx_stream(h). */
void *amg_hierx_stream(amg_hierx *h);
int amg_hierx_level_size(amg_hierx *h, int lvl);             /* rows of A_lvl, -1 for a bad level */
/* y = A_lvl x on DEVICE vectors (x and y distinct): each row summed from zero in stored order, as in the cycle */
int amg_hierx_apply(amg_hierx *h, int lvl, const void *x_dev, void *y_dev);
/* a zeroed device vector of n values, counted in amg_hierx_device_bytes until freed with the same n */
void *amg_hierx_vec_alloc(amg_hierx *h, long n);
void amg_hierx_vec_free(amg_hierx *h, void *p, long n);
/* the hierarchy's scratch of the amg_devx_* reductions: AMG_DEVX_PARTIALS partial sums, then AMG_DEVX_SLOTS result
 * slots (one value of the hierarchy's type each); allocated on first use, NULL on failure */
#define AMG_DEVX_PARTIALS 512
#define AMG_DEVX_SLOTS    8
void *amg_hierx_scratch(amg_hierx *h);
/* *host = ||v||_2 of n device values (v may point into a vector): the residual norm's two-stage reduction; one
 * 8-byte read-back, stream synchronised */
int amg_hierx_norm(amg_hierx *h, const void *v_dev, long n, double *host);

/* complex128 vector kernels on caller-supplied DEVICE pointers and stream (scratch: amg_hierx_scratch).
 * zdotc: slot <- sum_k conj(x_k) y_k in a fixed order that depends on n alone; host != NULL: also copied there
 * (two doubles) with the stream synchronised */
int amg_devx_zdotc(const void *x, const void *y, long n, void *scratch, int slot, double *host, void *stream);
int amg_devx_axpy(void *y, const void *x, double are, double aim, long n, void *stream);          /* y += a x */
/* y += (factor * slot) x, the complex scalar read from the result slot on the device */
int amg_devx_axpy_slot(void *y, const void *x, const void *scratch, int slot, double factor, long n, void *stream);
int amg_devx_xpby(void *p, double bre, double bim, const void *z, long n, void *stream);          /* p = beta p + z */
int amg_devx_scale(void *out, const void *x, double cre, double cim, long n, void *stream);       /* out = c x */
int amg_devx_sub(void *out, const void *a, const void *b, long n, void *stream);                  /* out = a - b */
int amg_devx_fill(void *x, double vre, double vim, long n, void *stream);
/* n values; kind: 0 host->device, 1 device->host, 2 device->device; host copies synchronous on return */
int amg_devx_copy(void *dst, const void *src, long n, int kind, void *stream);
/* for j = start, start + step, ... (stop excluded): v <- v - 2 <W[j], v> W[j] (amg_core/krylov.h:34-53).  W: HOST
 * array of nW device vectors.  Every inner product stays on the device (slot 0): no host synchronisation. */
int amg_devx_householders(void *v, const void *const *W, int nW, long n, int start, int stop, int step,
                          void *scratch, void *stream);
/* the same with v[j] += y[j] before reflector j (householder_hornerscheme, krylov.h:97-120); y: DEVICE vector */
int amg_devx_horner(void *v, const void *const *W, int nW, const void *y, long n, int start, int stop, int step,
                    void *scratch, void *stream);

/* ------------------------------------------------------------------------ */
/* 6. Resident float64 hierarchies for SEVERAL right-hand sides: the cycle   */
/*    of section 2 (multilevel.py:316-548) for k vectors at once.  Every     */
/*    operator entry is read once per application and applied to all columns,*/
/*    every Gauss-Seidel dependency level is one launch for all columns.     */
/*    Per column the iterates have the bits of amg_hier_solve; a column's    */
/*    iterates and residual history do not depend on k, on its position or   */
/*    on the other columns.  Plain CSR operators, eager launches.            */
/* ------------------------------------------------------------------------ */
typedef struct amg_hierm amg_hierm;

/* kmax in 1 .. 8: the most columns one call will carry (work vectors are n x {1, 2, 4, 8} doubles, the next width) */
int amg_hierm_create(int nlevels, int device, int kmax, amg_hierm **out);
void amg_hierm_destroy(amg_hierm *h);
/* as amg_hier_set_matrix (HOST arrays, copied): CSR, or BSR with 1 x 1 blocks (larger blocks: AMG_ENOTIMPL), which
 * multiplies like CSR and relaxes with the rounding of bsr_jacobi / bsr_gauss_seidel */
int amg_hierm_set_matrix(amg_hierm *h, int lvl, int which, int fmt, int nrows, int ncols, int R, int C,
                         const int *Ap, const int *Aj, const double *Ax);
/* kinds AMG_SM_NONE, _JACOBI, _GAUSS_SEIDEL, _SOR, _POLYNOMIAL; any other kind returns AMG_ENOTIMPL */
int amg_hierm_set_smoother(amg_hierm *h, int lvl, int which, const amg_smoother_desc *d);
/* coarse solve = the dense n x n operator M (row-major), sequential row sums per column */
int amg_hierm_set_coarse_dense(amg_hierm *h, const double *M, int n);
/* coarse solve = x = 0, then the smoother (same kinds) */
int amg_hierm_set_coarse_smoother(amg_hierm *h, const amg_smoother_desc *d);
/* builds the schedules and work vectors and seals the handle: setters called after it return AMG_ESTATE, and
 * calling it again returns 0 without doing anything */
int amg_hierm_finalize(amg_hierm *h);
/* multilevel_solver.solve for each of the k (1 .. kmax) columns of B; B and X are HOST arrays, row-major (n, k); X holds
 * the starting guesses on entry.  Column j stops by its own tol * ||b_j|| (tol when ||b_j|| = 0); what X receives for
 * it is the iterate at which it stopped, although the engine keeps cycling it while other columns are active.
 * residuals: k rows of maxiter + 1 doubles (column j's history), nres: k counts.  flags AMG_SOLVE_X0_ZERO and
 * AMG_SOLVE_NO_EARLY_STOP as for amg_hier_solve. */
int amg_hierm_solve(amg_hierm *h, int k, const double *B, double *X, double tol, int maxiter, int cycle,
                    double *residuals, int *nres, int flags);
/* one cycle (V, W, F) of every column; AMG_SOLVE_X0_ZERO: start from zero */
int amg_hierm_cycle(amg_hierm *h, int k, const double *B, double *X, int cycle, int flags);
long amg_hierm_device_bytes(amg_hierm *h);
double amg_hierm_last_solve_ms(amg_hierm *h);

#ifdef __cplusplus
}
#endif
#endif
