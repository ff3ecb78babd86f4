// K18: dense triangular solves and LU with partial pivoting (float32 / float64).
//
// replaces tensor/slinalg.py:280 SolveTriangular, :130 CholeskySolve, :365 Solve and
// tensor/nlinalg.py:100 MatrixInverse, :196 Det (scipy.linalg.solve_triangular / cho_solve / solve,
// np.linalg.inv / det: LAPACK trtrs, potrs, gesv, getrf + getri).
//
// Only the pieces of a BLOCKED algorithm that are not a product live here: the substitution on
// one NB x NB diagonal block, the factorisation of one NB-wide panel, the row interchanges, the
// determinant of a factor, the mirror of a triangle and the finiteness pass.  The block loops (and
// the ahip_gemm / ahip_gemv updates between these kernels) are the host's, exec_linalg.py.  Every
// dependency between workgroups is a launch boundary: no kernel here waits for another workgroup.
//
// All matrices are addressed by (row, col) element strides.  Errors travel through the optional
// info word (AHIP_LINALG_* in the header): one atomicMax, never a trap.
#include "common.h"

namespace {

constexpr int NB = AHIP_LINALG_NB;

inline bool float_dtype(int dt) { return dt == AHIP_F32 || dt == AHIP_F64; }

// info word: TAG | kind << 32 | (2^32 - 1 - k).  atomicMax keeps the highest kind and, within a
// kind, the SMALLEST 0-based index k (what LAPACK's info reports), whatever the order the
// workgroups and launches meet them in.
__device__ inline void report(unsigned long long* info, int kind, int64_t k) {
  if (info != nullptr)
    atomicMax(info, (unsigned long long)AHIP_LINALG_INFO_TAG | ((unsigned long long)kind << 32) |
                        (0xFFFFFFFFull - (unsigned long long)k));
}

// ------------------------------------------------------------------ triangular diagonal block ---
struct TrsmArgs {
  const void* T;   // nb x nb block on the diagonal of the triangular matrix
  void* X;         // nb x m block of right-hand sides, solved in place
  void* info;      // info word or null
  int64_t t_rs, t_cs, x_rs, x_cs, m, base;   // base: index of the block's first row in the whole matrix
  int nb, lower, unit;
};
AHIP_PTRS_BEGIN(TrsmArgs) AHIP_PTR1(T) AHIP_PTR1(X) AHIP_PTR1(info) AHIP_PTRS_END

// element (i, k) of the referenced triangle in packed storage (diagonal included)
__device__ inline int tri(int i, int k) {
  const int hi = i > k ? i : k, lo = i > k ? k : i;
  return hi * (hi + 1) / 2 + lo;
}

// Matrix right-hand side: one wave per 64 columns of X, each lane owns one column, so the
// substitution needs no cross-lane traffic; T is read from LDS as a broadcast.  Row-oriented:
// x_i = (b_i - sum_k t_ik x_k) / t_ii, k ascending (lower) / descending from the end (upper).
template <typename F>
__global__ __launch_bounds__(64) void trsm_diag_mat_kernel(TrsmArgs a) {
  __shared__ F Ts[NB * (NB + 1) / 2];
  __shared__ F Xs[NB][NB];
  const int lane = threadIdx.x, nb = a.nb;
  const F* T = static_cast<const F*>(a.T);
  F* X = static_cast<F*>(a.X);
  for (int e = lane; e < nb * nb; e += 64) {
    const int i = e / nb, k = e % nb;
    // the other triangle is never read; with unit_diagonal neither is the diagonal
    const bool ref = i == k ? !a.unit : (a.lower ? k < i : k > i);
    if (ref) Ts[tri(i, k)] = T[i * a.t_rs + k * a.t_cs];
    else if (i == k) Ts[tri(i, k)] = F(1);
  }
  const int64_t col = (int64_t)blockIdx.x * 64 + lane;
  const bool on = col < a.m;
  for (int i = 0; i < nb; ++i) Xs[i][lane] = on ? X[i * a.x_rs + col * a.x_cs] : F(0);
  __syncthreads();
  if (blockIdx.x == 0 && !a.unit && lane < nb && Ts[tri(lane, lane)] == F(0))
    report(static_cast<unsigned long long*>(a.info), AHIP_LINALG_SINGULAR, a.base + lane);
  if (a.lower) {
    for (int i = 0; i < nb; ++i) {
      F s = Xs[i][lane];
      for (int k = 0; k < i; ++k) s -= Ts[tri(i, k)] * Xs[k][lane];
      if (!a.unit) s = s / Ts[tri(i, i)];
      Xs[i][lane] = s;
    }
  } else {
    for (int i = nb - 1; i >= 0; --i) {
      F s = Xs[i][lane];
      for (int k = nb - 1; k > i; --k) s -= Ts[tri(i, k)] * Xs[k][lane];
      if (!a.unit) s = s / Ts[tri(i, i)];
      Xs[i][lane] = s;
    }
  }
  if (on)
    for (int i = 0; i < nb; ++i) X[i * a.x_rs + col * a.x_cs] = Xs[i][lane];
}

// Vector right-hand side: one wave, lane i owns x_i; column-oriented substitution with one
// broadcast (a lane read) per row.
template <typename F>
__global__ __launch_bounds__(64) void trsm_diag_vec_kernel(TrsmArgs a) {
  __shared__ F Ts[NB][NB + 1];
  const int lane = threadIdx.x, nb = a.nb;
  const F* T = static_cast<const F*>(a.T);
  F* X = static_cast<F*>(a.X);
  for (int e = lane; e < nb * nb; e += 64) {
    const int i = e / nb, k = e % nb;
    const bool ref = i == k ? !a.unit : (a.lower ? k < i : k > i);
    Ts[i][k] = ref ? T[i * a.t_rs + k * a.t_cs] : F(i == k ? 1 : 0);
  }
  F x = lane < nb ? X[lane * a.x_rs] : F(0);
  __syncthreads();
  if (!a.unit && lane < nb && Ts[lane][lane] == F(0))
    report(static_cast<unsigned long long*>(a.info), AHIP_LINALG_SINGULAR, a.base + lane);
  if (a.lower) {
    for (int k = 0; k < nb; ++k) {
      F xk = __shfl(x, k, 64);
      if (!a.unit) xk = xk / Ts[k][k];
      if (lane == k) x = xk;
      else if (lane > k && lane < nb) x -= Ts[lane][k] * xk;
    }
  } else {
    for (int k = nb - 1; k >= 0; --k) {
      F xk = __shfl(x, k, 64);
      if (!a.unit) xk = xk / Ts[k][k];
      if (lane == k) x = xk;
      else if (lane < k) x -= Ts[lane][k] * xk;
    }
  }
  if (lane < nb) X[lane * a.x_rs] = x;
}

// ------------------------------------------------------------------ LU panel -------------------
struct PanelArgs {
  void* A;         // rows x nb panel, factored in place: unit lower L below the diagonal, U on and above
  int* piv;        // piv[base + j] = base + (row interchanged with row j), 0-based, whole-matrix rows
  void* info;      // info word or null
  int64_t rs, cs, rows, base;
  int nb;
};
AHIP_PTRS_BEGIN(PanelArgs) AHIP_PTR1(A) AHIP_PTR1(piv) AHIP_PTR1(info) AHIP_PTRS_END

constexpr int PANEL_THREADS = 1024;

// ONE workgroup factors the panel (LAPACK getf2, right-looking, one column at a time): arg-max of
// |a| over the column (the lowest row wins ties, like i?amax), interchange inside the panel, divide
// the column by the pivot, rank-1 update of the columns to its right.  A thread owns whole rows; the
// arg-max of the NEXT column is taken while that column is updated, so a column costs one pass.
// A zero pivot is reported and the column is left as it is (it is all zero): no division by zero.
template <typename F>
__global__ __launch_bounds__(PANEL_THREADS) void getrf_panel_kernel(PanelArgs a) {
  __shared__ F rowj[NB];
  __shared__ F wave_val[PANEL_THREADS / 64];
  __shared__ int64_t wave_idx[PANEL_THREADS / 64];
  __shared__ int64_t pivot_row;
  const int tid = threadIdx.x, nb = a.nb, nthreads = blockDim.x;      // (a multiple of 64, see the launch)
  const int64_t rows = a.rows;
  F* A = static_cast<F*>(a.A);
  F best = F(-1);
  int64_t best_i = 0;
  for (int64_t r = tid; r < rows; r += nthreads) {
    const F v = fabs(A[r * a.rs]);
    if (v > best) { best = v; best_i = r; }
  }
  for (int j = 0; j < nb; ++j) {
    // workgroup arg-max of (best, best_i): larger value, then lower row
    for (int off = 32; off > 0; off >>= 1) {
      const F ov = __shfl_down(best, off, 64);
      const int64_t oi = __shfl_down(best_i, off, 64);
      if (ov > best || (ov == best && oi < best_i)) { best = ov; best_i = oi; }
    }
    if ((tid & 63) == 0) { wave_val[tid >> 6] = best; wave_idx[tid >> 6] = best_i; }
    __syncthreads();
    if (tid == 0) {
      F bv = wave_val[0];
      int64_t bi = wave_idx[0];
      for (int w = 1; w < nthreads / 64; ++w)
        if (wave_val[w] > bv || (wave_val[w] == bv && wave_idx[w] < bi)) { bv = wave_val[w]; bi = wave_idx[w]; }
      if (!(bv >= F(0)) || bi < j || bi >= rows) bi = j;       // nothing comparable in the column (NaNs)
      pivot_row = bi;
      a.piv[a.base + j] = (int)(a.base + bi);
    }
    __syncthreads();
    const int64_t p = pivot_row;
    if (tid < nb) {
      const F top = A[j * a.rs + tid * a.cs];
      if (p != j) {
        const F low = A[p * a.rs + tid * a.cs];
        A[p * a.rs + tid * a.cs] = top;
        A[j * a.rs + tid * a.cs] = low;
        rowj[tid] = low;
      } else {
        rowj[tid] = top;
      }
    }
    __syncthreads();
    const F pivot = rowj[j];
    const bool zero = pivot == F(0);
    if (zero && tid == 0) report(static_cast<unsigned long long*>(a.info), AHIP_LINALG_SINGULAR, a.base + j);
    best = F(-1);
    best_i = j + 1;
    for (int64_t r = j + 1 + tid; r < rows; r += nthreads) {
      F* row = A + r * a.rs;
      if (!zero) {
        const F l = row[j * a.cs] / pivot;
        row[j * a.cs] = l;
        for (int c = j + 1; c < nb; ++c) row[c * a.cs] -= l * rowj[c];
      }
      if (j + 1 < nb) {
        const F v = fabs(row[(j + 1) * a.cs]);
        if (v > best) { best = v; best_i = r; }
      }
    }
    __syncthreads();      // rowj is rewritten, and the rows are read by other threads, in the next column
  }
}

// ------------------------------------------------------------------ row interchanges -----------
struct LaswpArgs {
  void* B;
  const int* piv;
  int64_t rs, cs, nrows, ncols, skip0, skiplen;
  int k0, k1;
};
AHIP_PTRS_BEGIN(LaswpArgs) AHIP_PTR1(B) AHIP_PTR1(piv) AHIP_PTRS_END

// for k = k0 .. k1-1: rows k and piv[k] of B change places (LAPACK laswp, forward).  A thread owns
// a column, so the interchanges of a column stay in order; columns [skip0, skip0 + skiplen) are
// passed over (the panel itself, which was interchanged while it was factored).
template <typename F>
__global__ __launch_bounds__(256) void laswp_kernel(LaswpArgs a) {
  int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= a.ncols) return;
  if (c >= a.skip0) c += a.skiplen;
  F* B = static_cast<F*>(a.B) + c * a.cs;
  for (int k = a.k0; k < a.k1; ++k) {
    const int64_t p = a.piv[k];
    if (p != k && p >= 0 && p < a.nrows) {
      const F t = B[k * a.rs];
      B[k * a.rs] = B[p * a.rs];
      B[p * a.rs] = t;
    }
  }
}

// ------------------------------------------------------------------ determinant of a factor ----
struct DetArgs {
  const void* LU;
  const int* piv;
  void* out;
  int64_t rs, cs, n;
};
AHIP_PTRS_BEGIN(DetArgs) AHIP_PTR1(LU) AHIP_PTR1(piv) AHIP_PTR1(out) AHIP_PTRS_END

// One workgroup, a fixed fold order: lane t multiplies u_ii for i = t, t + 256, ..., then a tree
// over the 256 partial products; the sign is the parity of the interchanges.
template <typename F>
__global__ __launch_bounds__(256) void lu_det_kernel(DetArgs a) {
  __shared__ F prod[256];
  __shared__ int odd[256];
  const int tid = threadIdx.x;
  const F* LU = static_cast<const F*>(a.LU);
  F p = F(1);
  int o = 0;
  for (int64_t i = tid; i < a.n; i += 256) {
    p *= LU[i * (a.rs + a.cs)];
    o ^= (a.piv[i] != (int)i);
  }
  prod[tid] = p;
  odd[tid] = o;
  __syncthreads();
  for (int half = 128; half > 0; half >>= 1) {
    if (tid < half) { prod[tid] *= prod[tid + half]; odd[tid] ^= odd[tid + half]; }
    __syncthreads();
  }
  if (tid == 0) *static_cast<F*>(a.out) = odd[0] ? -prod[0] : prod[0];
}

// ------------------------------------------------------------------ mirror a triangle ----------
struct MirrorArgs {
  void* A;
  int64_t rs, cs, n;
  int lower;
};
AHIP_PTRS_BEGIN(MirrorArgs) AHIP_PTR1(A) AHIP_PTRS_END

template <typename F>
__global__ __launch_bounds__(256) void mirror_kernel(MirrorArgs a) {
  F* A = static_cast<F*>(a.A);
  const int64_t total = a.n * a.n;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t i = e / a.n, j = e % a.n;
    if (i > j) {
      if (a.lower) A[j * a.rs + i * a.cs] = A[i * a.rs + j * a.cs];
      else A[i * a.rs + j * a.cs] = A[j * a.rs + i * a.cs];
    }
  }
}

// ------------------------------------------------------------------ finiteness -----------------
struct FiniteArgs {
  const void* X;
  void* info;
  int64_t rs, cs, rows, cols;
};
AHIP_PTRS_BEGIN(FiniteArgs) AHIP_PTR1(X) AHIP_PTR1(info) AHIP_PTRS_END

template <typename F>
__global__ __launch_bounds__(256) void finite_kernel(FiniteArgs a) {
  const F* X = static_cast<const F*>(a.X);
  const int64_t total = a.rows * a.cols;
  bool bad = false;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const F v = X[(e / a.cols) * a.rs + (e % a.cols) * a.cs];
    bad = bad || !isfinite(v);
  }
  if (bad) report(static_cast<unsigned long long*>(a.info), AHIP_LINALG_NONFINITE, 0);
}

unsigned stream_grid(int64_t total) {
  int64_t cap = (int64_t)ahip_cu_count() * 8;
  if (cap < 1) cap = 1;
  const int64_t want = (total + 255) / 256;
  return (unsigned)(want < cap ? want : cap);
}

constexpr int64_t MAX_N = (int64_t)1 << 30;

}  // namespace

extern "C" {

int ahip_linalg_nb(void) { return NB; }

int ahip_trsm_diag(int dtype, int lower, int unit_diagonal, int64_t nb, int64_t m, const void* T,
                   int64_t t_rs, int64_t t_cs, void* X, int64_t x_rs, int64_t x_cs, int64_t base,
                   void* info, void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "linalg: float32 / float64 only, got dtype %d", dtype);
  AHIP_REQUIRE(nb >= 0 && nb <= NB, "trsm_diag: block of %lld rows (at most %d)", (long long)nb, NB);
  AHIP_REQUIRE(m >= 0 && m < MAX_N && base >= 0 && base < MAX_N, "trsm_diag: extent out of range");
  if (nb == 0 || m == 0) return AHIP_OK;
  AHIP_REQUIRE(T != nullptr && X != nullptr, "null pointer");
  TrsmArgs a;
  a.T = T; a.X = X; a.info = info;
  a.t_rs = t_rs; a.t_cs = t_cs; a.x_rs = x_rs; a.x_cs = x_cs; a.m = m; a.base = base;
  a.nb = (int)nb; a.lower = lower != 0; a.unit = unit_diagonal != 0;
  hipStream_t s = as_stream(stream);
  if (m == 1) {
    if (dtype == AHIP_F32) AHIP_LAUNCH(trsm_diag_vec_kernel<float>, dim3(1), dim3(64), 0, s, a);
    else AHIP_LAUNCH(trsm_diag_vec_kernel<double>, dim3(1), dim3(64), 0, s, a);
    return AHIP_OK;
  }
  const unsigned grid = (unsigned)((m + 63) / 64);
  if (dtype == AHIP_F32) AHIP_LAUNCH(trsm_diag_mat_kernel<float>, dim3(grid), dim3(64), 0, s, a);
  else AHIP_LAUNCH(trsm_diag_mat_kernel<double>, dim3(grid), dim3(64), 0, s, a);
  return AHIP_OK;
}

int ahip_getrf_panel(int dtype, int64_t rows, int64_t nb, void* A, int64_t a_rs, int64_t a_cs,
                     int* piv, int64_t base, void* info, void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "linalg: float32 / float64 only, got dtype %d", dtype);
  AHIP_REQUIRE(nb >= 0 && nb <= NB, "getrf_panel: panel of %lld columns (at most %d)", (long long)nb, NB);
  AHIP_REQUIRE(rows >= nb && rows < MAX_N && base >= 0 && base < MAX_N,
               "getrf_panel: %lld rows for %lld columns", (long long)rows, (long long)nb);
  if (nb == 0) return AHIP_OK;
  AHIP_REQUIRE(A != nullptr && piv != nullptr, "null pointer");
  PanelArgs a;
  a.A = A; a.piv = piv; a.info = info; a.rs = a_rs; a.cs = a_cs; a.rows = rows; a.base = base;
  a.nb = (int)nb;
  hipStream_t s = as_stream(stream);
  // one thread per row up to the largest workgroup: a short panel pays for the barriers of few waves only
  const unsigned threads = (unsigned)(rows >= PANEL_THREADS ? PANEL_THREADS : (rows + 63) / 64 * 64);
  if (dtype == AHIP_F32) AHIP_LAUNCH(getrf_panel_kernel<float>, dim3(1), dim3(threads), 0, s, a);
  else AHIP_LAUNCH(getrf_panel_kernel<double>, dim3(1), dim3(threads), 0, s, a);
  return AHIP_OK;
}

int ahip_laswp(int dtype, int64_t nrows, int64_t ncols, void* B, int64_t b_rs, int64_t b_cs,
               const int* piv, int64_t k0, int64_t k1, int64_t skip0, int64_t skiplen, void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "linalg: float32 / float64 only, got dtype %d", dtype);
  AHIP_REQUIRE(0 <= k0 && k0 <= k1 && k1 <= nrows && nrows < MAX_N, "laswp: interchanges [%lld, %lld) of %lld rows",
               (long long)k0, (long long)k1, (long long)nrows);
  AHIP_REQUIRE(ncols >= 0 && ncols < MAX_N && skip0 >= 0 && skiplen >= 0, "laswp: column range out of range");
  if (k0 == k1 || ncols == 0) return AHIP_OK;
  AHIP_REQUIRE(B != nullptr && piv != nullptr, "null pointer");
  LaswpArgs a;
  a.B = B; a.piv = piv; a.rs = b_rs; a.cs = b_cs; a.nrows = nrows; a.ncols = ncols;
  a.skip0 = skip0; a.skiplen = skiplen; a.k0 = (int)k0; a.k1 = (int)k1;
  const unsigned grid = (unsigned)((ncols + 255) / 256);
  hipStream_t s = as_stream(stream);
  if (dtype == AHIP_F32) AHIP_LAUNCH(laswp_kernel<float>, dim3(grid), dim3(256), 0, s, a);
  else AHIP_LAUNCH(laswp_kernel<double>, dim3(grid), dim3(256), 0, s, a);
  return AHIP_OK;
}

int ahip_lu_det(int dtype, int64_t n, const void* LU, int64_t rs, int64_t cs, const int* piv,
                void* out, void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "linalg: float32 / float64 only, got dtype %d", dtype);
  AHIP_REQUIRE(n >= 0 && n < MAX_N, "lu_det: n = %lld", (long long)n);
  AHIP_REQUIRE(out != nullptr && (n == 0 || (LU != nullptr && piv != nullptr)), "null pointer");
  DetArgs a;
  a.LU = LU; a.piv = piv; a.out = out; a.rs = rs; a.cs = cs; a.n = n;
  hipStream_t s = as_stream(stream);
  if (dtype == AHIP_F32) AHIP_LAUNCH(lu_det_kernel<float>, dim3(1), dim3(256), 0, s, a);
  else AHIP_LAUNCH(lu_det_kernel<double>, dim3(1), dim3(256), 0, s, a);
  return AHIP_OK;
}

int ahip_mirror_triangle(int dtype, int lower, int64_t n, void* A, int64_t rs, int64_t cs, void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "linalg: float32 / float64 only, got dtype %d", dtype);
  AHIP_REQUIRE(n >= 0 && n < MAX_N, "mirror_triangle: n = %lld", (long long)n);
  if (n < 2) return AHIP_OK;
  AHIP_REQUIRE(A != nullptr, "null pointer");
  MirrorArgs a;
  a.A = A; a.rs = rs; a.cs = cs; a.n = n; a.lower = lower != 0;
  hipStream_t s = as_stream(stream);
  if (dtype == AHIP_F32) AHIP_LAUNCH(mirror_kernel<float>, dim3(stream_grid(n * n)), dim3(256), 0, s, a);
  else AHIP_LAUNCH(mirror_kernel<double>, dim3(stream_grid(n * n)), dim3(256), 0, s, a);
  return AHIP_OK;
}

int ahip_check_finite(int dtype, int64_t rows, int64_t cols, const void* X, int64_t rs, int64_t cs,
                      void* info, void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "linalg: float32 / float64 only, got dtype %d", dtype);
  AHIP_REQUIRE(rows >= 0 && rows < MAX_N && cols >= 0 && cols < MAX_N, "check_finite: extent out of range");
  if (rows == 0 || cols == 0) return AHIP_OK;
  AHIP_REQUIRE(X != nullptr && info != nullptr, "null pointer");
  FiniteArgs a;
  a.X = X; a.info = info; a.rs = rs; a.cs = cs; a.rows = rows; a.cols = cols;
  hipStream_t s = as_stream(stream);
  if (dtype == AHIP_F32) AHIP_LAUNCH(finite_kernel<float>, dim3(stream_grid(rows * cols)), dim3(256), 0, s, a);
  else AHIP_LAUNCH(finite_kernel<double>, dim3(stream_grid(rows * cols)), dim3(256), 0, s, a);
  return AHIP_OK;
}

}  // extern "C"
