// K19: Householder QR (float32 / float64).
//
// replaces tensor/nlinalg.py:403 QRFull (perform :441 np.linalg.qr: LAPACK geqrf + orgqr).
//
// As in linalg.hip only the pieces of the BLOCKED algorithm that are not a product live here: the
// factorisation of one NB-wide panel (LAPACK geqr2, with a clean copy V of its reflectors), the
// triangular factor T of the compact WY form H_1 ... H_nb = I - V T V^T from G = V^T V (LAPACK larft,
// forward, columnwise) and the extraction of R.  The panel loop, G and the three products that apply
// a block reflector are the host's (exec_linalg.py, ahip_gemm).  Every dependency between
// workgroups is a launch boundary: no kernel here waits for another workgroup.
//
// All matrices are addressed by (row, col) element strides.  Nothing here can fail, so there is no
// info word: non-finite input gives non-finite output.  No float atomics: every fold has a fixed
// order (lane-strided partial sums, a shuffle tree inside the wave, the waves in order from LDS), so
// equal input gives equal bits.
#include "common.h"

namespace {

constexpr int NB = AHIP_LINALG_NB;
constexpr int PANEL_THREADS = 1024;
constexpr int PANEL_WAVES = PANEL_THREADS / 64;
constexpr int64_t MAX_N = (int64_t)1 << 30;

inline bool float_dtype(int dt) { return dt == AHIP_F32 || dt == AHIP_F64; }

// ------------------------------------------------------------------ panel ----------------------
struct Geqr2Args {
  void* A;     // rows x nb panel, factored in place: R on and above the diagonal, the reflectors below
  void* tau;   // nb scalar factors
  void* V;     // rows x nb: the reflectors alone, ones on the diagonal, exact zeros above it
  int64_t rs, cs, v_rs, v_cs, rows;
  int nb;
};
AHIP_PTRS_BEGIN(Geqr2Args) AHIP_PTR1(A) AHIP_PTR1(tau) AHIP_PTR1(V) AHIP_PTRS_END

// max that keeps a NaN once it has met one (fmax would drop it, and a column whose other entries are
// zero would then lose its NaN from R)
template <typename F>
__device__ inline F nanmax(F a, F b) { return (b > a || b != b) ? b : a; }

template <typename F>
__device__ inline F wave_sum(F v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return __shfl(v, 0, 64);
}

template <typename F>
__device__ inline F wave_nanmax(F v) {
  for (int off = 32; off > 0; off >>= 1) v = nanmax(v, __shfl_down(v, off, 64));
  return __shfl(v, 0, 64);
}

// ONE workgroup factors the panel (LAPACK geqr2), a column at a time:
//   1. ||x|| of the column x below the diagonal, max-scaled: scale = max |x_r| (all threads, lanes
//      stride over the rows), then scale * sqrt(sum (x_r / scale)^2) — entries of 1e30 or 1e-30
//      neither overflow nor vanish in float32;
//   2. larfg: ||x|| == 0 gives tau = 0 and leaves the column alone, else beta = -sign(alpha)
//      hypot(alpha, ||x||), tau = (beta - alpha) / beta, v = x / (alpha - beta), r_jj = beta
//      (LAPACK's rescaling loop for |beta| below the safe minimum is left out: hypot does not
//      underflow, and a column that small has lost its digits to denormals already);
//   3. the remaining columns c: w_c = a_jc + v^T a_c, a_c -= tau w_c (1; v): one wave per column,
//      its lanes stride over the rows.
template <typename F>
__global__ __launch_bounds__(PANEL_THREADS) void geqr2_panel_kernel(Geqr2Args a) {
  __shared__ F fold[PANEL_WAVES];
  __shared__ F bcast[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nb = a.nb;
  const int nthreads = blockDim.x, nwaves = nthreads >> 6;              // (a multiple of 64, see the launch)
  const int64_t rows = a.rows;
  F* A = static_cast<F*>(a.A);
  F* V = static_cast<F*>(a.V);
  F* tau = static_cast<F*>(a.tau);
  for (int j = 0; j < nb; ++j) {
    F* col = A + j * a.cs;
    F* vcol = V + j * a.v_cs;
    // 1. scale = max |x_r|
    F m = F(0);
#pragma unroll 4
    for (int64_t r = j + 1 + tid; r < rows; r += nthreads) m = nanmax(m, (F)fabs(col[r * a.rs]));
    m = wave_nanmax(m);
    if (lane == 0) fold[wave] = m;
    __syncthreads();
    if (tid == 0) {
      F s = fold[0];
      for (int w = 1; w < nwaves; ++w) s = nanmax(s, fold[w]);
      bcast[0] = s;
    }
    __syncthreads();
    const F scale = bcast[0];
    F tj = F(0);
    if (scale != F(0)) {                                                // (uniform; a NaN scale takes this path)
      F ss = F(0);
#pragma unroll 4
      for (int64_t r = j + 1 + tid; r < rows; r += nthreads) {
        const F q = col[r * a.rs] / scale;
        ss += q * q;
      }
      ss = wave_sum(ss);
      if (lane == 0) fold[wave] = ss;                                   // (fold was read before the last barrier)
      __syncthreads();
      if (tid == 0) {
        F s = fold[0];
        for (int w = 1; w < nwaves; ++w) s += fold[w];
        bcast[1] = scale * sqrt(s);
      }
      __syncthreads();
      // 2. larfg, by every thread on the same values
      const F xnorm = bcast[1];
      const F alpha = col[j * a.rs];
      const F beta = -copysign(hypot(alpha, xnorm), alpha);
      tj = (beta - alpha) / beta;
      const F den = alpha - beta;
      __syncthreads();                                                  // alpha is read by all before it is overwritten
#pragma unroll 4
      for (int64_t r = j + 1 + tid; r < rows; r += nthreads) {
        const F v = col[r * a.rs] / den;
        col[r * a.rs] = v;
        vcol[r * a.v_rs] = v;
      }
      if (tid == 0) col[j * a.rs] = beta;
    } else {
      for (int64_t r = j + 1 + tid; r < rows; r += nthreads) vcol[r * a.v_rs] = F(0);
    }
    if (tid <= j) vcol[tid * a.v_rs] = tid == j ? F(1) : F(0);
    if (tid == 0) tau[j] = tj;
    __syncthreads();                                                    // v is complete before the waves read it
    // 3. apply H_j to the columns to the right (skipped for tau == 0, like LAPACK's larf: H_j = I)
    if (tj != F(0)) {
      for (int c = j + 1 + wave; c < nb; c += nwaves) {
        F* ac = A + c * a.cs;
        F w = F(0);
#pragma unroll 8
        for (int64_t r = j + 1 + lane; r < rows; r += 64) w += vcol[r * a.v_rs] * ac[r * a.rs];
        w = wave_sum(w);
        const F top = ac[j * a.rs];                                     // (same address for all lanes)
        const F tw = tj * (top + w);
#pragma unroll 8
        for (int64_t r = j + 1 + lane; r < rows; r += 64) ac[r * a.rs] -= tw * vcol[r * a.v_rs];
        if (lane == 0) ac[j * a.rs] = top - tw;
      }
    }
    __syncthreads();                                                    // column j + 1 is complete before its norm
  }
}

// ------------------------------------------------------------------ T of the compact WY form ----
struct LarftArgs {
  const void* G;     // nb x nb: V^T V (only its strict upper triangle is read)
  const void* tau;
  void* T;           // nb x nb upper triangular, exact zeros below the diagonal
  int64_t g_rs, g_cs, t_rs, t_cs;
  int nb;
};
AHIP_PTRS_BEGIN(LarftArgs) AHIP_PTR1(G) AHIP_PTR1(tau) AHIP_PTR1(T) AHIP_PTRS_END

// LAPACK larft (forward, columnwise): T_jj = tau_j, T[0:j, j] = -tau_j T[0:j, 0:j] (V^T v_j)[0:j].
// One wave; lane i owns row i of T (in LDS), the columns go in order; lane k holds G_kj and hands
// it round by a lane read, over the whole row of T (its zeros left of the diagonal included) so
// that every lane takes every step.
template <typename F>
__global__ __launch_bounds__(64) void larft_kernel(LarftArgs a) {
  __shared__ F Ts[NB][NB + 1];
  const int lane = threadIdx.x, nb = a.nb;
  const F* G = static_cast<const F*>(a.G);
  const F* tau = static_cast<const F*>(a.tau);
  F* T = static_cast<F*>(a.T);
  for (int k = 0; k < NB; ++k) Ts[lane][k] = F(0);
  for (int j = 0; j < nb; ++j) {
    const F tj = tau[j];
    const F g = lane < j ? G[lane * a.g_rs + j * a.g_cs] : F(0);
    F s = F(0);
    for (int k = 0; k < j; ++k) s += Ts[lane][k] * __shfl(g, k, 64);
    if (lane == j) Ts[j][j] = tj;
    else if (lane < j && tj != F(0)) Ts[lane][j] = -tj * s;
  }
  __syncthreads();
  for (int e = lane; e < nb * nb; e += 64) {
    const int i = e / nb, k = e % nb;
    T[i * a.t_rs + k * a.t_cs] = Ts[i][k];
  }
}

// ------------------------------------------------------------------ R ---------------------------
struct ExtractArgs {
  const void* A;
  void* R;
  int64_t a_rs, a_cs, r_rs, r_cs, rows, cols;
};
AHIP_PTRS_BEGIN(ExtractArgs) AHIP_PTR1(A) AHIP_PTR1(R) AHIP_PTRS_END

// R[i, j] = A[i, j] on and above the diagonal (rows <= the rows of A), exact zeros everywhere else
template <typename F>
__global__ __launch_bounds__(256) void extract_r_kernel(ExtractArgs a) {
  const F* A = static_cast<const F*>(a.A);
  F* R = static_cast<F*>(a.R);
  const int64_t total = a.rows * a.cols;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t i = e / a.cols, j = e % a.cols;
    R[i * a.r_rs + j * a.r_cs] = i <= j ? A[i * a.a_rs + j * a.a_cs] : F(0);
  }
}

unsigned stream_grid(int64_t total) {
  int64_t cap = (int64_t)ahip_cu_count() * 8;
  if (cap < 1) cap = 1;
  const int64_t want = (total + 255) / 256;
  return (unsigned)(want < cap ? want : cap);
}

}  // namespace

extern "C" {

int ahip_geqr2_panel(int dtype, int64_t rows, int64_t nb, void* A, int64_t a_rs, int64_t a_cs, void* tau,
                     void* V, int64_t v_rs, int64_t v_cs, void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "qr: float32 / float64 only, got dtype %d", dtype);
  AHIP_REQUIRE(nb >= 0 && nb <= NB, "geqr2_panel: panel of %lld columns (at most %d)", (long long)nb, NB);
  AHIP_REQUIRE(rows >= nb && rows < MAX_N, "geqr2_panel: %lld rows for %lld columns", (long long)rows,
               (long long)nb);
  if (nb == 0) return AHIP_OK;
  AHIP_REQUIRE(A != nullptr && tau != nullptr && V != nullptr, "null pointer");
  Geqr2Args a;
  a.A = A; a.tau = tau; a.V = V; a.rs = a_rs; a.cs = a_cs; a.v_rs = v_rs; a.v_cs = v_cs; a.rows = rows;
  a.nb = (int)nb;
  hipStream_t s = as_stream(stream);
  // a wave per remaining column and a thread per row, up to the largest workgroup: a small panel
  // pays for the barriers of few waves only
  int64_t waves = (rows + 63) / 64;
  if (waves < nb - 1) waves = nb - 1;
  if (waves > PANEL_WAVES) waves = PANEL_WAVES;
  if (waves < 1) waves = 1;
  const unsigned threads = (unsigned)(waves * 64);
  if (dtype == AHIP_F32) AHIP_LAUNCH(geqr2_panel_kernel<float>, dim3(1), dim3(threads), 0, s, a);
  else AHIP_LAUNCH(geqr2_panel_kernel<double>, dim3(1), dim3(threads), 0, s, a);
  return AHIP_OK;
}

int ahip_larft(int dtype, int64_t nb, const void* G, int64_t g_rs, int64_t g_cs, const void* tau, void* T,
               int64_t t_rs, int64_t t_cs, void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "qr: float32 / float64 only, got dtype %d", dtype);
  AHIP_REQUIRE(nb >= 0 && nb <= NB, "larft: block of %lld reflectors (at most %d)", (long long)nb, NB);
  if (nb == 0) return AHIP_OK;
  AHIP_REQUIRE(G != nullptr && tau != nullptr && T != nullptr, "null pointer");
  LarftArgs a;
  a.G = G; a.tau = tau; a.T = T; a.g_rs = g_rs; a.g_cs = g_cs; a.t_rs = t_rs; a.t_cs = t_cs; a.nb = (int)nb;
  hipStream_t s = as_stream(stream);
  if (dtype == AHIP_F32) AHIP_LAUNCH(larft_kernel<float>, dim3(1), dim3(64), 0, s, a);
  else AHIP_LAUNCH(larft_kernel<double>, dim3(1), dim3(64), 0, s, a);
  return AHIP_OK;
}

int ahip_qr_extract_r(int dtype, int64_t rows, int64_t cols, const void* A, int64_t a_rs, int64_t a_cs,
                      void* R, int64_t r_rs, int64_t r_cs, void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "qr: float32 / float64 only, got dtype %d", dtype);
  AHIP_REQUIRE(rows >= 0 && rows < MAX_N && cols >= 0 && cols < MAX_N, "qr_extract_r: %lld x %lld",
               (long long)rows, (long long)cols);
  if (rows == 0 || cols == 0) return AHIP_OK;
  AHIP_REQUIRE(R != nullptr && A != nullptr, "null pointer");
  ExtractArgs a;
  a.A = A; a.R = R; a.a_rs = a_rs; a.a_cs = a_cs; a.r_rs = r_rs; a.r_cs = r_cs; a.rows = rows; a.cols = cols;
  hipStream_t s = as_stream(stream);
  if (dtype == AHIP_F32) AHIP_LAUNCH(extract_r_kernel<float>, dim3(stream_grid(rows * cols)), dim3(256), 0, s, a);
  else AHIP_LAUNCH(extract_r_kernel<double>, dim3(stream_grid(rows * cols)), dim3(256), 0, s, a);
  return AHIP_OK;
}

}  // extern "C"
