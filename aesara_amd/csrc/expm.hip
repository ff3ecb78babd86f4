// K23: the matrix exponential by scaling and squaring (float32 / float64).
//
// replaces tensor/slinalg.py:595 Expm (scipy.linalg.expm) and :631 ExpmGrad (the reference goes through
// scipy.linalg.eig and inv(V); here the gradient is the top-right block of expm([[A^T, G], [0, A^T]]),
// which needs no complex arithmetic and holds for a defective A: the caller assembles that matrix).
//
// Higham's 2005 algorithm: ||A||_1 picks the degree m of the diagonal Pade approximant r_m = q_m^-1 p_m
// from {3, 5, 7, 9, 13} and, beyond theta_13, the scaling s = ceil(log2(||A||_1 / theta_13)); p_m = V + U
// and q_m = V - U with U odd and V even in B = 2^-s A, built from B^2, B^4, B^6 (B^8 for m = 9); then
// (V - U) X = V + U by LU with partial pivoting and s squarings of X.  The float64 thresholds serve both
// dtypes: they are safe for float32 and cost it an occasional product.
//
// ahip_expm_tile runs all of it in ONE launch, one workgroup a matrix: seven matrices resident in LDS
// (A, A^2, A^4, A^6, a temporary, U, V), every product on the 16x16x4 matrix instructions from LDS
// operands, the LU and both substitutions in LDS as well.  Larger matrices take the blocked path, whose
// products and LU are the caller's (ahip_gemm, K18): ahip_expm_norm1 leaves ||A||_1, m and s in a status
// record that the host reads once, ahip_expm_combine forms the polynomials' linear combinations.
//
// Every fold has a fixed order (no float atomics): the same call gives the same bits.  Nothing fails:
// there is no info word, a non-finite operand gives s = 0 and a non-finite result.
#include "dense.h"

#include <cmath>

namespace {

// theta_m of Higham (2005), Table 2.3: the largest ||2^-s A||_1 for which r_m has backward error <= 2^-53
constexpr double THETA3 = 1.495585217958292e-2, THETA5 = 2.539398330063230e-1, THETA7 = 9.504178996162932e-1,
                 THETA9 = 2.097847961257068e0, THETA13 = 5.371920351148152e0;

// b_0 .. b_m of p_m(x) = sum b_i x^i, (2m - i)! m! / ((2m)! (m - i)! i!) scaled to integers
__device__ const double PADE3[4] = {120., 60., 12., 1.};
__device__ const double PADE5[6] = {30240., 15120., 3360., 420., 30., 1.};
__device__ const double PADE7[8] = {17297280., 8648640., 1995840., 277200., 25200., 1512., 56., 1.};
__device__ const double PADE9[10] = {17643225600., 8821612800., 2075673600., 302702400., 30270240.,
                                     2162160., 110880., 3960., 90., 1.};
__device__ const double PADE13[14] = {64764752532480000., 32382376266240000., 7771770303897600.,
                                      1187353796428800., 129060195264000., 10559470521600., 670442572800.,
                                      33522128640., 1323241920., 40840800., 960960., 16380., 182., 1.};

// (m, s) for a 1-norm.  The smallest s with norm <= 2^s theta_13, exactly: norm / theta_13 = f 2^e with f in
// [0.5, 1).  A norm that is not finite fails every comparison: m = 13, s = 0.
__device__ inline void pade_choice(double norm, int& m, int& s) {
  s = 0;
  if (norm <= THETA3) m = 3;
  else if (norm <= THETA5) m = 5;
  else if (norm <= THETA7) m = 7;
  else if (norm <= THETA9) m = 9;
  else {
    m = 13;
    if (norm > THETA13 && norm <= DBL_MAX) {
      int e;
      const double f = frexp(norm / THETA13, &e);
      s = f == 0.5 ? e - 1 : e;
    }
  }
}

// c_i = b_i / b_0 of degree m, in the working type (V = I + ..., whatever the degree)
template <typename F>
__device__ inline F pade_coeff(int m, int i) {
  const double* b = m == 3 ? PADE3 : m == 5 ? PADE5 : m == 7 ? PADE7 : m == 9 ? PADE9 : PADE13;
  return (F)(b[i] / b[0]);
}

// the larger of two column sums; a NaN wins and stays
__device__ inline double norm_max(double a, double b) { return (b > a || b != b) ? b : a; }

__device__ inline void write_status(void* status, int64_t record, double norm, int m, int s) {
  long long* st = static_cast<long long*>(status) + record * AHIP_EXPM_STATUS_WORDS;
  st[0] = __double_as_longlong(norm);
  st[1] = m;
  st[2] = s;
}

// ------------------------------------------------------------------ the LDS-resident solver ----
constexpr int TILE_THREADS = 512;
constexpr int TILE_WAVES = TILE_THREADS / 64;
constexpr int TILE_BUFFERS = 7;

template <typename F> struct Tile;
template <> struct Tile<float> { static constexpr int N = AHIP_EXPM_TILE_F32; };
template <> struct Tile<double> { static constexpr int N = AHIP_EXPM_TILE_F64; };
// a buffer is N rows at pitch N + 1 (a column walk is conflict-free): 116480 bytes for the seven in
// float32, 131712 in float64, of the 160 KiB a workgroup can have
template <typename F> constexpr size_t tile_lds() {
  return (size_t)TILE_BUFFERS * Tile<F>::N * (Tile<F>::N + 1) * sizeof(F);
}
static_assert(tile_lds<float>() <= 160 * 1024 && tile_lds<double>() <= 160 * 1024, "LDS budget");
static_assert(AHIP_EXPM_TILE_F32 <= 64 && AHIP_EXPM_TILE_F64 <= 64 && AHIP_EXPM_TILE_F32 % 16 == 0 &&
              AHIP_EXPM_TILE_F64 % 16 == 0, "a lane a row, whole 16 x 16 fragments");

extern __shared__ __align__(16) unsigned char expm_lds[];

struct TileArgs {
  const void* A;   // batch of n x n matrices
  void* out;       // their exponentials
  void* status;    // null, or AHIP_EXPM_STATUS_WORDS words a matrix: norm, m, s
  int64_t a_bs, a_rs, a_cs, o_bs, o_rs, o_cs;
  int n;
};
AHIP_PTRS_BEGIN(TileArgs) AHIP_PTR1(A) AHIP_PTR1(out) AHIP_PTR1(status) AHIP_PTRS_END

// C = X Y on the npad x npad (npad = 16 nt) leading blocks of three LDS buffers, C none of X, Y.  The
// 16 x 16 fragments of C are dealt to the waves two at a time — (ti, tj) and (ti, tj + 1), which share
// the X operand: three LDS reads feed two instructions.  Lane l reads x[ti 16 + l % 16][k + l / 16] and
// y[k + l / 16][tj 16 + l % 16]: at the odd pitch the sixteen rows of the first fall in sixteen
// different banks.  Ends with a barrier.
template <typename F, int LD>
__device__ inline void tile_product(F* Cm, const F* X, const F* Y, int nt) {
  typedef typename Mma<F>::acc_t acc_t;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
  const int half = (nt + 1) / 2, kmax = nt * 16;
  for (int u = wave; u < nt * half; u += TILE_WAVES) {
    const int ti = u / half, tj = (u % half) * 2;
    const bool two = tj + 1 < nt;
    const F* x = X + (ti * 16 + li) * LD + lk;
    const F* y = Y + lk * LD + tj * 16 + li;
    acc_t c0 = acc_t{0, 0, 0, 0}, c1 = acc_t{0, 0, 0, 0};
    if (two) {
      for (int k = 0; k < kmax; k += 4) {
        const F xv = x[k];
        Mma<F>::mma(c0, xv, y[k * LD]);
        Mma<F>::mma(c1, xv, y[k * LD + 16]);
      }
    } else {
      for (int k = 0; k < kmax; k += 4) Mma<F>::mma(c0, x[k], y[k * LD]);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      F* c = Cm + (ti * 16 + Mma<F>::row(lane, r)) * LD + tj * 16 + li;
      c[0] = c0[r];
      if (two) c[16] = c1[r];
    }
  }
  __syncthreads();
}

// dst = sum c[i] x[i] + d I on the npad x npad leading block (the identity on the first n rows only: the
// padding stays zero); dst may be one of the x.  Ends with a barrier.
template <typename F, int LD>
__device__ inline void tile_combine(F* dst, int npad, int n, int nops, const F* const* x, const F* c, F d) {
  for (int e = threadIdx.x; e < npad * npad; e += TILE_THREADS) {
    const int i = e / npad, j = e % npad, at = i * LD + j;
    F v = (i == j && i < n) ? d : F(0);
    for (int o = 0; o < nops; ++o) v += c[o] * x[o][at];
    dst[at] = v;
  }
  __syncthreads();
}

// L X = R for the n x n leading blocks of two LDS buffers, X left in R; L is destroyed.
//
// Elimination, step k: every wave finds the pivot of column k for itself (a lane a row, a butterfly
// whose order does not depend on the wave: no broadcast, no barrier), the rows k and p change places
// in the columns right of k and in R, a barrier, and row i > k takes -(l_ik / pivot) times row k in
// those columns: thread t owns column t % 128 of [L | R] and the rows k + 1 + t / 128, + 4, ...
// Column k itself is left as it was (its multipliers are read through the interchange, its pivot goes
// to diag[k]): the forward substitution happens on R in the same pass and nothing reads L's lower
// triangle again.  Two barriers a step.
// Back substitution, step k: x_k = r_k / diag[k] is formed by whoever needs it and row k is NOT
// rewritten while others read it, so a step is one barrier; one last pass divides the rows.
template <typename F, int LD>
__device__ inline void tile_solve(F* L, F* R, F* diag, int n) {
  const int tid = threadIdx.x, lane = tid & 63;
  {
    const int col = tid & 127, grp = tid >> 7;
    F* M = col < 64 ? L + col : R + (col - 64);
    for (int k = 0; k < n; ++k) {
      // the largest |l_ik|, i >= k; the lowest row wins a tie; a NaN counts as the largest
      F best = F(-1);
      int p = lane;
      if (lane >= k && lane < n) {
        const F v = L[lane * LD + k];
        best = v != v ? F(INFINITY) : fabs(v);
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const F ob = __shfl_xor(best, off, 64);
        const int op = __shfl_xor(p, off, 64);
        if (ob > best || (ob == best && op < p)) { best = ob; p = op; }
      }
      if (p < k || p >= n) p = k;            // (cannot happen: row k itself is a candidate)
      const F pivot = L[p * LD + k], lkk = L[k * LD + k];
      if (tid == 0) diag[k] = pivot;
      const bool live = col < 64 ? (col > k && col < n) : (col - 64 < n);
      if (live && grp == 0 && p != k) {
        const F t = M[k * LD];
        M[k * LD] = M[p * LD];
        M[p * LD] = t;
      }
      __syncthreads();
      if (live) {
        const F rp = F(1) / pivot, top = M[k * LD];
        for (int i = k + 1 + grp; i < n; i += TILE_THREADS / 128) {
          const F lik = i == p ? lkk : L[i * LD + k];
          M[i * LD] -= (lik * rp) * top;
        }
      }
      __syncthreads();
    }
  }
  const int j = lane, grp = tid >> 6;
  for (int k = n - 1; k >= 0; --k) {
    if (j < n) {
      const F xk = R[k * LD + j] / diag[k];
      for (int i = grp; i < k; i += TILE_WAVES) R[i * LD + j] -= L[i * LD + k] * xk;
    }
    __syncthreads();
  }
  for (int e = tid; e < n * n; e += TILE_THREADS) {
    const int i = e / n, jj = e % n;
    R[i * LD + jj] = R[i * LD + jj] / diag[i];
  }
  __syncthreads();
}

template <typename F>
__global__ __launch_bounds__(TILE_THREADS) void expm_tile_kernel(TileArgs a) {
  constexpr int N = Tile<F>::N, LD = N + 1, SZ = N * LD;
  __shared__ double colsum[64];
  __shared__ F diag[64];
  F* const A = reinterpret_cast<F*>(expm_lds);
  F *const A2 = A + SZ, *const A4 = A + 2 * SZ, *const A6 = A + 3 * SZ, *const T = A + 4 * SZ,
    *const U = A + 5 * SZ, *const V = A + 6 * SZ;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = a.n, npad = (n + 15) & ~15, nt = npad / 16;
  const int64_t b = blockIdx.x;
  const F* Ag = static_cast<const F*>(a.A) + b * a.a_bs;
  F* Og = static_cast<F*>(a.out) + b * a.o_bs;
  if (n == 1) {
    // the exponential of a 1 x 1 matrix is the exponential of its entry (scipy.linalg.expm's shortcut as
    // well): no Pade approximant, whose denominator cancels for a positive entry near theta_13
    if (tid == 0) {
      const F x = Ag[0];
      Og[0] = exp(x);
      if (a.status != nullptr) write_status(a.status, b, fabs((double)x), 0, 0);
    }
    return;
  }
  for (int e = tid; e < npad * npad; e += TILE_THREADS) {
    const int i = e / npad, j = e % npad;
    A[i * LD + j] = i < n && j < n ? Ag[i * a.a_rs + j * a.a_cs] : F(0);
  }
  __syncthreads();
  // ||A||_1: a wave a column, a lane a row, the sums in double
  for (int j = wave; j < n; j += TILE_WAVES) {
    const double v = wave_sum(lane < n ? fabs((double)A[lane * LD + j]) : 0.0);
    if (lane == 0) colsum[j] = v;
  }
  __syncthreads();
  double norm = 0;
  for (int j = 0; j < n; ++j) norm = norm_max(norm, colsum[j]);
  int m, s;
  pade_choice(norm, m, s);
  if (tid == 0 && a.status != nullptr) write_status(a.status, b, norm, m, s);
  if (s > 0) {
    for (int e = tid; e < npad * npad; e += TILE_THREADS) {
      const int at = (e / npad) * LD + e % npad;
      A[at] = ldexp(A[at], -s);              // exact (short of underflow)
    }
    __syncthreads();
  }
  // the powers, then U = A (sum of the odd coefficients' terms) and V = the even ones'
  tile_product<F, LD>(A2, A, A, nt);
  if (m >= 5) tile_product<F, LD>(A4, A2, A2, nt);
  if (m >= 7) tile_product<F, LD>(A6, A4, A2, nt);
  const F* x[4];
  F c[4];
  if (m <= 9) {
    if (m == 9) tile_product<F, LD>(T, A4, A4, nt);
    const int terms = m / 2;
    for (int odd = 1; odd >= 0; --odd) {
      for (int o = 0; o < terms; ++o) {
        x[o] = A + (o + 1) * SZ;           // A^2, A^4, A^6, A^8: adjacent buffers
        c[o] = pade_coeff<F>(m, 2 * o + 2 + odd);
      }
      tile_combine<F, LD>(V, npad, n, terms, x, c, pade_coeff<F>(m, odd));
      if (odd) tile_product<F, LD>(U, A, V, nt);
    }
  } else {
    // degree 13: A^6 (c_13 A^6 + c_11 A^4 + c_9 A^2) + c_7 A^6 + c_5 A^4 + c_3 A^2 + c_1 I, and the even twin
    for (int odd = 1; odd >= 0; --odd) {
      x[0] = A6; x[1] = A4; x[2] = A2;
      for (int o = 0; o < 3; ++o) c[o] = pade_coeff<F>(13, 12 - 2 * o + odd);
      tile_combine<F, LD>(T, npad, n, 3, x, c, F(0));
      tile_product<F, LD>(V, A6, T, nt);
      x[0] = V; x[1] = A6; x[2] = A4; x[3] = A2;
      c[0] = F(1);
      for (int o = 0; o < 3; ++o) c[o + 1] = pade_coeff<F>(13, 6 - 2 * o + odd);
      tile_combine<F, LD>(V, npad, n, 4, x, c, pade_coeff<F>(13, odd));
      if (odd) tile_product<F, LD>(U, A, V, nt);
    }
  }
  // (V - U) X = V + U; the powers are dead: their buffers take the two sides
  F *L = A2, *X = A4, *Y = A6;
  for (int e = tid; e < npad * npad; e += TILE_THREADS) {
    const int at = (e / npad) * LD + e % npad;
    const F u = U[at], v = V[at];
    L[at] = v - u;
    X[at] = v + u;
  }
  __syncthreads();
  tile_solve<F, LD>(L, X, diag, n);
  for (int q = 0; q < s; ++q) {
    tile_product<F, LD>(Y, X, X, nt);
    F* t = X; X = Y; Y = t;
  }
  for (int e = tid; e < n * n; e += TILE_THREADS) {
    const int i = e / n, j = e % n;
    Og[i * a.o_rs + j * a.o_cs] = X[i * LD + j];
  }
}

// ------------------------------------------------------------------ the blocked path -----------
struct NormArgs {
  const void* A;
  double* colsum;  // n column sums
  void* status;
  int64_t rs, cs, n;
};
AHIP_PTRS_BEGIN(NormArgs) AHIP_PTR1(A) AHIP_PTR1(colsum) AHIP_PTR1(status) AHIP_PTRS_END

// 64 columns a workgroup: thread t sums every fourth row of column t % 64 in double, the four partial
// sums of a column are added in a fixed order
template <typename F>
__global__ __launch_bounds__(256) void expm_colsum_kernel(NormArgs a) {
  __shared__ double part[4][64];
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int64_t j = (int64_t)blockIdx.x * 64 + lane;
  const F* A = static_cast<const F*>(a.A);
  double acc = 0;
  if (j < a.n) {
#pragma unroll 4
    for (int64_t i = grp; i < a.n; i += 4) acc += fabs((double)A[i * a.rs + j * a.cs]);
  }
  part[grp][lane] = acc;
  __syncthreads();
  if (grp == 0 && j < a.n) a.colsum[j] = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
}

// one workgroup: the largest column sum, then m and s into the status record
__global__ __launch_bounds__(256) void expm_fold_kernel(NormArgs a) {
  __shared__ double red[256];
  double top = 0;
  for (int64_t j = threadIdx.x; j < a.n; j += 256) top = norm_max(top, a.colsum[j]);
  red[threadIdx.x] = top;
  __syncthreads();
  for (int half = 128; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half) red[threadIdx.x] = norm_max(red[threadIdx.x], red[threadIdx.x + half]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    int m, s;
    pade_choice(red[0], m, s);
    write_status(a.status, 0, red[0], m, s);
  }
}

struct CombineArgs {
  const void* x[4];  // contiguous n x n operands, the first nops of them
  void* out;         // contiguous n x n; may be one of the operands
  double c[4], d;
  int64_t n;
  int nops;
};
AHIP_PTRS_BEGIN(CombineArgs) AHIP_PTRA(x, 4) AHIP_PTR1(out) AHIP_PTRS_END

template <typename F>
__global__ __launch_bounds__(256) void expm_combine_kernel(CombineArgs a) {
  const int64_t total = a.n * a.n, step = (int64_t)gridDim.x * 256;
  F* out = static_cast<F*>(a.out);
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += step) {
    F v = e % (a.n + 1) == 0 ? (F)a.d : F(0);
    for (int o = 0; o < a.nops; ++o) v += (F)a.c[o] * static_cast<const F*>(a.x[o])[e];
    out[e] = v;
  }
}

template <typename F>
int launch_tile(int64_t batch, TileArgs& a, hipStream_t s) {
  static bool allowed = false;
  if (!allowed) {
    if (int rc = allow_lds(expm_tile_kernel<F>, tile_lds<F>())) return rc;
    allowed = true;
  }
  AHIP_LAUNCH(expm_tile_kernel<F>, dim3((unsigned)batch), dim3(TILE_THREADS), tile_lds<F>(), s, a);
  return AHIP_OK;
}

}  // namespace

extern "C" {

int ahip_expm_tile(int dtype, int64_t batch, int64_t n, const void* A, int64_t a_bs, int64_t a_rs, int64_t a_cs,
                   void* out, int64_t o_bs, int64_t o_rs, int64_t o_cs, void* status, void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "expm: float32 / float64 only, got dtype %d", dtype);
  const int limit = dtype == AHIP_F32 ? AHIP_EXPM_TILE_F32 : AHIP_EXPM_TILE_F64;
  AHIP_REQUIRE(n >= 0 && n <= limit, "expm_tile: %lld rows (at most %d in this dtype)", (long long)n, limit);
  AHIP_REQUIRE(batch >= 0 && batch < MAX_N, "expm_tile: batch of %lld", (long long)batch);
  if (n == 0 || batch == 0) return AHIP_OK;
  AHIP_REQUIRE(A != nullptr && out != nullptr, "null pointer");
  TileArgs a;
  a.A = A; a.out = out; a.status = status;
  a.a_bs = a_bs; a.a_rs = a_rs; a.a_cs = a_cs; a.o_bs = o_bs; a.o_rs = o_rs; a.o_cs = o_cs;
  a.n = (int)n;
  return dtype == AHIP_F32 ? launch_tile<float>(batch, a, as_stream(stream))
                           : launch_tile<double>(batch, a, as_stream(stream));
}

int ahip_expm_norm1(int dtype, int64_t n, const void* A, int64_t rs, int64_t cs, double* colsum, void* status,
                    void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "expm: float32 / float64 only, got dtype %d", dtype);
  AHIP_REQUIRE(n > 0 && n < MAX_N, "expm_norm1: %lld rows", (long long)n);
  AHIP_REQUIRE(A != nullptr && colsum != nullptr && status != nullptr, "null pointer");
  NormArgs a;
  a.A = A; a.colsum = colsum; a.status = status; a.rs = rs; a.cs = cs; a.n = n;
  hipStream_t s = as_stream(stream);
  AHIP_LAUNCH_F(dtype, expm_colsum_kernel, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, s, a);
  AHIP_LAUNCH(expm_fold_kernel, dim3(1), dim3(256), 0, s, a);
  return AHIP_OK;
}

int ahip_expm_combine(int dtype, int64_t n, int nops, const void* x0, double c0, const void* x1, double c1,
                      const void* x2, double c2, const void* x3, double c3, double d, void* out, void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "expm: float32 / float64 only, got dtype %d", dtype);
  AHIP_REQUIRE(n > 0 && n < MAX_N && nops >= 1 && nops <= 4, "expm_combine: %d operands of %lld rows", nops,
               (long long)n);
  CombineArgs a;
  a.x[0] = x0; a.x[1] = x1; a.x[2] = x2; a.x[3] = x3;
  a.c[0] = c0; a.c[1] = c1; a.c[2] = c2; a.c[3] = c3;
  a.d = d; a.out = out; a.n = n; a.nops = nops;
  for (int o = 0; o < nops; ++o) AHIP_REQUIRE(a.x[o] != nullptr, "null pointer");
  AHIP_REQUIRE(out != nullptr, "null pointer");
  hipStream_t s = as_stream(stream);
  AHIP_LAUNCH_F(dtype, expm_combine_kernel, dim3(stream_grid(n * n)), dim3(256), 0, s, a);
  return AHIP_OK;
}

}  // extern "C"
