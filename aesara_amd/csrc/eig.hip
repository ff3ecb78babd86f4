// K21: symmetric eigenvalues by two-sided Jacobi, and the Cholesky step of the generalised problem
// (float32 / float64).
//
// replaces tensor/slinalg.py:446 Eigvalsh and :493 EigvalshGrad (scipy.linalg.eigvalsh / eigh:
// LAPACK syevr / sygvd).
//
// Jacobi with the round-robin ("circle") ordering (jacobi.h) needs no tridiagonalisation: the m/2
// rotations of a step touch disjoint pairs of rows and columns, so a step is two barriers, and the
// accumulated rotations ARE the eigenvectors the gradient needs.  ahip_syev_tile solves tiles of at most 64 x 64
// entirely in LDS, one workgroup a tile.  A larger matrix is a tournament of 32-wide blocks: per
// step ahip_syev_gather copies every pair of blocks into a 64 x 64 tile, the tile solver returns
// its rotation matrix J, and ahip_syev_apply multiplies the two block columns of every pair by J on
// the matrix instructions (A <- A J, A <- J^T A on the transposed view, V <- V J).  The tournament
// loop, the sweep loop and the convergence read are the host's (exec_eig.py); every dependency
// between workgroups is a launch boundary: no kernel here waits for another workgroup.
//
// All matrices are addressed by (row, col) element strides.  Errors travel through the optional
// info word of K18 (dense.h; kind AHIP_LINALG_EIG).  Every fold has a fixed order (no float
// atomics): the same call gives the same bits.
#include "jacobi.h"

namespace {

constexpr int PARTIALS = AHIP_SYEV_OFF_PARTIALS;
// words of the status record
constexpr int ST_DONE = 0, ST_SWEEPS = 1, ST_OFF2 = 2, ST_NORM2 = 3, ST_PARTIALS = 4;

template <typename F> struct Lim;
template <> struct Lim<float> { static constexpr float big = 1e18f; };     // theta^2 stays finite below it
template <> struct Lim<double> { static constexpr double big = 1e150; };

// sum over a workgroup, the same value in every thread: lanes by shuffles, waves in wave order
template <int WAVES>
__device__ inline double block_sum(double v, double* red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0;
  for (int w = 0; w < WAVES; ++w) t += red[w];
  __syncthreads();
  return t;
}

// ------------------------------------------------------------------ the LDS-resident solver ----
struct TileArgs {
  const void* A;   // batch of m x m symmetric tiles; only the triangle `lower` names is read
  void* S;         // the rotated tiles (diagonal = eigenvalues, unsorted), or null
  void* J;         // the accumulated rotations (columns = eigenvectors), or null
  void* w;         // the diagonals of the rotated tiles, or null
  void* status;    // status record or null: word ST_SWEEPS takes the largest sweep count
  void* info;      // info word or null: no convergence after NSWEEP sweeps
  int64_t a_bs, a_rs, a_cs, s_bs, s_rs, s_cs, j_bs, j_rs, j_cs, w_bs;
  double tol2;     // sweeps end at off_F^2 <= tol2 * ||A||_F^2
  int m, lower;
};
AHIP_PTRS_BEGIN(TileArgs) AHIP_PTR1(A) AHIP_PTR1(S) AHIP_PTR1(J) AHIP_PTR1(w) AHIP_PTR1(status)
  AHIP_PTR1(info) AHIP_PTRS_END

extern __shared__ __align__(16) unsigned char eig_lds[];

template <typename F>
__device__ inline double tile_sum(const F* S, int m, bool offdiag, double* red) {
  double acc = 0;
  for (int e = threadIdx.x; e < m * m; e += TILE_THREADS) {
    const int i = e / m, k = e % m;
    const double v = (double)S[i * LD + k];
    if (!offdiag || i != k) acc += v * v;
  }
  return block_sum<TILE_WAVES>(acc, red);
}

// One workgroup a tile.  S and J stay in LDS for the whole solve.  A step: the first m2 / 2 threads
// take (c, s) of their pair from a_pp, a_qq, a_pq; then apply_rotations (jacobi.h).  The norms are
// accumulated in double whatever F is: the squares of a float32 tile of entries near 1e-19 would be
// flushed to zero and stop the sweeps early.
template <typename F>
__global__ __launch_bounds__(TILE_THREADS) void syev_tile_kernel(TileArgs a) {
  __shared__ F rot_c[BS], rot_s[BS];
  __shared__ int rot_p[BS], rot_q[BS], rot_on[BS];
  const Rotations<F> rot{rot_c, rot_s, rot_p, rot_q, rot_on};
  __shared__ double red[TILE_WAVES];
  F* S = reinterpret_cast<F*>(eig_lds);
  F* J = S + TM * LD;
  const int tid = threadIdx.x, m = a.m;
  const int64_t b = blockIdx.x;
  const F* A = static_cast<const F*>(a.A) + b * a.a_bs;
  for (int e = tid; e < m * m; e += TILE_THREADS) {
    const int i = e / m, k = e % m;
    const bool named = a.lower ? i >= k : i <= k;
    S[i * LD + k] = named ? A[i * a.a_rs + k * a.a_cs] : A[k * a.a_rs + i * a.a_cs];
    J[i * LD + k] = F(i == k ? 1 : 0);
  }
  __syncthreads();
  const int m2 = (m + 1) & ~1, np = m2 / 2;
  const double norm2 = tile_sum(S, m, false, red);
  // an error already recorded for this node (B not positive definite): the operand is not what
  // it should be, so no sweeps are spent on it and nothing more is reported
  const bool skip = failed(a.info);
  int sweeps = 0;
  bool conv;
  while (true) {
    const double off2 = tile_sum(S, m, true, red);
    conv = !(off2 > a.tol2 * norm2);          // (a NaN ends the sweeps too)
    if (conv || skip || sweeps == NSWEEP) break;
    for (int k = 0; k < m2 - 1; ++k) {
      if (tid < np) {
        int p, q;
        rr_pair(m2, k, tid, p, q);
        F c = F(1), s = F(0);
        bool on = q < m;                       // the phantom index of an odd m sits out
        if (on) {
          const F apq = S[p * LD + q];
          if (apq != F(0)) {
            const F theta = (S[q * LD + q] - S[p * LD + p]) / (F(2) * apq);
            const F at = fabs(theta);
            const F t = at > Lim<F>::big ? F(0.5) / theta
                                         : copysign(F(1), theta) / (at + sqrt(theta * theta + F(1)));
            c = F(1) / sqrt(t * t + F(1));
            s = t * c;
          } else {
            on = false;                        // the exact identity
          }
        }
        rot.p[tid] = p; rot.q[tid] = q; rot.c[tid] = c; rot.s[tid] = s; rot.on[tid] = on;
      }
      __syncthreads();
      apply_rotations(S, J, rot, np, m);
    }
    ++sweeps;
  }
  F* So = static_cast<F*>(a.S);
  F* Jo = static_cast<F*>(a.J);
  for (int e = tid; e < m * m; e += TILE_THREADS) {
    const int i = e / m, k = e % m;
    if (So != nullptr) So[b * a.s_bs + i * a.s_rs + k * a.s_cs] = S[i * LD + k];
    if (Jo != nullptr) Jo[b * a.j_bs + i * a.j_rs + k * a.j_cs] = J[i * LD + k];
  }
  if (a.w != nullptr && tid < m) static_cast<F*>(a.w)[b * a.w_bs + tid] = S[tid * LD + tid];
  if (tid == 0) {
    if (a.status != nullptr)
      atomicMax(static_cast<unsigned long long*>(a.status) + ST_SWEEPS, (unsigned long long)sweeps);
    if (!conv && !skip) report(a.info, AHIP_LINALG_EIG, 0);
  }
}

// ------------------------------------------------------------------ the tournament's tiles -----
struct GatherArgs {
  const void* A;   // (32 nb) x (32 nb)
  void* T;         // nb / 2 contiguous 64 x 64 tiles
  int64_t rs, cs;
  int nb, step;
};
AHIP_PTRS_BEGIN(GatherArgs) AHIP_PTR1(A) AHIP_PTR1(T) AHIP_PTRS_END

template <typename F>
__global__ __launch_bounds__(256) void syev_gather_kernel(GatherArgs a) {
  int p, q;
  rr_pair(a.nb, a.step, blockIdx.x, p, q);
  const F* A = static_cast<const F*>(a.A);
  F* T = static_cast<F*>(a.T) + (int64_t)blockIdx.x * TM * TM;
  for (int e = threadIdx.x; e < TM * TM; e += 256)
    T[e] = A[pair_index(p, q, e / TM) * a.rs + pair_index(p, q, e % TM) * a.cs];
}

// ------------------------------------------------------------------ the blocked update ---------
struct ApplyArgs {
  const void* X;   // rows x (32 nb)
  const void* J;   // nb / 2 contiguous 64 x 64 rotation matrices, row-major
  void* Y;         // rows x (32 nb), not X
  int64_t x_rs, x_cs, y_rs, y_cs, rows;
  int nb, step;
};
AHIP_PTRS_BEGIN(ApplyArgs) AHIP_PTR1(X) AHIP_PTR1(J) AHIP_PTR1(Y) AHIP_PTRS_END

// Y[:, p|q] = X[:, p|q] J_pair for the pairs of a step: grid (pair, tile of 64 rows), four waves
// of 16 rows each.  J_pair is staged once in LDS; a wave's 16 x 64 strip of X goes from memory
// straight into the A operand of the 16x16x4 matrix instruction (lane l holds x[l % 16][4 ks +
// l / 16]), four accumulator fragments cover the 64 columns, K = 64 is 16 instructions each.
template <typename F>
__global__ __launch_bounds__(256) void syev_apply_kernel(ApplyArgs a) {
  typedef typename Mma<F>::acc_t acc_t;
  __shared__ F Js[TM][LD];
  int p, q;
  rr_pair(a.nb, a.step, blockIdx.x, p, q);
  const F* Jg = static_cast<const F*>(a.J) + (int64_t)blockIdx.x * TM * TM;
  for (int e = threadIdx.x; e < TM * TM; e += 256) Js[e / TM][e % TM] = Jg[e];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.y * TM + wave * 16;
  const F* X = static_cast<const F*>(a.X);
  F* Y = static_cast<F*>(a.Y);
  acc_t acc[4];
  for (int f = 0; f < 4; ++f) acc[f] = acc_t{0, 0, 0, 0};
  const bool in_rows = r0 + li < a.rows;
#pragma unroll 4
  for (int ks = 0; ks < TM / 4; ++ks) {
    const int kk = ks * 4 + lk;
    const F xv = in_rows ? X[(r0 + li) * a.x_rs + pair_index(p, q, kk) * a.x_cs] : F(0);
#pragma unroll
    for (int f = 0; f < 4; ++f) Mma<F>::mma(acc[f], xv, Js[kk][f * 16 + li]);
  }
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    const int64_t col = pair_index(p, q, f * 16 + li);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = r0 + Mma<F>::row(lane, r);
      if (row < a.rows) Y[row * a.y_rs + col * a.y_cs] = acc[f][r];
    }
  }
}

// ------------------------------------------------------------------ the convergence test -------
struct OffArgs {
  const void* A;
  void* status;
  const void* info;
  int64_t rs, cs, n;
  double tol2;
  int parts;
};
AHIP_PTRS_BEGIN(OffArgs) AHIP_PTR1(A) AHIP_PTR1(status) AHIP_PTR1(info) AHIP_PTRS_END

// workgroup partials of 2 sum_{i > j} a_ij^2 and sum_i a_ii^2 over the LOWER triangle (the one the
// tile solver reads), in double
template <typename F>
__global__ __launch_bounds__(256) void syev_off_partial_kernel(OffArgs a) {
  __shared__ double red[4];
  const F* A = static_cast<const F*>(a.A);
  const int64_t total = a.n * a.n;
  double off = 0, dia = 0;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t i = e / a.n, j = e % a.n;
    if (i < j) continue;
    const double v = (double)A[i * a.rs + j * a.cs];
    if (i == j) dia += v * v;
    else off += 2 * v * v;
  }
  off = block_sum<4>(off, red);
  dia = block_sum<4>(dia, red);
  if (threadIdx.x == 0) {
    double* part = reinterpret_cast<double*>(static_cast<unsigned long long*>(a.status) + ST_PARTIALS);
    part[2 * blockIdx.x] = off;
    part[2 * blockIdx.x + 1] = dia;
  }
}

// one workgroup folds the partials in a fixed tree and writes off_F^2, ||A||_F^2 and the done word:
// converged, not comparable (NaN), or an error already recorded for the node
__global__ __launch_bounds__(PARTIALS) void syev_off_final_kernel(OffArgs a) {
  __shared__ double so[PARTIALS], sd[PARTIALS];
  unsigned long long* st = static_cast<unsigned long long*>(a.status);
  const double* part = reinterpret_cast<const double*>(st + ST_PARTIALS);
  const int t = threadIdx.x;
  so[t] = t < a.parts ? part[2 * t] : 0.0;
  sd[t] = t < a.parts ? part[2 * t + 1] : 0.0;
  __syncthreads();
  for (int half = PARTIALS / 2; half > 0; half >>= 1) {
    if (t < half) { so[t] += so[t + half]; sd[t] += sd[t + half]; }
    __syncthreads();
  }
  if (t == 0) {
    const double off2 = so[0], norm2 = so[0] + sd[0];
    const bool fail = failed(a.info);
    st[ST_OFF2] = (unsigned long long)__double_as_longlong(off2);
    st[ST_NORM2] = (unsigned long long)__double_as_longlong(norm2);
    st[ST_DONE] = (!(off2 > a.tol2 * norm2) || fail) ? 1ull : 0ull;
  }
}

// ------------------------------------------------------------------ Cholesky diagonal block ----
struct PotrfArgs {
  void* B;         // nb x nb block on the diagonal, factored in place in the named triangle
  void* info;
  int64_t rs, cs, base;
  int nb, lower;
};
AHIP_PTRS_BEGIN(PotrfArgs) AHIP_PTR1(B) AHIP_PTR1(info) AHIP_PTRS_END

// ONE workgroup, unblocked right-looking (LAPACK potf2): B = L L^T (lower) or U^T U (upper; the
// upper triangle is held transposed in LDS, so both are the same loop).  A pivot that is not a
// positive finite number is reported (the 1-based order of the leading minor) and the block is
// left as it was.
template <typename F>
__global__ __launch_bounds__(256) void potrf_diag_kernel(PotrfArgs a) {
  __shared__ F S[TM][LD];
  const int tid = threadIdx.x, nb = a.nb;
  F* B = static_cast<F*>(a.B);
  for (int e = tid; e < nb * nb; e += 256) {
    const int i = e / nb, k = e % nb;
    if (i >= k) S[i][k] = a.lower ? B[i * a.rs + k * a.cs] : B[k * a.rs + i * a.cs];
  }
  __syncthreads();
  for (int j = 0; j < nb; ++j) {
    const F d = S[j][j];
    if (!(d > F(0)) || !isfinite(d)) {          // (the same value in every thread)
      if (tid == 0) report(a.info, AHIP_LINALG_EIG, a.base + j + 1);
      return;
    }
    const F l = sqrt(d);
    __syncthreads();
    if (tid == j) S[j][j] = l;
    else if (tid > j && tid < nb) S[tid][j] = S[tid][j] / l;
    __syncthreads();
    const int r = nb - j - 1;
    for (int e = tid; e < r * r; e += 256) {
      const int i = j + 1 + e / r, k = j + 1 + e % r;
      if (k <= i) S[i][k] -= S[i][j] * S[k][j];
    }
    __syncthreads();
  }
  for (int e = tid; e < nb * nb; e += 256) {
    const int i = e / nb, k = e % nb;
    if (i >= k) {
      if (a.lower) B[i * a.rs + k * a.cs] = S[i][k];
      else B[k * a.rs + i * a.cs] = S[i][k];
    }
  }
}

// ------------------------------------------------------------------ small helpers --------------
struct DiagArgs {
  const void* A;
  void* w;
  int64_t rs, cs, n;
};
AHIP_PTRS_BEGIN(DiagArgs) AHIP_PTR1(A) AHIP_PTR1(w) AHIP_PTRS_END

template <typename F>
__global__ __launch_bounds__(256) void diag_kernel(DiagArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < a.n) static_cast<F*>(a.w)[i] = static_cast<const F*>(a.A)[i * (a.rs + a.cs)];
}

struct ScaleArgs {
  const void* V;
  const int64_t* perm;   // or null: column j of the result is column perm[j] of V
  const void* g;         // or null
  const void* h;         // or null
  void* out;
  int64_t v_rs, v_cs, o_rs, o_cs, rows, cols;
};
AHIP_PTRS_BEGIN(ScaleArgs) AHIP_PTR1(V) AHIP_PTR1(perm) AHIP_PTR1(g) AHIP_PTR1(h) AHIP_PTR1(out) AHIP_PTRS_END

// out[:, j] = V[:, perm[j]] * g[j] * h[j]; a perm entry outside [0, cols) gives a zero column
template <typename F>
__global__ __launch_bounds__(256) void scale_cols_kernel(ScaleArgs a) {
  const F* V = static_cast<const F*>(a.V);
  const F* g = static_cast<const F*>(a.g);
  const F* h = static_cast<const F*>(a.h);
  F* out = static_cast<F*>(a.out);
  const int64_t total = a.rows * a.cols;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t i = e / a.cols, j = e % a.cols;
    const int64_t src = a.perm != nullptr ? a.perm[j] : j;
    F v = F(0);
    if (src >= 0 && src < a.cols) {
      v = V[i * a.v_rs + src * a.v_cs];
      if (g != nullptr) v *= g[j];
      if (h != nullptr) v *= h[j];
    }
    out[i * a.o_rs + j * a.o_cs] = v;
  }
}

struct FoldArgs {
  const void* G;
  void* out;
  int64_t g_rs, g_cs, o_rs, o_cs, n;
  int lower;
};
AHIP_PTRS_BEGIN(FoldArgs) AHIP_PTR1(G) AHIP_PTR1(out) AHIP_PTRS_END

// out = tri0(G) + tri1(G)^T (EigvalshGrad.perform): the named triangle takes g_ij + g_ji, the
// diagonal g_ii, the other triangle zero
template <typename F>
__global__ __launch_bounds__(256) void sym_fold_kernel(FoldArgs a) {
  const F* G = static_cast<const F*>(a.G);
  F* out = static_cast<F*>(a.out);
  const int64_t total = a.n * a.n;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t i = e / a.n, j = e % a.n;
    const bool named = a.lower ? i > j : i < j;
    F v = F(0);
    if (i == j) v = G[i * a.g_rs + i * a.g_cs];
    else if (named) v = G[i * a.g_rs + j * a.g_cs] + G[j * a.g_rs + i * a.g_cs];
    out[i * a.o_rs + j * a.o_cs] = v;
  }
}

}  // namespace

extern "C" {

int ahip_syev_tile(int dtype, int lower, int64_t batch, int64_t m, const void* A, int64_t a_bs,
                   int64_t a_rs, int64_t a_cs, void* S, int64_t s_bs, int64_t s_rs, int64_t s_cs,
                   void* J, int64_t j_bs, int64_t j_rs, int64_t j_cs, void* w, int64_t w_bs,
                   double tol_scale, void* status, void* info, void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "syev: float32 / float64 only, got dtype %d", dtype);
  AHIP_REQUIRE(m >= 0 && m <= TM, "syev_tile: tile of %lld rows (at most %d)", (long long)m, TM);
  AHIP_REQUIRE(batch >= 0 && batch < MAX_N, "syev_tile: batch of %lld", (long long)batch);
  AHIP_REQUIRE(tol_scale > 0 && tol_scale <= 1, "syev_tile: tol_scale outside (0, 1]");
  if (m == 0 || batch == 0) return AHIP_OK;
  AHIP_REQUIRE(A != nullptr, "null pointer");
  TileArgs a;
  a.A = A; a.S = S; a.J = J; a.w = w; a.status = status; a.info = info;
  a.a_bs = a_bs; a.a_rs = a_rs; a.a_cs = a_cs; a.s_bs = s_bs; a.s_rs = s_rs; a.s_cs = s_cs;
  a.j_bs = j_bs; a.j_rs = j_rs; a.j_cs = j_cs; a.w_bs = w_bs;
  a.m = (int)m; a.lower = lower != 0;
  a.tol2 = eps_of(dtype) * eps_of(dtype) * tol_scale;
  return launch_tiles<syev_tile_kernel<float>, syev_tile_kernel<double>>(dtype, batch, a, as_stream(stream));
}

int ahip_syev_gather(int dtype, int64_t nb, int64_t step, const void* A, int64_t rs, int64_t cs, void* T,
                     void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "syev: float32 / float64 only, got dtype %d", dtype);
  AHIP_REQUIRE(nb >= 2 && nb % 2 == 0 && nb * BS < MAX_N && step >= 0 && step < nb - 1,
               "syev_gather: step %lld of a tournament of %lld blocks", (long long)step, (long long)nb);
  AHIP_REQUIRE(A != nullptr && T != nullptr, "null pointer");
  GatherArgs a;
  a.A = A; a.T = T; a.rs = rs; a.cs = cs; a.nb = (int)nb; a.step = (int)step;
  hipStream_t s = as_stream(stream);
  AHIP_LAUNCH_F(dtype, syev_gather_kernel, dim3((unsigned)(nb / 2)), dim3(256), 0, s, a);
  return AHIP_OK;
}

int ahip_syev_apply(int dtype, int64_t nb, int64_t step, int64_t rows, const void* X, int64_t x_rs,
                    int64_t x_cs, const void* J, void* Y, int64_t y_rs, int64_t y_cs, void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "syev: float32 / float64 only, got dtype %d", dtype);
  AHIP_REQUIRE(nb >= 2 && nb % 2 == 0 && nb * BS < MAX_N && step >= 0 && step < nb - 1,
               "syev_apply: step %lld of a tournament of %lld blocks", (long long)step, (long long)nb);
  AHIP_REQUIRE(rows >= 0 && rows < MAX_N, "syev_apply: %lld rows", (long long)rows);
  if (rows == 0) return AHIP_OK;
  AHIP_REQUIRE(X != nullptr && J != nullptr && Y != nullptr && X != Y, "syev_apply: null or aliased pointers");
  ApplyArgs a;
  a.X = X; a.J = J; a.Y = Y; a.x_rs = x_rs; a.x_cs = x_cs; a.y_rs = y_rs; a.y_cs = y_cs; a.rows = rows;
  a.nb = (int)nb; a.step = (int)step;
  const dim3 grid((unsigned)(nb / 2), (unsigned)((rows + TM - 1) / TM));
  hipStream_t s = as_stream(stream);
  AHIP_LAUNCH_F(dtype, syev_apply_kernel, grid, dim3(256), 0, s, a);
  return AHIP_OK;
}

int ahip_syev_off(int dtype, int64_t n, const void* A, int64_t rs, int64_t cs, void* status, const void* info,
                  void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "syev: float32 / float64 only, got dtype %d", dtype);
  AHIP_REQUIRE(n > 0 && n < MAX_N, "syev_off: n = %lld", (long long)n);
  AHIP_REQUIRE(A != nullptr && status != nullptr, "null pointer");
  OffArgs a;
  a.A = A; a.status = status; a.info = info; a.rs = rs; a.cs = cs; a.n = n;
  a.tol2 = eps_of(dtype) * eps_of(dtype);
  const int64_t want = (n * n + 2047) / 2048;
  a.parts = (int)(want < PARTIALS ? want : PARTIALS);
  hipStream_t s = as_stream(stream);
  AHIP_LAUNCH_F(dtype, syev_off_partial_kernel, dim3(a.parts), dim3(256), 0, s, a);
  AHIP_LAUNCH(syev_off_final_kernel, dim3(1), dim3(PARTIALS), 0, s, a);
  return AHIP_OK;
}

int ahip_potrf_diag(int dtype, int lower, int64_t nb, void* B, int64_t rs, int64_t cs, int64_t base,
                    void* info, void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "potrf_diag: float32 / float64 only, got dtype %d", dtype);
  AHIP_REQUIRE(nb >= 0 && nb <= TM, "potrf_diag: block of %lld rows (at most %d)", (long long)nb, TM);
  AHIP_REQUIRE(base >= 0 && base < MAX_N, "potrf_diag: extent out of range");
  if (nb == 0) return AHIP_OK;
  AHIP_REQUIRE(B != nullptr, "null pointer");
  PotrfArgs a;
  a.B = B; a.info = info; a.rs = rs; a.cs = cs; a.base = base; a.nb = (int)nb; a.lower = lower != 0;
  hipStream_t s = as_stream(stream);
  AHIP_LAUNCH_F(dtype, potrf_diag_kernel, dim3(1), dim3(256), 0, s, a);
  return AHIP_OK;
}

int ahip_syev_diag(int dtype, int64_t n, const void* A, int64_t rs, int64_t cs, void* w, void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "syev: float32 / float64 only, got dtype %d", dtype);
  AHIP_REQUIRE(n >= 0 && n < MAX_N, "syev_diag: n = %lld", (long long)n);
  if (n == 0) return AHIP_OK;
  AHIP_REQUIRE(A != nullptr && w != nullptr, "null pointer");
  DiagArgs a;
  a.A = A; a.w = w; a.rs = rs; a.cs = cs; a.n = n;
  const unsigned grid = (unsigned)((n + 255) / 256);
  hipStream_t s = as_stream(stream);
  AHIP_LAUNCH_F(dtype, diag_kernel, dim3(grid), dim3(256), 0, s, a);
  return AHIP_OK;
}

int ahip_scale_cols(int dtype, int64_t rows, int64_t cols, const void* V, int64_t v_rs, int64_t v_cs,
                    const int64_t* perm, const void* g, const void* h, void* out, int64_t o_rs, int64_t o_cs,
                    void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "scale_cols: float32 / float64 only, got dtype %d", dtype);
  AHIP_REQUIRE(rows >= 0 && rows < MAX_N && cols >= 0 && cols < MAX_N, "scale_cols: extent out of range");
  if (rows == 0 || cols == 0) return AHIP_OK;
  AHIP_REQUIRE(V != nullptr && out != nullptr && V != out, "scale_cols: null or aliased pointers");
  ScaleArgs a;
  a.V = V; a.perm = perm; a.g = g; a.h = h; a.out = out;
  a.v_rs = v_rs; a.v_cs = v_cs; a.o_rs = o_rs; a.o_cs = o_cs; a.rows = rows; a.cols = cols;
  hipStream_t s = as_stream(stream);
  AHIP_LAUNCH_F(dtype, scale_cols_kernel, dim3(stream_grid(rows * cols)), dim3(256), 0, s, a);
  return AHIP_OK;
}

int ahip_sym_fold(int dtype, int lower, int64_t n, const void* G, int64_t g_rs, int64_t g_cs, void* out,
                  int64_t o_rs, int64_t o_cs, void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "sym_fold: float32 / float64 only, got dtype %d", dtype);
  AHIP_REQUIRE(n >= 0 && n < MAX_N, "sym_fold: n = %lld", (long long)n);
  if (n == 0) return AHIP_OK;
  AHIP_REQUIRE(G != nullptr && out != nullptr && G != out, "sym_fold: null or aliased pointers");
  FoldArgs a;
  a.G = G; a.out = out; a.g_rs = g_rs; a.g_cs = g_cs; a.o_rs = o_rs; a.o_cs = o_cs; a.n = n;
  a.lower = lower != 0;
  hipStream_t s = as_stream(stream);
  AHIP_LAUNCH_F(dtype, sym_fold_kernel, dim3(stream_grid(n * n)), dim3(256), 0, s, a);
  return AHIP_OK;
}

}  // extern "C"
