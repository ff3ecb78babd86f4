// K22: the singular value decomposition under the pseudo-inverse, by one-sided (Hestenes) Jacobi
// (float32 / float64).
//
// replaces tensor/nlinalg.py:16 MatrixPinv (np.linalg.pinv: LAPACK gesdd, then V diag(1/s) U^T).
//
// One-sided Jacobi works on A itself: a rotation of the columns p and q makes them orthogonal, the
// accumulated rotations are V, the rotated matrix is W = A V = U diag(s).  A pair rotates only if
// |x_p . x_q| > tol ||x_p|| ||x_q|| (Demmel and Veselic): a threshold relative to the two columns,
// not to the matrix, which is what keeps the small singular values — the ones a pseudo-inverse
// divides by — as accurate as the large ones.  ahip_gesvj_tile solves tiles of at most 64 x 64
// entirely in LDS, one workgroup a tile, ONE barrier a step.  Above 64 columns 32-wide column blocks
// play a tournament in the round-robin ordering of jacobi.h: per step ahip_gesvj_gram forms the
// 64 x 64 Gram matrix of every pair of blocks on the matrix instructions (slab partials, no atomics),
// ahip_gesvj_gram_tile folds the partials, diagonalises each Gram matrix by two-sided rotations
// under the same scaled threshold and returns its rotation matrix J, and ahip_syev_apply (a kernel
// of eig.hip) multiplies the block columns of A and V by J.  ahip_gesvj_done sums a sweep's rotation counts; ahip_pinv_weights turns column norms
// (or eigenvalues) into the reciprocals the pseudo-inverse scales by.
//
// Every dependency between workgroups is a launch boundary: no kernel here waits for another
// workgroup.  Every fold has a fixed order (no float atomics): the same call gives the same bits.
// Errors travel through the info word of K18 (dense.h; kind AHIP_LINALG_EIG, k = 0).
#include "jacobi.h"

#include <cmath>

namespace {

constexpr int SLAB = AHIP_GESVJ_SLAB;       // rows of A behind one partial Gram matrix
constexpr int HEAD = AHIP_GESVJ_STATUS_HEAD;
// words of the status record
constexpr int ST_DONE = 0, ST_SWEEPS = 1, ST_ROTATIONS = 2, ST_TILE_SWEEPS = 3;

// sum of small counts over a workgroup, the same value in every thread
template <int WAVES>
__device__ inline int block_count(int v, int* red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
  for (int w = 0; w < WAVES; ++w) t += red[w];
  __syncthreads();
  return t;
}

// (c, s) of the rotation that makes two columns of squared norms al, be and inner product ga
// orthogonal: theta = (be - al) / (2 ga), t the smaller root of t^2 + 2 theta t - 1, in double
__device__ inline void rotation(double al, double be, double ga, double& c, double& s) {
  const double theta = (be - al) / (2.0 * ga);
  const double at = fabs(theta);
  const double t = at > 1e150 ? 0.5 / theta : copysign(1.0, theta) / (at + sqrt(theta * theta + 1.0));
  c = 1.0 / sqrt(t * t + 1.0);
  s = t * c;
}

extern __shared__ __align__(16) unsigned char svd_lds[];

// ------------------------------------------------------------------ the LDS-resident solver ----
struct TileArgs {
  const void* X;   // batch of rows x cols tiles
  void* W;         // the rotated tiles X V (orthogonal columns of norms s), rows x cols
  void* V;         // the accumulated rotations, cols x cols
  double* norm2;   // the squared norms of the columns of W, cols a tile, or null
  void* status;    // status record or null: word ST_TILE_SWEEPS takes the largest sweep count
  void* info;      // info word or null: no convergence after NSWEEP sweeps
  int64_t x_bs, x_rs, x_cs, w_bs, w_rs, w_cs, v_bs, v_rs, v_cs, n_bs;
  double tol;
  int rows, cols;
};
AHIP_PTRS_BEGIN(TileArgs) AHIP_PTR1(X) AHIP_PTR1(W) AHIP_PTR1(V) AHIP_PTR1(norm2) AHIP_PTR1(status)
  AHIP_PTR1(info) AHIP_PTRS_END

// One workgroup a tile; X and V stay in LDS for the whole solve.  A step of the circle ordering has
// cols / 2 disjoint column pairs: a wave takes a pair and a lane a row, the three sums fold across
// the wave in double, and the same wave rotates both columns of X and of V.  No wave touches a
// column of another wave's pair, so a step is ONE barrier.  A zero column has ga = 0 exactly: it
// never rotates and stays zero.
template <typename F>
__global__ __launch_bounds__(TILE_THREADS) void gesvj_tile_kernel(TileArgs a) {
  __shared__ int red[TILE_WAVES];
  F* X = reinterpret_cast<F*>(svd_lds);
  F* V = X + TM * LD;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, rows = a.rows, cols = a.cols;
  const int64_t b = blockIdx.x;
  const F* Xg = static_cast<const F*>(a.X) + b * a.x_bs;
  for (int e = tid; e < TM * TM; e += TILE_THREADS) {
    const int i = e / TM, k = e % TM;
    X[i * LD + k] = i < rows && k < cols ? Xg[i * a.x_rs + k * a.x_cs] : F(0);
    V[i * LD + k] = F(i == k ? 1 : 0);
  }
  __syncthreads();
  const int m2 = (cols + 1) & ~1, np = m2 / 2;
  // an error already recorded for this node (a non-finite operand): no sweeps are spent on it
  const bool skip = failed(a.info);
  int sweeps = 0;
  bool conv = false;
  while (!skip && !conv && sweeps < NSWEEP) {
    int rotated = 0;
    for (int k = 0; k < m2 - 1; ++k) {
      for (int i = wave; i < np; i += TILE_WAVES) {
        int p, q;
        rr_pair(m2, k, i, p, q);
        if (q >= cols) continue;                 // the phantom index of an odd count sits out
        const F xp = X[lane * LD + p], xq = X[lane * LD + q];
        const double dp = (double)xp, dq = (double)xq;
        const double al = wave_sum(dp * dp), be = wave_sum(dq * dq), ga = wave_sum(dp * dq);
        if (!(fabs(ga) > a.tol * (sqrt(al) * sqrt(be)))) continue;   // (the same in every lane; a NaN too)
        double cd, sd;
        rotation(al, be, ga, cd, sd);
        const F c = (F)cd, s = (F)sd;
        X[lane * LD + p] = c * xp - s * xq;
        X[lane * LD + q] = s * xp + c * xq;
        const F vp = V[lane * LD + p], vq = V[lane * LD + q];
        V[lane * LD + p] = c * vp - s * vq;
        V[lane * LD + q] = s * vp + c * vq;
        ++rotated;
      }
      __syncthreads();
    }
    ++sweeps;
    conv = block_count<TILE_WAVES>(lane == 0 ? rotated : 0, red) == 0;
  }
  F* Wo = static_cast<F*>(a.W) + b * a.w_bs;
  F* Vo = static_cast<F*>(a.V) + b * a.v_bs;
  for (int e = tid; e < rows * cols; e += TILE_THREADS) {
    const int i = e / cols, k = e % cols;
    Wo[i * a.w_rs + k * a.w_cs] = X[i * LD + k];
  }
  for (int e = tid; e < cols * cols; e += TILE_THREADS) {
    const int i = e / cols, k = e % cols;
    Vo[i * a.v_rs + k * a.v_cs] = V[i * LD + k];
  }
  if (a.norm2 != nullptr) {
    for (int k = wave; k < cols; k += TILE_WAVES) {
      const double x = (double)X[lane * LD + k];
      const double n2 = wave_sum(x * x);
      if (lane == 0) a.norm2[b * a.n_bs + k] = n2;
    }
  }
  if (tid == 0) {
    if (a.status != nullptr)
      atomicMax(static_cast<unsigned long long*>(a.status) + ST_TILE_SWEEPS, (unsigned long long)sweeps);
    if (!conv && !skip) report(a.info, AHIP_LINALG_EIG, 0);
  }
}

// ------------------------------------------------------------------ the Gram matrices ----------
struct GramArgs {
  const void* A;   // rows x (32 nb)
  void* P;         // (pair, slab) contiguous 64 x 64 partial Gram matrices
  int64_t rs, cs, rows;
  int nb, step, slabs;
};
AHIP_PTRS_BEGIN(GramArgs) AHIP_PTR1(A) AHIP_PTR1(P) AHIP_PTRS_END

// the ten 16 x 16 fragments (fi <= fj) of the upper triangle of a 64 x 64 symmetric matrix, by rows
__host__ __device__ constexpr int frag(int fi, int fj) { return fi * 4 - fi * (fi - 1) / 2 + fj - fi; }

// P[pair, slab] = C^T C for the SLAB rows of the slab, C = [A_p A_q] (rows beyond `rows` read as
// zero): grid (pair, slab), four waves.  A wave takes the 16-row strips wave, wave + 4, ... of the
// slab, four rows an instruction: lane l loads c[r + l / 16][16 f + l % 16], f = 0 .. 3, and the
// four values are the A operand (C^T: lane l holds row l % 16, k = l / 16) of fragment row f and
// the B operand (lane l holds k = l / 16, column l % 16) of fragment column f alike — nothing is
// staged.  Only the ten fragments of the upper triangle are accumulated; the waves' fragments are
// added into one LDS tile in wave order and mirrored on the way out.
template <typename F>
__global__ __launch_bounds__(256) void gesvj_gram_kernel(GramArgs a) {
  typedef typename Mma<F>::acc_t acc_t;
  __shared__ F part[TM][LD];
  int p, q;
  rr_pair(a.nb, a.step, blockIdx.x, p, q);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const F* A = static_cast<const F*>(a.A);
  int64_t coff[4];
#pragma unroll
  for (int f = 0; f < 4; ++f) coff[f] = pair_index(p, q, f * 16 + li) * a.cs;
  acc_t acc[10];
#pragma unroll
  for (int g = 0; g < 10; ++g) acc[g] = acc_t{0, 0, 0, 0};
  const int64_t slab0 = (int64_t)blockIdx.y * SLAB;
  for (int strip = wave; strip < SLAB / 16; strip += 4) {
    const int64_t r0 = slab0 + strip * 16;
    if (r0 >= a.rows) break;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int64_t r = r0 + ks * 4 + lk;
      F x[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) x[f] = r < a.rows ? A[r * a.rs + coff[f]] : F(0);
#pragma unroll
      for (int fi = 0; fi < 4; ++fi)
#pragma unroll
        for (int fj = fi; fj < 4; ++fj) Mma<F>::mma(acc[frag(fi, fj)], x[fi], x[fj]);
    }
  }
  for (int turn = 0; turn < 4; ++turn) {
    if (wave == turn) {
#pragma unroll
      for (int fi = 0; fi < 4; ++fi)
#pragma unroll
        for (int fj = fi; fj < 4; ++fj)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            F& cell = part[fi * 16 + Mma<F>::row(lane, r)][fj * 16 + li];
            cell = turn == 0 ? acc[frag(fi, fj)][r] : cell + acc[frag(fi, fj)][r];
          }
    }
    __syncthreads();
  }
  F* P = static_cast<F*>(a.P) + ((int64_t)blockIdx.x * a.slabs + blockIdx.y) * TM * TM;
  for (int e = threadIdx.x; e < TM * TM; e += 256) {
    const int i = e / TM, j = e % TM;
    // a diagonal fragment holds both of its triangles; elsewhere the upper fragment is the source
    P[e] = (i / 16 <= j / 16) ? part[i][j] : part[j][i];
  }
}

// ------------------------------------------------------------------ the Gram tile solver -------
struct GramTileArgs {
  const void* P;   // (pair, slab) partial Gram matrices
  void* J;         // pair contiguous 64 x 64 rotation matrices, row-major
  void* status;    // slot HEAD + slot0 + pair takes the tile's rotation count
  int64_t slot0;
  double tol;
  int slabs;
};
AHIP_PTRS_BEGIN(GramTileArgs) AHIP_PTR1(P) AHIP_PTR1(J) AHIP_PTR1(status) AHIP_PTRS_END

// One workgroup a pair: G = sum of the slab partials in slab order, then two-sided Jacobi on G in
// LDS (apply_rotations of jacobi.h on a full tile) — a pair rotates only if |g_pq| > tol sqrt(g_pp
// g_qq), and the sweeps end with the first that rotates nothing.  A norm-wise stop would leave the couplings of columns of small norm
// unresolved.  A zero column of A is a zero row and column of G: it never rotates.
template <typename F>
__global__ __launch_bounds__(TILE_THREADS) void gesvj_gram_tile_kernel(GramTileArgs a) {
  __shared__ F rot_c[BS], rot_s[BS];
  __shared__ int rot_p[BS], rot_q[BS], rot_on[BS];
  const Rotations<F> rot{rot_c, rot_s, rot_p, rot_q, rot_on};
  __shared__ int red[TILE_WAVES];
  F* S = reinterpret_cast<F*>(svd_lds);
  F* J = S + TM * LD;
  const int tid = threadIdx.x;
  const F* P = static_cast<const F*>(a.P) + (int64_t)blockIdx.x * a.slabs * TM * TM;
  for (int e = tid; e < TM * TM; e += TILE_THREADS) {
    F g = F(0);
    for (int sl = 0; sl < a.slabs; ++sl) g += P[(int64_t)sl * TM * TM + e];
    S[(e / TM) * LD + e % TM] = g;
    J[(e / TM) * LD + e % TM] = F(e / TM == e % TM ? 1 : 0);
  }
  __syncthreads();
  const F tol = (F)a.tol;
  int total = 0;
  for (int sweep = 0; sweep < NSWEEP; ++sweep) {
    int mine = 0;
    for (int k = 0; k < TM - 1; ++k) {
      if (tid < BS) {
        int p, q;
        rr_pair(TM, k, tid, p, q);
        const F gpq = S[p * LD + q], gpp = S[p * LD + p], gqq = S[q * LD + q];
        F c = F(1), s = F(0);
        // (false for a NaN, and for a zero column: 0 > 0)
        const bool on = fabs(gpq) > tol * (sqrt(fabs(gpp)) * sqrt(fabs(gqq)));
        if (on) {
          double cd, sd;
          rotation((double)gpp, (double)gqq, (double)gpq, cd, sd);
          c = (F)cd; s = (F)sd;
          ++mine;
        }
        rot.p[tid] = p; rot.q[tid] = q; rot.c[tid] = c; rot.s[tid] = s; rot.on[tid] = on;
      }
      __syncthreads();
      apply_rotations(S, J, rot, BS, TM);
    }
    const int count = block_count<TILE_WAVES>(mine, red);
    total += count;
    if (count == 0) break;
  }
  F* Jo = static_cast<F*>(a.J) + (int64_t)blockIdx.x * TM * TM;
  for (int e = tid; e < TM * TM; e += TILE_THREADS) Jo[e] = J[(e / TM) * LD + e % TM];
  if (tid == 0)
    static_cast<unsigned long long*>(a.status)[HEAD + a.slot0 + blockIdx.x] = (unsigned long long)total;
}

// ------------------------------------------------------------------ the end of a sweep ---------
struct DoneArgs {
  void* status;
  const void* info;
  int64_t slots;
};
AHIP_PTRS_BEGIN(DoneArgs) AHIP_PTR1(status) AHIP_PTR1(info) AHIP_PTRS_END

// one workgroup: the rotations of the sweep, one more sweep counted, and the done word — no tile
// rotated, or an error already recorded for the node
__global__ __launch_bounds__(256) void gesvj_done_kernel(DoneArgs a) {
  __shared__ unsigned long long red[256];
  unsigned long long* st = static_cast<unsigned long long*>(a.status);
  unsigned long long acc = 0;
  for (int64_t i = threadIdx.x; i < a.slots; i += 256) acc += st[HEAD + i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int half = 128; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half) red[threadIdx.x] += red[threadIdx.x + half];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    st[ST_ROTATIONS] = red[0];
    st[ST_SWEEPS] = st[ST_SWEEPS] + 1;
    st[ST_DONE] = (red[0] == 0 || failed(a.info)) ? 1ull : 0ull;
  }
}

// ------------------------------------------------------------------ the weights ----------------
struct WeightArgs {
  const void* W;   // rows x cols with orthogonal columns, or null
  const void* w;   // cols signed eigenvalues (used when W is null)
  double* sigma;   // cols singular values, in double
  void* d;         // cols reciprocals in the working type
  int64_t w_rs, w_cs, rows, cols;
};
AHIP_PTRS_BEGIN(WeightArgs) AHIP_PTR1(W) AHIP_PTR1(w) AHIP_PTR1(sigma) AHIP_PTR1(d) AHIP_PTRS_END

constexpr int WT_THREADS = 1024, WT_WAVES = WT_THREADS / 64;

// ONE workgroup: sigma_j = ||W[:, j]|| (a wave takes every 16th row of 64 adjacent columns, the 16
// partial sums of a column are added in wave order; all in double) or |w_j|; their maximum; the
// cutoff 1e-15 max sigma of np.linalg.pinv, in double; d_j = 1 / sigma_j (1 / w_j for eigenvalues:
// the sign stays) where sigma_j > cutoff, else 0.
template <typename F>
__global__ __launch_bounds__(WT_THREADS) void pinv_weights_kernel(WeightArgs a) {
  __shared__ double part[WT_WAVES][64];
  __shared__ double wmax[WT_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const F* W = static_cast<const F*>(a.W);
  const F* w = static_cast<const F*>(a.w);
  double top = 0;
  if (W != nullptr) {
    for (int64_t c0 = 0; c0 < a.cols; c0 += 64) {
      const int64_t j = c0 + lane;
      double acc = 0;
      if (j < a.cols) {
#pragma unroll 4
        for (int64_t i = wave; i < a.rows; i += WT_WAVES) {
          const double v = (double)W[i * a.w_rs + j * a.w_cs];
          acc += v * v;
        }
      }
      part[wave][lane] = acc;
      __syncthreads();
      if (wave == 0 && j < a.cols) {
        double n2 = 0;
        for (int k = 0; k < WT_WAVES; ++k) n2 += part[k][lane];
        const double s = sqrt(n2);
        a.sigma[j] = s;
        top = fmax(top, s);
      }
      __syncthreads();
    }
  } else {
    for (int64_t j = tid; j < a.cols; j += WT_THREADS) {
      const double s = fabs((double)w[j]);
      a.sigma[j] = s;
      top = fmax(top, s);
    }
  }
  for (int off = 32; off > 0; off >>= 1) top = fmax(top, __shfl_xor(top, off, 64));
  if (lane == 0) wmax[wave] = top;
  __syncthreads();                              // (and sigma, written by this workgroup, is visible)
  for (int k = 0; k < WT_WAVES; ++k) top = fmax(top, wmax[k]);
  const double cutoff = AHIP_PINV_RCOND * top;
  F* d = static_cast<F*>(a.d);
  for (int64_t j = tid; j < a.cols; j += WT_THREADS) {
    const double s = a.sigma[j];
    const double v = W != nullptr ? s : (double)w[j];
    d[j] = s > cutoff ? (F)(1.0 / v) : F(0);
  }
}

}  // namespace

extern "C" {

int ahip_gesvj_tile(int dtype, int64_t batch, int64_t rows, int64_t cols, const void* X, int64_t x_bs,
                    int64_t x_rs, int64_t x_cs, void* W, int64_t w_bs, int64_t w_rs, int64_t w_cs, void* V,
                    int64_t v_bs, int64_t v_rs, int64_t v_cs, double* norm2, int64_t n_bs, void* status,
                    void* info, void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "gesvj: float32 / float64 only, got dtype %d", dtype);
  AHIP_REQUIRE(rows >= 0 && rows <= TM && cols >= 0 && cols <= rows,
               "gesvj_tile: tile of %lld x %lld (at most %d rows, no more columns than rows)",
               (long long)rows, (long long)cols, TM);
  AHIP_REQUIRE(batch >= 0 && batch < MAX_N, "gesvj_tile: batch of %lld", (long long)batch);
  if (cols == 0 || batch == 0) return AHIP_OK;
  AHIP_REQUIRE(X != nullptr && W != nullptr && V != nullptr, "null pointer");
  TileArgs a;
  a.X = X; a.W = W; a.V = V; a.norm2 = norm2; a.status = status; a.info = info;
  a.x_bs = x_bs; a.x_rs = x_rs; a.x_cs = x_cs; a.w_bs = w_bs; a.w_rs = w_rs; a.w_cs = w_cs;
  a.v_bs = v_bs; a.v_rs = v_rs; a.v_cs = v_cs; a.n_bs = n_bs;
  a.tol = AHIP_GESVJ_TOL(rows, eps_of(dtype));
  a.rows = (int)rows; a.cols = (int)cols;
  return launch_tiles<gesvj_tile_kernel<float>, gesvj_tile_kernel<double>>(dtype, batch, a, as_stream(stream));
}

int ahip_gesvj_gram(int dtype, int64_t nb, int64_t step, int64_t rows, const void* A, int64_t rs, int64_t cs,
                    void* P, void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "gesvj: float32 / float64 only, got dtype %d", dtype);
  AHIP_REQUIRE(nb >= 2 && nb % 2 == 0 && nb * BS < MAX_N && step >= 0 && step < nb - 1,
               "gesvj_gram: step %lld of a tournament of %lld blocks", (long long)step, (long long)nb);
  AHIP_REQUIRE(rows > 0 && rows < MAX_N, "gesvj_gram: %lld rows", (long long)rows);
  AHIP_REQUIRE(A != nullptr && P != nullptr, "null pointer");
  GramArgs a;
  a.A = A; a.P = P; a.rs = rs; a.cs = cs; a.rows = rows; a.nb = (int)nb; a.step = (int)step;
  a.slabs = (int)((rows + SLAB - 1) / SLAB);
  AHIP_REQUIRE(a.slabs <= 65535, "gesvj_gram: %lld rows are more than 65535 slabs", (long long)rows);
  const dim3 grid((unsigned)(nb / 2), (unsigned)a.slabs);
  hipStream_t s = as_stream(stream);
  AHIP_LAUNCH_F(dtype, gesvj_gram_kernel, grid, dim3(256), 0, s, a);
  return AHIP_OK;
}

int ahip_gesvj_gram_tile(int dtype, int64_t pairs, int64_t slabs, int64_t rows, const void* P, void* J,
                         void* status, int64_t slot0, void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "gesvj: float32 / float64 only, got dtype %d", dtype);
  AHIP_REQUIRE(pairs > 0 && pairs < MAX_N && slabs > 0 && slabs <= 65535 && rows > 0 && rows < MAX_N &&
                   slot0 >= 0 && slot0 < MAX_N * 32,
               "gesvj_gram_tile: %lld pairs of %lld slabs", (long long)pairs, (long long)slabs);
  AHIP_REQUIRE(P != nullptr && J != nullptr && status != nullptr, "null pointer");
  GramTileArgs a;
  a.P = P; a.J = J; a.status = status; a.slot0 = slot0; a.slabs = (int)slabs;
  a.tol = AHIP_GESVJ_TOL(rows, eps_of(dtype));
  return launch_tiles<gesvj_gram_tile_kernel<float>, gesvj_gram_tile_kernel<double>>(dtype, pairs, a,
                                                                                       as_stream(stream));
}

int ahip_gesvj_done(int64_t slots, void* status, const void* info, void* stream) {
  AHIP_REQUIRE(slots > 0 && slots < MAX_N * 32, "gesvj_done: %lld slots", (long long)slots);
  AHIP_REQUIRE(status != nullptr, "null pointer");
  DoneArgs a;
  a.status = status; a.info = info; a.slots = slots;
  AHIP_LAUNCH(gesvj_done_kernel, dim3(1), dim3(256), 0, as_stream(stream), a);
  return AHIP_OK;
}

int ahip_pinv_weights(int dtype, int64_t rows, int64_t cols, const void* W, int64_t w_rs, int64_t w_cs,
                      const void* w, double* sigma, void* d, void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "pinv_weights: float32 / float64 only, got dtype %d", dtype);
  AHIP_REQUIRE(rows >= 0 && rows < MAX_N && cols >= 0 && cols < MAX_N, "pinv_weights: extent out of range");
  if (cols == 0) return AHIP_OK;
  AHIP_REQUIRE((W != nullptr) != (w != nullptr), "pinv_weights: one of W and w");
  AHIP_REQUIRE(sigma != nullptr && d != nullptr, "null pointer");
  WeightArgs a;
  a.W = W; a.w = w; a.sigma = sigma; a.d = d; a.w_rs = w_rs; a.w_cs = w_cs; a.rows = rows; a.cols = cols;
  hipStream_t s = as_stream(stream);
  AHIP_LAUNCH_F(dtype, pinv_weights_kernel, dim3(1), dim3(WT_THREADS), 0, s, a);
  return AHIP_OK;
}

}  // extern "C"
