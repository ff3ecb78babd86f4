// K18t: LU with partial pivoting of a STACK of small matrices, one launch for the whole stack
// (float32 / float64, n <= AHIP_LU_TILE): the determinant and / or the inverse of every matrix.
//
// The batched form of tensor/nlinalg.py:100 MatrixInverse and :196 Det (np.linalg.inv / det on a
// [T, n, n] operand: LAPACK getrf + getri per matrix).  The algorithm is the one of csrc/linalg.hip —
// right-looking, one column at a time, the lowest row wins a pivot tie, det = sign of the interchanges
// times the diagonal of U folded in ahip_lu_det's order, inverse = both substitutions on the columns of
// P I — but a matrix never leaves LDS between its first load and its last store: HBM is read once and
// written once per matrix.
//
// LDS, per matrix: the tile S (n rows at pitch ld = n | 1: odd, so a walk down a column touches every
// bank once), the right-hand block B of the same shape when the inverse is wanted, the row permutation
// and one word for the next pivot row.
//
// A GROUP of threads owns a matrix.  n <= 32: a group is one wavefront, four groups a workgroup, and the
// only synchronisation is the wavefront's own (no workgroup barrier on this path, so a wave of the
// ragged last workgroup that has no matrix just leaves).  33 <= n <= 64: a group is the workgroup of 256
// threads and the synchronisation is __syncthreads, two per column.  Thread t of a group is (r, q) =
// (t mod R, t div R) with R = 32 / 64 rows: in a column step it owns row r and every Q-th column of the
// rank-1 update (Q = 2 / 4), in a substitution step column r of B and every Q-th row.
//
// A column step j:   [sync]  rows j and p change places (p: found in step j - 1)   [sync]
//                    row r > j:  l = s_rj / s_jj;  s_rk -= l s_jk for the thread's columns k > j;
//                    the threads q = 0 (the first wavefront) took column j + 1 first and now hold its new
//                    values: their cross-lane arg-max is p of step j + 1.
// The multipliers are NOT written back during the factorisation (another wavefront may still be reading
// the unscaled column): every reader divides by the same pivot, and one pass after the last column
// stores l = s_rj / s_jj — the same quotient, the same bits.  The substitutions are column-oriented (one
// sync a step) and leave the rows of U x = y unscaled for the same reason; the final store divides.
//
// The 16x16x4 matrix instructions are not used: a column step is a rank-1 update, and at n <= 64 a
// substitution blocked by 16 would still walk 16 dependent steps per block on the vector ALU.
#include "dense.h"

namespace {

constexpr int TILE = AHIP_LU_TILE;
constexpr int WAVE_N = AHIP_LU_TILE_WAVE;     // up to here: one wavefront a matrix
constexpr int THREADS = 256;
constexpr size_t MAX_LDS = 72 * 1024;

struct LuTileArgs {
  const void* A;   // [batch, n, n] by element strides
  void* inv;       // [batch, n, n] contiguous, or null
  void* det;       // [batch], or null
  void* info;      // info word or null
  int64_t a_bs, a_rs, a_cs, batch;
  int n, ld;
};
AHIP_PTRS_BEGIN(LuTileArgs) AHIP_PTR1(A) AHIP_PTR1(inv) AHIP_PTR1(det) AHIP_PTR1(info) AHIP_PTRS_END

// what a group needs in LDS: (elements of F, ints)
__host__ __device__ inline size_t tile_elems(int n, int ld, bool inv) { return (size_t)(inv ? 2 : 1) * n * ld; }
__host__ __device__ inline size_t tile_ints(int n) { return (size_t)n + 1; }

// the lanes of ONE wavefront see each other's LDS traffic in program order; this only keeps the
// compiler from moving LDS accesses across the point
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <bool WG>
__device__ __forceinline__ void group_sync() {
  if (WG) __syncthreads();
  else wave_sync();
}

// arg-max over the 64 lanes of (v, i): the larger value, then the lower row; lane 0's answer is the
// one that is used
template <typename F>
__device__ __forceinline__ void wave_argmax(F& v, int& i) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const F ov = __shfl_xor(v, off, 64);
    const int oi = __shfl_xor(i, off, 64);
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
}

// |x| as a pivot candidate; a NaN is never chosen (like the `v > best` of getrf_panel_kernel)
template <typename F>
__device__ __forceinline__ F candidate(F x) { return x == x ? fabs(x) : F(-1); }

// One matrix by one group of NT = R * Q threads, t the thread's index in the group.  Every thread of
// the group runs every sync of this function.
template <typename F, bool WG>
__device__ __forceinline__ void lu_tile(const LuTileArgs& a, int64_t b, int t, F* S, int* ip) {
  constexpr int NT = WG ? THREADS : 64, R = WG ? 64 : 32, Q = NT / R;
  const int n = a.n, ld = a.ld, r = t % R, q = t / R;
  const bool rowfast = (a.a_rs < 0 ? -a.a_rs : a.a_rs) < (a.a_cs < 0 ? -a.a_cs : a.a_cs);
  const F* A = static_cast<const F*>(a.A) + b * a.a_bs;
  F* B = S + n * ld;                      // (only touched when a.inv is set)
  int* perm = ip;                         // perm[i]: the row of A that stands in row i
  int* pnext = ip + n;

  // ---- the only read of HBM: consecutive threads along the operand's faster dimension
  for (int e = t; e < n * n; e += NT) {
    const int i = rowfast ? e % n : e / n, k = rowfast ? e / n : e % n;
    S[i * ld + k] = A[i * a.a_rs + k * a.a_cs];
  }
  if (t < n) perm[t] = t;
  group_sync<WG>();
  if (t < 64 && n > 0) {
    F v = (q == 0 && r < n) ? candidate(S[r * ld]) : F(-1);
    int i = r;
    wave_argmax(v, i);
    if (t == 0) *pnext = (v >= F(0) && i < n) ? i : 0;
  }

  // ---- factorisation
  int odd = 0;
  bool singular = false;
  for (int j = 0; j < n; ++j) {
    group_sync<WG>();                     // the updates of step j - 1 and its choice of p
    const int p = *pnext;
    if (p != j) {
      odd ^= 1;
      if (t < n) {
        const F top = S[j * ld + t];
        S[j * ld + t] = S[p * ld + t];
        S[p * ld + t] = top;
      }
      if (t == 0) {
        const int pj = perm[j];
        perm[j] = perm[p];
        perm[p] = pj;
      }
    }
    group_sync<WG>();
    const F pivot = S[j * ld + j];
    const bool zero = pivot == F(0);      // the column is all zero from here down: nothing to eliminate
    singular = singular || zero;
    F v = F(-1);
    if (r > j && r < n) {
      F* row = S + r * ld;
      if (!zero) {
        const F l = row[j] / pivot;
        const F* top = S + j * ld;
        for (int k = j + 1 + q; k < n; k += Q) row[k] -= l * top[k];
      }
      if (q == 0 && j + 1 < n) v = candidate(row[j + 1]);
    }
    if (t < 64 && j + 1 < n) {
      int i = r;
      wave_argmax(v, i);
      if (t == 0) *pnext = (v >= F(0) && i > j && i < n) ? i : j + 1;
    }
  }
  group_sync<WG>();
  if (singular && t == 0 && a.inv != nullptr) report(a.info, AHIP_LINALG_SINGULAR, b);

  // ---- determinant: the fold of lu_det_kernel (lane t holds u_tt, then a tree from 32 down)
  if (a.det != nullptr && t < 64) {
    F prod = t < n ? S[t * ld + t] : F(1);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) prod *= __shfl_down(prod, off, 64);
    if (t == 0) static_cast<F*>(a.det)[b] = odd ? -prod : prod;
  }
  if (a.inv == nullptr) return;

  // ---- inverse
  F* out = static_cast<F*>(a.inv) + b * (int64_t)n * n;
  if (singular) {                         // (uniform over the group; nothing divides by a zero pivot)
    for (int e = t; e < n * n; e += NT) out[e] = F(NAN);
    return;
  }
  for (int e = t; e < n * n; e += NT) {
    const int i = e / n, k = e % n;
    if (i > k) S[i * ld + k] = S[i * ld + k] / S[k * ld + k];
    B[i * ld + k] = perm[i] == k ? F(1) : F(0);
  }
  // L y = P I, unit lower: after step k rows <= k + 1 of B are final
  for (int k = 0; k + 1 < n; ++k) {
    group_sync<WG>();
    if (r < n) {
      const F yk = B[k * ld + r];
      for (int i = k + 1 + q; i < n; i += Q) B[i * ld + r] -= S[i * ld + k] * yk;
    }
  }
  // U x = y: row k of B stays u_kk x_k, every reader divides
  for (int k = n - 1; k > 0; --k) {
    group_sync<WG>();
    if (r < n) {
      const F xk = B[k * ld + r] / S[k * ld + k];
      for (int i = q; i < k; i += Q) B[i * ld + r] -= S[i * ld + k] * xk;
    }
  }
  group_sync<WG>();
  // ---- the only write to HBM
  for (int e = t; e < n * n; e += NT) {
    const int i = e / n, k = e % n;
    out[e] = B[i * ld + k] / S[i * ld + i];
  }
}

// n <= WAVE_N: a wavefront a matrix, four a workgroup, no workgroup barrier anywhere
template <typename F>
__global__ __launch_bounds__(THREADS) void lu_tile_wave_kernel(LuTileArgs a) {
  extern __shared__ __align__(16) unsigned char lds[];
  constexpr int G = THREADS / 64;
  const int w = threadIdx.x >> 6;
  const int64_t b = (int64_t)blockIdx.x * G + w;
  if (b >= a.batch) return;
  const size_t elems = tile_elems(a.n, a.ld, a.inv != nullptr);
  F* S = reinterpret_cast<F*>(lds) + w * elems;
  int* ip = reinterpret_cast<int*>(reinterpret_cast<F*>(lds) + G * elems) + w * tile_ints(a.n);
  lu_tile<F, false>(a, b, threadIdx.x & 63, S, ip);
}

// WAVE_N < n <= TILE: the workgroup a matrix
template <typename F>
__global__ __launch_bounds__(THREADS) void lu_tile_group_kernel(LuTileArgs a) {
  extern __shared__ __align__(16) unsigned char lds[];
  F* S = reinterpret_cast<F*>(lds);
  int* ip = reinterpret_cast<int*>(S + tile_elems(a.n, a.ld, a.inv != nullptr));
  lu_tile<F, true>(a, blockIdx.x, threadIdx.x, S, ip);
}

template <typename F>
int launch_lu_tile(LuTileArgs& a, hipStream_t s) {
  static bool allowed = false;
  if (!allowed) {
    if (int rc = allow_lds(lu_tile_wave_kernel<F>, MAX_LDS)) return rc;
    if (int rc = allow_lds(lu_tile_group_kernel<F>, MAX_LDS)) return rc;
    allowed = true;
  }
  const bool inv = a.inv != nullptr;
  if (a.n <= WAVE_N) {
    constexpr int G = THREADS / 64;
    const size_t lds = G * (tile_elems(a.n, a.ld, inv) * sizeof(F) + tile_ints(a.n) * sizeof(int));
    const unsigned grid = (unsigned)((a.batch + G - 1) / G);
    AHIP_LAUNCH(lu_tile_wave_kernel<F>, dim3(grid), dim3(THREADS), lds, s, a);
  } else {
    const size_t lds = tile_elems(a.n, a.ld, inv) * sizeof(F) + tile_ints(a.n) * sizeof(int);
    AHIP_LAUNCH(lu_tile_group_kernel<F>, dim3((unsigned)a.batch), dim3(THREADS), lds, s, a);
  }
  return AHIP_OK;
}

}  // namespace

extern "C" {

int ahip_lu_tile_max(void) { return TILE; }

int ahip_lu_tile(int dtype, int64_t batch, int64_t n, const void* A, int64_t a_bs, int64_t a_rs, int64_t a_cs,
                 void* inv, void* det, void* info, void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "linalg: float32 / float64 only, got dtype %d", dtype);
  AHIP_REQUIRE(n >= 0 && n <= TILE, "lu_tile: %lld rows (at most %d)", (long long)n, TILE);
  AHIP_REQUIRE(batch >= 0 && batch < MAX_N, "lu_tile: batch of %lld", (long long)batch);
  if (batch == 0 || (n == 0 && det == nullptr)) return AHIP_OK;
  AHIP_REQUIRE(inv != nullptr || det != nullptr, "lu_tile: neither inverse nor determinant asked for");
  AHIP_REQUIRE(n == 0 || A != nullptr, "null pointer");
  LuTileArgs a;
  a.A = A; a.inv = n == 0 ? nullptr : inv; a.det = det; a.info = info;
  a.a_bs = a_bs; a.a_rs = a_rs; a.a_cs = a_cs; a.batch = batch;
  a.n = (int)n; a.ld = (int)n | 1;
  hipStream_t s = as_stream(stream);
  return dtype == AHIP_F32 ? launch_lu_tile<float>(a, s) : launch_lu_tile<double>(a, s);
}

}  // extern "C"
