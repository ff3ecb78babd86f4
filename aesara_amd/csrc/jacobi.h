// What the two Jacobi solvers share (eig.hip: two-sided, symmetric eigenvalues; svd.hip: one-sided,
// singular values): the tile geometry, the round-robin ordering, the rotation record of a step and
// its application to an LDS-resident tile, and the launch of a tile kernel.  How a rotation's angle
// is chosen is NOT shared: each solver has its own numerics, next to its kernel.
//
// The kernels stay in their translation units; this header, like dense.h, has internal linkage only.
#pragma once
#include "dense.h"

namespace {

constexpr int TM = AHIP_SYEV_TILE;          // rows / columns of a tile
constexpr int BS = TM / 2;                  // rows / columns of a block of the tournament
constexpr int LD = TM + 1;                  // LDS row pitch: a column walk is conflict-free
constexpr int NSWEEP = AHIP_SYEV_NSWEEP;
constexpr int TILE_THREADS = 512;
constexpr int TILE_WAVES = TILE_THREADS / 64;

// The circle method for m2 players (m2 even): in step k of m2 - 1, pair 0 is (m2 - 1, k) and pair i
// is ((k + i) mod (m2 - 1), (k - i) mod (m2 - 1)).  The pairs of a step are disjoint and every two
// players meet once in m2 - 1 steps.  Returns p < q.
__device__ inline void rr_pair(int m2, int k, int i, int& p, int& q) {
  const int r = m2 - 1;
  const int a = i == 0 ? r : (k + i) % r;
  const int b = (k - i + r) % r;
  p = a < b ? a : b;
  q = a < b ? b : a;
}

// row / column of the whole matrix that row / column e of the tile of blocks (p, q) stands for
__device__ inline int64_t pair_index(int p, int q, int e) {
  return e < BS ? (int64_t)p * BS + e : (int64_t)q * BS + (e - BS);
}

// The rotations of one step of a two-sided solve, one a pair: five LDS arrays of BS entries that
// the tile kernel declares (its own, so that their addresses stay link-time constants).  The first
// threads of the workgroup write them, a barrier, every wave reads them.  `on` is 0 for the exact
// identity.
template <typename F>
struct Rotations {
  F *c, *s;
  int *p, *q, *on;
};

// The `np` rotations of a step applied to the m x m tile S and to the accumulated J, both in LDS at
// pitch LD, by a workgroup of TILE_THREADS: the column rotations S <- S G, J <- J G (a wave takes a
// pair, a lane a row), a barrier, the row rotations S <- G^T S (a lane a column), a barrier.
template <typename F>
__device__ inline void apply_rotations(F* S, F* J, const Rotations<F>& rot, int np, int m) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = wave; i < np; i += TILE_WAVES) {
    if (!rot.on[i] || lane >= m) continue;
    const int p = rot.p[i], q = rot.q[i];
    const F c = rot.c[i], s = rot.s[i];
    F x = S[lane * LD + p], y = S[lane * LD + q];
    S[lane * LD + p] = c * x - s * y;
    S[lane * LD + q] = s * x + c * y;
    x = J[lane * LD + p]; y = J[lane * LD + q];
    J[lane * LD + p] = c * x - s * y;
    J[lane * LD + q] = s * x + c * y;
  }
  __syncthreads();
  for (int i = wave; i < np; i += TILE_WAVES) {
    if (!rot.on[i] || lane >= m) continue;
    const int p = rot.p[i], q = rot.q[i];
    const F c = rot.c[i], s = rot.s[i];
    const F x = S[p * LD + lane], y = S[q * LD + lane];
    // a_pq = a_qp = 0 exactly: what the angle was chosen for
    S[p * LD + lane] = lane == q ? F(0) : c * x - s * y;
    S[q * LD + lane] = lane == p ? F(0) : s * x + c * y;
  }
  __syncthreads();
}

// One workgroup of TILE_THREADS a tile, the tile and its rotations (2 x TM x LD elements) in dynamic
// LDS.  In double that is 65 KiB of the 160: above the default limit, so it is asked for once.
template <auto KERNEL_F32, auto KERNEL_F64, typename Args>
int launch_tiles(int dtype, int64_t tiles, Args& a, hipStream_t s) {
  const dim3 grid((unsigned)tiles), block(TILE_THREADS);
  if (dtype == AHIP_F32) {
    AHIP_LAUNCH(KERNEL_F32, grid, block, 2 * TM * LD * sizeof(float), s, a);
    return AHIP_OK;
  }
  const size_t lds = 2 * TM * LD * sizeof(double);
  static bool allowed = false;
  if (!allowed) {
    if (int rc = allow_lds(KERNEL_F64, lds)) return rc;
    allowed = true;
  }
  AHIP_LAUNCH(KERNEL_F64, grid, block, lds, s, a);
  return AHIP_OK;
}

}  // namespace
