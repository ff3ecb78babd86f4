// What the dense-algebra translation units share (linalg, qr, eig, svd, sparse, fft, and the few
// helpers copy / pool / rng need).  Everything here has internal linkage: the library's dynamic
// symbols are the C-ABI of include/aesara_hip.h and nothing else.
#pragma once
#include "common.h"

#include <cfloat>

namespace {

inline bool float_dtype(int dt) { return dt == AHIP_F32 || dt == AHIP_F64; }
inline double eps_of(int dt) { return dt == AHIP_F32 ? (double)FLT_EPSILON : (double)DBL_EPSILON; }

// every extent of a dense operand stays below it: an int holds one, an int64_t the product of two
constexpr int64_t MAX_N = (int64_t)1 << 30;

// workgroups of 256 threads for a grid-stride loop over `items`: 8 a CU at the most, 1 at the least
inline unsigned stream_grid(int64_t items) {
  int64_t want = (items + 255) / 256;
  int64_t cap = (int64_t)ahip_cu_count() * 8;
  if (want > cap) want = cap;
  if (want < 1) want = 1;
  return (unsigned)want;
}

// lets a kernel take `lds` bytes of dynamic LDS: more than the default limit needs asking for
template <typename K>
int allow_lds(K kernel, size_t lds) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) {
    ahip_set_error("hipFuncSetAttribute: %s", hipGetErrorString(e));
    return AHIP_EHIP;
  }
  return AHIP_OK;
}

// kernel<float> or kernel<double> by dtype (checked with float_dtype before): for kernel templates
// whose only parameter is the element type
#define AHIP_LAUNCH_F(dtype, kernel, grid, block, shmem, stream, arg)                    \
  do {                                                                                   \
    if ((dtype) == AHIP_F32) AHIP_LAUNCH(kernel<float>, grid, block, shmem, stream, arg); \
    else AHIP_LAUNCH(kernel<double>, grid, block, shmem, stream, arg);                   \
  } while (0)

// ------------------------------------------------------------------ the info word of K18 -------
// TAG | kind << 32 | payload, written by one atomicMax, never a trap: the highest kind wins.
__device__ inline unsigned long long info_word(int kind, unsigned long long payload) {
  return (unsigned long long)AHIP_LINALG_INFO_TAG | ((unsigned long long)kind << 32) | payload;
}

// The payload 2^32 - 1 - k keeps, within a kind, the SMALLEST 0-based index k (what LAPACK's info
// reports), whatever the order the workgroups and launches meet them in.
__device__ inline void report(void* info, int kind, int64_t k) {
  if (info != nullptr)
    atomicMax(static_cast<unsigned long long*>(info), info_word(kind, 0xFFFFFFFFull - (unsigned long long)k));
}

// an error is already recorded for the node: its operands are not what they should be
__device__ inline bool failed(const void* info) {
  return info != nullptr && *static_cast<const unsigned long long*>(info) != 0;
}

// ------------------------------------------------------------------ device helpers -------------
// sum over the 64 lanes in a fixed order (xor butterfly: every lane ends with the same bits)
template <typename T>
__device__ inline T wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// The 16x16x4 matrix instruction: lane l gives a[l % 16][l / 16] and b[l / 16][l % 16]; element r
// of its accumulator is c[row(l, r)][l % 16].
template <typename F> struct Mma;
template <> struct Mma<float> {
  typedef float acc_t __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ void mma(acc_t& c, float x, float y) {
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(x, y, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int row(int lane, int r) { return (lane >> 4) * 4 + r; }
};
template <> struct Mma<double> {
  typedef double acc_t __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ void mma(acc_t& c, double x, double y) {
    c = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int row(int lane, int r) { return (lane >> 4) + 4 * r; }
};

}  // namespace
