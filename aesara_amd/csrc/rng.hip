// K17 — random streams: mrg_uniform of sandbox/rng_mrg.py (:373; C body :452-537) and
// MultinomialFromUniform / ChoiceFromUniform of sandbox/multinomial.py (C bodies :84-161, :279-388),
// restated for the device.  Every result has the bits of the reference's C code.
//
// MRG31k3p keeps six 31-bit words per stream: (x11, x12, x13) under MRG_M1 = 2^31 - 1 and
// (x21, x22, x23) under MRG_M2 = 2^31 - 21069.  One step is 32-bit integer arithmetic (shifts, masks,
// wrapping additions, six conditional subtractions); the sample is the difference of the two leading
// words, converted once and multiplied once.  Element i of the flattened sample belongs to stream
// i % n_streams, so stream s produces J_s = n_elements / n_streams (+1 for s < the remainder) samples
// one after another.
//
// The step is linear: the state after k steps is A1^k (x11, x12, x13) mod MRG_M1 and A2^k (x21, x22, x23)
// mod MRG_M2.  A stream's run is therefore cut into `parts` pieces of c = ceil(J_max / parts) steps: lane
// (p, s) loads stream s, jumps p*c steps with two 3x3 matrix-vector products in 64-bit integers
// (entries and words below 2^31: a product below 2^62, a row sum below 2^64) and produces the steps
// [p*c, min((p+1)*c, J_s)).  The matrices depend on p*c only and come from the host as a [parts, 18]
// table.  s is the fast lane index: for one step a wavefront's 64 stores are 64 consecutive elements.
// Loop bounds are functions of n_elements, n_streams and parts, never of state values.
//
// The two multinomial kernels run one lane per row of pvals, sequentially over the outcomes: the
// running sum is a double added in the reference's order (a parallel prefix sum would round
// differently and move a draw across a boundary).
#include "common.h"

namespace {

constexpr int32_t MRG_M1 = 2147483647;  // 2^31 - 1
constexpr int32_t MRG_M2 = 2147462579;  // 2^31 - 21069
constexpr int32_t MRG_MASK12 = 511;
constexpr int32_t MRG_MASK13 = 16777215;
constexpr int32_t MRG_MASK2 = 65535;
constexpr int32_t MRG_MULT2 = 21069;

struct MrgArgs {
  const int32_t* in;     // [n_streams][6]
  int32_t* out;          // [n_streams][6]; may be `in` when parts == 1
  void* sample;          // n_elements values, flat
  const int64_t* table;  // [parts][18]: A1^(p*c) then A2^(p*c), row-major (unused when parts == 1)
  int64_t n_elements, n_streams, parts, c;
};
AHIP_PTRS_BEGIN(MrgArgs) AHIP_PTR1(in) AHIP_PTR1(out) AHIP_PTR1(sample) AHIP_PTR1(table) AHIP_PTRS_END

// `if (y < 0 || y >= M) y -= M` on the wrapped 32-bit value (rng_mrg.py:487 ff.)
__device__ __forceinline__ uint32_t correct(uint32_t y, int32_t M) {
  const int32_t v = (int32_t)y;
  return (v < 0 || v >= M) ? y - (uint32_t)M : y;
}

struct State {
  int32_t x11, x12, x13, x21, x22, x23;
};

// One step (rng_mrg.py:486-511).  Additions wrap: done in uint32; shifts are those of int32.
__device__ __forceinline__ void step(State& st) {
  uint32_t y1 = (uint32_t)((st.x12 & MRG_MASK12) << 22) + (uint32_t)(st.x12 >> 9) +
                (uint32_t)((st.x13 & MRG_MASK13) << 7) + (uint32_t)(st.x13 >> 24);
  y1 = correct(y1, MRG_M1);
  y1 += (uint32_t)st.x13;
  y1 = correct(y1, MRG_M1);
  st.x13 = st.x12;
  st.x12 = st.x11;
  st.x11 = (int32_t)y1;

  y1 = (uint32_t)((st.x21 & MRG_MASK2) << 15) + (uint32_t)MRG_MULT2 * (uint32_t)(st.x21 >> 16);
  y1 = correct(y1, MRG_M2);
  uint32_t y2 = (uint32_t)((st.x23 & MRG_MASK2) << 15) + (uint32_t)MRG_MULT2 * (uint32_t)(st.x23 >> 16);
  y2 = correct(y2, MRG_M2);
  y2 += (uint32_t)st.x23;
  y2 = correct(y2, MRG_M2);
  y2 += y1;
  y2 = correct(y2, MRG_M2);
  st.x23 = st.x22;
  st.x22 = st.x21;
  st.x21 = (int32_t)y2;
}

__device__ __forceinline__ int32_t mat_row(const int64_t* a, uint64_t v0, uint64_t v1, uint64_t v2, uint64_t M) {
  return (int32_t)(((uint64_t)a[0] * v0 + (uint64_t)a[1] * v1 + (uint64_t)a[2] * v2) % M);
}

__device__ __forceinline__ void jump(State& st, const int64_t* t) {
  uint64_t a = (uint32_t)st.x11, b = (uint32_t)st.x12, c = (uint32_t)st.x13;
  st.x11 = mat_row(t, a, b, c, (uint64_t)MRG_M1);
  st.x12 = mat_row(t + 3, a, b, c, (uint64_t)MRG_M1);
  st.x13 = mat_row(t + 6, a, b, c, (uint64_t)MRG_M1);
  a = (uint32_t)st.x21; b = (uint32_t)st.x22; c = (uint32_t)st.x23;
  st.x21 = mat_row(t + 9, a, b, c, (uint64_t)MRG_M2);
  st.x22 = mat_row(t + 12, a, b, c, (uint64_t)MRG_M2);
  st.x23 = mat_row(t + 15, a, b, c, (uint64_t)MRG_M2);
}

// int32 -> T (round to nearest even for float), then ONE multiplication (rng_mrg.py:515 / :520)
__device__ __forceinline__ float scale(int32_t v, float) { return (float)v * 4.6566126e-10f; }
__device__ __forceinline__ double scale(int32_t v, double) { return (double)v * 4.656612873077392578125e-10; }

template <typename T>
__global__ __launch_bounds__(256) void mrg_uniform_kernel(MrgArgs a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= a.n_streams * a.parts) return;
  const int64_t p = t / a.n_streams, s = t - p * a.n_streams;
  const int64_t q = a.n_elements / a.n_streams, r = a.n_elements - q * a.n_streams;
  const int64_t J = q + (s < r ? 1 : 0);      // samples of this stream
  const int64_t j0 = p * a.c;
  const int64_t j1 = (j0 + a.c < J) ? j0 + a.c : J;
  const int32_t* src = a.in + s * 6;
  int32_t* dst = a.out + s * 6;
  if (J == 0) {
    // a stream that produces nothing keeps its state
    if (p == 0 && dst != src)
      for (int k = 0; k < 6; ++k) dst[k] = src[k];
    return;
  }
  if (j0 >= j1) return;
  State st = {src[0], src[1], src[2], src[3], src[4], src[5]};
  if (p > 0) jump(st, a.table + p * 18);
  T* out = static_cast<T*>(a.sample);
  for (int64_t j = j0; j < j1; ++j) {
    step(st);
    const uint32_t d = (uint32_t)st.x11 - (uint32_t)st.x21;
    const int32_t v = (int32_t)(st.x11 <= st.x21 ? d + (uint32_t)MRG_M1 : d);
    out[j * a.n_streams + s] = scale(v, T());
  }
  if (j1 == J) {
    dst[0] = st.x11; dst[1] = st.x12; dst[2] = st.x13;
    dst[3] = st.x21; dst[4] = st.x22; dst[5] = st.x23;
  }
}

// ---- multinomial ----------------------------------------------------------------------------------

struct MultiArgs {
  const void* pvals;   // [nb_multi][nb_outcomes] through p_rs / p_cs (multinomial) — unused by choice
  const void* unis;    // [n_samples * nb_multi] through u_s
  void* ws;            // choice: private copy of pvals, element (n, m) at n*w_rs + m*w_cs
  void* out;           // contiguous: [nb_multi][nb_outcomes] counts / [nb_multi][n_samples] indices
  int64_t p_rs, p_cs, u_s, w_rs, w_cs;
  int64_t nb_multi, nb_outcomes, n_samples;
  int odtype;
};
AHIP_PTRS_BEGIN(MultiArgs) AHIP_PTR1(pvals) AHIP_PTR1(unis) AHIP_PTR1(ws) AHIP_PTR1(out) AHIP_PTRS_END

__device__ __forceinline__ void store_int(void* out, int dt, int64_t i, int64_t v) {
  switch (dt) {
    case AHIP_BOOL: static_cast<uint8_t*>(out)[i] = v != 0; break;
    case AHIP_I8: case AHIP_U8: static_cast<uint8_t*>(out)[i] = (uint8_t)v; break;
    case AHIP_I16: case AHIP_U16: static_cast<uint16_t*>(out)[i] = (uint16_t)v; break;
    case AHIP_I32: case AHIP_U32: static_cast<uint32_t*>(out)[i] = (uint32_t)v; break;
    case AHIP_I64: case AHIP_U64: static_cast<int64_t*>(out)[i] = v; break;
    case AHIP_F32: static_cast<float*>(out)[i] = (float)v; break;
    default: static_cast<double*>(out)[i] = (double)v; break;
  }
}

// multinomial.py:127-160.  The running sum does not depend on the sample c, so the lane walks the
// outcomes once: sample c is counted at outcome m when cummul_m > u_c and no earlier cummul was
// (`best` = the largest earlier cummul; NaN sums never compare greater, as in the reference).
template <typename P, typename U>
__global__ __launch_bounds__(256) void multinomial_kernel(MultiArgs a) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= a.nb_multi) return;
  const P* p = static_cast<const P*>(a.pvals) + n * a.p_rs;
  const U* u = static_cast<const U*>(a.unis);
  double cummul = 0., best = -INFINITY;
  for (int64_t m = 0; m < a.nb_outcomes; ++m) {
    cummul += (double)p[m * a.p_cs];
    int64_t cnt = 0;
    for (int64_t c = 0; c < a.n_samples; ++c) {
      const double uc = (double)u[(c * a.nb_multi + n) * a.u_s];
      if (cummul > uc && !(best > uc)) ++cnt;
    }
    if (cummul > best) best = cummul;
    store_int(a.out, a.odtype, n * a.nb_outcomes + m, cnt);
  }
}

// multinomial.py:344-382 with replace = 0.  Where no outcome is reached the reference leaves the
// cell as allocated; here it is 0.
template <typename P, typename U>
__global__ __launch_bounds__(256) void choice_kernel(MultiArgs a) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= a.nb_multi) return;
  P* w = static_cast<P*>(a.ws) + n * a.w_rs;
  const U* u = static_cast<const U*>(a.unis);
  const int64_t K = a.nb_outcomes, cs = a.w_cs;
  for (int64_t c = 0; c < a.n_samples; ++c) {
    const double uc = (double)u[(c * a.nb_multi + n) * a.u_s];
    double cummul = 0.;
    int64_t z = 0;
    for (int64_t m = 0; m < K; ++m) {
      const P pv = w[m * cs];
      cummul += (double)pv;
      if (cummul > uc) {
        z = m;
        if (c == a.n_samples - 1) break;     // no need to renormalise after the last sample
        P sum = (P)(cummul - (double)pv);
        w[m * cs] = (P)0;
        for (int64_t k = m; k < K; ++k) sum = sum + w[k * cs];
        for (int64_t k = 0; k < K; ++k) w[k * cs] = w[k * cs] / sum;
        break;
      }
    }
    store_int(a.out, a.odtype, n * a.n_samples + c, z);
  }
}

bool float_dtype(int dt) { return dt == AHIP_F32 || dt == AHIP_F64; }

int fill_multi(MultiArgs& a, int odtype, const void* unis, int64_t u_s, int64_t nb_multi, int64_t nb_outcomes,
               int64_t n_samples, void* out) {
  AHIP_REQUIRE(ahip_itemsize(odtype) > 0, "multinomial: unknown output dtype %d", odtype);
  AHIP_REQUIRE(nb_multi >= 0 && nb_outcomes >= 0 && n_samples >= 0, "multinomial: negative extent");
  AHIP_REQUIRE(nb_multi < ((int64_t)1 << 31) && nb_outcomes < ((int64_t)1 << 31) && n_samples < ((int64_t)1 << 31),
               "multinomial: extents stay below 2^31");
  a.unis = unis; a.u_s = u_s; a.out = out; a.odtype = odtype;
  a.nb_multi = nb_multi; a.nb_outcomes = nb_outcomes; a.n_samples = n_samples;
  a.pvals = nullptr; a.ws = nullptr; a.p_rs = a.p_cs = a.w_rs = a.w_cs = 0;
  return AHIP_OK;
}

}  // namespace

extern "C" {

int ahip_mrg_uniform(int dtype, const void* rstate_in, void* rstate_out, int64_t n_streams, void* sample,
                     int64_t n_elements, int64_t parts, const int64_t* table, void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "mrg_uniform: float32 / float64 samples only, got dtype %d", dtype);
  AHIP_REQUIRE(n_streams >= 1 && n_streams <= 0x7fffffffLL, "mrg_uniform: %lld streams", (long long)n_streams);
  AHIP_REQUIRE(n_elements >= 0 && n_elements <= 0x7fffffffLL,
               "mrg_uniform: at most 2**31 - 1 samples, got %lld", (long long)n_elements);
  AHIP_REQUIRE(parts >= 1, "mrg_uniform: parts = %lld", (long long)parts);
  AHIP_REQUIRE(rstate_in != nullptr && rstate_out != nullptr, "null pointer");
  if (n_elements == 0 && rstate_in == rstate_out) return AHIP_OK;
  AHIP_REQUIRE(n_elements == 0 || sample != nullptr, "null pointer");
  const int64_t jmax = (n_elements + n_streams - 1) / n_streams;
  AHIP_REQUIRE(parts == 1 || (table != nullptr && rstate_in != rstate_out),
               "mrg_uniform: a split run needs the jump table and a state buffer of its own");
  const int64_t lanes = n_streams * parts;
  AHIP_REQUIRE((lanes + 255) / 256 <= 0x7fffffffLL, "mrg_uniform: %lld lanes", (long long)lanes);
  MrgArgs a;
  a.in = static_cast<const int32_t*>(rstate_in);
  a.out = static_cast<int32_t*>(rstate_out);
  a.sample = sample;
  a.table = table;
  a.n_elements = n_elements; a.n_streams = n_streams; a.parts = parts;
  a.c = jmax > 0 ? (jmax + parts - 1) / parts : 1;
  const dim3 grid((unsigned)((lanes + 255) / 256));
  hipStream_t s = as_stream(stream);
  if (dtype == AHIP_F32) AHIP_LAUNCH(mrg_uniform_kernel<float>, grid, dim3(256), 0, s, a);
  else AHIP_LAUNCH(mrg_uniform_kernel<double>, grid, dim3(256), 0, s, a);
  return AHIP_OK;
}

int ahip_multinomial_from_uniform(int pdtype, int udtype, int odtype, const void* pvals, int64_t p_rs, int64_t p_cs,
                                  const void* unis, int64_t u_s, int64_t nb_multi, int64_t nb_outcomes,
                                  int64_t n_samples, void* out, void* stream) {
  AHIP_REQUIRE(float_dtype(pdtype) && float_dtype(udtype), "multinomial: float32 / float64 pvals and unis only");
  MultiArgs a;
  int rc = fill_multi(a, odtype, unis, u_s, nb_multi, nb_outcomes, n_samples, out);
  if (rc) return rc;
  if (nb_multi == 0 || nb_outcomes == 0) return AHIP_OK;
  AHIP_REQUIRE(pvals != nullptr && out != nullptr && (unis != nullptr || n_samples == 0), "null pointer");
  a.pvals = pvals; a.p_rs = p_rs; a.p_cs = p_cs;
  const dim3 grid((unsigned)((nb_multi + 255) / 256));
  hipStream_t s = as_stream(stream);
  if (pdtype == AHIP_F32) {
    if (udtype == AHIP_F32) AHIP_LAUNCH((multinomial_kernel<float, float>), grid, dim3(256), 0, s, a);
    else AHIP_LAUNCH((multinomial_kernel<float, double>), grid, dim3(256), 0, s, a);
  } else {
    if (udtype == AHIP_F32) AHIP_LAUNCH((multinomial_kernel<double, float>), grid, dim3(256), 0, s, a);
    else AHIP_LAUNCH((multinomial_kernel<double, double>), grid, dim3(256), 0, s, a);
  }
  return AHIP_OK;
}

int ahip_choice_from_uniform(int pdtype, int udtype, int odtype, void* pvals_copy, int64_t w_rs, int64_t w_cs,
                             const void* unis, int64_t u_s, int64_t nb_multi, int64_t nb_outcomes,
                             int64_t n_samples, void* out, void* stream) {
  AHIP_REQUIRE(float_dtype(pdtype) && float_dtype(udtype), "choice: float32 / float64 pvals and unis only");
  MultiArgs a;
  int rc = fill_multi(a, odtype, unis, u_s, nb_multi, nb_outcomes, n_samples, out);
  if (rc) return rc;
  AHIP_REQUIRE(n_samples <= nb_outcomes,
               "Cannot sample without replacement n samples bigger than the size of the distribution.");
  if (nb_multi == 0 || n_samples == 0) return AHIP_OK;
  AHIP_REQUIRE(pvals_copy != nullptr && out != nullptr && unis != nullptr, "null pointer");
  a.ws = pvals_copy; a.w_rs = w_rs; a.w_cs = w_cs;
  const dim3 grid((unsigned)((nb_multi + 255) / 256));
  hipStream_t s = as_stream(stream);
  if (pdtype == AHIP_F32) {
    if (udtype == AHIP_F32) AHIP_LAUNCH((choice_kernel<float, float>), grid, dim3(256), 0, s, a);
    else AHIP_LAUNCH((choice_kernel<float, double>), grid, dim3(256), 0, s, a);
  } else {
    if (udtype == AHIP_F32) AHIP_LAUNCH((choice_kernel<double, float>), grid, dim3(256), 0, s, a);
    else AHIP_LAUNCH((choice_kernel<double, double>), grid, dim3(256), 0, s, a);
  }
  return AHIP_OK;
}

}  // extern "C"
