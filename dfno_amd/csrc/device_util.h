// What every kernel file needs: element IO for the three storage types
// (float, double, bf16 held as unsigned short), the wave butterfly sum, and
// the host-side grid clamp and tensor check.
//
// bf16 storage always computes in fp32: widen on load (<< 16), round to
// nearest even on store.  Single elements go through __float2bfloat16, pairs
// through __float22bfloat162_rn (one v_cvt_pk_bf16_f32 per pair; the first
// integer-math version cost ~5 VALU per element and made every store-side
// kernel conversion-bound).  Both round the same way; call sites keep the
// form that matches how they pack.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <torch/extension.h>

namespace dfno_io {

// accumulate type of a storage type
template <typename T> struct acc_of { using type = float; };
template <> struct acc_of<double> { using type = double; };
template <typename T> using acc_t = typename acc_of<T>::type;

// accumulator fragment of v_mfma_f32_16x16x4_f32
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float b2f(unsigned short h) {
  return __uint_as_float(((unsigned int)h) << 16);
}

__device__ __forceinline__ unsigned short f2b(float f) {
  __hip_bfloat16 h = __float2bfloat16(f);
  return *reinterpret_cast<unsigned short*>(&h);
}

__device__ __forceinline__ unsigned int f2b2(float lo, float hi) {
  __hip_bfloat162 h2 = __float22bfloat162_rn(float2{lo, hi});
  return *reinterpret_cast<unsigned int*>(&h2);
}

__device__ __forceinline__ float ld(const float* p) { return *p; }
__device__ __forceinline__ double ld(const double* p) { return *p; }
__device__ __forceinline__ float ld(const unsigned short* p) { return b2f(*p); }
__device__ __forceinline__ void st(float* p, float v) { *p = v; }
__device__ __forceinline__ void st(double* p, double v) { *p = v; }
__device__ __forceinline__ void st(unsigned short* p, float v) { *p = f2b(v); }

// 16-byte / 8-byte bf16 vector IO (hipcc does not vectorize bf16 accesses
// by itself)
__device__ __forceinline__ void load8(const unsigned short* p, float* out) {
  const uint4 raw = *reinterpret_cast<const uint4*>(p);
  const unsigned int w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    out[2 * k] = b2f((unsigned short)(w[k] & 0xffffu));
    out[2 * k + 1] = b2f((unsigned short)(w[k] >> 16));
  }
}

__device__ __forceinline__ void store8(unsigned short* p, const float* v) {
  uint4 raw;
  raw.x = f2b2(v[0], v[1]);
  raw.y = f2b2(v[2], v[3]);
  raw.z = f2b2(v[4], v[5]);
  raw.w = f2b2(v[6], v[7]);
  *reinterpret_cast<uint4*>(p) = raw;
}

__device__ __forceinline__ void load4(const unsigned short* p, float* out) {
  const uint2 raw = *reinterpret_cast<const uint2*>(p);
  const unsigned int w[2] = {raw.x, raw.y};
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    out[2 * k] = b2f((unsigned short)(w[k] & 0xffffu));
    out[2 * k + 1] = b2f((unsigned short)(w[k] >> 16));
  }
}

__device__ __forceinline__ void store4(unsigned short* p, const float* v) {
  uint2 raw;
  raw.x = f2b2(v[0], v[1]);
  raw.y = f2b2(v[2], v[3]);
  *reinterpret_cast<uint2*>(p) = raw;
}

// VEC consecutive elements in one access; p must be VEC*sizeof(T)-aligned
// (16 bytes at most).  float moves as float4, bf16 as 8 or 4 packed halves.
template <int VEC>
__device__ __forceinline__ void ldv(const float* p, float* out) {
  static_assert(VEC == 4, "float vector IO is float4");
  const float4 v = *reinterpret_cast<const float4*>(p);
  out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
}
template <int VEC>
__device__ __forceinline__ void stv(float* p, const float* v) {
  static_assert(VEC == 4, "float vector IO is float4");
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
template <int VEC>
__device__ __forceinline__ void ldv(const unsigned short* p, float* out) {
  static_assert(VEC == 8 || VEC == 4, "bf16 vector IO is 8- or 4-wide");
  if constexpr (VEC == 8) load8(p, out); else load4(p, out);
}
template <int VEC>
__device__ __forceinline__ void stv(unsigned short* p, const float* v) {
  static_assert(VEC == 8 || VEC == 4, "bf16 vector IO is 8- or 4-wide");
  if constexpr (VEC == 8) store8(p, v); else store4(p, v);
}

// VEC elements either as one vector access or element by element
template <int VEC, bool VECTOR, typename T>
__device__ __forceinline__ void ldn(const T* p, acc_t<T>* out) {
  if constexpr (VECTOR) {
    ldv<VEC>(p, out);
  } else {
#pragma unroll
    for (int k = 0; k < VEC; ++k) out[k] = ld(p + k);
  }
}
// stores f(0..VEC-1); element by element each value is stored as soon as it
// is computed, so no more than one is live
template <int VEC, bool VECTOR, typename T, typename F>
__device__ __forceinline__ void stn(T* p, F f) {
  if constexpr (VECTOR) {
    acc_t<T> v[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[k] = f(k);
    stv<VEC>(p, v);
  } else {
#pragma unroll
    for (int k = 0; k < VEC; ++k) st(p + k, f(k));
  }
}

// butterfly sum over the 64-lane wave
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// blocks for `work` items at `block` items per block, clamped to [1, cap];
// kernels grid-stride over the rest.  cap is a few blocks per CU (256 CUs).
inline int launch_grid(long work, int block, long cap) {
  long g = (work + block - 1) / block;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

// whether a float4 / uint4 access at p is aligned
inline bool aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

inline void check_real(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == at::kFloat || t.scalar_type() == at::kDouble,
              name, " must be float32/float64");
}

inline void check_bf16(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
              t.scalar_type() == at::kBFloat16, name,
              " must be a contiguous CUDA bf16 tensor");
}

// a bf16 tensor's storage as the kernels see it
inline const unsigned short* usp(const at::Tensor& t) {
  return reinterpret_cast<const unsigned short*>(t.data_ptr());
}
inline unsigned short* usp_mut(at::Tensor& t) {
  return reinterpret_cast<unsigned short*>(t.data_ptr());
}

}  // namespace dfno_io
