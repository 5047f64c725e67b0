// gfx950 (CDNA4) fused pointwise kernels for dfno_amd.
//
// These ops are HBM-bandwidth-bound on MI355X (see ops/pointwise.py header);
// the kernels are written to stream at the float4/128B-coalesced rate with
// all contraction work fused into one pass:
//  * channel_mix: y[b,o,s] = gelu(sum_i W[o,i] x[b,i,s] + bias[o])
//    - weights staged in LDS (wave-uniform broadcast reads),
//    - x vec4-resident in registers for small I (the width<=32 hot case),
//    - accumulator-resident variant for large-I / small-O (the 128->1
//      projection head),
//    - LDS-staged generic fallback for anything else.
//  * gelu / add+gelu elementwise epilogues (exact erf form, matching
//    torch.nn.functional.gelu default).
// One kernel family serves fp32, fp64 and bf16 storage (fp32 arithmetic);
// the launch tables further down carry the per-dtype tuning.
//
// Replaces the reference's einsum + bias-add + separate F.gelu passes
// (/root/reference/dfno/dfno.py:62-65,291,335-350): 3 activation-sized HBM
// round trips become 1.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp8.h>
#include <torch/extension.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <map>
#include <vector>

#include "kernels.h"
#include "gelu_math.h"
#include "device_util.h"

#define DFNO_CHECK(x, msg) TORCH_CHECK(x, msg)

namespace {

using namespace dfno_io;

constexpr int kBlock = 256;

// All kernels below are templated on the STORAGE type T (float, double, or
// bf16 held as unsigned short) and compute in acc_t<T>; elements move only
// through ld/st and ldv/stv (device_util.h).  VECTOR selects the VEC-wide
// vector access (the host has checked size and alignment) over per-element
// access with a ragged tail.

// ---------------------------------------------------------------------------
// elementwise gelu / add+gelu (VEC per thread, grid-stride)
// ---------------------------------------------------------------------------

template <typename T, int VEC, bool VECTOR>
__global__ void gelu_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, long n) {
  long i0 = (long)(blockIdx.x) * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  const long nvec = n / VEC;   // whole vectors only when VECTOR
  for (long i = i0; VECTOR ? i < nvec : i * VEC < n; i += stride) {
    long base = i * VEC;
    if (VECTOR || base + VEC <= n) {
      acc_t<T> v[VEC];
      ldn<VEC, VECTOR>(x + base, v);
      stn<VEC, VECTOR>(y + base, [&](int k) { return dfno_gelu::gelu(v[k]); });
    } else {
      for (long j = base; j < n; ++j) st(y + j, dfno_gelu::gelu(ld(x + j)));
    }
  }
}

template <typename T, int VEC, bool VECTOR>
__global__ void gelu_bwd_kernel(const T* __restrict__ gy, const T* __restrict__ z,
                                T* __restrict__ gz, long n) {
  long i0 = (long)(blockIdx.x) * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  const long nvec = n / VEC;   // whole vectors only when VECTOR
  for (long i = i0; VECTOR ? i < nvec : i * VEC < n; i += stride) {
    long base = i * VEC;
    if (VECTOR || base + VEC <= n) {
      acc_t<T> g[VEC], zv[VEC];
      ldn<VEC, VECTOR>(gy + base, g);
      ldn<VEC, VECTOR>(z + base, zv);
      stn<VEC, VECTOR>(gz + base,
                       [&](int k) { return g[k] * dfno_gelu::gelu_grad(zv[k]); });
    } else {
      for (long j = base; j < n; ++j)
        st(gz + j, ld(gy + j) * dfno_gelu::gelu_grad(ld(z + j)));
    }
  }
}

template <typename T, int VEC, bool VECTOR>
__global__ void add_gelu_kernel(const T* __restrict__ a, const T* __restrict__ b,
                                T* __restrict__ y, T* __restrict__ z, long n) {
  long i0 = (long)(blockIdx.x) * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  const long nvec = n / VEC;   // whole vectors only when VECTOR
  for (long i = i0; VECTOR ? i < nvec : i * VEC < n; i += stride) {
    long base = i * VEC;
    if (VECTOR || base + VEC <= n) {
      acc_t<T> av[VEC], bv[VEC];
      ldn<VEC, VECTOR>(a + base, av);
      ldn<VEC, VECTOR>(b + base, bv);
#pragma unroll
      for (int k = 0; k < VEC; ++k) av[k] = av[k] + bv[k];
      stn<VEC, VECTOR>(z + base, [&](int k) { return av[k]; });
      stn<VEC, VECTOR>(y + base, [&](int k) { return dfno_gelu::gelu(av[k]); });
    } else {
      for (long j = base; j < n; ++j) {
        acc_t<T> zz = ld(a + j) + ld(b + j);
        st(z + j, zz);
        st(y + j, dfno_gelu::gelu(zz));
      }
    }
  }
}

// ---------------------------------------------------------------------------
// channel mix: x-resident path (I <= IMAX), one thread = VEC consecutive s.
// W (O x I or transposed) and bias staged in LDS in the accumulate type;
// reads are wave-uniform broadcasts.  Pre-activation order: bias, i
// ascending, residual; z (when asked for) is that sum, stored before GELU.
// ---------------------------------------------------------------------------

// IT/OT > 0 pin the channel counts at compile time: the loops fully unroll
// with folded LDS offsets (see proj_head / dft note: the runtime-bound loop
// serializes on a per-iteration uniform-load wait)
template <typename T, int IMAX, int VEC, bool ACT, bool VECTOR,
          int IT = 0, int OT = 0>
__global__ __launch_bounds__(kBlock) void channel_mix_xres_kernel(
    const T* __restrict__ x, const T* __restrict__ W, const T* __restrict__ bias,
    T* __restrict__ y, T* __restrict__ z,
    int B, int I_, int O_, long S, bool wt, bool has_bias, bool write_z,
    const T* __restrict__ res) {
  using A = acc_t<T>;
  const int I = IT > 0 ? IT : I_;
  const int O = OT > 0 ? OT : O_;
  extern __shared__ __align__(16) char smem_raw[];
  A* Wl = reinterpret_cast<A*>(smem_raw);        // [O*I]
  A* bl = Wl + (size_t)O * I;                     // [O]
  for (int k = threadIdx.x; k < O * I; k += blockDim.x) Wl[k] = ld(W + k);
  if (has_bias)
    for (int k = threadIdx.x; k < O; k += blockDim.x) bl[k] = ld(bias + k);
  __syncthreads();

  long nchunks = (S + VEC - 1) / VEC;
  long t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;

  for (long t = t0; t < (long)B * nchunks; t += stride) {
    int b = (int)(t / nchunks);
    long s = (t % nchunks) * VEC;
    bool full = (s + VEC) <= S;
    int nv = full ? VEC : (int)(S - s);

    A xr[IMAX][VEC];
    const T* xb = x + ((long)b * I) * S + s;
#pragma unroll
    for (int i = 0; i < IMAX; ++i) {
      if (i < I) {
        if constexpr (VECTOR) {
          ldv<VEC>(xb + (long)i * S, xr[i]);
        } else {
#pragma unroll
          for (int k = 0; k < VEC; ++k)
            xr[i][k] = (full || k < nv) ? ld(xb + (long)i * S + k) : A(0);
        }
      }
    }

    const long off = ((long)b * O) * S + s;
    T* yb = y + off;
    T* zb = write_z ? z + off : nullptr;
#pragma unroll 4
    for (int o = 0; o < (OT > 0 ? OT : 512); ++o) {
      if (OT == 0 && o >= O) break;
      A acc[VEC];
      A bv = has_bias ? bl[o] : A(0);
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] = bv;
#pragma unroll
      for (int i = 0; i < IMAX; ++i) {
        if (i < I) {
          A wv = wt ? Wl[(size_t)i * O + o] : Wl[(size_t)o * I + i];
#pragma unroll
          for (int k = 0; k < VEC; ++k) acc[k] += wv * xr[i][k];
        }
      }
      if constexpr (VECTOR) {
        if (res != nullptr) {
          A rv[VEC];
          ldv<VEC>(res + off + (long)o * S, rv);
#pragma unroll
          for (int k = 0; k < VEC; ++k) acc[k] += rv[k];
        }
        if (write_z) stv<VEC>(zb + (long)o * S, acc);
        if (ACT) {
#pragma unroll
          for (int k = 0; k < VEC; ++k) acc[k] = dfno_gelu::gelu(acc[k]);
        }
        stv<VEC>(yb + (long)o * S, acc);
      } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          if (!full && k >= nv) break;
          if (res != nullptr) acc[k] += ld(res + off + (long)o * S + k);
          if (write_z) st(zb + (long)o * S + k, acc[k]);
          st(yb + (long)o * S + k, ACT ? dfno_gelu::gelu(acc[k]) : acc[k]);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// channel mix: accumulator-resident path (O <= OMAX; streams over I).
// Used for the projection head 128 -> 1 and for grad-x of the lift 1 -> C.
// IU is the unroll of the I stream (part of the per-dtype launch tuning).
// RES compiles the residual in: unlike in the x-resident kernel, where the
// test of `res` is free, here even the untaken branch costs the fp32 O <= 8
// instantiation a VGPR and with it a wave of occupancy.
// ---------------------------------------------------------------------------

template <typename T, int OMAX, int VEC, bool ACT, bool VECTOR,
          int IT, int OT, int IU, bool RES>
__global__ __launch_bounds__(kBlock) void channel_mix_ores_kernel(
    const T* __restrict__ x, const T* __restrict__ W, const T* __restrict__ bias,
    T* __restrict__ y, T* __restrict__ z,
    int B, int I_, int O_, long S, bool wt, bool has_bias, bool write_z,
    const T* __restrict__ res) {
  using A = acc_t<T>;
  const int I = IT > 0 ? IT : I_;
  const int O = OT > 0 ? OT : O_;
  extern __shared__ __align__(16) char smem_raw[];
  A* Wl = reinterpret_cast<A*>(smem_raw);
  A* bl = Wl + (size_t)O * I;
  for (int k = threadIdx.x; k < O * I; k += blockDim.x) Wl[k] = ld(W + k);
  if (has_bias)
    for (int k = threadIdx.x; k < O; k += blockDim.x) bl[k] = ld(bias + k);
  __syncthreads();

  long nchunks = (S + VEC - 1) / VEC;
  long t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;

  for (long t = t0; t < (long)B * nchunks; t += stride) {
    int b = (int)(t / nchunks);
    long s = (t % nchunks) * VEC;
    bool full = (s + VEC) <= S;
    int nv = full ? VEC : (int)(S - s);

    A acc[OMAX][VEC];
#pragma unroll
    for (int o = 0; o < OMAX; ++o) {
      if (o < O) {
        A bv = has_bias ? bl[o] : A(0);
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[o][k] = bv;
      }
    }

    const T* xb = x + ((long)b * I) * S + s;
#pragma unroll IU
    for (int i = 0; i < (IT > 0 ? IT : 512); ++i) {
      if (IT == 0 && i >= I) break;
      A xv[VEC];
      if constexpr (VECTOR) {
        ldv<VEC>(xb + (long)i * S, xv);
      } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k)
          xv[k] = (full || k < nv) ? ld(xb + (long)i * S + k) : A(0);
      }
#pragma unroll
      for (int o = 0; o < OMAX; ++o) {
        if (o < O) {
          A wv = wt ? Wl[(size_t)i * O + o] : Wl[(size_t)o * I + i];
#pragma unroll
          for (int k = 0; k < VEC; ++k) acc[o][k] += wv * xv[k];
        }
      }
    }

    const long off = ((long)b * O) * S + s;
    T* yb = y + off;
    T* zb = write_z ? z + off : nullptr;
#pragma unroll
    for (int o = 0; o < OMAX; ++o) {
      if (o < O) {
        if constexpr (VECTOR) {
          if constexpr (RES) {
            A rv[VEC];
            ldv<VEC>(res + off + (long)o * S, rv);
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[o][k] += rv[k];
          }
          if (write_z) stv<VEC>(zb + (long)o * S, acc[o]);
          if (ACT) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[o][k] = dfno_gelu::gelu(acc[o][k]);
          }
          stv<VEC>(yb + (long)o * S, acc[o]);
        } else {
#pragma unroll
          for (int k = 0; k < VEC; ++k) {
            if (!full && k >= nv) break;
            if constexpr (RES) acc[o][k] += ld(res + off + (long)o * S + k);
            if (write_z) st(zb + (long)o * S + k, acc[o][k]);
            st(yb + (long)o * S + k, ACT ? dfno_gelu::gelu(acc[o][k]) : acc[o][k]);
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// generic LDS-staged fallback: block stages x[I][TS] tile; each thread owns
// VEC s-positions and loops over all O.
// ---------------------------------------------------------------------------

template <typename T, bool ACT, int TS>
__global__ __launch_bounds__(kBlock) void channel_mix_lds_kernel(
    const T* __restrict__ x, const T* __restrict__ W, const T* __restrict__ bias,
    T* __restrict__ y, T* __restrict__ z,
    int B, int I, int O, long S, bool wt, bool has_bias, bool write_z) {
  // tile of TS spatial positions staged in LDS as [I][TS], then W, then bias
  extern __shared__ __align__(16) char smem_raw[];
  T* xt = reinterpret_cast<T*>(smem_raw);  // [I][TS]
  T* Wl = xt + (size_t)I * TS;             // [O*I]
  T* bl = Wl + (size_t)O * I;              // [O]
  for (int k = threadIdx.x; k < O * I; k += blockDim.x) Wl[k] = W[k];
  if (has_bias)
    for (int k = threadIdx.x; k < O; k += blockDim.x) bl[k] = bias[k];

  long ntiles = (S + TS - 1) / TS;
  for (long tile = blockIdx.x; tile < (long)B * ntiles; tile += gridDim.x) {
    int b = (int)(tile / ntiles);
    long s0 = (tile % ntiles) * TS;
    int ts = (int)min((long)TS, S - s0);

    const T* xb = x + ((long)b * I) * S + s0;
    __syncthreads();
    for (int k = threadIdx.x; k < I * ts; k += blockDim.x) {
      int i = k / ts;
      int s = k % ts;
      xt[i * TS + s] = xb[(long)i * S + s];
    }
    __syncthreads();

    for (int s = threadIdx.x; s < ts; s += blockDim.x) {
      T* yb = y + ((long)b * O) * S + s0 + s;
      T* zb = write_z ? z + ((long)b * O) * S + s0 + s : nullptr;
      for (int o = 0; o < O; ++o) {
        T acc = has_bias ? bl[o] : T(0);
        for (int i = 0; i < I; ++i) {
          T wv = wt ? Wl[(size_t)i * O + o] : Wl[(size_t)o * I + i];
          acc += wv * xt[i * TS + s];
        }
        if (write_z) zb[(long)o * S] = acc;
        yb[(long)o * S] = ACT ? dfno_gelu::gelu(acc) : acc;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// launch tables: the per-dtype tuning (caps, vector width, compile-time
// pins, grid cap), one table for fp32/fp64 and one for bf16
// ---------------------------------------------------------------------------

// 256 CUs, a few blocks each; grid-stride the rest
constexpr long kGridCap = 256L * 8;
constexpr long kGridCapBf16 = 256L * 16;

// what every channel-mix kernel takes, plus the launch geometry
template <typename T>
struct MixLaunch {
  const T* x; const T* W; const T* bias; T* y; T* z;
  int B, I, O; long S;
  bool wt, has_bias, act, write_z;
  const T* res;
  int grid; hipStream_t stream;
};

// KERNEL<T, CAP, VEC, act, VECTOR, pins...>; W and bias sit in LDS
#define CMIX(KERNEL, CAP, VEC, V, ...)                                          \
  do {                                                                          \
    const size_t smem = sizeof(acc_t<T>) * ((size_t)a.O * a.I + a.O);           \
    if (a.act) {                                                                \
      hipLaunchKernelGGL((KERNEL<T, CAP, VEC, true, V, __VA_ARGS__>),           \
                         dim3(a.grid), dim3(kBlock), smem, a.stream, a.x, a.W,  \
                         a.bias, a.y, a.z, a.B, a.I, a.O, a.S, a.wt,            \
                         a.has_bias, a.write_z, a.res);                         \
    } else {                                                                    \
      hipLaunchKernelGGL((KERNEL<T, CAP, VEC, false, V, __VA_ARGS__>),          \
                         dim3(a.grid), dim3(kBlock), smem, a.stream, a.x, a.W,  \
                         a.bias, a.y, a.z, a.B, a.I, a.O, a.S, a.wt,            \
                         a.has_bias, a.write_z, a.res);                         \
    }                                                                           \
  } while (0)

bool can_vectorize(const float* x, const float* y, const float* z, long S,
                   bool write_z) {
  if (S % 4 != 0) return false;
  auto aligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  return aligned(x) && aligned(y) && (!write_z || aligned(z));
}
bool can_vectorize(const double*, const double*, const double*, long, bool) {
  return false;
}

// LDS-staged generic path (fp32/fp64 only); pick the largest tile that keeps
// the x tile within 64 KiB (>= 2 blocks/CU of LDS headroom)
template <typename T>
void launch_channel_mix_lds(const MixLaunch<T>& a) {
  const int grid = launch_grid((long)a.B * ((a.S + kBlock - 1) / kBlock) * kBlock,
                               kBlock, kGridCap);
#define CMIX_LDS(TS)                                                            \
  {                                                                             \
    size_t smem_lds = sizeof(T) * ((size_t)a.I * TS + (size_t)a.O * a.I + a.O); \
    if (a.act) {                                                                \
      hipLaunchKernelGGL((channel_mix_lds_kernel<T, true, TS>), dim3(grid),     \
                         dim3(kBlock), smem_lds, a.stream, a.x, a.W, a.bias,    \
                         a.y, a.z, a.B, a.I, a.O, a.S, a.wt, a.has_bias,        \
                         a.write_z);                                            \
    } else {                                                                    \
      hipLaunchKernelGGL((channel_mix_lds_kernel<T, false, TS>), dim3(grid),    \
                         dim3(kBlock), smem_lds, a.stream, a.x, a.W, a.bias,    \
                         a.y, a.z, a.B, a.I, a.O, a.S, a.wt, a.has_bias,        \
                         a.write_z);                                            \
    }                                                                           \
  }
  size_t per_s = sizeof(T) * (size_t)a.I;
  size_t wbytes = sizeof(T) * ((size_t)a.O * a.I + a.O);
  if (per_s * 256 + wbytes <= 64 * 1024) { CMIX_LDS(256) }
  else if (per_s * 128 + wbytes <= 96 * 1024) { CMIX_LDS(128) }
  else if (per_s * 64 + wbytes <= 128 * 1024) { CMIX_LDS(64) }
  else {
    TORCH_CHECK(per_s * 32 + wbytes <= 160 * 1024,
                "channel_mix: I/O too large for LDS tile");
    CMIX_LDS(32)
  }
#undef CMIX_LDS
}

// fp32 / fp64: VEC 4, float4 access when size and alignment allow
template <typename T>
void launch_channel_mix(const T* x, const T* W, const T* bias, T* y, T* z,
                        int B, int I, int O, long S, bool wt, bool has_bias,
                        bool act, bool write_z, hipStream_t stream,
                        const T* res = nullptr) {
  constexpr bool kFloat = std::is_same<T, float>::value;
  const MixLaunch<T> a{x, W, bias, y, z, B, I, O, S, wt, has_bias, act, write_z,
                       res, launch_grid((long)B * ((S + 3) / 4), kBlock, kGridCap),
                       stream};
  const bool vec = can_vectorize(x, y, z, S, write_z);
#define CMIX_V(KERNEL, CAP, ...)                                                \
  do {                                                                          \
    if constexpr (kFloat) {                                                     \
      if (vec) CMIX(KERNEL, CAP, 4, true, __VA_ARGS__);                         \
      else CMIX(KERNEL, CAP, 4, false, __VA_ARGS__);                            \
    } else {                                                                    \
      CMIX(KERNEL, CAP, 4, false, __VA_ARGS__);                                 \
    }                                                                           \
  } while (0)
  TORCH_CHECK(res == nullptr || I <= 32, "channel_mix with residual needs I <= 32");
  // the flagship channel counts fold at compile time (see kernel note)
  if (I == 20 && O == 20) CMIX_V(channel_mix_xres_kernel, 24, 20, 20);
  else if (I <= 8) CMIX_V(channel_mix_xres_kernel, 8, 0, 0);
  else if (I <= 16) CMIX_V(channel_mix_xres_kernel, 16, 0, 0);
  else if (I <= 24) CMIX_V(channel_mix_xres_kernel, 24, 0, 0);
  else if (I <= 32) CMIX_V(channel_mix_xres_kernel, 32, 0, 0);
  else if (O <= 4) CMIX_V(channel_mix_ores_kernel, 4, 0, 0, 8, false);
  else if (O <= 8) CMIX_V(channel_mix_ores_kernel, 8, 0, 0, 8, false);
  else if (O <= 16) CMIX_V(channel_mix_ores_kernel, 16, 0, 0, 8, false);
  else if (kFloat && O <= 32) {
    if constexpr (kFloat) {   // float only: the wide caps are not built for double
      if (I == 128 && O == 20) CMIX_V(channel_mix_ores_kernel, 24, 128, 20, 8, false);
      else if (O <= 24) CMIX_V(channel_mix_ores_kernel, 24, 0, 0, 8, false);
      else CMIX_V(channel_mix_ores_kernel, 32, 0, 0, 8, false);
    }
  } else {
    launch_channel_mix_lds(a);
  }
#undef CMIX_V
}

// bf16: always vector access (S % 8 == 0 is required); VEC 8 at the narrow
// caps, VEC 4 at the wide ones (xr[24][8] / acc[24][8] = 192 VGPRs would
// spill).  Shapes outside the table raise.
void launch_channel_mix_bf16(const MixLaunch<unsigned short>& a) {
  using T = unsigned short;
  const int I = a.I, O = a.O;
  // the accumulator-resident kernel compiles its residual in or out
#define CMIX_ORES(CAP, VEC, IT, OT)                                             \
  do {                                                                          \
    if (a.res != nullptr)                                                       \
      CMIX(channel_mix_ores_kernel, CAP, VEC, true, IT, OT, 4, true);           \
    else                                                                        \
      CMIX(channel_mix_ores_kernel, CAP, VEC, true, IT, OT, 4, false);          \
  } while (0)
  // compile-time-pinned hot shapes first (block mixes, projection lift and
  // its transpose, channel lift, projection head)
  if (I == 20 && O == 20) CMIX(channel_mix_xres_kernel, 24, 4, true, 20, 20);
  else if (I == 20 && O == 128) CMIX(channel_mix_xres_kernel, 24, 4, true, 20, 128);
  else if (I == 2 && O == 20) CMIX(channel_mix_xres_kernel, 8, 8, true, 2, 20);
  else if (I == 128 && O == 20) CMIX_ORES(24, 4, 128, 20);
  else if (I == 128 && O == 1) CMIX_ORES(8, 8, 128, 1);
  else if (I <= 8) CMIX(channel_mix_xres_kernel, 8, 8, true, 0, 0);
  else if (I <= 24) CMIX(channel_mix_xres_kernel, 24, 4, true, 0, 0);
  else if (I <= 32) CMIX(channel_mix_xres_kernel, 32, 4, true, 0, 0);
  else if (O <= 8) CMIX_ORES(8, 8, 0, 0);
  else if (O <= 24) CMIX_ORES(24, 4, 0, 0);
  else TORCH_CHECK(false, "bf16 channel mix: unsupported shape I=", I, " O=", O);
#undef CMIX_ORES
}
#undef CMIX

}  // namespace

// ---------------------------------------------------------------------------
// host entry points
// ---------------------------------------------------------------------------

std::vector<at::Tensor> channel_mix_fwd(const at::Tensor& x, const at::Tensor& W,
                                        const at::Tensor& b, bool act) {
  check_real(x, "x"); check_real(W, "W");
  TORCH_CHECK(x.dim() == 3, "x must be [B,I,S]");
  int B = (int)x.size(0), I = (int)x.size(1);
  long S = x.size(2);
  int O = (int)W.size(0);
  TORCH_CHECK((int)W.size(1) == I, "W/I mismatch");
  bool has_bias = b.numel() > 0;

  auto y = at::empty({B, O, S}, x.options());
  at::Tensor z = act ? at::empty({B, O, S}, x.options()) : y;

  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  if (x.numel() == 0 || y.numel() == 0) return {y, z};

  AT_DISPATCH_FLOATING_TYPES(x.scalar_type(), "channel_mix_fwd", [&] {
    launch_channel_mix<scalar_t>(
        x.data_ptr<scalar_t>(), W.data_ptr<scalar_t>(),
        has_bias ? b.data_ptr<scalar_t>() : nullptr,
        y.data_ptr<scalar_t>(), z.data_ptr<scalar_t>(),
        B, I, O, S, /*wt=*/false, has_bias, act, /*write_z=*/act, stream);
  });
  return {y, z};
}

at::Tensor channel_mix_fwd_t(const at::Tensor& gz, const at::Tensor& W) {
  check_real(gz, "gz"); check_real(W, "W");
  TORCH_CHECK(gz.dim() == 3, "gz must be [B,O,S]");
  int B = (int)gz.size(0), O = (int)gz.size(1);
  long S = gz.size(2);
  int I = (int)W.size(1);
  TORCH_CHECK((int)W.size(0) == O, "W/O mismatch");

  auto gx = at::empty({B, I, S}, gz.options());
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  if (gz.numel() == 0 || gx.numel() == 0) return gx;

  AT_DISPATCH_FLOATING_TYPES(gz.scalar_type(), "channel_mix_fwd_t", [&] {
    // roles swapped: "input channels" = O, "output channels" = I, transposed W
    launch_channel_mix<scalar_t>(
        gz.data_ptr<scalar_t>(), W.data_ptr<scalar_t>(), nullptr,
        gx.data_ptr<scalar_t>(), gx.data_ptr<scalar_t>(),
        B, O, I, S, /*wt=*/true, /*has_bias=*/false, /*act=*/false,
        /*write_z=*/false, stream);
  });
  return gx;
}

std::vector<at::Tensor> linear_res_gelu_fwd(const at::Tensor& x, const at::Tensor& W,
                                            const at::Tensor& res) {
  check_real(x, "x"); check_real(W, "W"); check_real(res, "res");
  TORCH_CHECK(x.dim() == 3 && res.dim() == 3, "x/res must be [B,*,S]");
  int B = (int)x.size(0), I = (int)x.size(1);
  long S = x.size(2);
  int O = (int)W.size(0);
  TORCH_CHECK((int)W.size(1) == I, "W/I mismatch");
  TORCH_CHECK(res.size(0) == B && (int)res.size(1) == O && res.size(2) == S,
              "res shape mismatch");

  auto y = at::empty({B, O, S}, x.options());
  auto z = at::empty({B, O, S}, x.options());
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  if (x.numel() == 0) return {y, z};
  AT_DISPATCH_FLOATING_TYPES(x.scalar_type(), "linear_res_gelu_fwd", [&] {
    launch_channel_mix<scalar_t>(
        x.data_ptr<scalar_t>(), W.data_ptr<scalar_t>(), nullptr,
        y.data_ptr<scalar_t>(), z.data_ptr<scalar_t>(),
        B, I, O, S, /*wt=*/false, /*has_bias=*/false, /*act=*/true,
        /*write_z=*/true, stream, res.data_ptr<scalar_t>());
  });
  return {y, z};
}

at::Tensor gelu_fwd(const at::Tensor& x) {
  check_real(x, "x");
  auto y = at::empty_like(x);
  long n = x.numel();
  if (n == 0) return y;
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  AT_DISPATCH_FLOATING_TYPES(x.scalar_type(), "gelu_fwd", [&] {
    int grid = launch_grid((n + 3) / 4, kBlock, kGridCap);
    hipLaunchKernelGGL((gelu_fwd_kernel<scalar_t, 4, false>), dim3(grid), dim3(kBlock), 0,
                       stream, x.data_ptr<scalar_t>(), y.data_ptr<scalar_t>(), n);
  });
  return y;
}

at::Tensor gelu_bwd(const at::Tensor& gy, const at::Tensor& z) {
  check_real(gy, "gy"); check_real(z, "z");
  TORCH_CHECK(gy.numel() == z.numel(), "gelu_bwd size mismatch");
  auto gz = at::empty_like(gy);
  long n = gy.numel();
  if (n == 0) return gz;
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  AT_DISPATCH_FLOATING_TYPES(gy.scalar_type(), "gelu_bwd", [&] {
    int grid = launch_grid((n + 3) / 4, kBlock, kGridCap);
    hipLaunchKernelGGL((gelu_bwd_kernel<scalar_t, 4, false>), dim3(grid), dim3(kBlock), 0,
                       stream, gy.data_ptr<scalar_t>(), z.data_ptr<scalar_t>(),
                       gz.data_ptr<scalar_t>(), n);
  });
  return gz;
}

std::vector<at::Tensor> add_gelu_fwd(const at::Tensor& a, const at::Tensor& b) {
  check_real(a, "a"); check_real(b, "b");
  TORCH_CHECK(a.sizes() == b.sizes(), "add_gelu shape mismatch");
  auto y = at::empty_like(a);
  auto z = at::empty_like(a);
  long n = a.numel();
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  if (n == 0) return {y, z};
  AT_DISPATCH_FLOATING_TYPES(a.scalar_type(), "add_gelu_fwd", [&] {
    int grid = launch_grid((n + 3) / 4, kBlock, kGridCap);
    hipLaunchKernelGGL((add_gelu_kernel<scalar_t, 4, false>), dim3(grid), dim3(kBlock), 0,
                       stream, a.data_ptr<scalar_t>(), b.data_ptr<scalar_t>(),
                       y.data_ptr<scalar_t>(), z.data_ptr<scalar_t>(), n);
  });
  return {y, z};
}

// ---------------------------------------------------------------------------
// bf16-storage entry points (the bf16 compute config).  Storage is bf16
// (halves every activation's HBM traffic; these ops are bandwidth-bound),
// arithmetic is fp32.  Vector IO is 8 bf16 per lane (16 B, the coalescing
// sweet spot), so sizes must be multiples of 8.
// ---------------------------------------------------------------------------

std::vector<at::Tensor> bf16_channel_mix(const at::Tensor& x, const at::Tensor& W,
                                         const at::Tensor& b, bool act, bool wt,
                                         bool write_z, const at::Tensor& res) {
  check_bf16(x, "x"); check_bf16(W, "W");
  const int B = (int)x.size(0);
  const int I = (int)x.size(1);
  const long S = x.size(2);
  const int O = wt ? (int)W.size(1) : (int)W.size(0);
  TORCH_CHECK(S % 8 == 0, "bf16 channel mix: S must be a multiple of 8");
  const bool has_bias = b.defined() && b.numel() > 0;
  if (has_bias) check_bf16(b, "b");
  const bool has_res = res.defined() && res.numel() > 0;
  if (has_res) check_bf16(res, "res");

  auto y = at::empty({B, O, S}, x.options());
  auto z = write_z ? at::empty({B, O, S}, x.options()) : at::empty({0}, x.options());
  if (x.numel() == 0) return {y, z};

  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  launch_channel_mix_bf16(
      {usp(x), usp(W), has_bias ? usp(b) : nullptr, usp_mut(y),
       write_z ? usp_mut(z) : nullptr, B, I, O, S, wt, has_bias, act, write_z,
       has_res ? usp(res) : nullptr,
       launch_grid((long)B * (S / 8), kBlock, kGridCapBf16), stream});
  DFNO_CHECK_LAUNCH("bf16_channel_mix");
  return {y, z};
}

at::Tensor bf16_gelu_fwd(const at::Tensor& x) {
  check_bf16(x, "x");
  TORCH_CHECK(x.numel() % 8 == 0, "bf16 gelu: numel must be a multiple of 8");
  auto y = at::empty_like(x);
  if (x.numel() == 0) return y;
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  const long n = x.numel();
  hipLaunchKernelGGL((gelu_fwd_kernel<unsigned short, 8, true>),
                     dim3(launch_grid(n / 8, kBlock, kGridCapBf16)), dim3(kBlock),
                     0, stream, usp(x), usp_mut(y), n);
  DFNO_CHECK_LAUNCH("bf16_gelu");
  return y;
}

at::Tensor bf16_gelu_bwd(const at::Tensor& gy, const at::Tensor& z) {
  check_bf16(gy, "gy"); check_bf16(z, "z");
  TORCH_CHECK(gy.numel() % 8 == 0, "bf16 gelu bwd: numel % 8");
  auto gz = at::empty_like(gy);
  if (gy.numel() == 0) return gz;
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  const long n = gy.numel();
  hipLaunchKernelGGL((gelu_bwd_kernel<unsigned short, 8, true>),
                     dim3(launch_grid(n / 8, kBlock, kGridCapBf16)), dim3(kBlock),
                     0, stream, usp(gy), usp(z), usp_mut(gz), n);
  DFNO_CHECK_LAUNCH("bf16_gelu_bwd");
  return gz;
}

std::vector<at::Tensor> bf16_add_gelu(const at::Tensor& a, const at::Tensor& b) {
  check_bf16(a, "a"); check_bf16(b, "b");
  TORCH_CHECK(a.numel() == b.numel() && a.numel() % 8 == 0, "bf16 add_gelu shape");
  auto y = at::empty_like(a);
  auto z = at::empty_like(a);
  if (a.numel() == 0) return {y, z};
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  const long n = a.numel();
  hipLaunchKernelGGL((add_gelu_kernel<unsigned short, 8, true>),
                     dim3(launch_grid(n / 8, kBlock, kGridCapBf16)), dim3(kBlock),
                     0, stream, usp(a), usp(b), usp_mut(y), usp_mut(z), n);
  DFNO_CHECK_LAUNCH("bf16_add_gelu");
  return {y, z};
}

// ---------------------------------------------------------------------------
// grad-W outer-product reduction: gW[o,i] = sum_{b,s} A[b,o,s] B[b,i,s]
// (optionally gb[o] = sum A[b,o,s]).
//
// rocBLAS picks a no-split-K schedule for these M,N<=128 / K~10^7 GEMMs
// (observed: ~2 workgroups on 256 CUs, 3.2 ms for a 1.3 GB reduction); here
// the s axis is split across blocks (grid ordered s-chunk-major so the
// o-tiles sweeping one s-chunk hit L2/L3 on the B re-reads), each wave owns
// one A row with the <=32 B rows accumulated in registers, and partials are
// wave-shuffle-reduced then atomically added into gW once per block.
// ---------------------------------------------------------------------------

namespace {

template <typename T, int ICAP, int OW, bool BIAS, bool VECTOR, bool ISLAB = false>
__global__ __launch_bounds__(kBlock) void gw_outer_kernel(
    const T* __restrict__ A, const T* __restrict__ Bm,
    T* __restrict__ gW, T* __restrict__ gb,
    int B, int O, int I_, long S, int n_schunk) {
  // grid: blockIdx.x = schunk * o_tiles + o_tile (s-chunk-major); each wave
  // owns OW consecutive output rows (cuts B re-reads by OW and raises the
  // fma:load ratio).  ISLAB (I_ > ICAP): blockIdx.y picks the slab of ICAP
  // B rows this block reduces; slab 0 owns the bias.
  const int i0 = ISLAB ? (int)blockIdx.y * ICAP : 0;
  const int I = ISLAB ? min(ICAP, I_ - i0) : I_;   // rows of this slab
  const bool do_bias = BIAS && (!ISLAB || blockIdx.y == 0);
  const int o_tiles = (O + 4 * OW - 1) / (4 * OW);
  const int schunk = blockIdx.x / o_tiles;
  const int o_tile = blockIdx.x % o_tiles;
  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  const int o0 = (o_tile * 4 + wave) * OW;

  // chunk boundaries on 256-element grain so the float4 lanes stay aligned
  long chunk_sz = ((S + n_schunk - 1) / n_schunk + 255) & ~255L;
  long s0 = (long)schunk * chunk_sz;
  long s1 = min(S, s0 + chunk_sz);

  T acc[OW][ICAP];
#pragma unroll
  for (int w = 0; w < OW; ++w)
#pragma unroll
    for (int i = 0; i < ICAP; ++i) acc[w][i] = T(0);
  T bacc[OW];
#pragma unroll
  for (int w = 0; w < OW; ++w) bacc[w] = T(0);

  if (o0 < O) {
    for (int b = 0; b < B; ++b) {
      const T* Ab = A + ((long)b * O + o0) * S;
      const T* Bb = Bm + ((long)b * I_ + i0) * S;
      if constexpr (VECTOR && std::is_same<T, float>::value) {
        const long tail0 = s0 + ((s1 - s0) / (64 * 4)) * (64 * 4);
        for (long s = s0 + (long)lane * 4; s < tail0; s += 64 * 4) {
          float4 av[OW];
#pragma unroll
          for (int w = 0; w < OW; ++w) {
            if (o0 + w < O) {
              av[w] = *reinterpret_cast<const float4*>(Ab + (long)w * S + s);
              if (do_bias) bacc[w] += av[w].x + av[w].y + av[w].z + av[w].w;
            }
          }
#pragma unroll
          for (int i = 0; i < ICAP; ++i) {
            if (i < I) {
              const float4 bv = *reinterpret_cast<const float4*>(Bb + (long)i * S + s);
#pragma unroll
              for (int w = 0; w < OW; ++w) {
                if (o0 + w < O)
                  acc[w][i] += av[w].x * bv.x + av[w].y * bv.y +
                               av[w].z * bv.z + av[w].w * bv.w;
              }
            }
          }
        }
        for (long s = tail0 + lane; s < s1; s += 64) {
#pragma unroll
          for (int w = 0; w < OW; ++w) {
            if (o0 + w < O) {
              T av = Ab[(long)w * S + s];
              if (do_bias) bacc[w] += av;
#pragma unroll
              for (int i = 0; i < ICAP; ++i)
                if (i < I) acc[w][i] += av * Bb[(long)i * S + s];
            }
          }
        }
      } else {
        for (long s = s0 + lane; s < s1; s += 64) {
#pragma unroll
          for (int w = 0; w < OW; ++w) {
            if (o0 + w < O) {
              T av = Ab[(long)w * S + s];
              if (do_bias) bacc[w] += av;
#pragma unroll
              for (int i = 0; i < ICAP; ++i)
                if (i < I) acc[w][i] += av * Bb[(long)i * S + s];
            }
          }
        }
      }
    }
  }

  // flush: wave-reduce each acc, lane 0 atomically accumulates
#pragma unroll
  for (int w = 0; w < OW; ++w) {
    if (o0 + w < O) {
#pragma unroll
      for (int i = 0; i < ICAP; ++i) {
        if (i < I) {
          T v = wave_sum(acc[w][i]);
          if (lane == 0 && v != T(0)) atomicAdd(&gW[(size_t)(o0 + w) * I_ + i0 + i], v);
        }
      }
      if (do_bias) {
        T v = wave_sum(bacc[w]);
        if (lane == 0 && v != T(0)) atomicAdd(&gb[o0 + w], v);
      }
    }
  }
}


// All-glds pipelined variant.  Both operand tiles (the I<=32 narrow B rows
// AND this block's 4*OW A rows) are staged into a 3-deep LDS ring by
// global_load_lds DMA; the loop keeps exactly one tile's DMA in flight and
// waits for the current tile with a COUNTED s_waitcnt vmcnt(NG) + raw
// s_barrier.  The previous version kept A in registers via ordinary loads:
// hipcc then inserted s_waitcnt vmcnt(0) before every A use (76 of them in
// the unrolled body), draining the in-flight next-tile DMA each step and
// serializing the ring at ~1.8 TB/s.  Counted vmcnt needs a compile-time
// exact per-wave instruction count, so the issue loops are padded to fixed
// trip counts (NB = ICAP/4 for B, OW for A) with out-of-range rows clamped
// to a valid source row; compute masks those lanes out as before.  3
// buffers (not 2) so a tile's DMA lands in a buffer whose last readers are
// two barriers back.  LDS = 3*(ICAP+4*OW)*1KB -> 1-2 blocks/CU; the low
// occupancy is by design, latency hides in the pipeline depth.
template <typename T, int ICAP, int OW, int TS = 256, int NBUF = 3>
__global__ __launch_bounds__(kBlock) void gw_outer_glds3_kernel(
    const T* __restrict__ A, const T* __restrict__ Bm,
    T* __restrict__ gW, T* __restrict__ gb,
    int B, int O, int I, long S, int n_schunk, bool want_bias) {
  // TS = floats per s-tile row: bigger rows read longer contiguous HBM
  // bursts per stream (TS=512 -> 2 KB sequential per row per tile).
  static_assert((ICAP * TS) % (kBlock * 4) == 0, "B image must tile evenly");
  static_assert((OW * TS) % 256 == 0, "A image must tile evenly");
  constexpr int NB = ICAP * TS / (kBlock * 4);  // B glds instrs per wave
  constexpr int NA = OW * TS / 256;             // A glds instrs per wave
  constexpr int NG = NB + NA;                   // per wave per tile
  constexpr int AROWS = 4 * OW;     // A rows staged per block
  constexpr int PASS = TS >= 256 ? TS / 256 : 1;  // compute passes per tile
  __shared__ float ring[NBUF][(ICAP + AROWS) * TS];

  const int o_tiles = (O + 4 * OW - 1) / (4 * OW);
  // XCD-aware decode: workgroups are dealt round-robin to the 8 XCDs, each
  // with its own L2.  All o-tiles of one s-chunk share the B rows, so place
  // them on ONE XCD (ids congruent mod 8): the 2nd..Nth o-tile then reads B
  // from that XCD's L2 instead of re-fetching HBM (gW3's O=128 shape was 16x
  // amplified).  Identity when o_tiles == 1; host rounds n_schunk up to a
  // multiple of 8 when o_tiles > 1 so the decode stays a bijection.
  const int xr = blockIdx.x % 8;
  const int xq = blockIdx.x / 8;
  const int o_tile = xq % o_tiles;
  const int schunk = (xq / o_tiles) * 8 + xr;
  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  const int o0 = (o_tile * 4 + wave) * OW;
  const int ob0 = o_tile * 4 * OW;  // first A row of the whole block

  long chunk_sz = ((S + n_schunk - 1) / n_schunk + (TS - 1)) & ~((long)TS - 1);
  long s0 = (long)schunk * chunk_sz;
  long s1 = min(S, s0 + chunk_sz);
  long full_end = (s0 < s1) ? s0 + ((s1 - s0) / TS) * TS : s0;

  float acc[OW][ICAP];
#pragma unroll
  for (int w = 0; w < OW; ++w)
#pragma unroll
    for (int i = 0; i < ICAP; ++i) acc[w][i] = 0.f;
  float bacc[OW];
#pragma unroll
  for (int w = 0; w < OW; ++w) bacc[w] = 0.f;

  for (int b = 0; b < B; ++b) {
    const float* Ab = reinterpret_cast<const float*>(A) + ((long)b * O + o0) * S;
    const float* Abl = reinterpret_cast<const float*>(A) + ((long)b * O) * S;
    const float* Bb = reinterpret_cast<const float*>(Bm) + ((long)b * I) * S;

    // one tile's DMA: exactly NG glds instructions per wave, every wave.
    auto issue_tile = [&](int buf, long st) {
      float* dst = ring[buf];
#pragma unroll
      for (int k = 0; k < NB; ++k) {            // B rows, lane-linear image
        int slot = wave * 64 + k * kBlock + lane;
        int fo = slot * 4;
        int row = fo / TS, col = fo % TS;
        int srow = row < I ? row : I - 1;       // pad: clamp to a valid row
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)
                (Bb + (long)srow * S + st + col),
            (__attribute__((address_space(3))) void*)&dst[slot * 4],
            16, 0, 0);
      }
#pragma unroll
      for (int k = 0; k < NA; ++k) {            // this wave's own A rows
        int fa = k * 256 + lane * 4;            // flat offset in OW*TS image
        int w = fa / TS, col = fa % TS;
        int row = ob0 + wave * OW + w;
        int srow = row < O ? row : O - 1;
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)
                (Abl + (long)srow * S + st + col),
            (__attribute__((address_space(3))) void*)
                &dst[(ICAP + wave * OW + w) * TS + col],
            16, 0, 0);
      }
    };

    if (s0 < full_end) {
      const long nt = (full_end - s0) / TS;
      issue_tile(0, s0);
      for (long t = 0; t < nt; ++t) {
        if (t + 1 < nt) {
          if constexpr (NBUF == 2) {
            // 2-buffer ring: the issue target is the buffer read LAST
            // iteration; fence all waves out of it first
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
          }
          issue_tile((int)((t + 1) % NBUF), s0 + (t + 1) * TS);
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NG) : "memory");
        } else {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        // raw barrier (no implicit vmcnt drain), fenced so the compiler
        // cannot hoist the LDS reads above it
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const float* cur = ring[t % NBUF];
        if (o0 < O) {
          if constexpr (TS >= 256) {
#pragma unroll
            for (int p = 0; p < PASS; ++p) {
              float4 av[OW];
#pragma unroll
              for (int w = 0; w < OW; ++w) {
                if (o0 + w < O) {
                  av[w] = *reinterpret_cast<const float4*>(
                      &cur[(ICAP + wave * OW + w) * TS + p * 256 + lane * 4]);
                  if (want_bias)
                    bacc[w] += av[w].x + av[w].y + av[w].z + av[w].w;
                }
              }
#pragma unroll
              for (int i = 0; i < ICAP; ++i) {
                if (i < I) {
                  const float4 bv = *reinterpret_cast<const float4*>(
                      &cur[i * TS + p * 256 + lane * 4]);
#pragma unroll
                  for (int w = 0; w < OW; ++w) {
                    if (o0 + w < O)
                      acc[w][i] += av[w].x * bv.x + av[w].y * bv.y +
                                   av[w].z * bv.z + av[w].w * bv.w;
                  }
                }
              }
            }
          } else {                              // TS == 128: float2 per lane
            float2 av[OW];
#pragma unroll
            for (int w = 0; w < OW; ++w) {
              if (o0 + w < O) {
                av[w] = *reinterpret_cast<const float2*>(
                    &cur[(ICAP + wave * OW + w) * TS + lane * 2]);
                if (want_bias) bacc[w] += av[w].x + av[w].y;
              }
            }
#pragma unroll
            for (int i = 0; i < ICAP; ++i) {
              if (i < I) {
                const float2 bv = *reinterpret_cast<const float2*>(
                    &cur[i * TS + lane * 2]);
#pragma unroll
                for (int w = 0; w < OW; ++w) {
                  if (o0 + w < O)
                    acc[w][i] += av[w].x * bv.x + av[w].y * bv.y;
                }
              }
            }
          }
        }
      }
      __syncthreads();  // next b (or tail) may overwrite ring buffers
    }

    // ragged tail of the last (partial) tile, direct from global
    if (o0 < O) {
      for (long s = full_end + lane; s < s1; s += 64) {
#pragma unroll
        for (int w = 0; w < OW; ++w) {
          if (o0 + w < O) {
            float av = Ab[(long)w * S + s];
            if (want_bias) bacc[w] += av;
#pragma unroll
            for (int i = 0; i < ICAP; ++i)
              if (i < I) acc[w][i] += av * Bb[(long)i * S + s];
          }
        }
      }
    }
  }

#pragma unroll
  for (int w = 0; w < OW; ++w) {
    if (o0 + w < O) {
#pragma unroll
      for (int i = 0; i < ICAP; ++i) {
        if (i < I) {
          float v = wave_sum(acc[w][i]);
          if (lane == 0 && v != 0.f)
            atomicAdd(reinterpret_cast<float*>(&gW[(size_t)(o0 + w) * I + i]), v);
        }
      }
      if (want_bias) {
        float v = wave_sum(bacc[w]);
        if (lane == 0 && v != 0.f)
          atomicAdd(reinterpret_cast<float*>(&gb[o0 + w]), v);
      }
    }
  }
}

}  // namespace

// ---------------------------------------------------------------------------
// fp32-MFMA grad-W for big-O shapes (the projection lift's gW3 [128, 20]).
// gW[o,i] = sum_s gz[o,s] x[i,s] is GEMM-shaped with K = S ~ 10^7; the VALU
// glds3 kernel sits at the round-1 "0.9 TB/s per resident block" ceiling
// (2.8 ms at this shape).  v_mfma_f32_16x16x4_f32 runs the identical-
// numerics contraction at the f32 matrix rate with one f32 operand register
// per lane (cdna_hip_programming.md section 3: an untuned f32-MFMA tile
// outruns a VALU f32 GEMM 122 vs 52 TF) — LDS-staged [rows][TS] tiles,
// wave-per-(16x16)-output-tile, fp32 accumulate, atomic flush.
// ---------------------------------------------------------------------------

namespace {

typedef float f32x4_pw __attribute__((ext_vector_type(4)));

template <int NPAIR, int XR = 32, int OSL = 64, bool BIAS = false>
__global__ __launch_bounds__(kBlock) void gw_mfma_f32_kernel(
    const float* __restrict__ gz, const float* __restrict__ x,
    float* __restrict__ gW, int B, int O, int I, long S,
    float* __restrict__ gb = nullptr) {
  constexpr int TS = 128;          // s per tile (32 MFMA K-steps)
  constexpr int LD = TS + 4;       // float4-aligned row pad
  // OSL: o-rows per blockIdx.y slab; XR: x-row capacity (I <= XR).  The
  // I <= 64 instantiation halves the slab, keeping the tile pair near 50 KB.
  // BIAS: B column I is a constant one, so D column I is gb (as in
  // mix_bwd_fused); o-slabs partition the rows, each gb[o] has one owner.
  extern __shared__ __align__(16) char smem_raw[];
  float* xs = reinterpret_cast<float*>(smem_raw);    // [I<=XR][LD]
  float* gs = xs + (size_t)XR * LD;                  // [O_sl][LD]

  const int o0 = (int)blockIdx.y * OSL;
  const int O_sl = min(OSL, O - o0);
  const int iT = (I + (BIAS ? 1 : 0) + 15) / 16;
  const int npairs = ((O_sl + 15) / 16) * iT;

  const int lane = (int)(threadIdx.x & 63);
  const int wave = (int)(threadIdx.x >> 6);
  const int l16 = lane & 15;
  const int kg = lane >> 4;        // k-group within the MFMA K=4

  f32x4_pw acc[NPAIR];
#pragma unroll
  for (int p = 0; p < NPAIR; ++p) acc[p] = f32x4_pw{0.f, 0.f, 0.f, 0.f};

  const long ntiles = (S / TS) * (long)B;
  for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int b = (int)(t / (S / TS));
    const long s0 = (t % (S / TS)) * TS;
    for (int r = threadIdx.x; r < (I + O_sl) * (TS / 4); r += kBlock) {
      const int row = r / (TS / 4);
      const int col = (r - row * (TS / 4)) * 4;
      if (row < I) {
        *reinterpret_cast<float4*>(&xs[row * LD + col]) =
            *reinterpret_cast<const float4*>(x + ((long)b * I + row) * S + s0 + col);
      } else {
        const int ro = row - I;
        *reinterpret_cast<float4*>(&gs[ro * LD + col]) =
            *reinterpret_cast<const float4*>(gz + ((long)b * O + o0 + ro) * S + s0 + col);
      }
    }
    __syncthreads();
#pragma unroll
    for (int pp = 0; pp < NPAIR; ++pp) {
      const int p = wave + 4 * pp;
      if (p < npairs) {
        const int mt = p / iT, nt = p - mt * iT;
        const float* gr = gs + (mt * 16 + l16) * LD;         // A row
        const float* xr = xs + (nt * 16 + l16) * LD;         // B col's row
        const bool av = (mt * 16 + l16) < O_sl;
        const bool bv = (nt * 16 + l16) < I;
#pragma unroll
        for (int k = 0; k < TS; k += 4) {
          const float a = av ? gr[k + kg] : 0.f;
          const float bb = bv ? xr[k + kg]
                              : ((BIAS && nt * 16 + l16 == I) ? 1.f : 0.f);
          acc[pp] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bb, acc[pp], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

#pragma unroll
  for (int pp = 0; pp < NPAIR; ++pp) {
    const int p = wave + 4 * pp;
    if (p >= npairs) continue;
    const int mt = p / iT, nt = p - mt * iT;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = o0 + mt * 16 + kg * 4 + r;   // D row
      const int i = nt * 16 + l16;               // D col
      if (o < O && (mt * 16 + kg * 4 + r) < O_sl) {
        if (i < I) atomicAdd(&gW[(size_t)o * I + i], acc[pp][r]);
        else if (BIAS && i == I) atomicAdd(&gb[o], acc[pp][r]);
      }
    }
  }
}

}  // namespace

std::vector<at::Tensor> channel_mix_bwd_w(const at::Tensor& gz, const at::Tensor& x,
                                          bool want_bias) {
  check_real(gz, "gz"); check_real(x, "x");
  TORCH_CHECK(gz.dim() == 3 && x.dim() == 3, "gz/x must be [B,*,S]");
  int B = (int)gz.size(0), O = (int)gz.size(1), I = (int)x.size(1);
  long S = gz.size(2);
  TORCH_CHECK(x.size(0) == B && x.size(2) == S, "shape mismatch");
  TORCH_CHECK(I <= 64, "channel_mix_bwd_w: I must be <= 64");

  auto gW = at::zeros({O, I}, gz.options());
  auto gb = want_bias ? at::zeros({O}, gz.options())
                      : at::empty({0}, gz.options());
  if (gz.numel() == 0) return {gW, gb};

  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  bool is_f32 = gz.scalar_type() == at::kFloat;
  bool vec = is_f32 && (S % 4 == 0) &&
             ((reinterpret_cast<uintptr_t>(gz.data_ptr()) & 15) == 0) &&
             ((reinterpret_cast<uintptr_t>(x.data_ptr()) & 15) == 0);
  static const bool no_glds = []() {
    const char* e = getenv("DFNO_GW_NO_GLDS");  // A/B knob: force generic path
    return e && e[0] == '1';
  }();
  // rows per wave: wider cuts B re-reads but costs registers/occupancy.
  // The glds3 OW=5 variant covers O<=20 in ONE o-tile so B is read once.
  // For big-O shapes (gW3: O=128), wider OW (4: 9 GB, 6: 7.8 GB vs OW=2's
  // 14 GB of o-tile-amplified traffic) measured NO faster: per-block
  // throughput here scales with resident blocks (3/CU at the 48 KB OW=2
  // ring vs 2/CU at 60-72 KB), which exactly offsets the traffic cut.
  const bool ow5 = vec && !no_glds && I > 8 && I <= 20 && O <= 20 && O >= 8;
  const int OW = ow5 ? 5 : ((O >= 8) ? ((I <= 8) ? 4 : 2) : 1);
  int o_tiles = (O + 4 * OW - 1) / (4 * OW);
  static const long ns_cap = []() {
    const char* e = getenv("DFNO_GW_NSCHUNK");  // sweep knob
    return e ? atol(e) : 0L;
  }();
  // Grid sizing: every block atomically flushes its whole O*I accumulator,
  // so the flush cost scales with grid and serializes per cache line
  // (measured: 4096 s-chunks -> 1.84 ms, 256 -> 0.52 ms on the 20x20
  // S=7.9M flagship shape).  The glds3 kernels are 1-2 blocks/CU by LDS,
  // so one grid-wave exactly fills the 256 CUs; the generic kernel gets a
  // few more for latency-hiding.
  const bool use_glds = vec && !no_glds && O >= 8;
  int bpc = use_glds ? (ow5 ? 1 : (I <= 8 ? 2 : (o_tiles >= 8 ? 3 : 1))) : 4;
  int n_schunk = (int)std::max(
      1L, std::min((long)(256 * bpc / o_tiles), S / (64 * 16)));
  if (ns_cap > 0)
    n_schunk = (int)std::max(1L, std::min(ns_cap, S / (64 * 16)));
  // the glds3 XCD swizzle decodes schunk mod 8: keep it a bijection
  if (use_glds && o_tiles > 1) n_schunk = (n_schunk + 7) & ~7;
  int grid = n_schunk * o_tiles;

#define GW_LAUNCH(ICAP_, OW_, BIAS_, V)                                         \
  hipLaunchKernelGGL((gw_outer_kernel<scalar_t, ICAP_, OW_, BIAS_, V>),         \
                     dim3(grid), dim3(kBlock), 0, stream,                       \
                     gz.data_ptr<scalar_t>(),                                   \
                     x.data_ptr<scalar_t>(), gW.data_ptr<scalar_t>(),           \
                     want_bias ? gb.data_ptr<scalar_t>() : nullptr,             \
                     B, O, I, S, n_schunk);
#define GW_DISPATCH2(ICAP_, OW_)                                                \
    if (want_bias) {                                                            \
      if (vec) { GW_LAUNCH(ICAP_, OW_, true, true) }                            \
      else { GW_LAUNCH(ICAP_, OW_, true, false) }                               \
    } else {                                                                    \
      if (vec) { GW_LAUNCH(ICAP_, OW_, false, true) }                           \
      else { GW_LAUNCH(ICAP_, OW_, false, false) }                              \
    }
#define GW_LDS(ICAP_, OW_, TS_, NBUF_)                                          \
      hipLaunchKernelGGL(                                                       \
          (gw_outer_glds3_kernel<scalar_t, ICAP_, OW_, TS_, NBUF_>),            \
          dim3(grid), dim3(kBlock), 0, stream,                                  \
          gz.data_ptr<scalar_t>(),                                              \
          x.data_ptr<scalar_t>(), gW.data_ptr<scalar_t>(),                      \
          want_bias ? gb.data_ptr<scalar_t>() : nullptr,                        \
          B, O, I, S, n_schunk, want_bias);
  static const bool no_mfma_gw = []() {
    const char* e = getenv("DFNO_GW_NO_MFMA");  // A/B knob
    return e && e[0] == '1';
  }();
  // big-O no-bias shapes (the projection lift's gW3 [128, 20]) take the
  // f32-MFMA tile kernel; identical numerics (f32-in MFMA is a bitwise
  // fmaf chain, cdna_hip_programming.md section 3)
  if (is_f32 && vec && !no_mfma_gw && (!want_bias || I > 32) &&
      (long)O * I >= 1024 && S % 128 == 0) {
    long ntiles = (S / 128) * (long)B;
    if (I <= 32) {
      int nslab = (O + 63) / 64;
      int gx_ = (int)std::min(ntiles, (long)(256 * 3 / std::max(nslab, 1)));
      size_t smem = sizeof(float) * (size_t)(32 + std::min(O, 64)) * 132;
      hipLaunchKernelGGL((gw_mfma_f32_kernel<2>), dim3(gx_, nslab),
                         dim3(kBlock), smem, stream, gz.data_ptr<float>(),
                         x.data_ptr<float>(), gW.data_ptr<float>(), B, O,
                         (int)I, S, static_cast<float*>(nullptr));
    } else {   // 33..64 x rows: 4 i-tiles x 2 o-tiles per 32-row slab
      int nslab = (O + 31) / 32;
      int gx_ = (int)std::min(ntiles, (long)(256 * 3 / std::max(nslab, 1)));
      size_t smem = sizeof(float) * (size_t)(64 + std::min(O, 32)) * 132;
      if (want_bias) {   // 2 o-tiles x (4 i-tiles + the ones column's)
        hipLaunchKernelGGL((gw_mfma_f32_kernel<3, 64, 32, true>),
                           dim3(gx_, nslab), dim3(kBlock), smem, stream,
                           gz.data_ptr<float>(), x.data_ptr<float>(),
                           gW.data_ptr<float>(), B, O, (int)I, S,
                           gb.data_ptr<float>());
      } else {
        hipLaunchKernelGGL((gw_mfma_f32_kernel<2, 64, 32>), dim3(gx_, nslab),
                           dim3(kBlock), smem, stream, gz.data_ptr<float>(),
                           x.data_ptr<float>(), gW.data_ptr<float>(), B, O,
                           (int)I, S, static_cast<float*>(nullptr));
      }
    }
    hipError_t merr = hipGetLastError();
    TORCH_CHECK(merr == hipSuccess, "gw_mfma launch failed: ",
                hipGetErrorString(merr));
    return {gW, gb};
  }
  if (I > 32) {
    // 33..64 x rows off the MFMA conditions (ragged or unaligned S, small
    // O * I, fp64): the generic kernel with a second grid dimension over 32-row
    // i-slabs, no channel-slice copies
    const int n_islab = (I + 31) / 32;
    n_schunk = std::max(1, n_schunk / n_islab);
    grid = n_schunk * o_tiles;
#define GW_SLAB(OW_, BIAS_, V)                                                  \
    hipLaunchKernelGGL((gw_outer_kernel<scalar_t, 32, OW_, BIAS_, V, true>),    \
                       dim3(grid, n_islab), dim3(kBlock), 0, stream,            \
                       gz.data_ptr<scalar_t>(), x.data_ptr<scalar_t>(),         \
                       gW.data_ptr<scalar_t>(),                                 \
                       want_bias ? gb.data_ptr<scalar_t>() : nullptr,           \
                       B, O, I, S, n_schunk);
#define GW_SLAB2(OW_)                                                           \
    if (want_bias) {                                                            \
      if (vec) { GW_SLAB(OW_, true, true) } else { GW_SLAB(OW_, true, false) }  \
    } else {                                                                    \
      if (vec) { GW_SLAB(OW_, false, true) } else { GW_SLAB(OW_, false, false) }\
    }
    AT_DISPATCH_FLOATING_TYPES(gz.scalar_type(), "channel_mix_bwd_w", [&] {
      if (OW == 2) { GW_SLAB2(2) } else { GW_SLAB2(1) }
    });
#undef GW_SLAB2
#undef GW_SLAB
    hipError_t serr = hipGetLastError();
    TORCH_CHECK(serr == hipSuccess, "channel_mix_bwd_w launch failed: ",
                hipGetErrorString(serr));
    return {gW, gb};
  }
  AT_DISPATCH_FLOATING_TYPES(gz.scalar_type(), "channel_mix_bwd_w", [&] {
    if (ow5) { GW_LDS(20, 5, 256, 3) }
    else if (vec && !no_glds && OW == 4) { GW_LDS(8, 4, 256, 3) }
    else if (vec && !no_glds && OW == 2) {
      // big-O shapes (gW3: O=128) re-read B o_tiles times; occupancy (3
      // blocks/CU at a 48 KB TS=128 ring) beats per-stream burst length
      // there (measured 2.7 ms vs 4.4 ms at 1 block/CU, matmul 3.8 ms)
      if (I <= 24) {
        if (o_tiles >= 8) { GW_LDS(24, 2, 128, 3) }
        else { GW_LDS(24, 2, 256, 3) }
      } else {
        if (o_tiles >= 8) { GW_LDS(32, 2, 128, 3) }
        else { GW_LDS(32, 2, 256, 3) }
      }
    } else if (OW == 4) { GW_DISPATCH2(8, 4) }
    else if (OW == 2) {
      if (I <= 24) { GW_DISPATCH2(24, 2) } else { GW_DISPATCH2(32, 2) }
    } else { GW_DISPATCH2(32, 1) }
  });
#undef GW_LDS
#undef GW_DISPATCH2
#undef GW_LAUNCH
  // the glds3 kernels carry 72-120 KB static LDS: surface a refused launch
  // loudly instead of silently returning the zero-initialized gW
  hipError_t lerr = hipGetLastError();
  TORCH_CHECK(lerr == hipSuccess, "channel_mix_bwd_w launch failed: ",
              hipGetErrorString(lerr));
  return {gW, gb};
}

// ---------------------------------------------------------------------------
// fused Adam step (flat real view; complex params are elementwise-identical
// to their real views under torch's Adam). One vec4 pass over p/g/m/v.
// ---------------------------------------------------------------------------

namespace {

template <typename T, bool VECTOR>
__global__ void adam_step_kernel(T* __restrict__ p, const T* __restrict__ g,
                                 T* __restrict__ m, T* __restrict__ v,
                                 long n, T lr, T b1, T b2, T eps, T wd,
                                 T c1, T c2) {
  long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  if constexpr (VECTOR && std::is_same<T, float>::value) {
    for (long i = i0; i * 4 < n; i += stride) {
      float4 pv = *reinterpret_cast<float4*>(p + i * 4);
      const float4 gv = *reinterpret_cast<const float4*>(g + i * 4);
      float4 mv = *reinterpret_cast<float4*>(m + i * 4);
      float4 vv = *reinterpret_cast<float4*>(v + i * 4);
      float pr[4] = {pv.x, pv.y, pv.z, pv.w};
      float gr[4] = {gv.x, gv.y, gv.z, gv.w};
      float mr[4] = {mv.x, mv.y, mv.z, mv.w};
      float vr[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float gg = gr[k] + wd * pr[k];
        mr[k] = b1 * mr[k] + (1.f - b1) * gg;
        vr[k] = b2 * vr[k] + (1.f - b2) * gg * gg;
        float mh = mr[k] / c1;
        float vh = vr[k] / c2;
        pr[k] -= lr * mh / (sqrtf(vh) + eps);
      }
      *reinterpret_cast<float4*>(p + i * 4) = make_float4(pr[0], pr[1], pr[2], pr[3]);
      *reinterpret_cast<float4*>(m + i * 4) = make_float4(mr[0], mr[1], mr[2], mr[3]);
      *reinterpret_cast<float4*>(v + i * 4) = make_float4(vr[0], vr[1], vr[2], vr[3]);
    }
  } else {
    for (long i = i0; i < n; i += stride) {
      T gg = g[i] + wd * p[i];
      T mi = b1 * m[i] + (T(1) - b1) * gg;
      T vi = b2 * v[i] + (T(1) - b2) * gg * gg;
      m[i] = mi;
      v[i] = vi;
      T mh = mi / c1;
      T vh = vi / c2;
      p[i] -= lr * mh / (sqrt(vh) + eps);
    }
  }
}

// Multi-tensor Adam: the whole parameter set updates in ONE launch.  The
// pointer/size table travels by value in kernargs (fits: 40 tensors x 48 B
// < the 4 KB kernarg segment); blocks grid-stride over the concatenated
// vec4 index space and locate their tensor with a short uniform search.
constexpr int kAdamMaxT = 40;
struct AdamTab {
  float* p[kAdamMaxT];
  const float* g[kAdamMaxT];
  float* m[kAdamMaxT];
  float* v[kAdamMaxT];
  long end4[kAdamMaxT];   // exclusive prefix sum of n/4 per tensor
  float c1[kAdamMaxT], c2[kAdamMaxT];
  int nt;
};

// fp8 quantize-in-Adam side table (the spectral-weight group): the update
// pass emits the e4m3 copy for the NEXT forward using the PREVIOUS step's
// amax (delayed scaling; e4m3 conversion saturates), and reduces the new
// amax into am_out — re-quantization costs nothing beyond the bytes the
// optimizer already streams (docs/ROADMAP.md item 5).
struct AdamFp8Tab {
  unsigned char* q[kAdamMaxT];
  const float* am_in[kAdamMaxT];
  float* am_out[kAdamMaxT];
};

__global__ __launch_bounds__(kBlock) void adam_multi_kernel(
    AdamTab tab, long total4, float lr, float b1, float b2, float eps,
    float wd) {
  long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  int t = 0;
  for (long i = i0; i < total4; i += stride) {
    while (i >= tab.end4[t]) ++t;          // monotone: i increases
    long base = (t == 0) ? 0 : tab.end4[t - 1];
    long j = (i - base) * 4;
    float4 pv = *reinterpret_cast<float4*>(tab.p[t] + j);
    const float4 gv = *reinterpret_cast<const float4*>(tab.g[t] + j);
    float4 mv = *reinterpret_cast<float4*>(tab.m[t] + j);
    float4 vv = *reinterpret_cast<float4*>(tab.v[t] + j);
    float pr[4] = {pv.x, pv.y, pv.z, pv.w};
    float gr[4] = {gv.x, gv.y, gv.z, gv.w};
    float mr[4] = {mv.x, mv.y, mv.z, mv.w};
    float vr[4] = {vv.x, vv.y, vv.z, vv.w};
    const float c1 = tab.c1[t], c2 = tab.c2[t];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float gg = gr[k] + wd * pr[k];
      mr[k] = b1 * mr[k] + (1.f - b1) * gg;
      vr[k] = b2 * vr[k] + (1.f - b2) * gg * gg;
      pr[k] -= lr * (mr[k] / c1) / (sqrtf(vr[k] / c2) + eps);
    }
    *reinterpret_cast<float4*>(tab.p[t] + j) = make_float4(pr[0], pr[1], pr[2], pr[3]);
    *reinterpret_cast<float4*>(tab.m[t] + j) = make_float4(mr[0], mr[1], mr[2], mr[3]);
    *reinterpret_cast<float4*>(tab.v[t] + j) = make_float4(vr[0], vr[1], vr[2], vr[3]);
  }
}

// bf16 multi-tensor variant (the bf16 config's linear parameters): bf16
// storage for p/g/m/v (matching torch's state dtype for bf16 params), fp32
// arithmetic, 8-wide vector IO.  Replaces the stock-torch fallback's ~100
// tiny eager launches per step.
struct AdamTabB {
  unsigned short* p[kAdamMaxT];
  const unsigned short* g[kAdamMaxT];
  unsigned short* m[kAdamMaxT];
  unsigned short* v[kAdamMaxT];
  long end8[kAdamMaxT];   // exclusive prefix sum of ceil(n/8) per tensor
  long nn[kAdamMaxT];     // exact element count (ragged-tail guard)
  float c1[kAdamMaxT], c2[kAdamMaxT];
  int nt;
};

__global__ __launch_bounds__(kBlock) void adam_multi_bf16_kernel(
    AdamTabB tab, long total8, float lr, float b1, float b2, float eps,
    float wd) {
  long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  int t = 0;
  for (long i = i0; i < total8; i += stride) {
    while (i >= tab.end8[t]) ++t;
    long base = (t == 0) ? 0 : tab.end8[t - 1];
    long j = (i - base) * 8;
    const float c1 = tab.c1[t], c2 = tab.c2[t];
    if (j + 8 <= tab.nn[t]) {
      float pr[8], gr[8], mr[8], vr[8];
      load8(tab.p[t] + j, pr);
      load8(tab.g[t] + j, gr);
      load8(tab.m[t] + j, mr);
      load8(tab.v[t] + j, vr);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        float gg = gr[k] + wd * pr[k];
        mr[k] = b1 * mr[k] + (1.f - b1) * gg;
        vr[k] = b2 * vr[k] + (1.f - b2) * gg * gg;
        pr[k] -= lr * (mr[k] / c1) / (sqrtf(vr[k] / c2) + eps);
      }
      store8(tab.p[t] + j, pr);
      store8(tab.m[t] + j, mr);
      store8(tab.v[t] + j, vr);
    } else {
      for (long e = j; e < tab.nn[t]; ++e) {   // ragged tail, scalar
        float pv = __uint_as_float(((unsigned int)tab.p[t][e]) << 16);
        float gv = __uint_as_float(((unsigned int)tab.g[t][e]) << 16);
        float mv = __uint_as_float(((unsigned int)tab.m[t][e]) << 16);
        float vv = __uint_as_float(((unsigned int)tab.v[t][e]) << 16);
        float gg = gv + wd * pv;
        mv = b1 * mv + (1.f - b1) * gg;
        vv = b2 * vv + (1.f - b2) * gg * gg;
        pv -= lr * (mv / c1) / (sqrtf(vv / c2) + eps);
        __hip_bfloat16 hp = __float2bfloat16(pv);
        __hip_bfloat16 hm = __float2bfloat16(mv);
        __hip_bfloat16 hv = __float2bfloat16(vv);
        tab.p[t][e] = *reinterpret_cast<unsigned short*>(&hp);
        tab.m[t][e] = *reinterpret_cast<unsigned short*>(&hm);
        tab.v[t][e] = *reinterpret_cast<unsigned short*>(&hv);
      }
    }
  }
}

// Uniform-size variant: a group of SAME-length tensors (the 32 spectral
// corner weights dominate the parameter set) updates with blockIdx.y as the
// tensor index — no per-iteration tensor search / end4 kernarg loads at all
// (docs/ROADMAP.md item 4: runtime-trip-count folding for the Adam loop).
template <bool QOUT>
__global__ __launch_bounds__(kBlock) void adam_multi_uniform_kernel(
    AdamTab tab, AdamFp8Tab qt, long n4, float lr, float b1, float b2,
    float eps, float wd) {
  const int t = blockIdx.y;
  float* __restrict__ p = tab.p[t];
  const float* __restrict__ g = tab.g[t];
  float* __restrict__ m = tab.m[t];
  float* __restrict__ v = tab.v[t];
  const float c1 = tab.c1[t], c2 = tab.c2[t];
  float inv = 0.f, amax = 0.f;
  if constexpr (QOUT) inv = 448.f / fmaxf(*qt.am_in[t], 1e-30f);
  long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (long i = i0; i < n4; i += stride) {
    long j = i * 4;
    float4 pv = *reinterpret_cast<float4*>(p + j);
    const float4 gv = *reinterpret_cast<const float4*>(g + j);
    float4 mv = *reinterpret_cast<float4*>(m + j);
    float4 vv = *reinterpret_cast<float4*>(v + j);
    float pr[4] = {pv.x, pv.y, pv.z, pv.w};
    float gr[4] = {gv.x, gv.y, gv.z, gv.w};
    float mr[4] = {mv.x, mv.y, mv.z, mv.w};
    float vr[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float gg = gr[k] + wd * pr[k];
      mr[k] = b1 * mr[k] + (1.f - b1) * gg;
      vr[k] = b2 * vr[k] + (1.f - b2) * gg * gg;
      pr[k] -= lr * (mr[k] / c1) / (sqrtf(vr[k] / c2) + eps);
    }
    *reinterpret_cast<float4*>(p + j) = make_float4(pr[0], pr[1], pr[2], pr[3]);
    *reinterpret_cast<float4*>(m + j) = make_float4(mr[0], mr[1], mr[2], mr[3]);
    *reinterpret_cast<float4*>(v + j) = make_float4(vr[0], vr[1], vr[2], vr[3]);
    if constexpr (QOUT) {
      uchar4 qb;
      __hip_fp8_e4m3 h0(pr[0] * inv), h1(pr[1] * inv), h2(pr[2] * inv),
          h3(pr[3] * inv);
      qb.x = h0.__x; qb.y = h1.__x; qb.z = h2.__x; qb.w = h3.__x;
      *reinterpret_cast<uchar4*>(qt.q[t] + j) = qb;
#pragma unroll
      for (int k = 0; k < 4; ++k) amax = fmaxf(amax, fabsf(pr[k]));
    }
  }
  if constexpr (QOUT) {
    // block-reduce the new amax, one device atomicMax per block
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
      amax = fmaxf(amax, __shfl_down(amax, off, 64));
    __shared__ float wred[4];
    if ((threadIdx.x & 63) == 0) wred[threadIdx.x >> 6] = amax;
    __syncthreads();
    if (threadIdx.x == 0) {
      amax = fmaxf(fmaxf(wred[0], wred[1]), fmaxf(wred[2], wred[3]));
      atomicMax(reinterpret_cast<unsigned int*>(qt.am_out[t]),
                __float_as_uint(amax));
    }
  }
}

}  // namespace

static std::vector<int64_t> adam_step_batch_impl(
    std::vector<at::Tensor>& ps, std::vector<at::Tensor>& gs,
    std::vector<at::Tensor>& ms, std::vector<at::Tensor>& vs,
    double lr, double beta1, double beta2, double eps,
    double weight_decay, std::vector<int64_t>& steps,
    std::vector<at::Tensor>* qs, std::vector<at::Tensor>* am_ins,
    std::vector<at::Tensor>* am_outs) {
  TORCH_CHECK(ps.size() == gs.size() && ps.size() == ms.size() &&
              ps.size() == vs.size() && ps.size() == steps.size(),
              "adam batch: length mismatch");
  std::vector<int64_t> quantized;
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();

  // bucket vec4-eligible tensors by length: same-size groups (>= 2) take
  // the uniform kernel, the ragged rest the searched multi-tensor kernel;
  // bf16 tensors batch into the bf16 multi-tensor kernel
  std::vector<size_t> vec_idx;
  std::map<long, std::vector<size_t>> by_len;
  AdamTabB btab;
  btab.nt = 0;
  long btotal8 = 0;
  auto flush_bf16 = [&]() {
    if (btab.nt == 0) return;
    int grid = launch_grid(btotal8, kBlock, kGridCap);
    hipLaunchKernelGGL(adam_multi_bf16_kernel, dim3(grid), dim3(kBlock), 0,
                       stream, btab, btotal8, (float)lr, (float)beta1,
                       (float)beta2, (float)eps, (float)weight_decay);
    btab.nt = 0;
    btotal8 = 0;
  };
  for (size_t i = 0; i < ps.size(); ++i) {
    long n = ps[i].numel();
    bool aligned = ((reinterpret_cast<uintptr_t>(ps[i].data_ptr()) & 15) == 0) &&
                   ((reinterpret_cast<uintptr_t>(gs[i].data_ptr()) & 15) == 0) &&
                   ((reinterpret_cast<uintptr_t>(ms[i].data_ptr()) & 15) == 0) &&
                   ((reinterpret_cast<uintptr_t>(vs[i].data_ptr()) & 15) == 0);
    if (ps[i].scalar_type() == at::kBFloat16 && n > 0 && aligned) {
      int t = btab.nt++;
      btab.p[t] = reinterpret_cast<unsigned short*>(ps[i].data_ptr());
      btab.g[t] = reinterpret_cast<const unsigned short*>(gs[i].data_ptr());
      btab.m[t] = reinterpret_cast<unsigned short*>(ms[i].data_ptr());
      btab.v[t] = reinterpret_cast<unsigned short*>(vs[i].data_ptr());
      btotal8 += (n + 7) / 8;
      btab.end8[t] = btotal8;
      btab.nn[t] = n;
      btab.c1[t] = (float)(1.0 - std::pow(beta1, (double)steps[i]));
      btab.c2[t] = (float)(1.0 - std::pow(beta2, (double)steps[i]));
      if (btab.nt == kAdamMaxT) flush_bf16();
      continue;
    }
    bool vec = ps[i].scalar_type() == at::kFloat && (n % 4 == 0) && n > 0 &&
               aligned;
    if (!vec) {  // rare: odd-sized or fp64 tensor keeps the single-tensor path
      adam_step_(ps[i], gs[i], ms[i], vs[i], lr, beta1, beta2, eps,
                 weight_decay, steps[i]);
      continue;
    }
    by_len[n].push_back(i);
  }
  flush_bf16();

  auto fill = [&](AdamTab& tab, size_t i, int t) {
    tab.p[t] = ps[i].data_ptr<float>();
    tab.g[t] = gs[i].data_ptr<float>();
    tab.m[t] = ms[i].data_ptr<float>();
    tab.v[t] = vs[i].data_ptr<float>();
    tab.c1[t] = (float)(1.0 - std::pow(beta1, (double)steps[i]));
    tab.c2[t] = (float)(1.0 - std::pow(beta2, (double)steps[i]));
  };

  AdamTab rag;
  rag.nt = 0;
  long total4 = 0;
  auto flush_ragged = [&]() {
    if (rag.nt == 0) return;
    int grid = launch_grid(total4, kBlock, kGridCap);
    hipLaunchKernelGGL(adam_multi_kernel, dim3(grid), dim3(kBlock), 0, stream,
                       rag, total4, (float)lr, (float)beta1, (float)beta2,
                       (float)eps, (float)weight_decay);
    rag.nt = 0;
    total4 = 0;
  };

  for (auto& [n, idxs] : by_len) {
    if (idxs.size() < 2) {
      for (size_t i : idxs) {
        int t = rag.nt++;
        fill(rag, i, t);
        total4 += n / 4;
        rag.end4[t] = total4;
        if (rag.nt == kAdamMaxT) flush_ragged();
      }
      continue;
    }
    long n4 = n / 4;
    for (size_t off = 0; off < idxs.size(); off += kAdamMaxT) {
      AdamTab tab;
      AdamFp8Tab qt{};
      int cnt = (int)std::min<size_t>(kAdamMaxT, idxs.size() - off);
      bool all_q = qs != nullptr;
      for (int t = 0; t < cnt; ++t) {
        size_t i = idxs[off + t];
        fill(tab, i, t);
        if (all_q && (*qs)[i].defined() && (*qs)[i].numel() > 0) {
          qt.q[t] = reinterpret_cast<unsigned char*>((*qs)[i].data_ptr());
          qt.am_in[t] = (*am_ins)[i].data_ptr<float>();
          qt.am_out[t] = (*am_outs)[i].data_ptr<float>();
        } else {
          all_q = false;
        }
      }
      tab.nt = cnt;
      // size grid.x so that grid.x * cnt covers the chip at ~8 blocks/CU
      long gx = (n4 + kBlock - 1) / kBlock;
      long cap = std::max(1L, (256L * 8) / cnt);
      if (gx > cap) gx = cap;
      if (all_q) {
        for (int t = 0; t < cnt; ++t) quantized.push_back((int64_t)idxs[off + t]);
        hipLaunchKernelGGL(adam_multi_uniform_kernel<true>, dim3((int)gx, cnt),
                           dim3(kBlock), 0, stream, tab, qt, n4, (float)lr,
                           (float)beta1, (float)beta2, (float)eps,
                           (float)weight_decay);
      } else {
        hipLaunchKernelGGL(adam_multi_uniform_kernel<false>, dim3((int)gx, cnt),
                           dim3(kBlock), 0, stream, tab, qt, n4, (float)lr,
                           (float)beta1, (float)beta2, (float)eps,
                           (float)weight_decay);
      }
    }
  }
  flush_ragged();
  hipError_t lerr = hipGetLastError();
  TORCH_CHECK(lerr == hipSuccess, "adam_multi launch failed: ",
              hipGetErrorString(lerr));
  return quantized;
}

void adam_step_batch_(std::vector<at::Tensor> ps, std::vector<at::Tensor> gs,
                      std::vector<at::Tensor> ms, std::vector<at::Tensor> vs,
                      double lr, double beta1, double beta2, double eps,
                      double weight_decay, std::vector<int64_t> steps) {
  adam_step_batch_impl(ps, gs, ms, vs, lr, beta1, beta2, eps, weight_decay,
                       steps, nullptr, nullptr, nullptr);
}

std::vector<int64_t> adam_step_batch_fp8_(
    std::vector<at::Tensor> ps, std::vector<at::Tensor> gs,
    std::vector<at::Tensor> ms, std::vector<at::Tensor> vs,
    double lr, double beta1, double beta2, double eps, double weight_decay,
    std::vector<int64_t> steps, std::vector<at::Tensor> qs,
    std::vector<at::Tensor> am_ins, std::vector<at::Tensor> am_outs) {
  TORCH_CHECK(qs.size() == ps.size() && am_ins.size() == ps.size() &&
              am_outs.size() == ps.size(), "adam fp8: list size mismatch");
  // returns the indices whose e4m3 copies were refreshed in-kernel
  return adam_step_batch_impl(ps, gs, ms, vs, lr, beta1, beta2, eps,
                              weight_decay, steps, &qs, &am_ins, &am_outs);
}

void adam_step_(at::Tensor& p, const at::Tensor& g, at::Tensor& m, at::Tensor& v,
                double lr, double beta1, double beta2, double eps,
                double weight_decay, int64_t step) {
  check_real(p, "p"); check_real(g, "g"); check_real(m, "m"); check_real(v, "v");
  long n = p.numel();
  TORCH_CHECK(g.numel() == n && m.numel() == n && v.numel() == n, "adam: size mismatch");
  if (n == 0) return;
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  double c1 = 1.0 - std::pow(beta1, (double)step);
  double c2 = 1.0 - std::pow(beta2, (double)step);
  AT_DISPATCH_FLOATING_TYPES(p.scalar_type(), "adam_step_", [&] {
    bool vec = std::is_same<scalar_t, float>::value && (n % 4 == 0) &&
               ((reinterpret_cast<uintptr_t>(p.data_ptr()) & 15) == 0) &&
               ((reinterpret_cast<uintptr_t>(g.data_ptr()) & 15) == 0) &&
               ((reinterpret_cast<uintptr_t>(m.data_ptr()) & 15) == 0) &&
               ((reinterpret_cast<uintptr_t>(v.data_ptr()) & 15) == 0);
    int grid = launch_grid(vec ? (n + 3) / 4 : n, kBlock, kGridCap);
    if (vec) {
      hipLaunchKernelGGL((adam_step_kernel<scalar_t, true>), dim3(grid), dim3(kBlock),
                         0, stream, p.data_ptr<scalar_t>(), g.data_ptr<scalar_t>(),
                         m.data_ptr<scalar_t>(), v.data_ptr<scalar_t>(), n,
                         (scalar_t)lr, (scalar_t)beta1, (scalar_t)beta2,
                         (scalar_t)eps, (scalar_t)weight_decay,
                         (scalar_t)c1, (scalar_t)c2);
    } else {
      hipLaunchKernelGGL((adam_step_kernel<scalar_t, false>), dim3(grid), dim3(kBlock),
                         0, stream, p.data_ptr<scalar_t>(), g.data_ptr<scalar_t>(),
                         m.data_ptr<scalar_t>(), v.data_ptr<scalar_t>(), n,
                         (scalar_t)lr, (scalar_t)beta1, (scalar_t)beta2,
                         (scalar_t)eps, (scalar_t)weight_decay,
                         (scalar_t)c1, (scalar_t)c2);
    }
  });
}
