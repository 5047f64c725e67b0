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
#include <torch/extension.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <vector>

#include "kernels.h"
#include "gelu_math.h"
#include "device_util.h"

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
  return aligned16(x) && aligned16(y) && (!write_z || aligned16(z));
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
