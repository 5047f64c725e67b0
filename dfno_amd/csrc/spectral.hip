// gfx950 (CDNA4) fused corner-block complex spectral contraction.
//
// y[b,o,f] = sum_i x[b,i,f] * w[i,o,f_box] for every frequency f inside a
// corner box of the truncated spectrum (see ops/spectral.py header for the
// roofline argument: weight-stream bandwidth-bound at batch ~1, so this is a
// streaming VALU kernel, not an MFMA one).
//
// The corner gather/scatter is fused into the addressing: threads walk the
// box in linear order (coalesced in the innermost frequency dim for both the
// weight [i][o][box] stream and the spectrum [b][c][F] stream), so no
// per-corner slice of the spectrum is ever materialized — unlike the
// reference's y[sl] = einsum(x[sl], w) over a zeroed clone
// (/root/reference/dfno/dfno.py:269-271).
//
// Parallelism: one thread owns one box element for a tile of output channels
// (OTILE accumulators); the o-tiling multiplies thread count so small
// per-rank corner shards still fill the 256-CU chip, at the price of
// re-reading the (I-element) x column once per tile — noise next to the
// I*O-element weight column.

#include <hip/hip_runtime.h>
#include <hip/hip_fp8.h>
#include <torch/extension.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <cstdlib>

#include "kernels.h"
#include "device_util.h"
#include "adam_update.h"

namespace {

using namespace dfno_io;

constexpr int kBlock = 256;
constexpr int kMaxDims = 6;

struct BoxGeom {
  // box extents and the global strides (in complex elements) of the
  // spectrum's frequency dims, plus the global offset of the box origin.
  long box[kMaxDims];
  long fstride[kMaxDims];
  long origin;   // sum(starts[d] * fstride[d])
  int nd;
  long nelem;    // prod(box)
};

template <typename T>
struct Cplx {
  T re, im;
};

// acc += a * b (complex)
template <typename T>
__device__ __forceinline__ void cmac(T& ar, T& ai, T br, T bi, T cr, T ci) {
  ar += br * cr - bi * ci;
  ai += br * ci + bi * cr;
}

// acc += conj(a) * b
template <typename T>
__device__ __forceinline__ void cmac_conj(T& ar, T& ai, T br, T bi, T cr, T ci) {
  ar += br * cr + bi * ci;
  ai += br * ci - bi * cr;
}

// OCP e4m3fn dequant (gfx950's FP8 format — NOT the MI300X fnuz variant):
// 1 sign, 4 exponent (bias 7), 3 mantissa; S.1111.111 is NaN, no infinities.
__device__ __forceinline__ float fp8_e4m3_to_f32(unsigned int v) {
  const unsigned int s = v >> 7, e = (v >> 3) & 0xf, m = v & 7;
  float f;
  if (e == 0) {
    f = (float)m * (1.f / 512.f);                 // subnormal: m * 2^-9
  } else {
    // (1 + m/8) * 2^(e-7) via exponent-bit construction
    f = __uint_as_float(((e + 120u) << 23) | (m << 20));
  }
  return s ? -f : f;
}

__device__ __forceinline__ long box_to_global(long e, const BoxGeom& g) {
  long off = g.origin;
  // innermost dim last in box[]; decompose right-to-left
  for (int d = g.nd - 1; d >= 0; --d) {
    long c = e % g.box[d];
    e /= g.box[d];
    off += c * g.fstride[d];
  }
  return off;
}

// FWD: y[b, o, f] = sum_i x[b, i, f] w[i, o, e]
// CONJT (bwd-x): gx[b, i, f] = sum_o conj(w[i, o, e]) gy[b, o, f]
//   (same code with the roles of the w indices swapped and conjugation)
template <typename T, int OTILE, bool CONJT>
__global__ __launch_bounds__(kBlock) void spectral_corner_kernel(
    const T* __restrict__ x,   // [B, CI, Ftot] complex interleaved
    const T* __restrict__ w,   // [I, O, E] complex interleaved
    T* __restrict__ y,         // [B, CO, Ftot] complex interleaved
    BoxGeom g, int B, int I, int O, long Ftot) {
  // CONJT: contraction index is o (CI = O), output index is i (CO = I)
  const int n_out = CONJT ? I : O;
  const int n_in = CONJT ? O : I;
  const long ntiles = (n_out + OTILE - 1) / OTILE;
  const long total = g.nelem * ntiles * B;

  long t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;

  for (long t = t0; t < total; t += stride) {
    long e = t % g.nelem;
    long rest = t / g.nelem;
    int tile = (int)(rest % ntiles);
    int b = (int)(rest / ntiles);

    long f = box_to_global(e, g);
    int o0 = tile * OTILE;
    int olim = min(OTILE, n_out - o0);

    T accr[OTILE], acci[OTILE];
#pragma unroll
    for (int k = 0; k < OTILE; ++k) { accr[k] = T(0); acci[k] = T(0); }

    const T* xb = x + 2 * (((long)b * n_in) * Ftot + f);
    for (int i = 0; i < n_in; ++i) {
      T xr = xb[2 * (long)i * Ftot];
      T xi = xb[2 * (long)i * Ftot + 1];
      if (CONJT) {
        // w index: [out=i_out][in=i(=o)][e]; here i iterates o (the weight's
        // second index), output k iterates the weight's first index.
#pragma unroll
        for (int k = 0; k < OTILE; ++k) {
          if (k < olim) {
          long widx = 2 * ((((long)(o0 + k)) * O + i) * g.nelem + e);
          cmac_conj(accr[k], acci[k], w[widx], w[widx + 1], xr, xi);
                  }
        }
      } else {
        const T* wb = w + 2 * (((long)i * O + o0) * g.nelem + e);
#pragma unroll
        for (int k = 0; k < OTILE; ++k) {
          if (k < olim) {
          cmac(accr[k], acci[k], xr, xi, wb[2 * (long)k * g.nelem],
               wb[2 * (long)k * g.nelem + 1]);
                  }
        }
      }
    }

    T* yb = y + 2 * (((long)b * n_out + o0) * Ftot + f);
#pragma unroll
    for (int k = 0; k < OTILE; ++k) {
      if (k < olim) {
      yb[2 * (long)k * Ftot] = accr[k];
      yb[2 * (long)k * Ftot + 1] = acci[k];
          }
    }
  }
}

// -------- multi-corner single-launch variant --------------------------------
constexpr int kMaxCorners = 8;

template <typename T>
struct MultiGeom {
  BoxGeom g[kMaxCorners];
  const T* w[kMaxCorners];    // complex-interleaved reals, or (FP8) packed
                              // re/im fp8 byte pairs reinterpreted
  const float* amax[kMaxCorners];  // FP8: device amax per corner (scale =
                                   // amax/448, computed on device — no
                                   // host sync anywhere in the fp8 path)
  long cum[kMaxCorners + 1];  // cumulative work (nelem * ntiles) per corner
  int ncorners;
};

__device__ __forceinline__ float fp8_scale_from_amax(const float* amax) {
  return fmaxf(*amax, 1e-30f) * (1.f / 448.f);
}

// NIN > 0 pins the contraction depth (n_in) at compile time: the channel
// loop fully unrolls with folded weight offsets (the round-1 probe lesson:
// runtime trip counts serialize on a uniform-load wait per iteration,
// docs/ROADMAP.md item 4; folding recovered 1.5-2x on the dft/head kernels).
template <typename T, int OTILE, bool CONJT, int NIN = 0, bool FP8 = false>
__global__ __launch_bounds__(kBlock) void spectral_corners_kernel(
    const T* __restrict__ x, MultiGeom<T> mg, T* __restrict__ y,
    int B, int I, int O, long Ftot) {
  const int n_out = CONJT ? I : O;
  const int n_in = NIN > 0 ? NIN : (CONJT ? O : I);
  const long ntiles = (n_out + OTILE - 1) / OTILE;
  const long total = mg.cum[mg.ncorners] * B;

  long t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;

  for (long t = t0; t < total; t += stride) {
    long work = t % mg.cum[mg.ncorners];
    int b = (int)(t / mg.cum[mg.ncorners]);
    int c = 0;
    while (work >= mg.cum[c + 1]) ++c;
    work -= mg.cum[c];
    const BoxGeom& g = mg.g[c];
    const T* w = mg.w[c];
    const float wscale = FP8 ? fp8_scale_from_amax(mg.amax[c]) : 1.f;
    long e = work % g.nelem;
    int tile = (int)(work / g.nelem);

    long f = box_to_global(e, g);
    int o0 = tile * OTILE;
    int olim = min(OTILE, n_out - o0);

    T accr[OTILE], acci[OTILE];
#pragma unroll
    for (int k = 0; k < OTILE; ++k) { accr[k] = T(0); acci[k] = T(0); }

    const T* xb = x + 2 * (((long)b * n_in) * Ftot + f);
    // complex weight load: fp32/fp64 interleaved reals, or (FP8) a packed
    // re/im byte pair dequantized on the fly (the weight stream is what
    // this kernel is bandwidth-bound on — fp8 storage cuts it 4x)
    auto wload = [&](long pidx, T& wr, T& wi) {
      if constexpr (FP8) {
        const unsigned short pv =
            reinterpret_cast<const unsigned short*>(w)[pidx];
        wr = (T)(fp8_e4m3_to_f32(pv & 0xffu) * wscale);
        wi = (T)(fp8_e4m3_to_f32(pv >> 8) * wscale);
      } else {
        wr = w[2 * pidx];
        wi = w[2 * pidx + 1];
      }
    };
    auto chan = [&](int i) {
      T xr = xb[2 * (long)i * Ftot];
      T xi = xb[2 * (long)i * Ftot + 1];
      if (CONJT) {
#pragma unroll
        for (int k = 0; k < OTILE; ++k) {
          if (k < olim) {
            T wr, wi;
            wload((((long)(o0 + k)) * O + i) * g.nelem + e, wr, wi);
            cmac_conj(accr[k], acci[k], wr, wi, xr, xi);
          }
        }
      } else {
#pragma unroll
        for (int k = 0; k < OTILE; ++k) {
          if (k < olim) {
            T wr, wi;
            wload(((long)i * O + o0 + k) * g.nelem + e, wr, wi);
            cmac(accr[k], acci[k], xr, xi, wr, wi);
          }
        }
      }
    };
    if constexpr (NIN > 0) {
#pragma unroll
      for (int i = 0; i < NIN; ++i) chan(i);
    } else {
      for (int i = 0; i < n_in; ++i) chan(i);
    }

    T* yb = y + 2 * (((long)b * n_out + o0) * Ftot + f);
#pragma unroll
    for (int k = 0; k < OTILE; ++k) {
      if (k < olim) {
        yb[2 * (long)k * Ftot] = accr[k];
        yb[2 * (long)k * Ftot + 1] = acci[k];
      }
    }
  }
}

// Element-pair variant (complex64): a thread owns two innermost-consecutive
// box elements, so the weight stream, x and y all move 16 bytes per lane
// (a wave touches 1 KB contiguous per access instead of 512 B).  Each
// element goes through the operations of the kernel above in the same
// order, so the results are bit-identical.  The host checks what the
// float4 accesses need (pair_ok) and keeps the kernel above otherwise.
// mg.cum counts pairs: (nelem / 2) * ntiles per corner.
template <int OTILE, bool CONJT, int NIN = 0>
__global__ __launch_bounds__(kBlock) void spectral_corners_pair_kernel(
    const float* __restrict__ x, MultiGeom<float> mg, float* __restrict__ y,
    int B, int I, int O, long Ftot) {
  const int n_out = CONJT ? I : O;
  const int n_in = NIN > 0 ? NIN : (CONJT ? O : I);
  const long total = mg.cum[mg.ncorners] * B;

  long t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;

  for (long t = t0; t < total; t += stride) {
    long work = t % mg.cum[mg.ncorners];
    int b = (int)(t / mg.cum[mg.ncorners]);
    int c = 0;
    while (work >= mg.cum[c + 1]) ++c;
    work -= mg.cum[c];
    const BoxGeom& g = mg.g[c];
    const float* w = mg.w[c];
    const long npair = g.nelem / 2;
    const long e = (work % npair) * 2;
    const int tile = (int)(work / npair);

    const long f = box_to_global(e, g);
    const int o0 = tile * OTILE;
    const int olim = min(OTILE, n_out - o0);

    float4 acc[OTILE];   // (re0, im0, re1, im1)
#pragma unroll
    for (int k = 0; k < OTILE; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);

    const float* xb = x + 2 * (((long)b * n_in) * Ftot + f);
    auto chan = [&](int i) {
      const float4 xv = *reinterpret_cast<const float4*>(xb + 2 * (long)i * Ftot);
#pragma unroll
      for (int k = 0; k < OTILE; ++k) {
        if (k < olim) {
          const long pidx = CONJT
              ? (((long)(o0 + k)) * O + i) * g.nelem + e
              : ((long)i * O + o0 + k) * g.nelem + e;
          const float4 wv = *reinterpret_cast<const float4*>(w + 2 * pidx);
          if (CONJT) {
            cmac_conj(acc[k].x, acc[k].y, wv.x, wv.y, xv.x, xv.y);
            cmac_conj(acc[k].z, acc[k].w, wv.z, wv.w, xv.z, xv.w);
          } else {
            cmac(acc[k].x, acc[k].y, xv.x, xv.y, wv.x, wv.y);
            cmac(acc[k].z, acc[k].w, xv.z, xv.w, wv.z, wv.w);
          }
        }
      }
    };
    if constexpr (NIN > 0) {
#pragma unroll
      for (int i = 0; i < NIN; ++i) chan(i);
    } else {
      for (int i = 0; i < n_in; ++i) chan(i);
    }

    float* yb = y + 2 * (((long)b * n_out + o0) * Ftot + f);
#pragma unroll
    for (int k = 0; k < OTILE; ++k) {
      if (k < olim) *reinterpret_cast<float4*>(yb + 2 * (long)k * Ftot) = acc[k];
    }
  }
}

// BWD-W: gw[i, o, e] = sum_b gy[b, o, F(e)] * conj(x[b, i, F(e)]) per
// corner -- at batch ~1 this is a pure per-frequency outer product; fusing
// the corner gather into the addressing replaces the python-side per-corner
// slice + conj materialization + complex-mul einsum chain (~0.6 ms/step of
// eager kernels at the flagship config).  One thread owns (corner, e, o)
// and streams the I outputs; writes for fixed (i, o) are e-consecutive
// across lanes (coalesced), as are the x/gy reads.
// ITILE (I_ > ICAP): the i-tile of ICAP channels joins the work index, so a
// thread's accumulators stay ICAP wide (gy is re-read once per tile).
template <typename T, int ICAP, bool ITILE = false>
__global__ __launch_bounds__(kBlock) void spectral_corners_bwd_w_kernel(
    const T* __restrict__ x, const T* __restrict__ gy, MultiGeom<T> mg,
    int B, int I_, int O, long Ftot) {
  const int ntile = ITILE ? (I_ + ICAP - 1) / ICAP : 1;
  const long total = mg.cum[mg.ncorners] * O * ntile;
  long t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;

  for (long t = t0; t < total; t += stride) {
    long work = t % mg.cum[mg.ncorners];
    int o = (int)(t / mg.cum[mg.ncorners]);
    int i0 = 0;
    if (ITILE) { i0 = (o / O) * ICAP; o %= O; }
    const int I = ITILE ? min(ICAP, I_ - i0) : I_;   // channels of this tile
    int c = 0;
    while (work >= mg.cum[c + 1]) ++c;
    long e = work - mg.cum[c];
    const BoxGeom& g = mg.g[c];
    T* gw = const_cast<T*>(mg.w[c]);

    long f = box_to_global(e, g);
    T accr[ICAP], acci[ICAP];
#pragma unroll
    for (int k = 0; k < ICAP; ++k) { accr[k] = T(0); acci[k] = T(0); }
    for (int b = 0; b < B; ++b) {
      const T* gyb = gy + 2 * (((long)b * O + o) * Ftot + f);
      const T gr = gyb[0], gi = gyb[1];
      const T* xb = x + 2 * (((long)b * I_ + i0) * Ftot + f);
#pragma unroll
      for (int k = 0; k < ICAP; ++k) {
        if (k < I) {
          // acc += gy * conj(x)  (the reference's einsum conjugates x)
          const T xr = xb[2 * (long)k * Ftot], xi = xb[2 * (long)k * Ftot + 1];
          accr[k] += xr * gr + xi * gi;
          acci[k] += xr * gi - xi * gr;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < ICAP; ++k) {
      if (k < I) {
        long widx = 2 * (((long)(i0 + k) * O + o) * g.nelem + e);
        gw[widx] = accr[k];
        gw[widx + 1] = acci[k];
      }
    }
  }
}

// GRAD-W + ADAM: the gradient above is a per-frequency outer product of two
// small spectra, and Adam is its only reader.  This kernel rebuilds
// g[i,o,e] in registers (the expressions and b order of the kernel above)
// and applies adam_update to p/m/v in the same pass, so the gradient tensor
// never reaches memory: 6 passes over the weight set instead of 7.
// One thread owns (corner, EPT innermost-consecutive box elements, o) and
// streams the I input channels.  EPT = 2: every access is 16 bytes per lane
// (the host checks what that needs); EPT = 1: 8 bytes, any shape.
// NI > 0 pins I at compile time, as NIN does in spectral_corners_kernel.
struct GradwAdamTab {
  BoxGeom g[kMaxCorners];
  float* p[kMaxCorners];
  float* m[kMaxCorners];
  float* v[kMaxCorners];
  float c1[kMaxCorners], c2[kMaxCorners];   // bias corrections per corner
  long cum[kMaxCorners + 1];   // cumulative nelem / EPT per corner
  int ncorners;
};

template <int EPT>
__device__ __forceinline__ void ldc(const float* p, float* out) {
  if constexpr (EPT == 2) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    out[0] = t.x; out[1] = t.y; out[2] = t.z; out[3] = t.w;
  } else {
    const float2 t = *reinterpret_cast<const float2*>(p);
    out[0] = t.x; out[1] = t.y;
  }
}

template <int EPT>
__device__ __forceinline__ void stc(float* p, const float* v) {
  if constexpr (EPT == 2) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
  }
}

template <int NI, int EPT>
__global__ __launch_bounds__(kBlock) void spectral_gradw_adam_kernel(
    const float* __restrict__ x, const float* __restrict__ gy,
    GradwAdamTab tab, int B, int I_, int O, long Ftot, float lr, float b1,
    float b2, float eps, float wd) {
  const int I = NI > 0 ? NI : I_;
  const long total = tab.cum[tab.ncorners] * O;
  long t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;

  for (long t = t0; t < total; t += stride) {
    long work = t % tab.cum[tab.ncorners];
    const int o = (int)(t / tab.cum[tab.ncorners]);
    int c = 0;
    while (work >= tab.cum[c + 1]) ++c;
    const long e = (work - tab.cum[c]) * EPT;
    const BoxGeom& g = tab.g[c];
    float* __restrict__ p = tab.p[c];
    float* __restrict__ m = tab.m[c];
    float* __restrict__ v = tab.v[c];
    const float c1 = tab.c1[c], c2 = tab.c2[c];

    const long f = box_to_global(e, g);
    const float* gy0 = gy + 2 * ((long)o * Ftot + f);
    const float* x0 = x + 2 * f;
    float gv0[2 * EPT];
    ldc<EPT>(gy0, gv0);

    auto chan = [&](int i) {
      float acc[2 * EPT];
#pragma unroll
      for (int k = 0; k < 2 * EPT; ++k) acc[k] = 0.f;
      for (int b = 0; b < B; ++b) {
        float gv[2 * EPT], xv[2 * EPT];
        if (b == 0) {
#pragma unroll
          for (int k = 0; k < 2 * EPT; ++k) gv[k] = gv0[k];
        } else {
          ldc<EPT>(gy0 + 2 * (long)b * O * Ftot, gv);
        }
        ldc<EPT>(x0 + 2 * ((long)b * I + i) * Ftot, xv);
#pragma unroll
        for (int k = 0; k < EPT; ++k) {
          const float xr = xv[2 * k], xi = xv[2 * k + 1];
          const float gr = gv[2 * k], gi = gv[2 * k + 1];
          acc[2 * k] += xr * gr + xi * gi;
          acc[2 * k + 1] += xr * gi - xi * gr;
        }
      }
      const long widx = 2 * (((long)i * O + o) * g.nelem + e);
      float pr[2 * EPT], mr[2 * EPT], vr[2 * EPT];
      ldc<EPT>(p + widx, pr);
      ldc<EPT>(m + widx, mr);
      ldc<EPT>(v + widx, vr);
#pragma unroll
      for (int k = 0; k < 2 * EPT; ++k)
        adam_update(pr[k], acc[k], mr[k], vr[k], lr, b1, b2, eps, wd, c1, c2);
      stc<EPT>(p + widx, pr);
      stc<EPT>(m + widx, mr);
      stc<EPT>(v + widx, vr);
    };
    if constexpr (NI > 0) {
#pragma unroll
      for (int i = 0; i < NI; ++i) chan(i);
    } else {
#pragma unroll 4
      for (int i = 0; i < I; ++i) chan(i);
    }
  }
}


BoxGeom make_geom(const at::Tensor& x, const at::Tensor& w,
                  const std::vector<int64_t>& starts) {
  BoxGeom g{};
  int nd = (int)x.dim() - 2;
  TORCH_CHECK(nd >= 1 && nd <= kMaxDims, "spectral: bad ndim");
  TORCH_CHECK((int)w.dim() - 2 == nd, "spectral: w ndim mismatch");
  TORCH_CHECK((int)starts.size() == nd, "spectral: starts size mismatch");
  g.nd = nd;
  g.nelem = 1;
  // frequency strides of the spectrum (contiguous layout)
  long stride = 1;
  long fs[kMaxDims];
  for (int d = nd - 1; d >= 0; --d) {
    fs[d] = stride;
    stride *= x.size(d + 2);
  }
  g.origin = 0;
  for (int d = 0; d < nd; ++d) {
    g.box[d] = w.size(d + 2);
    g.fstride[d] = fs[d];
    g.origin += starts[d] * fs[d];
    g.nelem *= g.box[d];
  }
  return g;
}

// What the element-pair kernels need of one corner: a 16-byte aligned
// weight tensor, and pairs that stay inside one innermost row of the box
// and start on an even element of the spectrum's innermost row.  The
// spectra themselves must be 16-byte aligned as well (checked by the caller).
bool pair_ok(const at::Tensor& spec, const at::Tensor& w,
             const std::vector<int64_t>& starts) {
  const int64_t last = spec.dim() - 1;
  return aligned16(w.data_ptr()) && w.size(last) % 2 == 0 &&
         spec.size(last) % 2 == 0 && starts.back() % 2 == 0;
}

void check_c(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == at::kComplexFloat || t.scalar_type() == at::kComplexDouble,
              name, " must be complex64/complex128");
}

}  // namespace

void spectral_corner_fwd(const at::Tensor& x, const at::Tensor& w, at::Tensor& y,
                         std::vector<int64_t> starts) {
  check_c(x, "x"); check_c(w, "w"); check_c(y, "y");
  int B = (int)x.size(0), I = (int)x.size(1), O = (int)y.size(1);
  TORCH_CHECK((int)w.size(0) == I && (int)w.size(1) == O, "spectral: w shape");
  long Ftot = 1;
  for (int d = 2; d < x.dim(); ++d) Ftot *= x.size(d);
  BoxGeom g = make_geom(x, w, starts);
  if (g.nelem == 0 || B == 0) return;

  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  constexpr int OT = 8;
  long ntiles = (O + OT - 1) / OT;
  int grid = launch_grid(g.nelem * ntiles * B, kBlock, 256L * 16);

  if (x.scalar_type() == at::kComplexFloat) {
    hipLaunchKernelGGL((spectral_corner_kernel<float, OT, false>), dim3(grid),
                       dim3(kBlock), 0, stream,
                       reinterpret_cast<const float*>(x.data_ptr()),
                       reinterpret_cast<const float*>(w.data_ptr()),
                       reinterpret_cast<float*>(y.data_ptr()), g, B, I, O, Ftot);
  } else {
    hipLaunchKernelGGL((spectral_corner_kernel<double, OT, false>), dim3(grid),
                       dim3(kBlock), 0, stream,
                       reinterpret_cast<const double*>(x.data_ptr()),
                       reinterpret_cast<const double*>(w.data_ptr()),
                       reinterpret_cast<double*>(y.data_ptr()), g, B, I, O, Ftot);
  }
}

void spectral_corner_bwd_x(const at::Tensor& gy, const at::Tensor& w, at::Tensor& gx,
                           std::vector<int64_t> starts) {
  check_c(gy, "gy"); check_c(w, "w"); check_c(gx, "gx");
  int B = (int)gy.size(0), O = (int)gy.size(1), I = (int)gx.size(1);
  TORCH_CHECK((int)w.size(0) == I && (int)w.size(1) == O, "spectral: w shape");
  long Ftot = 1;
  for (int d = 2; d < gy.dim(); ++d) Ftot *= gy.size(d);
  BoxGeom g = make_geom(gy, w, starts);
  if (g.nelem == 0 || B == 0) return;

  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  constexpr int OT = 8;
  long ntiles = (I + OT - 1) / OT;
  int grid = launch_grid(g.nelem * ntiles * B, kBlock, 256L * 16);

  if (gy.scalar_type() == at::kComplexFloat) {
    hipLaunchKernelGGL((spectral_corner_kernel<float, OT, true>), dim3(grid),
                       dim3(kBlock), 0, stream,
                       reinterpret_cast<const float*>(gy.data_ptr()),
                       reinterpret_cast<const float*>(w.data_ptr()),
                       reinterpret_cast<float*>(gx.data_ptr()), g, B, I, O, Ftot);
  } else {
    hipLaunchKernelGGL((spectral_corner_kernel<double, OT, true>), dim3(grid),
                       dim3(kBlock), 0, stream,
                       reinterpret_cast<const double*>(gy.data_ptr()),
                       reinterpret_cast<const double*>(w.data_ptr()),
                       reinterpret_cast<double*>(gx.data_ptr()), g, B, I, O, Ftot);
  }
}

// single-launch multi-corner entries ----------------------------------------

// device-side fp8 quantization: one amax-reduce kernel + one encode kernel
// over all corners (the eager-torch version cost ~160 launches and a
// device->host scale sync per step)

__global__ __launch_bounds__(kBlock) void fp8_amax_kernel(
    const float* const* __restrict__ srcs, const long* __restrict__ numels,
    float* const* __restrict__ amaxes) {
  const int c = blockIdx.y;
  const float* src = srcs[c];
  const long n = numels[c];
  float m = 0.f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x)
    m = fmaxf(m, fabsf(src[i]));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    m = fmaxf(m, __shfl_down(m, off, 64));
  __shared__ float wred[4];
  if ((threadIdx.x & 63) == 0) wred[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(wred[0], wred[1]), fmaxf(wred[2], wred[3]));
    // non-negative floats compare correctly as raw uints
    atomicMax(reinterpret_cast<unsigned int*>(amaxes[c]),
              __float_as_uint(m));
  }
}

__global__ __launch_bounds__(kBlock) void fp8_encode_kernel(
    const float* const* __restrict__ srcs, const long* __restrict__ numels,
    float* const* __restrict__ amaxes, unsigned char* const* __restrict__ dsts) {
  const int c = blockIdx.y;
  const float* src = srcs[c];
  unsigned char* dst = dsts[c];
  const long n = numels[c];
  const float inv = 1.f / fp8_scale_from_amax(amaxes[c]);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x) {
    __hip_fp8_e4m3 h(src[i] * inv);
    dst[i] = h.__x;
  }
}

template <typename T, bool CONJT, bool FP8 = false>
static void launch_corners(const at::Tensor& x,
                           const std::vector<at::Tensor>& ws,
                           at::Tensor& y,
                           const std::vector<std::vector<int64_t>>& starts,
                           int B, int I, int O, long Ftot,
                           const std::vector<at::Tensor>* amaxes = nullptr) {
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  const int n_out = CONJT ? I : O;
  const int n_in = CONJT ? O : I;

  if constexpr (std::is_same<T, float>::value && !FP8) {
    // element-pair kernel where every corner of the call allows it
    // (DFNO_SPECTRAL_PAIR=0 keeps the 8-byte kernel, for A/B runs)
    const char* env = std::getenv("DFNO_SPECTRAL_PAIR");
    bool pair = !(env && env[0] == '0') && aligned16(x.data_ptr()) &&
                aligned16(y.data_ptr());
    for (size_t k = 0; pair && k < ws.size(); ++k)
      pair = ws[k].dim() == x.dim() &&
             (int64_t)starts[k].size() == x.dim() - 2 &&
             (ws[k].numel() == 0 || pair_ok(x, ws[k], starts[k]));
    // o-tile 4 with half the threads: 4 and 5 measured alike in the step
    // trace (97 us per call at the flagship), 8 no faster than the 8-byte
    // kernel (136 us: 88 VGPRs, 5 waves/SIMD)
    constexpr int ot = 4;
    if (pair) {
      size_t idx = 0;
      while (idx < ws.size()) {
        MultiGeom<float> mg{};
        mg.ncorners = 0;
        mg.cum[0] = 0;
        const long ntiles = (n_out + ot - 1) / ot;
        while (idx < ws.size() && mg.ncorners < kMaxCorners) {
          BoxGeom g = make_geom(x, ws[idx], starts[idx]);
          if (g.nelem == 0) { ++idx; continue; }
          int c = mg.ncorners++;
          mg.g[c] = g;
          mg.w[c] = reinterpret_cast<const float*>(ws[idx].data_ptr());
          mg.cum[c + 1] = mg.cum[c] + (g.nelem / 2) * ntiles;
          ++idx;
        }
        if (mg.ncorners == 0) continue;
        int grid = launch_grid(mg.cum[mg.ncorners] * B, kBlock, 256L * 16);
#define SPP_LAUNCH(NINV)                                                       \
        hipLaunchKernelGGL((spectral_corners_pair_kernel<ot, CONJT, NINV>),    \
                           dim3(grid), dim3(kBlock), 0, stream,                \
                           reinterpret_cast<const float*>(x.data_ptr()), mg,   \
                           reinterpret_cast<float*>(y.data_ptr()), B, I, O,    \
                           Ftot);
        if (n_in == 20) { SPP_LAUNCH(20) }
        else if (n_in == 32) { SPP_LAUNCH(32) }
        else if (n_in == 8) { SPP_LAUNCH(8) }
        else { SPP_LAUNCH(0) }
#undef SPP_LAUNCH
      }
      return;
    }
  }

  constexpr int OT = 8;
  long ntiles = (n_out + OT - 1) / OT;

  size_t idx = 0;
  while (idx < ws.size()) {
    MultiGeom<T> mg{};
    mg.ncorners = 0;
    mg.cum[0] = 0;
    while (idx < ws.size() && mg.ncorners < kMaxCorners) {
      BoxGeom g = make_geom(x, ws[idx], starts[idx]);
      if (g.nelem == 0) { ++idx; continue; }
      int c = mg.ncorners++;
      mg.g[c] = g;
      mg.w[c] = reinterpret_cast<const T*>(ws[idx].data_ptr());
      mg.amax[c] = amaxes ? (*amaxes)[idx].data_ptr<float>() : nullptr;
      mg.cum[c + 1] = mg.cum[c] + g.nelem * ntiles;
      ++idx;
    }
    if (mg.ncorners == 0) continue;
    int grid = launch_grid(mg.cum[mg.ncorners] * B, kBlock, 256L * 16);
#define SPC_LAUNCH(NINV)                                                       \
    hipLaunchKernelGGL((spectral_corners_kernel<T, OT, CONJT, NINV, FP8>),     \
                       dim3(grid), dim3(kBlock), 0, stream,                    \
                       reinterpret_cast<const T*>(x.data_ptr()), mg,           \
                       reinterpret_cast<T*>(y.data_ptr()), B, I, O, Ftot);
    // compile-time channel depth for the common widths (flagship 20)
    if (n_in == 20) { SPC_LAUNCH(20) }
    else if (n_in == 32) { SPC_LAUNCH(32) }
    else if (n_in == 8) { SPC_LAUNCH(8) }
    else { SPC_LAUNCH(0) }
#undef SPC_LAUNCH
  }
}

void spectral_corners_fwd(const at::Tensor& x, std::vector<at::Tensor> ws,
                          at::Tensor& y, std::vector<std::vector<int64_t>> starts) {
  check_c(x, "x"); check_c(y, "y");
  TORCH_CHECK(ws.size() == starts.size(), "ws/starts size mismatch");
  int B = (int)x.size(0), I = (int)x.size(1), O = (int)y.size(1);
  long Ftot = 1;
  for (int d = 2; d < x.dim(); ++d) Ftot *= x.size(d);
  for (auto& w : ws) {
    check_c(w, "w");
    TORCH_CHECK((int)w.size(0) == I && (int)w.size(1) == O, "spectral: w shape");
  }
  if (B == 0 || ws.empty()) return;
  if (x.scalar_type() == at::kComplexFloat) {
    launch_corners<float, false>(x, ws, y, starts, B, I, O, Ftot);
  } else {
    launch_corners<double, false>(x, ws, y, starts, B, I, O, Ftot);
  }
  DFNO_CHECK_LAUNCH("spectral");
}

// fp8 spectral-weight variants (BASELINE.json config #5): weights arrive as
// packed e4m3 re/im byte pairs (uint16 view, same index space as the master
// complex tensor) with one dequant scale per corner; the spectrum stays
// complex64.  grad-W is unchanged (straight-through to the fp32 master).

static void check_w16(const at::Tensor& t) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
              t.scalar_type() == at::kUInt16,
              "spectral fp8: weights must be contiguous uint16 (packed e4m3 pairs)");
}

void spectral_corners_fwd_fp8(const at::Tensor& x, std::vector<at::Tensor> w16s,
                              std::vector<at::Tensor> amaxes, at::Tensor& y,
                              std::vector<std::vector<int64_t>> starts) {
  check_c(x, "x"); check_c(y, "y");
  TORCH_CHECK(w16s.size() == starts.size() && amaxes.size() == w16s.size(),
              "fp8 ws/starts/amaxes size mismatch");
  TORCH_CHECK(x.scalar_type() == at::kComplexFloat, "fp8 spectral: c64 only");
  int B = (int)x.size(0), I = (int)x.size(1), O = (int)y.size(1);
  long Ftot = 1;
  for (int d = 2; d < x.dim(); ++d) Ftot *= x.size(d);
  for (auto& w : w16s) {
    check_w16(w);
    TORCH_CHECK((int)w.size(0) == I && (int)w.size(1) == O, "fp8 w shape");
  }
  if (B == 0 || w16s.empty()) return;
  launch_corners<float, false, true>(x, w16s, y, starts, B, I, O, Ftot, &amaxes);
  DFNO_CHECK_LAUNCH("spectral_fp8");
}

void spectral_corners_bwd_x_fp8(const at::Tensor& gy, std::vector<at::Tensor> w16s,
                                std::vector<at::Tensor> amaxes, at::Tensor& gx,
                                std::vector<std::vector<int64_t>> starts) {
  check_c(gy, "gy"); check_c(gx, "gx");
  TORCH_CHECK(w16s.size() == starts.size() && amaxes.size() == w16s.size(),
              "fp8 ws/starts/amaxes size mismatch");
  TORCH_CHECK(gy.scalar_type() == at::kComplexFloat, "fp8 spectral: c64 only");
  int B = (int)gy.size(0), O = (int)gy.size(1), I = (int)gx.size(1);
  long Ftot = 1;
  for (int d = 2; d < gy.dim(); ++d) Ftot *= gy.size(d);
  for (auto& w : w16s) {
    check_w16(w);
    TORCH_CHECK((int)w.size(0) == I && (int)w.size(1) == O, "fp8 w shape");
  }
  if (B == 0 || w16s.empty()) return;
  launch_corners<float, true, true>(gy, w16s, gx, starts, B, I, O, Ftot, &amaxes);
  DFNO_CHECK_LAUNCH("spectral_fp8");
}

void fp8_quant_corners(std::vector<at::Tensor> ws, std::vector<at::Tensor> w16s,
                       std::vector<at::Tensor> amaxes) {
  // device-only re-quantization of complex64 masters into packed e4m3
  // pairs: amax-reduce then encode, two launches for ALL corners, no sync
  const int n = (int)ws.size();
  TORCH_CHECK((int)w16s.size() == n && (int)amaxes.size() == n,
              "fp8 quant: list size mismatch");
  if (n == 0) return;
  TORCH_CHECK(n <= 64, "fp8 quant: too many corners per call");
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();

  std::vector<int64_t> host(4 * n);
  long max_numel = 1;
  for (int i = 0; i < n; ++i) {
    TORCH_CHECK(ws[i].is_cuda() && ws[i].is_contiguous() &&
                ws[i].scalar_type() == at::kComplexFloat, "fp8 quant: c64 masters");
    check_w16(w16s[i]);
    TORCH_CHECK(amaxes[i].is_cuda() && amaxes[i].scalar_type() == at::kFloat &&
                amaxes[i].numel() == 1, "fp8 quant: amax slots");
    long numel = ws[i].numel() * 2;   // real words
    TORCH_CHECK(w16s[i].numel() == ws[i].numel(), "fp8 quant: shape mismatch");
    host[i] = (int64_t)ws[i].data_ptr();
    host[n + i] = numel;
    host[2 * n + i] = (int64_t)amaxes[i].data_ptr();
    host[3 * n + i] = (int64_t)w16s[i].data_ptr();
    max_numel = std::max(max_numel, numel);
    amaxes[i].zero_();
  }
  auto opts = at::TensorOptions().dtype(at::kLong);
  auto dev_tab = at::from_blob(host.data(), {4 * (long)n}, opts)
                     .to(ws[0].device(), /*non_blocking=*/false);
  auto tab = dev_tab.data_ptr<int64_t>();
  auto srcs = reinterpret_cast<const float* const*>(tab);
  auto numels = reinterpret_cast<const long*>(tab + n);
  auto amx = reinterpret_cast<float* const*>(tab + 2 * n);
  auto dsts = reinterpret_cast<unsigned char* const*>(tab + 3 * n);

  long gx = std::min((max_numel + kBlock - 1) / kBlock, 512L);
  hipLaunchKernelGGL(fp8_amax_kernel, dim3((int)gx, n), dim3(kBlock), 0,
                     stream, srcs, numels, amx);
  hipLaunchKernelGGL(fp8_encode_kernel, dim3((int)gx, n), dim3(kBlock), 0,
                     stream, srcs, numels, amx, dsts);
  DFNO_CHECK_LAUNCH("fp8_quant");
}

void spectral_corners_bwd_w(const at::Tensor& x, const at::Tensor& gy,
                            std::vector<at::Tensor> gws,
                            std::vector<std::vector<int64_t>> starts) {
  check_c(x, "x"); check_c(gy, "gy");
  TORCH_CHECK(gws.size() == starts.size(), "gws/starts size mismatch");
  int B = (int)x.size(0), I = (int)x.size(1), O = (int)gy.size(1);
  TORCH_CHECK(I <= 64, "spectral_bwd_w: I must be <= 64");
  long Ftot = 1;
  for (int d = 2; d < x.dim(); ++d) Ftot *= x.size(d);
  for (auto& w : gws) {
    check_c(w, "gw");
    TORCH_CHECK((int)w.size(0) == I && (int)w.size(1) == O, "spectral: gw shape");
  }
  if (B == 0 || gws.empty()) return;
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
#define SBW(T, ICAP_, ...)                                                        \
  {                                                                            \
    size_t idx = 0;                                                            \
    while (idx < gws.size()) {                                                 \
      MultiGeom<T> mg{};                                                       \
      mg.ncorners = 0;                                                         \
      mg.cum[0] = 0;                                                           \
      while (idx < gws.size() && mg.ncorners < kMaxCorners) {                  \
        BoxGeom g = make_geom(x, gws[idx], starts[idx]);                       \
        if (g.nelem == 0) { ++idx; continue; }                                 \
        int c = mg.ncorners++;                                                 \
        mg.g[c] = g;                                                           \
        mg.w[c] = reinterpret_cast<const T*>(gws[idx].data_ptr());             \
        mg.cum[c + 1] = mg.cum[c] + g.nelem;                                   \
        ++idx;                                                                 \
      }                                                                        \
      if (mg.ncorners == 0) continue;                                          \
      int grid = launch_grid(mg.cum[mg.ncorners] * O * ((I + ICAP_ - 1) / ICAP_),\
                             kBlock, 256L * 16);                               \
      hipLaunchKernelGGL((spectral_corners_bwd_w_kernel<T, ICAP_ __VA_ARGS__>),\
                         dim3(grid), dim3(kBlock), 0, stream,                  \
                         reinterpret_cast<const T*>(x.data_ptr()),             \
                         reinterpret_cast<const T*>(gy.data_ptr()), mg,        \
                         B, I, O, Ftot);                                       \
    }                                                                          \
  }
  if (x.scalar_type() == at::kComplexFloat) {
    if (I <= 8) { SBW(float, 8) } else if (I <= 24) { SBW(float, 24) }
    else if (I <= 32) { SBW(float, 32) } else { SBW(float, 32, , true) }
  } else {
    if (I <= 8) { SBW(double, 8) } else if (I <= 24) { SBW(double, 24) }
    else if (I <= 32) { SBW(double, 32) } else { SBW(double, 32, , true) }
  }
#undef SBW
  DFNO_CHECK_LAUNCH("spectral");
}

void spectral_corners_bwd_x(const at::Tensor& gy, std::vector<at::Tensor> ws,
                            at::Tensor& gx, std::vector<std::vector<int64_t>> starts) {
  check_c(gy, "gy"); check_c(gx, "gx");
  TORCH_CHECK(ws.size() == starts.size(), "ws/starts size mismatch");
  int B = (int)gy.size(0), O = (int)gy.size(1), I = (int)gx.size(1);
  long Ftot = 1;
  for (int d = 2; d < gy.dim(); ++d) Ftot *= gy.size(d);
  for (auto& w : ws) {
    check_c(w, "w");
    TORCH_CHECK((int)w.size(0) == I && (int)w.size(1) == O, "spectral: w shape");
  }
  if (B == 0 || ws.empty()) return;
  if (gy.scalar_type() == at::kComplexFloat) {
    launch_corners<float, true>(gy, ws, gx, starts, B, I, O, Ftot);
  } else {
    launch_corners<double, true>(gy, ws, gx, starts, B, I, O, Ftot);
  }
  DFNO_CHECK_LAUNCH("spectral");
}

// fused grad-W + Adam over one block's corners (complex64 only): see
// spectral_gradw_adam_kernel.  ps/ms/vs are the corner weights and their
// exp_avg / exp_avg_sq, steps the already-incremented step counts.
void spectral_gradw_adam_(const at::Tensor& x, const at::Tensor& gy,
                          std::vector<at::Tensor> ps,
                          std::vector<at::Tensor> ms,
                          std::vector<at::Tensor> vs,
                          std::vector<std::vector<int64_t>> starts,
                          double lr, double beta1, double beta2, double eps,
                          double weight_decay, std::vector<int64_t> steps) {
  check_c(x, "x"); check_c(gy, "gy");
  TORCH_CHECK(x.scalar_type() == at::kComplexFloat &&
              gy.scalar_type() == at::kComplexFloat,
              "spectral_gradw_adam_: complex64 only");
  const size_t n = ps.size();
  TORCH_CHECK(ms.size() == n && vs.size() == n && starts.size() == n &&
              steps.size() == n, "spectral_gradw_adam_: list size mismatch");
  TORCH_CHECK(x.dim() == gy.dim() && x.size(0) == gy.size(0),
              "spectral_gradw_adam_: x/gy shape mismatch");
  const int nd = (int)x.dim() - 2;
  for (int d = 0; d < nd; ++d)
    TORCH_CHECK(x.size(d + 2) == gy.size(d + 2),
                "spectral_gradw_adam_: x/gy shape mismatch");
  int B = (int)x.size(0), I = (int)x.size(1), O = (int)gy.size(1);
  long Ftot = 1;
  for (int d = 2; d < x.dim(); ++d) Ftot *= x.size(d);
  if (B == 0 || n == 0 || I == 0 || O == 0) return;

  // 16-byte accesses: see pair_ok
  bool vec = aligned16(x.data_ptr()) && aligned16(gy.data_ptr());
  for (size_t k = 0; k < n; ++k) {
    const at::Tensor& p = ps[k];
    check_c(p, "p"); check_c(ms[k], "exp_avg"); check_c(vs[k], "exp_avg_sq");
    TORCH_CHECK(p.scalar_type() == at::kComplexFloat &&
                ms[k].scalar_type() == at::kComplexFloat &&
                vs[k].scalar_type() == at::kComplexFloat,
                "spectral_gradw_adam_: complex64 only");
    TORCH_CHECK(p.dim() == x.dim() && (int)p.size(0) == I &&
                (int)p.size(1) == O, "spectral_gradw_adam_: p shape");
    TORCH_CHECK(ms[k].sizes() == p.sizes() && vs[k].sizes() == p.sizes(),
                "spectral_gradw_adam_: state shape");
    TORCH_CHECK((int)starts[k].size() == nd, "spectral_gradw_adam_: starts");
    for (int d = 0; d < nd; ++d)
      TORCH_CHECK(starts[k][d] >= 0 &&
                  starts[k][d] + p.size(d + 2) <= x.size(d + 2),
                  "spectral_gradw_adam_: corner box outside the spectrum");
    vec = vec && pair_ok(x, p, starts[k]) && aligned16(ms[k].data_ptr()) &&
          aligned16(vs[k].data_ptr());
  }

  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  const int ept = vec ? 2 : 1;
  size_t idx = 0;
  while (idx < n) {
    GradwAdamTab tab{};
    tab.ncorners = 0;
    tab.cum[0] = 0;
    while (idx < n && tab.ncorners < kMaxCorners) {
      BoxGeom g = make_geom(x, ps[idx], starts[idx]);
      if (g.nelem == 0) { ++idx; continue; }
      int c = tab.ncorners++;
      tab.g[c] = g;
      tab.p[c] = reinterpret_cast<float*>(ps[idx].data_ptr());
      tab.m[c] = reinterpret_cast<float*>(ms[idx].data_ptr());
      tab.v[c] = reinterpret_cast<float*>(vs[idx].data_ptr());
      tab.c1[c] = (float)(1.0 - std::pow(beta1, (double)steps[idx]));
      tab.c2[c] = (float)(1.0 - std::pow(beta2, (double)steps[idx]));
      tab.cum[c + 1] = tab.cum[c] + g.nelem / ept;   // nelem even when ept 2
      ++idx;
    }
    if (tab.ncorners == 0) continue;
    int grid = launch_grid(tab.cum[tab.ncorners] * O, kBlock, 256L * 32);
#define SGA_LAUNCH(NI_, EPT_)                                                  \
    hipLaunchKernelGGL((spectral_gradw_adam_kernel<NI_, EPT_>), dim3(grid),    \
                       dim3(kBlock), 0, stream,                                \
                       reinterpret_cast<const float*>(x.data_ptr()),           \
                       reinterpret_cast<const float*>(gy.data_ptr()), tab, B,  \
                       I, O, Ftot, (float)lr, (float)beta1, (float)beta2,      \
                       (float)eps, (float)weight_decay);
#define SGA_EPT(NI_) if (vec) { SGA_LAUNCH(NI_, 2) } else { SGA_LAUNCH(NI_, 1) }
    if (I == 20) { SGA_EPT(20) }
    else if (I == 32) { SGA_EPT(32) }
    else if (I == 8) { SGA_EPT(8) }
    else { SGA_EPT(0) }
#undef SGA_EPT
#undef SGA_LAUNCH
  }
  DFNO_CHECK_LAUNCH("spectral_gradw_adam");
}
