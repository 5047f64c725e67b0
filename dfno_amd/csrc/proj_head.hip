// gfx950 fused FNO projection head: out = W4 @ gelu(W3 @ x + b3) + b4.
//
// The reference computes this as two BroadcastedLinear einsums with a
// separate GELU between (/root/reference/dfno/dfno.py:348-352), which at the
// flagship config materializes a [1,128,64^3*30] fp32 intermediate (~4 GB)
// three times over (einsum out, bias add, gelu out).  On MI355X that is
// ~25 GB of pointless HBM traffic per forward (and ~2x in backward).
//
// Here the whole head is one pass: each thread holds its x column (I<=32
// channels) in registers, walks the M<=512 hidden channels recomputing
// z3 = W3 x + b3 on the fly (weights via wave-uniform scalar loads), and
// accumulates the O2<=8 outputs.  Forward traffic = read x + write out.
//
// Backward, flagship shape (I=20, M=128, O2<=2, fp32/bf16 IO):
// proj_head_bwd_fused_kernel — ONE kernel over 64-column S-tiles that
// recomputes z3 via v_mfma_f32_16x16x4, produces grad-x (second MFMA
// pair), grad-W3 (fragments carried across tiles), grad-b3/grad-W4
// (register partials, one shfl per tile) and grad-b4; the [B,128,S]
// hidden-grad tensor (~4 GB at the flagship) never exists in HBM.
// Generic shapes keep the original proj_head_bwd_kernel, which DOES
// materialize gz3 for the channel_mix grad-x / grad-W3 reductions.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <torch/extension.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include "kernels.h"
#include "gelu_math.h"
#include "device_util.h"

namespace {

using namespace dfno_io;

constexpr int kBlock = 256;

typedef float f32x4_ph __attribute__((ext_vector_type(4)));

template <typename T, int IMAX, int O2MAX, int VEC, bool VECTOR,
          int MT = 0, int IT = 0, typename TIO = T>
__global__ __launch_bounds__(kBlock) void proj_head_fwd_kernel(
    const TIO* __restrict__ x, const T* __restrict__ W3l, const T* __restrict__ b3l,
    const T* __restrict__ W4l, const T* __restrict__ b4l, TIO* __restrict__ out,
    int B, int I_, int M_, int O2, long S) {
  // MT/IT > 0 pin the hidden width and input channels at compile time: the
  // M-loop fully unrolls with weight offsets folded into the scalar loads
  // (runtime-M serializes a scalar-load wait per hidden unit; the same fix
  // bought 1.9x on the r2c kernels)
  const int I = IT > 0 ? IT : I_;
  const int M = MT > 0 ? MT : M_;
  // weights are read straight through the kernel-arg pointers: every access
  // index is wave-uniform, so they lower to scalar loads (s-cache) instead
  // of per-MAC LDS reads that double the issue count.

  long nchunks = (S + VEC - 1) / VEC;
  long t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;

  for (long t = t0; t < (long)B * nchunks; t += stride) {
    int b = (int)(t / nchunks);
    long s = (t % nchunks) * VEC;
    bool full = (s + VEC) <= S;
    int nv = full ? VEC : (int)(S - s);

    T xr[IMAX][VEC];
    const TIO* xb = x + ((long)b * I) * S + s;
    if constexpr (VECTOR && std::is_same<T, float>::value &&
                  std::is_same<TIO, float>::value) {
#pragma unroll
      for (int i = 0; i < IMAX; ++i) {
        if (i < I) {
        const float4 v = *reinterpret_cast<const float4*>(
            reinterpret_cast<const float*>(xb) + (long)i * S);
        xr[i][0] = v.x; xr[i][1] = v.y; xr[i][2] = v.z; xr[i][3] = v.w;
              }
      }
    } else {
#pragma unroll
      for (int i = 0; i < IMAX; ++i) {
        if (i < I) {
#pragma unroll
        for (int k = 0; k < VEC; ++k)
          xr[i][k] = (full || k < nv) ? (T)ld(xb + (long)i * S + k) : T(0);
              }
      }
    }

    T acc[O2MAX][VEC];
#pragma unroll
    for (int o = 0; o < O2MAX; ++o) {
      if (o < O2) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[o][k] = b4l[o];
          }
    }

#pragma unroll 8
    for (int j = 0; j < (MT > 0 ? MT : 512); ++j) {
      if (MT == 0 && j >= M) break;
      T zk[VEC];
      T bj = b3l[j];
#pragma unroll
      for (int k = 0; k < VEC; ++k) zk[k] = bj;
#pragma unroll
      for (int i = 0; i < IMAX; ++i) {
        if (i < I) {
        T wv = W3l[(size_t)j * I + i];
#pragma unroll
        for (int k = 0; k < VEC; ++k) zk[k] += wv * xr[i][k];
              }
      }
#pragma unroll
      for (int k = 0; k < VEC; ++k) zk[k] = dfno_gelu::gelu(zk[k]);
#pragma unroll
      for (int o = 0; o < O2MAX; ++o) {
        if (o < O2) {
        T w4 = W4l[(size_t)o * M + j];
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[o][k] += w4 * zk[k];
              }
      }
    }

    TIO* ob = out + ((long)b * O2) * S + s;
#pragma unroll
    for (int o = 0; o < O2MAX; ++o) {
      if (o < O2) {
      if constexpr (VECTOR && std::is_same<T, float>::value &&
                    std::is_same<TIO, float>::value) {
        *reinterpret_cast<float4*>(
            reinterpret_cast<float*>(ob) + (long)o * S) =
            make_float4(acc[o][0], acc[o][1], acc[o][2], acc[o][3]);
      } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          if (!full && k >= nv) break;
          st(ob + (long)o * S + k, acc[o][k]);
        }
      }
          }
    }
  }
}

// Tiled MFMA forward for the flagship head (I=20, M=128, O2<=2): the
// per-thread kernel above walks all 128 hidden channels per element
// (VALU z3 + scalar-broadcast weights) and measures ~1.04 ms; here z3
// runs as v_mfma_f32_16x16x4 over a [128 x 64] LDS tile, gelu is applied
// in place, and the W4 contraction is one thin MFMA M-tile (rows 0..O2-1
// of a padded 16-row A).  TIO = unsigned short selects bf16 activations.
template <int IT, int MT, int O2T, typename TIO = float>
__global__ __launch_bounds__(kBlock, 3) void proj_head_fwd_fused_kernel(
    const TIO* __restrict__ x, const float* __restrict__ W3,
    const float* __restrict__ b3, const float* __restrict__ W4,
    const float* __restrict__ b4, TIO* __restrict__ out,
    int B, int O2, long S) {
  constexpr int TS = 64;
  constexpr int LD = TS + 4;
  extern __shared__ __align__(16) char smem_raw[];
  float* ht = reinterpret_cast<float*>(smem_raw);    // [MT][LD]
  float* xt = ht + (size_t)MT * LD;                  // [IT][LD]
  float* W3l = xt + (size_t)IT * LD;                 // [MT*IT]
  float* b3l = W3l + (size_t)MT * IT;                // [MT]
  float* W4l = b3l + MT;                             // [O2T*MT]
#pragma clang loop unroll(disable)
  for (int k = threadIdx.x; k < MT * IT; k += kBlock) W3l[k] = W3[k];
  for (int k = threadIdx.x; k < MT; k += kBlock) b3l[k] = b3[k];
  for (int k = threadIdx.x; k < O2T * MT; k += kBlock) W4l[k] = W4[k];

  const int lane = (int)(threadIdx.x & 63);
  const int wave = (int)(threadIdx.x >> 6);
  const int l16 = lane & 15;
  const int kg = lane >> 4;

  const long stiles = (S + TS - 1) / TS;
  const long tend = (long)B * stiles;
  constexpr int NPF = (IT * TS + kBlock - 1) / kBlock;
  float pf[NPF];
  auto prefetch = [&](long tt) {
    if (tt >= tend) return;
    const int b = (int)(tt / stiles);
    const long s0 = (tt % stiles) * TS;
    const int nv = (int)min((long)TS, S - s0);
#pragma unroll
    for (int q = 0; q < NPF; ++q) {
      const int r = (int)threadIdx.x + q * kBlock;
      if (r >= IT * TS) break;
      const int row = r / TS;
      const int c = r - row * TS;
      pf[q] = (c < nv) ? ld(x + ((long)b * IT + row) * S + s0 + c) : 0.f;
    }
  };
  prefetch(blockIdx.x);

  for (long t = blockIdx.x; t < tend; t += gridDim.x) {
    const int b = (int)(t / stiles);
    const long s0 = (t % stiles) * TS;
    __syncthreads();               // prior tile's phase reads done
#pragma unroll
    for (int q = 0; q < NPF; ++q) {
      const int r = (int)threadIdx.x + q * kBlock;
      if (r >= IT * TS) break;
      const int row = r / TS;
      const int c = r - row * TS;
      xt[row * LD + c] = pf[q];
    }
    prefetch(t + gridDim.x);
    __syncthreads();
    // phase 1: z3 tile = W3 @ x (8 m-tiles x 4 n-tiles, K = IT)
#pragma unroll
    for (int pp = 0; pp < 8; ++pp) {
      const int p = wave + 4 * pp;
      const int mt = p >> 2, nt = p & 3;
      const int m = mt * 16 + l16;
      const int n = nt * 16 + l16;
      f32x4_ph z4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < IT; k += 4) {
        const float a = W3l[m * IT + k + kg];
        const float bb = xt[(k + kg) * LD + n];
        z4 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bb, z4, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
        ht[(mt * 16 + kg * 4 + r) * LD + nt * 16 + l16] = z4[r];
    }
    __syncthreads();
    // phase 2: h = gelu(z3 + b3) in place (pair of threads per channel)
    {
      const int jj = (int)(threadIdx.x >> 1);
      const int half = (int)(threadIdx.x & 1) * 4;
      const float bj = b3l[jj];
#pragma unroll
      for (int k = 0; k < TS / 8; ++k) {
        const int c4 = half + k * 8;
        float4 zv = *reinterpret_cast<float4*>(ht + jj * LD + c4);
        zv.x = dfno_gelu::gelu(zv.x + bj);
        zv.y = dfno_gelu::gelu(zv.y + bj);
        zv.z = dfno_gelu::gelu(zv.z + bj);
        zv.w = dfno_gelu::gelu(zv.w + bj);
        *reinterpret_cast<float4*>(ht + jj * LD + c4) = zv;
      }
    }
    __syncthreads();
    // phase 3: out = W4 @ h + b4 — one thin MFMA tile (A rows 0..O2-1
    // hold W4, the rest zero); wave = n-tile
    {
      const int n = wave * 16 + l16;
      f32x4_ph c4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
      for (int k = 0; k < MT; k += 4) {
        float a = 0.f;
        if (l16 == 0) a = W4l[k + kg];
        else if (O2T == 2 && l16 == 1) a = W4l[MT + k + kg];
        const float bb = ht[(k + kg) * LD + n];
        c4 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bb, c4, 0, 0, 0);
      }
      const long sc = s0 + n;
      if (kg == 0 && sc < S) {
#pragma unroll
        for (int r = 0; r < O2T; ++r)
          st(out + ((long)b * O2T + r) * S + sc, c4[r] + b4[r]);
      }
    }
  }
}

// Backward: one pass producing gx, gb3, gW4, gb4 and materializing gz3
// (grad wrt z3 = pre-gelu hidden) for the grad-W3 library GEMM.
template <typename T, int IMAX, int O2MAX, int VEC, bool VECTOR,
          int MT = 0, int IT = 0>
__global__ __launch_bounds__(kBlock) void proj_head_bwd_kernel(
    const T* __restrict__ gy, const T* __restrict__ x,
    const T* __restrict__ W3, const T* __restrict__ b3,
    const T* __restrict__ W4,
    T* __restrict__ gz3,
    T* __restrict__ gb3, T* __restrict__ gW4, T* __restrict__ gb4,
    int B, int I_, int M_, int O2, long S) {
  const int I = IT > 0 ? IT : I_;     // see fwd kernel note
  const int M = MT > 0 ? MT : M_;
  extern __shared__ __align__(16) char smem_raw[];
  T* W3l = reinterpret_cast<T*>(smem_raw);   // [M*I]
  T* b3l = W3l + (size_t)M * I;              // [M]
  T* W4l = b3l + M;                          // [O2*M]
  // per-wave partial accumulators for gb3 [4][M] and gW4 [4][O2*M]
  T* gb3w = W4l + (size_t)O2 * M;            // [4*M]
  T* gW4w = gb3w + 4 * (size_t)M;            // [4*O2*M]
  for (int k = threadIdx.x; k < M * I; k += blockDim.x) W3l[k] = W3[k];
  for (int k = threadIdx.x; k < M; k += blockDim.x) b3l[k] = b3[k];
  for (int k = threadIdx.x; k < O2 * M; k += blockDim.x) W4l[k] = W4[k];
  for (int k = threadIdx.x; k < 4 * M; k += blockDim.x) gb3w[k] = T(0);
  for (int k = threadIdx.x; k < 4 * O2 * M; k += blockDim.x) gW4w[k] = T(0);
  __syncthreads();

  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x % 64;

  T gb4acc[O2MAX];
#pragma unroll
  for (int o = 0; o < O2MAX; ++o) gb4acc[o] = T(0);

  long nchunks = (S + VEC - 1) / VEC;
  long t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;

  for (long t = t0; t < (long)B * nchunks; t += stride) {
    int b = (int)(t / nchunks);
    long s = (t % nchunks) * VEC;
    bool full = (s + VEC) <= S;
    int nv = full ? VEC : (int)(S - s);

    T xr[IMAX][VEC];
    const T* xb = x + ((long)b * I) * S + s;
    T gyv[O2MAX][VEC];
    const T* gyb = gy + ((long)b * O2) * S + s;
    if constexpr (VECTOR && std::is_same<T, float>::value) {
#pragma unroll
      for (int i = 0; i < IMAX; ++i) {
        if (i < I) {
        const float4 v = *reinterpret_cast<const float4*>(xb + (long)i * S);
        xr[i][0] = v.x; xr[i][1] = v.y; xr[i][2] = v.z; xr[i][3] = v.w;
              }
      }
#pragma unroll
      for (int o = 0; o < O2MAX; ++o) {
        if (o < O2) {
        const float4 v = *reinterpret_cast<const float4*>(gyb + (long)o * S);
        gyv[o][0] = v.x; gyv[o][1] = v.y; gyv[o][2] = v.z; gyv[o][3] = v.w;
              }
      }
    } else {
#pragma unroll
      for (int i = 0; i < IMAX; ++i) {
        if (i < I) {
#pragma unroll
        for (int k = 0; k < VEC; ++k)
          xr[i][k] = (full || k < nv) ? xb[(long)i * S + k] : T(0);
              }
      }
#pragma unroll
      for (int o = 0; o < O2MAX; ++o) {
        if (o < O2) {
#pragma unroll
        for (int k = 0; k < VEC; ++k)
          gyv[o][k] = (full || k < nv) ? gyb[(long)o * S + k] : T(0);
              }
      }
    }

#pragma unroll
    for (int o = 0; o < O2MAX; ++o) {
      if (o < O2) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) gb4acc[o] += gyv[o][k];
          }
    }


    T* gz3b = gz3 + ((long)b * M) * S + s;
#pragma unroll 8
    for (int j = 0; j < (MT > 0 ? MT : 512); ++j) {
      if (MT == 0 && j >= M) break;
      // recompute z3 and gelu pieces
      T zk[VEC];
      T bj = b3l[j];
#pragma unroll
      for (int k = 0; k < VEC; ++k) zk[k] = bj;
#pragma unroll
      for (int i = 0; i < IMAX; ++i) {
        if (i < I) {
        T wv = W3l[(size_t)j * I + i];
#pragma unroll
        for (int k = 0; k < VEC; ++k) zk[k] += wv * xr[i][k];
              }
      }
      T gk[VEC], dgk[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k)
        dfno_gelu::gelu_and_grad(zk[k], gk[k], dgk[k]);
      // gz3_j = (sum_o W4[o,j] gy[o]) * gelu'(z3_j)
      T gzk[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) gzk[k] = T(0);
#pragma unroll
      for (int o = 0; o < O2MAX; ++o) {
        if (o < O2) {
        T w4 = W4l[(size_t)o * M + j];
#pragma unroll
        for (int k = 0; k < VEC; ++k) gzk[k] += w4 * gyv[o][k];
              }
      }
#pragma unroll
      for (int k = 0; k < VEC; ++k) gzk[k] *= dgk[k];

      // store gz3 (grad-x and grad-W3 are computed from it afterwards)
      if constexpr (VECTOR && std::is_same<T, float>::value) {
        *reinterpret_cast<float4*>(gz3b + (long)j * S) =
            make_float4(gzk[0], gzk[1], gzk[2], gzk[3]);
      } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          if (full || k < nv) gz3b[(long)j * S + k] = gzk[k];
        }
      }

      // wave-reduced gb3[j] and gW4[o][j] partials
      T pb = T(0);
#pragma unroll
      for (int k = 0; k < VEC; ++k) pb += (full || k < nv) ? gzk[k] : T(0);
      pb = wave_sum(pb);
      if (lane == 0) gb3w[wave * M + j] += pb;
#pragma unroll
      for (int o = 0; o < O2MAX; ++o) {
        if (o < O2) {
        T pw = T(0);
#pragma unroll
        for (int k = 0; k < VEC; ++k) pw += (full || k < nv) ? gyv[o][k] * gk[k] : T(0);
        pw = wave_sum(pw);
        if (lane == 0) gW4w[(wave * O2 + o) * M + j] += pw;
              }
      }
    }

  }

  // block-level flush: per-wave partials -> global atomics
#pragma unroll
  for (int o = 0; o < O2MAX; ++o) {
    if (o < O2) {
    T v = wave_sum(gb4acc[o]);
    if (lane == 0 && v != T(0)) atomicAdd(&gb4[o], v);
      }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < M; k += blockDim.x) {
    T v = gb3w[k] + gb3w[M + k] + gb3w[2 * M + k] + gb3w[3 * M + k];
    if (v != T(0)) atomicAdd(&gb3[k], v);
  }
  for (int k = threadIdx.x; k < O2 * M; k += blockDim.x) {
    T v = gW4w[k] + gW4w[O2 * M + k] + gW4w[2 * O2 * M + k] + gW4w[3 * O2 * M + k];
    if (v != T(0)) atomicAdd(&gW4[k], v);
  }
}

// ---------------------------------------------------------------------------
// Fully-fused flagship backward (I=20, M=128, O2<=2, fp32): one kernel
// produces gx, gW3, gb3, gW4, gb4 with the [M, S] hidden-grad living only
// as a [M x 64] LDS tile — the 4 GB gz3 intermediate of the three-kernel
// chain (proj_head_bwd 1.67 ms + channel_mix_fwd_t 1.22 ms + gw_mfma
// 1.85 ms, kernel_stats_r02_final.csv) is never written to HBM.  Traffic
// drops from ~13 GB to read x + gy, write gx (~1.3 GB).  grad-W3 runs as
// v_mfma_f32_16x16x4 on the LDS tile with per-wave fragment accumulators
// carried across tiles (identical numerics to the library chain up to
// fp32 atomic reduction order, like every gw kernel here).
// ---------------------------------------------------------------------------

template <int IT, int MT, int O2T, typename TIO = float>
__global__ __launch_bounds__(kBlock, 3) void proj_head_bwd_fused_kernel(
    const TIO* __restrict__ gy, const TIO* __restrict__ x,
    const float* __restrict__ W3, const float* __restrict__ b3,
    const float* __restrict__ W4,
    TIO* __restrict__ gx, float* __restrict__ gW3,
    float* __restrict__ gb3, float* __restrict__ gW4,
    float* __restrict__ gb4, int B, int O2, long S) {
  constexpr int TS = 64;           // s-columns per tile (16 MFMA K-steps)
  constexpr int LD = TS + 4;       // row pad (float4-aligned, 4-bank skew)
  // gz tile + staged x tile + weights in LDS (52 KB -> 3 blocks/CU; an
  // x/W3-from-global variant at 4 blocks/CU measured 2x slower: the cold
  // per-lane B-operand loads serialize inside the MFMA chains)
  extern __shared__ __align__(16) char smem_raw[];
  float* gzt = reinterpret_cast<float*>(smem_raw);   // [MT][LD]
  float* xt = gzt + (size_t)MT * LD;                 // [IT][LD]
  float* gyt = xt + (size_t)IT * LD;                 // [O2T][TS]
  float* W3l = gyt + O2T * TS;                       // [MT*IT]
  float* b3l = W3l + (size_t)MT * IT;                // [MT]
  float* W4l = b3l + MT;                             // [O2T*MT]
  float* gb3s = W4l + O2T * MT;                      // [MT]
  float* gW4s = gb3s + MT;                           // [O2T*MT]
#pragma clang loop unroll(disable)
  for (int k = threadIdx.x; k < MT * IT; k += kBlock) W3l[k] = W3[k];
  for (int k = threadIdx.x; k < MT; k += kBlock) {
    b3l[k] = b3[k];
    gb3s[k] = 0.f;
  }
  for (int k = threadIdx.x; k < O2T * MT; k += kBlock) {
    W4l[k] = W4[k];
    gW4s[k] = 0.f;
  }

  const int lane = (int)(threadIdx.x & 63);
  const int wave = (int)(threadIdx.x >> 6);
  const int l16 = lane & 15;
  const int kg = lane >> 4;

  f32x4_ph wacc[4];                // gW3 frags: 8 mt-tiles x 2 nt-tiles
#pragma unroll
  for (int p = 0; p < 4; ++p) wacc[p] = f32x4_ph{0.f, 0.f, 0.f, 0.f};
  float gb4a0 = 0.f, gb4a1 = 0.f;

  const long stiles = (S + TS - 1) / TS;
  const long tend = (long)B * stiles;
  // software-pipelined staging: tile t+grid's x/gy columns load into
  // registers while tile t computes
  constexpr int NPF = ((IT + 2) * TS + kBlock - 1) / kBlock;
  float pf[NPF];
  auto prefetch = [&](long tt) {
    if (tt >= tend) return;
    const int b = (int)(tt / stiles);
    const long s0 = (tt % stiles) * TS;
    const int nv = (int)min((long)TS, S - s0);
#pragma unroll
    for (int q = 0; q < NPF; ++q) {
      const int r = (int)threadIdx.x + q * kBlock;
      if (r >= (IT + O2T) * TS) break;
      const int row = r / TS;
      const int c = r - row * TS;
      float v = 0.f;
      if (c < nv) {
        v = (row < IT) ? ld(x + ((long)b * IT + row) * S + s0 + c)
                       : ld(gy + ((long)b * O2T + (row - IT)) * S + s0 + c);
      }
      pf[q] = v;
    }
  };
  prefetch(blockIdx.x);
  for (long t = blockIdx.x; t < tend; t += gridDim.x) {
    const int b = (int)(t / stiles);
    const long s0 = (t % stiles) * TS;
    const int nv = (int)min((long)TS, S - s0);
    __syncthreads();               // prior tile's phase reads done
#pragma unroll
    for (int q = 0; q < NPF; ++q) {
      const int r = (int)threadIdx.x + q * kBlock;
      if (r >= (IT + O2T) * TS) break;
      const int row = r / TS;
      const int c = r - row * TS;
      const float v = pf[q];
      if (row < IT) {
        xt[row * LD + c] = v;
      } else {
        gyt[(row - IT) * TS + c] = v;
        if (row == IT) gb4a0 += v; else gb4a1 += v;
      }
    }
    prefetch(t + gridDim.x);
    __syncthreads();               // xt/gyt staged
    // phase 1a: z3 tile = W3 @ x via MFMA (bias-free, into gzt).
    // 8 m-tiles x 4 n-tiles over K = IT = 20; 8 pairs per wave.
#pragma unroll
    for (int pp = 0; pp < 8; ++pp) {
      const int p = wave + 4 * pp;
      const int mt = p >> 2, nt = p & 3;
      const int m = mt * 16 + l16;
      const int n = nt * 16 + l16;
      f32x4_ph z4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < IT; k += 4) {
        const float a = W3l[m * IT + k + kg];
        const float bb = xt[(k + kg) * LD + n];
        z4 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bb, z4, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
        gzt[(mt * 16 + kg * 4 + r) * LD + nt * 16 + l16] = z4[r];
    }
    __syncthreads();
    // phase 1b: gz = (W4^T gy) * gelu'(z3 + b3) in place over the tile.
    // Each PAIR of threads owns one hidden channel j, so the gb3/gW4
    // partials accumulate in registers with one shfl_xor(1) per tile.
    {
      const int jj = (int)(threadIdx.x >> 1);        // 0..127
      const int half = (int)(threadIdx.x & 1) * 4;   // 0 or 4
      const float bj = b3l[jj];
      const float w40 = W4l[jj];
      const float w41 = (O2T == 2) ? W4l[MT + jj] : 0.f;
      float pb = 0.f, pw0 = 0.f, pw1 = 0.f;
#pragma unroll
      for (int k = 0; k < TS / 8; ++k) {
        const int c4 = half + k * 8;
        float4 zv = *reinterpret_cast<float4*>(gzt + jj * LD + c4);
        float z[4] = {zv.x + bj, zv.y + bj, zv.z + bj, zv.w + bj};
        float g[4], dg[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
          dfno_gelu::gelu_and_grad(z[q], g[q], dg[q]);
        const float4 gy4 = *reinterpret_cast<const float4*>(gyt + c4);
        float gz[4] = {w40 * gy4.x, w40 * gy4.y, w40 * gy4.z, w40 * gy4.w};
        pw0 += gy4.x * g[0] + gy4.y * g[1] + gy4.z * g[2] + gy4.w * g[3];
        if (O2T == 2) {
          const float4 gy4b =
              *reinterpret_cast<const float4*>(gyt + TS + c4);
          gz[0] += w41 * gy4b.x; gz[1] += w41 * gy4b.y;
          gz[2] += w41 * gy4b.z; gz[3] += w41 * gy4b.w;
          pw1 += gy4b.x * g[0] + gy4b.y * g[1] + gy4b.z * g[2] +
                 gy4b.w * g[3];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) gz[q] *= dg[q];
        *reinterpret_cast<float4*>(gzt + jj * LD + c4) =
            make_float4(gz[0], gz[1], gz[2], gz[3]);
        pb += gz[0] + gz[1] + gz[2] + gz[3];
      }
      pb += __shfl_xor(pb, 1, 64);
      pw0 += __shfl_xor(pw0, 1, 64);
      if (O2T == 2) pw1 += __shfl_xor(pw1, 1, 64);
      if ((lane & 1) == 0) {
        atomicAdd(&gb3s[jj], pb);
        atomicAdd(&gW4s[jj], pw0);
        if (O2T == 2) atomicAdd(&gW4s[MT + jj], pw1);
      }
    }
    __syncthreads();
    // phase 2a: gx tile = W3^T @ gz via MFMA.  A[m=i][k=j] = W3[k*IT+m]
    // (per-lane global), B[n=c][k=j] = gzt[k*LD+n]; K = MT.
#pragma unroll
    for (int pp = 0; pp < 2; ++pp) {
      const int p = wave + 4 * pp;
      const int mt = p >> 2, nt = p & 3;
      const int m = mt * 16 + l16;
      const int n = nt * 16 + l16;
      const bool av = m < IT;
      f32x4_ph c4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
      for (int k = 0; k < MT; k += 4) {
        const float a = av ? W3l[(k + kg) * IT + m] : 0.f;
        const float bb = gzt[(k + kg) * LD + n];
        c4 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bb, c4, 0, 0, 0);
      }
      const long sc = s0 + nt * 16 + l16;
      if (sc < S) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = mt * 16 + kg * 4 + r;
          if (i < IT) st(gx + ((long)b * IT + i) * S + sc, c4[r]);
        }
      }
    }
    // phase 2b: gW3 fragments += gz_tile @ x_tile^T (reads only; the
    // tile loop's top sync fences the next staging pass)
#pragma unroll
    for (int pp = 0; pp < 4; ++pp) {
      const int p = wave + 4 * pp;
      const int mt = p >> 1, nt = p & 1;
      const float* gr = gzt + (mt * 16 + l16) * LD;
      const float* xr = xt + (nt * 16 + l16) * LD;
      const bool bv = (nt * 16 + l16) < IT;
#pragma unroll 8
      for (int k = 0; k < TS; k += 4) {
        const float a = gr[k + kg];
        const float bb = bv ? xr[k + kg] : 0.f;
        wacc[pp] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bb, wacc[pp],
                                                        0, 0, 0);
      }
    }
  }

  // flush: gW3 fragments, gb4 wave sums, gb3/gW4 LDS partials
#pragma unroll
  for (int pp = 0; pp < 4; ++pp) {
    const int p = wave + 4 * pp;
    const int mt = p >> 1, nt = p & 1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = mt * 16 + kg * 4 + r;
      const int i = nt * 16 + l16;
      if (i < IT && wacc[pp][r] != 0.f)
        atomicAdd(&gW3[(size_t)j * IT + i], wacc[pp][r]);
    }
  }
  float v0 = wave_sum(gb4a0);
  if (lane == 0 && v0 != 0.f) atomicAdd(&gb4[0], v0);
  if (O2T == 2) {
    float v1 = wave_sum(gb4a1);
    if (lane == 0 && v1 != 0.f) atomicAdd(&gb4[1], v1);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < MT; k += kBlock)
    if (gb3s[k] != 0.f) atomicAdd(&gb3[k], gb3s[k]);
  for (int k = threadIdx.x; k < O2T * MT; k += kBlock)
    if (gW4s[k] != 0.f) atomicAdd(&gW4[k], gW4s[k]);
}

template <typename T>
bool vec_ok(long S, std::initializer_list<const void*> ptrs) {
  if (!std::is_same<T, float>::value) return false;
  if (S % 4 != 0) return false;
  for (auto p : ptrs)
    if ((reinterpret_cast<uintptr_t>(p) & 15) != 0) return false;
  return true;
}

}  // namespace

at::Tensor proj_head_fwd(const at::Tensor& x, const at::Tensor& W3,
                         const at::Tensor& b3, const at::Tensor& W4,
                         const at::Tensor& b4) {
  const bool bf16 = x.scalar_type() == at::kBFloat16;
  if (!bf16) { check_real(x, "x"); }
  TORCH_CHECK(x.is_cuda() && x.is_contiguous(), "x must be contiguous GPU");
  TORCH_CHECK(x.dim() == 3, "x must be [B,I,S]");
  int B = (int)x.size(0), I = (int)x.size(1);
  long S = x.size(2);
  int M = (int)W3.size(0), O2 = (int)W4.size(0);
  TORCH_CHECK((int)W3.size(1) == I && (int)W4.size(1) == M, "proj_head shapes");
  TORCH_CHECK(I <= 32 && O2 <= 8 && M <= 512, "proj_head: unsupported dims");

  auto out = at::empty({B, O2, S}, x.options());
  if (x.numel() == 0) return out;
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  int grid = launch_grid((long)B * ((S + 3) / 4), kBlock, 256L * 8);
  // The tiled-MFMA forward below is correct but measured SLOWER than the
  // register-resident per-thread kernel (1.48 vs 1.06 ms within-process
  // A/B at the flagship): the z3 tile costs 4 LDS passes + 3 barriers
  // that the per-thread scheme (weights via s_loads, z/h/out all in
  // registers) never pays; the per-thread bf16-IO variant likewise wins
  // for bf16 (1.15 vs ~1.6 ms).  Kept as an opt-in (DFNO_PF_FUSED=1)
  // for shapes where the VALU z3 walk dominates.
  static const bool want_fused_fwd = []() {
    const char* e = getenv("DFNO_PF_FUSED");   // A/B knob
    return e && e[0] == '1';
  }();
  if (want_fused_fwd && I == 20 && M == 128 && O2 <= 2 &&
      (bf16 || x.scalar_type() == at::kFloat)) {
    // flagship: tiled MFMA forward (z3 as 16x16x4 fragments over a
    // [128 x 64] LDS tile instead of per-thread hidden-channel walks)
    auto W3f = bf16 ? W3.to(at::kFloat).contiguous() : W3.contiguous();
    auto b3f = bf16 ? b3.to(at::kFloat).contiguous() : b3.contiguous();
    auto W4f = bf16 ? W4.to(at::kFloat).contiguous() : W4.contiguous();
    auto b4f = bf16 ? b4.to(at::kFloat).contiguous() : b4.contiguous();
    constexpr int TS = 64, LD = TS + 4;
    size_t smem = sizeof(float) *
        ((size_t)128 * LD + 20 * LD + (size_t)128 * 20 + 128 +
         2 * (size_t)128);
    long stiles = (S + TS - 1) / TS;
    int grid2 = (int)std::min((long)B * stiles, 768L);
#define PH_FWD_F(O2T, TIO)                                                    \
    hipLaunchKernelGGL((proj_head_fwd_fused_kernel<20, 128, O2T, TIO>),       \
                       dim3(grid2), dim3(kBlock), smem, stream,               \
                       reinterpret_cast<const TIO*>(x.data_ptr()),            \
                       W3f.data_ptr<float>(), b3f.data_ptr<float>(),          \
                       W4f.data_ptr<float>(), b4f.data_ptr<float>(),          \
                       reinterpret_cast<TIO*>(out.data_ptr()), B, O2, S);
    if (bf16) {
      if (O2 == 2) { PH_FWD_F(2, unsigned short) }
      else { PH_FWD_F(1, unsigned short) }
    } else {
      if (O2 == 2) { PH_FWD_F(2, float) } else { PH_FWD_F(1, float) }
    }
#undef PH_FWD_F
    DFNO_CHECK_LAUNCH("proj_head");
    return out;
  }
  if (bf16) {
    // bf16 activations, fp32 weights/math (host-casts the tiny weights)
    auto W3f = W3.to(at::kFloat).contiguous();
    auto b3f = b3.to(at::kFloat).contiguous();
    auto W4f = W4.to(at::kFloat).contiguous();
    auto b4f = b4.to(at::kFloat).contiguous();
    auto inp = reinterpret_cast<const unsigned short*>(x.data_ptr());
    auto op = reinterpret_cast<unsigned short*>(out.data_ptr());
#define PH_LAUNCH_BF(IM, OM, MTV, ITV)                                        \
    hipLaunchKernelGGL((proj_head_fwd_kernel<float, IM, OM, 4, false, MTV,    \
                                             ITV, unsigned short>),           \
                       dim3(grid), dim3(kBlock), 0, stream, inp,              \
                       W3f.data_ptr<float>(), b3f.data_ptr<float>(),          \
                       W4f.data_ptr<float>(), b4f.data_ptr<float>(), op,      \
                       B, I, M, O2, S);
    if (I == 20 && M == 128 && O2 <= 2) { PH_LAUNCH_BF(24, 2, 128, 20) }
    else if (I <= 24 && O2 <= 2) { PH_LAUNCH_BF(24, 2, 0, 0) }
    else { PH_LAUNCH_BF(32, 8, 0, 0) }
#undef PH_LAUNCH_BF
    DFNO_CHECK_LAUNCH("proj_head");
    return out;
  }
  check_real(W3, "W3"); check_real(b3, "b3");
  check_real(W4, "W4"); check_real(b4, "b4");

#define PH_LAUNCH_FT(V)                                                       \
    hipLaunchKernelGGL((proj_head_fwd_kernel<scalar_t, IM, OM, 4, V, 128, 20>), \
                       dim3(grid), dim3(kBlock), smem, stream,                \
                       x.data_ptr<scalar_t>(), W3.data_ptr<scalar_t>(),       \
                       b3.data_ptr<scalar_t>(), W4.data_ptr<scalar_t>(),      \
                       b4.data_ptr<scalar_t>(), out.data_ptr<scalar_t>(),     \
                       B, I, M, O2, S);
#define PH_LAUNCH_F(V)                                                        \
    hipLaunchKernelGGL((proj_head_fwd_kernel<scalar_t, IM, OM, 4, V>),        \
                       dim3(grid), dim3(kBlock), smem, stream,                \
                       x.data_ptr<scalar_t>(), W3.data_ptr<scalar_t>(),       \
                       b3.data_ptr<scalar_t>(), W4.data_ptr<scalar_t>(),      \
                       b4.data_ptr<scalar_t>(), out.data_ptr<scalar_t>(),     \
                       B, I, M, O2, S);
  AT_DISPATCH_FLOATING_TYPES(x.scalar_type(), "proj_head_fwd", [&] {
    size_t smem = 0;
    bool vec = vec_ok<scalar_t>(S, {x.data_ptr(), out.data_ptr()});
    if (I == 20 && M == 128 && O2 <= 2) {
      constexpr int IM = 24, OM = 2;   // flagship: fold M/I at compile time
      if (vec) { PH_LAUNCH_FT(true) } else { PH_LAUNCH_FT(false) }
    } else if (I <= 24 && O2 <= 2) {
      constexpr int IM = 24, OM = 2;
      if (vec) { PH_LAUNCH_F(true) } else { PH_LAUNCH_F(false) }
    } else {
      constexpr int IM = 32, OM = 8;
      if (vec) { PH_LAUNCH_F(true) } else { PH_LAUNCH_F(false) }
    }
  });
  DFNO_CHECK_LAUNCH("proj_head");
#undef PH_LAUNCH_F
  return out;
}

std::vector<at::Tensor> proj_head_bwd(const at::Tensor& gy, const at::Tensor& x,
                                      const at::Tensor& W3, const at::Tensor& b3,
                                      const at::Tensor& W4) {
  check_real(gy, "gy"); check_real(x, "x"); check_real(W3, "W3");
  check_real(b3, "b3"); check_real(W4, "W4");
  int B = (int)x.size(0), I = (int)x.size(1);
  long S = x.size(2);
  int M = (int)W3.size(0), O2 = (int)W4.size(0);
  TORCH_CHECK(I <= 32 && O2 <= 8 && M <= 512, "proj_head: unsupported dims");

  auto gz3 = at::empty({B, M, S}, x.options());
  auto gb3 = at::zeros({M}, x.options());
  auto gW4 = at::zeros({O2, M}, x.options());
  auto gb4 = at::zeros({O2}, x.options());
  if (x.numel() == 0) return {gz3, gb3, gW4, gb4};

  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  int grid = launch_grid((long)B * ((S + 3) / 4), kBlock, 256L * 8);

#define PH_LAUNCH_BT(V)                                                       \
    hipLaunchKernelGGL((proj_head_bwd_kernel<scalar_t, IM, OM, 4, V, 128, 20>), \
                       dim3(grid), dim3(kBlock), smem, stream,                \
                       gy.data_ptr<scalar_t>(), x.data_ptr<scalar_t>(),       \
                       W3.data_ptr<scalar_t>(), b3.data_ptr<scalar_t>(),      \
                       W4.data_ptr<scalar_t>(), gz3.data_ptr<scalar_t>(),     \
                       gb3.data_ptr<scalar_t>(),                              \
                       gW4.data_ptr<scalar_t>(), gb4.data_ptr<scalar_t>(),    \
                       B, I, M, O2, S);
#define PH_LAUNCH_B(V)                                                        \
    hipLaunchKernelGGL((proj_head_bwd_kernel<scalar_t, IM, OM, 4, V>),        \
                       dim3(grid), dim3(kBlock), smem, stream,                \
                       gy.data_ptr<scalar_t>(), x.data_ptr<scalar_t>(),       \
                       W3.data_ptr<scalar_t>(), b3.data_ptr<scalar_t>(),      \
                       W4.data_ptr<scalar_t>(), gz3.data_ptr<scalar_t>(),     \
                       gb3.data_ptr<scalar_t>(),                              \
                       gW4.data_ptr<scalar_t>(), gb4.data_ptr<scalar_t>(),    \
                       B, I, M, O2, S);
  AT_DISPATCH_FLOATING_TYPES(x.scalar_type(), "proj_head_bwd", [&] {
    size_t smem = sizeof(scalar_t) *
        ((size_t)M * I + M + (size_t)O2 * M + 4 * (size_t)M + 4 * (size_t)O2 * M);
    TORCH_CHECK(smem <= 160 * 1024, "proj_head_bwd: LDS overflow");
    bool vec = vec_ok<scalar_t>(S, {x.data_ptr(), gy.data_ptr(), gz3.data_ptr()});
    if (I == 20 && M == 128 && O2 <= 2) {
      constexpr int IM = 24, OM = 2;   // flagship fold
      if (vec) { PH_LAUNCH_BT(true) } else { PH_LAUNCH_BT(false) }
    } else if (I <= 24 && O2 <= 2) {
      constexpr int IM = 24, OM = 2;
      if (vec) { PH_LAUNCH_B(true) } else { PH_LAUNCH_B(false) }
    } else {
      constexpr int IM = 32, OM = 8;
      if (vec) { PH_LAUNCH_B(true) } else { PH_LAUNCH_B(false) }
    }
  });
  DFNO_CHECK_LAUNCH("proj_head");
#undef PH_LAUNCH_B
  return {gz3, gb3, gW4, gb4};
}

std::vector<at::Tensor> proj_head_bwd_fused(const at::Tensor& gy,
                                            const at::Tensor& x,
                                            const at::Tensor& W3,
                                            const at::Tensor& b3,
                                            const at::Tensor& W4) {
  const bool bf16 = x.scalar_type() == at::kBFloat16;
  TORCH_CHECK(gy.is_cuda() && gy.is_contiguous() && x.is_contiguous() &&
              gy.scalar_type() == x.scalar_type(), "proj_head_bwd_fused IO");
  int B = (int)x.size(0), I = (int)x.size(1);
  long S = x.size(2);
  int M = (int)W3.size(0), O2 = (int)W4.size(0);
  TORCH_CHECK(I == 20 && M == 128 && O2 <= 2 &&
              (bf16 || x.scalar_type() == at::kFloat),
              "proj_head_bwd_fused: flagship shape only");

  auto W3f = bf16 ? W3.to(at::kFloat).contiguous() : W3;
  auto b3f = bf16 ? b3.to(at::kFloat).contiguous() : b3;
  auto W4f = bf16 ? W4.to(at::kFloat).contiguous() : W4;
  check_real(W3f, "W3"); check_real(b3f, "b3"); check_real(W4f, "W4");
  auto fopt = x.options().dtype(at::kFloat);   // weight grads accumulate fp32
  auto gx = at::empty({B, I, S}, x.options());
  auto gW3 = at::zeros({M, I}, fopt);
  auto gb3 = at::zeros({M}, fopt);
  auto gW4 = at::zeros({O2, M}, fopt);
  auto gb4 = at::zeros({O2}, fopt);
  if (x.numel() == 0) return {gx, gW3, gb3, gW4, gb4};

  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  constexpr int TS = 64, LD = TS + 4;
  // gzt + xt + gyt + W3l + b3l + W4l + gb3s + gW4s (kernel layout order)
  size_t smem = sizeof(float) *
      ((size_t)128 * LD + 20 * LD + (size_t)O2 * TS + (size_t)128 * 20 +
       128 + 2 * (size_t)O2 * 128 + 128);
  long stiles = (S + TS - 1) / TS;
  int grid = (int)std::min((long)B * stiles, 768L);
#define PH_FUSED(O2T, TIO)                                                   \
  hipLaunchKernelGGL((proj_head_bwd_fused_kernel<20, 128, O2T, TIO>),        \
                     dim3(grid), dim3(kBlock), smem, stream,                 \
                     reinterpret_cast<const TIO*>(gy.data_ptr()),            \
                     reinterpret_cast<const TIO*>(x.data_ptr()),             \
                     W3f.data_ptr<float>(), b3f.data_ptr<float>(),           \
                     W4f.data_ptr<float>(),                                  \
                     reinterpret_cast<TIO*>(gx.data_ptr()),                  \
                     gW3.data_ptr<float>(), gb3.data_ptr<float>(),           \
                     gW4.data_ptr<float>(), gb4.data_ptr<float>(),           \
                     B, O2, S)
  if (bf16) {
    if (O2 == 2) PH_FUSED(2, unsigned short); else PH_FUSED(1, unsigned short);
  } else {
    if (O2 == 2) PH_FUSED(2, float); else PH_FUSED(1, float);
  }
#undef PH_FUSED
  DFNO_CHECK_LAUNCH("proj_head_bwd_fused");
  return {gx, gW3, gb3, gW4, gb4};
}
