// gfx950 fused FNO lift head: y = gelu(W2 @ gelu(W1 @t x + b1) + b2).
//
// The reference runs this as a time-lift einsum (T_in -> T_out along the
// trailing dim), a GELU pass, a channel-lift einsum (C_in -> width) and
// another GELU (/root/reference/dfno/dfno.py:310-311,333-338).  rocBLAS
// handles the T_in = 1 time lift (an outer product, M ~ 5e5, K = 1)
// pathologically (~1.25 ms for a 250 MB write), and the unfused chain
// costs ~4 ms/step at the flagship config.  Here the whole lift is one
// pass: read the (tiny) input column, produce the [width, T_out] output
// column per grid point.  The first set of kernels is for T_in == 1,
// T_out <= 32 (the two-phase flagship); the "general lift" kernels further
// down take 1 <= T_in <= 16, T_out <= 64 (the Navier-Stokes config).
// Shapes outside both use the unfused path in the model.
//
// fp32/bf16 forward+backward run the lane-per-k variants: each 64-lane
// wave covers TWO s-points with one time column per lane, so every out
// write / gy read is a contiguous Tn-dword run; backward's gW2/gb2
// reduce as v_mfma_f32_16x16x4 over per-wave LDS tiles (ones-column
// trick for gb2) with fragments carried across pairs, and gW1/gb1
// accumulate per-lane (k is fixed).  fp64 (the gradient-check path) runs
// the chunked general-lift kernels for every T_in, 1 included.

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

// fp32 lane-per-k variants: each 64-lane wave covers TWO s-points with
// lanes 0..Tn-1 / 32..32+Tn-1 owning one time column each, so every gy
// read and out write is a contiguous Tn-dword run (a one-point-per-thread
// layout streams 30-float runs per lane -> fully scattered wave accesses;
// measured 699/843 us vs ~110/130 us of traffic).  Per-lane state is
// ~40 VGPRs; gW1/gb1 partials accumulate in registers (k fixed per lane).
template <int WT, typename TIO = float>
__global__ __launch_bounds__(kBlock) void lift_head_fwd_lk_kernel(
    const TIO* __restrict__ x, const float* __restrict__ W1,
    const float* __restrict__ b1, const float* __restrict__ W2,
    const float* __restrict__ b2, TIO* __restrict__ out,
    int B, int C, int W, int Tn, long S) {
  constexpr int CC = 4;
  __shared__ float w1[32], bb1[32], w2[24 * CC], bb2[24];
  for (int k = threadIdx.x; k < Tn; k += kBlock) { w1[k] = W1[k]; bb1[k] = b1[k]; }
  for (int k = threadIdx.x; k < W * C; k += kBlock) w2[k] = W2[k];
  for (int k = threadIdx.x; k < W; k += kBlock) bb2[k] = b2[k];
  __syncthreads();

  const int lane = (int)(threadIdx.x & 63);
  const int half = lane >> 5;                 // 0 or 1: which s of the pair
  const int k = lane & 31;
  const bool kv = k < Tn;
  const long npair = ((long)B * S + 1) / 2;
  long t0 = (long)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  long stride = (long)gridDim.x * (blockDim.x / 64);
  for (long t = t0; t < npair; t += stride) {
    const long e = 2 * t + half;              // element index
    const bool ev = e < (long)B * S;
    const long b = e / S;
    const long s = e - b * S;

    float h[CC];
#pragma unroll
    for (int c = 0; c < CC; ++c) {
      if (c < C) {
        const float xv = ev ? ld(x + (b * C + c) * S + s) : 0.f;
        h[c] = kv ? dfno_gelu::gelu(w1[k] * xv + bb1[k]) : 0.f;
      }
    }
#pragma unroll 4
    for (int w = 0; w < (WT > 0 ? WT : 512); ++w) {
      if (WT == 0 && w >= W) break;
      float acc = bb2[w];
#pragma unroll
      for (int c = 0; c < CC; ++c)
        if (c < C) acc += w2[w * C + c] * h[c];
      if (ev && kv)
        st(out + ((b * W + w) * S + s) * Tn + k, dfno_gelu::gelu(acc));
    }
  }
}

typedef float f32x4_lh __attribute__((ext_vector_type(4)));

template <int WT, typename TIO = float>
__global__ __launch_bounds__(kBlock) void lift_head_bwd_lk_kernel(
    const TIO* __restrict__ gy, const TIO* __restrict__ x,
    const float* __restrict__ W1, const float* __restrict__ b1,
    const float* __restrict__ W2, const float* __restrict__ b2,
    TIO* __restrict__ gx, float* __restrict__ gW1, float* __restrict__ gb1,
    float* __restrict__ gW2, float* __restrict__ gb2,
    int B, int C, int W, int Tn, long S) {
  constexpr int CC = 4;
  constexpr int GLD = 68;                     // gz/h tile row pad (banks)
  __shared__ float w1[32], bb1[32], w2[24 * CC], bb2[24];
  // per-wave tiles: gz [24 w][64 lanes] and h [4 c][64 lanes]; the gW2 and
  // gb2 reductions run as v_mfma_f32_16x16x4 over these (B-operand column
  // 4 is a constant ones column giving gb2) with the C fragments carried
  // in registers across pairs — the per-pair 6-shuffle wave_sum chains of
  // the first cut were the whole kernel's latency.
  __shared__ float gzt[4][24 * GLD];
  __shared__ float ht[4][CC * GLD];
  for (int k = threadIdx.x; k < Tn; k += kBlock) { w1[k] = W1[k]; bb1[k] = b1[k]; }
  for (int k = threadIdx.x; k < W * C; k += kBlock) w2[k] = W2[k];
  for (int k = threadIdx.x; k < W; k += kBlock) bb2[k] = b2[k];
  __syncthreads();

  const int wave = (int)(threadIdx.x >> 6);
  const int lane = (int)(threadIdx.x & 63);
  const int half = lane >> 5;
  const int k = lane & 31;
  const bool kv = k < Tn;
  const int l16 = lane & 15;
  const int kg = lane >> 4;
  float pgW1 = 0.f, pgb1 = 0.f;               // per-lane: k is fixed
  f32x4_lh wacc[2];                           // gW2/gb2 frags (2 m-tiles)
  wacc[0] = f32x4_lh{0.f, 0.f, 0.f, 0.f};
  wacc[1] = f32x4_lh{0.f, 0.f, 0.f, 0.f};
  float* gzw = &gzt[wave][0];
  float* hw = &ht[wave][0];

  const long npair = ((long)B * S + 1) / 2;
  long t0 = (long)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  long stride = (long)gridDim.x * (blockDim.x / 64);
  for (long t = t0; t < npair; t += stride) {
    const long e = 2 * t + half;
    const bool ev = e < (long)B * S;
    const long b = e / S;
    const long s = e - b * S;

    float xv[CC], h[CC], gh[CC];
#pragma unroll
    for (int c = 0; c < CC; ++c) {
      if (c < C) {
        xv[c] = ev ? ld(x + (b * C + c) * S + s) : 0.f;
        h[c] = kv ? dfno_gelu::gelu(w1[k] * xv[c] + bb1[k]) : 0.f;
        gh[c] = 0.f;
        hw[c * GLD + lane] = h[c];
      }
    }
    // all W gy columns preloaded back-to-back: one memory round trip per
    // pair instead of one per unroll batch (the loads were the kernel's
    // whole latency — all reduction variants measured the same ~900 us)
    float gyv[WT > 0 ? WT : 24];
#pragma unroll
    for (int w = 0; w < (WT > 0 ? WT : 24); ++w) {
      gyv[w] = (w < W && ev && kv)
                   ? ld(gy + ((b * W + w) * S + s) * Tn + k) : 0.f;
    }
#pragma unroll 4
    for (int w = 0; w < (WT > 0 ? WT : 512); ++w) {
      if (WT == 0 && w >= W) break;
      float z2 = bb2[w];
#pragma unroll
      for (int c = 0; c < CC; ++c)
        if (c < C) z2 += w2[w * C + c] * h[c];
      const float gz2 = gyv[w] * dfno_gelu::gelu_grad(z2);
      gzw[w * GLD + lane] = gz2;
#pragma unroll
      for (int c = 0; c < CC; ++c)
        if (c < C) gh[c] += w2[w * C + c] * gz2;
    }
    // gW2/gb2 fragment update from this pair's tiles (wave-synchronous:
    // same wave wrote gzt/ht just above)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const int wrow = mt * 16 + l16;
      const bool av = wrow < W;
#pragma unroll 4
      for (int k0 = 0; k0 < 64; k0 += 4) {
        const float a = av ? gzw[wrow * GLD + k0 + kg] : 0.f;
        const float bb = (l16 < C) ? hw[l16 * GLD + k0 + kg]
                                   : (l16 == C ? 1.f : 0.f);
        wacc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bb, wacc[mt],
                                                        0, 0, 0);
      }
    }
    // gz1 = gh * gelu'(z1); per-lane gW1/gb1 partials; gx via 32-lane
    // segmented reduce (k lanes of each s-half)
#pragma unroll
    for (int c = 0; c < CC; ++c) {
      if (c < C) {
        const float gz1 = kv ? gh[c] * dfno_gelu::gelu_grad(w1[k] * xv[c] + bb1[k]) : 0.f;
        pgW1 += gz1 * xv[c];
        pgb1 += gz1;
        float gxa = kv ? w1[k] * gz1 : 0.f;
#pragma unroll
        for (int off = 16; off > 0; off >>= 1)
          gxa += __shfl_xor(gxa, off, 64);
        if (ev && k == 0) st(gx + (b * C + c) * S + s, gxa);
      }
    }
  }

  // flush: pair the two s-halves for gW1/gb1, then one atomic per (wave, k);
  // gW2/gb2 from the MFMA fragments (D[m=w][n]: n<C -> gW2, n==C -> gb2)
  pgW1 += __shfl_xor(pgW1, 32, 64);
  pgb1 += __shfl_xor(pgb1, 32, 64);
  if (half == 0 && kv) {
    atomicAdd(&gW1[k], pgW1);
    atomicAdd(&gb1[k], pgb1);
  }
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int w = mt * 16 + kg * 4 + r;
      const float v = wacc[mt][r];
      if (w < W && v != 0.f) {
        if (l16 < C) atomicAdd(&gW2[w * C + l16], v);
        else if (l16 == C) atomicAdd(&gb2[w], v);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// General lift (T_in >= 1): x [B, C, S, Ti] -> out [B, W, S, To] with
//   h[c][k] = gelu(sum_i W1[k,i] x[c][i] + b1[k]),  y[w][k] = gelu(W2 h + b2).
// Same lane-per-k layout as the T_in == 1 kernels above: a wave covers
// PW = 64/LP grid points (LP = 32 lanes per point when To <= 32, else 64),
// lane k of a point owns time column k, so out writes / gy reads stay
// contiguous To-element runs.  The wave's x columns (PW points x C x Ti) go
// through a small per-wave LDS tile: loaded coalesced (prefetched one
// iteration ahead), then read back with same-address (broadcast) reads for
// the z1 dot product against the lane's W1[k, :] row held in registers.
// Rows are zero-padded to the TIC cap so the dot product has no guards.
// The tiles are wave-private: ordering is by lh_wave_sync(), no s_barrier.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void lh_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

template <int LP, int TIC, int WT, typename TIO>
__global__ __launch_bounds__(kBlock) void lift_head_fwd_gen_kernel(
    const TIO* __restrict__ x, const TIO* __restrict__ W1,
    const TIO* __restrict__ b1, const TIO* __restrict__ W2,
    const TIO* __restrict__ b2, TIO* __restrict__ out,
    int C, int W, int Ti, int To, int S, int N) {
  constexpr int CC = 4;
  constexpr int PW = 64 / LP;                 // points per wave
  constexpr int XT = PW * CC * TIC;           // x tile floats per wave
  constexpr int NPASS = (XT + 63) / 64;
  __shared__ float w2[24 * CC], bb2[24];
  __shared__ float xt[kBlock / 64][XT];
  for (int j = threadIdx.x; j < W * C; j += kBlock) w2[j] = ld(W2 + j);
  for (int j = threadIdx.x; j < W; j += kBlock) bb2[j] = ld(b2 + j);
  for (int j = threadIdx.x; j < (kBlock / 64) * XT; j += kBlock)
    (&xt[0][0])[j] = 0.f;
  __syncthreads();

  const int wave = (int)(threadIdx.x >> 6);
  const int lane = (int)(threadIdx.x & 63);
  const int p = lane / LP;                    // which point of the wave
  const int k = lane % LP;
  const bool kv = k < To;
  float* xw = &xt[wave][0];

  float w1r[TIC];
#pragma unroll
  for (int i = 0; i < TIC; ++i)
    w1r[i] = (kv && i < Ti) ? ld(W1 + k * Ti + i) : 0.f;
  const float b1k = kv ? ld(b1 + k) : 0.f;

  // staging roles: lane (+64 per pass) <-> (point, channel, step) of the tile
  int sp[NPASS], sc[NPASS], si[NPASS];
  bool sv[NPASS];
#pragma unroll
  for (int j = 0; j < NPASS; ++j) {
    const int idx = lane + 64 * j;
    const int ct = C * Ti;
    sv[j] = idx < PW * ct;
    sp[j] = idx / ct;
    const int r = idx - sp[j] * ct;
    sc[j] = r / Ti;
    si[j] = r - sc[j] * Ti;
  }
  const int nwork = (N + PW - 1) / PW;
  auto ldx = [&](int t, int j) -> float {
    const int e = PW * t + sp[j];
    if (!sv[j] || t >= nwork || e >= N) return 0.f;
    const int b = e / S;
    const int s = e - b * S;
    return ld(x + ((long)(b * C + sc[j]) * S + s) * Ti + si[j]);
  };

  const int t0 = (int)blockIdx.x * (kBlock / 64) + wave;
  const int stride = (int)gridDim.x * (kBlock / 64);
  float xn[NPASS];
#pragma unroll
  for (int j = 0; j < NPASS; ++j) xn[j] = ldx(t0, j);
  for (int t = t0; t < nwork; t += stride) {
#pragma unroll
    for (int j = 0; j < NPASS; ++j)
      if (sv[j]) xw[(sp[j] * CC + sc[j]) * TIC + si[j]] = xn[j];
    lh_wave_sync();
#pragma unroll
    for (int j = 0; j < NPASS; ++j) xn[j] = ldx(t + stride, j);

    const int e = PW * t + p;
    const bool ev = e < N;
    const int b = e / S;
    const int s = e - b * S;
    float h[CC];
#pragma unroll
    for (int c = 0; c < CC; ++c) {
      if (c < C) {
        float z = b1k;
#pragma unroll
        for (int i = 0; i < TIC; ++i) z += w1r[i] * xw[(p * CC + c) * TIC + i];
        h[c] = kv ? dfno_gelu::gelu(z) : 0.f;
      }
    }
    lh_wave_sync();                           // tile reads done before refill
#pragma unroll 4
    for (int w = 0; w < (WT > 0 ? WT : 512); ++w) {
      if (WT == 0 && w >= W) break;
      float acc = bb2[w];
#pragma unroll
      for (int c = 0; c < CC; ++c)
        if (c < C) acc += w2[w * C + c] * h[c];
      if (ev && kv)
        st(out + ((long)(b * W + w) * S + s) * To + k, dfno_gelu::gelu(acc));
    }
  }
}

// Backward of the general lift.  gW2/gb2 reduce as in the T_in == 1 kernel
// (per-wave gz/h tiles, v_mfma_f32_16x16x4 with the ones column, fragments
// carried across iterations).  gW1[k, :] / gb1[k] accumulate per lane in
// registers (k is fixed).  gx[c, s, i] = sum_k W1[k,i] gz1[c,k] reduces over
// the lanes of a point: gz1 goes through the (then free) h tile and the
// staging lanes (point, c, i) each run one To-long dot product against W1
// in LDS, storing a contiguous Ti run per (b, c, s).  Weight-grad partials
// of the block's waves are summed in LDS before the global atomics: the
// destinations are one ~2 KB row shared by every block, where contended
// float atomics are an order of magnitude slower than streaming ones.
template <int LP, int TIC, int WT, typename TIO>
__global__ __launch_bounds__(kBlock) void lift_head_bwd_gen_kernel(
    const TIO* __restrict__ gy, const TIO* __restrict__ x,
    const TIO* __restrict__ W1, const TIO* __restrict__ b1,
    const TIO* __restrict__ W2, const TIO* __restrict__ b2,
    TIO* __restrict__ gx, float* __restrict__ gW1, float* __restrict__ gb1,
    float* __restrict__ gW2, float* __restrict__ gb2,
    int C, int W, int Ti, int To, int S, int N) {
  constexpr int CC = 4;
  constexpr int GLD = 68;                     // gz/h tile row pad (banks)
  constexpr int PW = 64 / LP;
  constexpr int XT = PW * CC * TIC;
  constexpr int NPASS = (XT + 63) / 64;
  constexpr int NW = kBlock / 64;
  __shared__ float w1s[64 * 16], w2[24 * CC], bb2[24];
  __shared__ float gzt[NW][24 * GLD];
  __shared__ float ht[NW][CC * GLD];
  __shared__ float xt[NW][XT];
  for (int j = threadIdx.x; j < To * Ti; j += kBlock) w1s[j] = ld(W1 + j);
  for (int j = threadIdx.x; j < W * C; j += kBlock) w2[j] = ld(W2 + j);
  for (int j = threadIdx.x; j < W; j += kBlock) bb2[j] = ld(b2 + j);
  for (int j = threadIdx.x; j < NW * XT; j += kBlock) (&xt[0][0])[j] = 0.f;
  __syncthreads();

  const int wave = (int)(threadIdx.x >> 6);
  const int lane = (int)(threadIdx.x & 63);
  const int p = lane / LP;
  const int k = lane % LP;
  const bool kv = k < To;
  const int l16 = lane & 15;
  const int kg = lane >> 4;
  float* gzw = &gzt[wave][0];
  float* hw = &ht[wave][0];
  float* xw = &xt[wave][0];

  float w1r[TIC], pgW1[TIC];
#pragma unroll
  for (int i = 0; i < TIC; ++i) {
    w1r[i] = (kv && i < Ti) ? ld(W1 + k * Ti + i) : 0.f;
    pgW1[i] = 0.f;
  }
  const float b1k = kv ? ld(b1 + k) : 0.f;
  float pgb1 = 0.f;
  f32x4_lh wacc[2];                           // gW2/gb2 frags (2 m-tiles)
  wacc[0] = f32x4_lh{0.f, 0.f, 0.f, 0.f};
  wacc[1] = f32x4_lh{0.f, 0.f, 0.f, 0.f};
  // one point per wave: lanes >= To hold zeros, skip their MFMA k-steps
  const int kend = (PW == 1) ? ((To + 3) & ~3) : 64;

  int sp[NPASS], sc[NPASS], si[NPASS];
  bool sv[NPASS];
#pragma unroll
  for (int j = 0; j < NPASS; ++j) {
    const int idx = lane + 64 * j;
    const int ct = C * Ti;
    sv[j] = idx < PW * ct;
    sp[j] = idx / ct;
    const int r = idx - sp[j] * ct;
    sc[j] = r / Ti;
    si[j] = r - sc[j] * Ti;
  }
  const int nwork = (N + PW - 1) / PW;
  auto xoff = [&](int t, int j) -> long {     // -1: nothing to load/store
    const int e = PW * t + sp[j];
    if (!sv[j] || t >= nwork || e >= N) return -1L;
    const int b = e / S;
    const int s = e - b * S;
    return ((long)(b * C + sc[j]) * S + s) * Ti + si[j];
  };

  const int t0 = (int)blockIdx.x * NW + wave;
  const int stride = (int)gridDim.x * NW;
  float xn[NPASS];
#pragma unroll
  for (int j = 0; j < NPASS; ++j) {
    const long o = xoff(t0, j);
    xn[j] = o >= 0 ? ld(x + o) : 0.f;
  }
  for (int t = t0; t < nwork; t += stride) {
    long xo[NPASS];                           // this iteration's gx targets
#pragma unroll
    for (int j = 0; j < NPASS; ++j) {
      xo[j] = xoff(t, j);
      if (sv[j]) xw[(sp[j] * CC + sc[j]) * TIC + si[j]] = xn[j];
    }
    lh_wave_sync();
#pragma unroll
    for (int j = 0; j < NPASS; ++j) {
      const long o = xoff(t + stride, j);
      xn[j] = o >= 0 ? ld(x + o) : 0.f;
    }

    const int e = PW * t + p;
    const bool ev = e < N;
    const int b = e / S;
    const int s = e - b * S;
    // all W gy columns preloaded back-to-back: one memory round trip
    float gyv[WT > 0 ? WT : 24];
#pragma unroll
    for (int w = 0; w < (WT > 0 ? WT : 24); ++w) {
      gyv[w] = (w < W && ev && kv)
                   ? ld(gy + ((long)(b * W + w) * S + s) * To + k) : 0.f;
    }
    float z1[CC], h[CC], gh[CC];
#pragma unroll
    for (int c = 0; c < CC; ++c) {
      if (c < C) {
        float z = b1k;
#pragma unroll
        for (int i = 0; i < TIC; ++i) z += w1r[i] * xw[(p * CC + c) * TIC + i];
        z1[c] = z;
        h[c] = kv ? dfno_gelu::gelu(z) : 0.f;
        gh[c] = 0.f;
        hw[c * GLD + lane] = h[c];
      }
    }
#pragma unroll 4
    for (int w = 0; w < (WT > 0 ? WT : 512); ++w) {
      if (WT == 0 && w >= W) break;
      float z2 = bb2[w];
#pragma unroll
      for (int c = 0; c < CC; ++c)
        if (c < C) z2 += w2[w * C + c] * h[c];
      const float gz2 = gyv[w] * dfno_gelu::gelu_grad(z2);
      gzw[w * GLD + lane] = gz2;
#pragma unroll
      for (int c = 0; c < CC; ++c)
        if (c < C) gh[c] += w2[w * C + c] * gz2;
    }
    lh_wave_sync();
    // gW2/gb2 fragment update from this iteration's tiles
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      if (mt * 16 < W) {
        const int wrow = mt * 16 + l16;
        const bool av = wrow < W;
#pragma unroll 4
        for (int k0 = 0; k0 < kend; k0 += 4) {
          const float a = av ? gzw[wrow * GLD + k0 + kg] : 0.f;
          const float bb = (l16 < C) ? hw[l16 * GLD + k0 + kg]
                                     : (l16 == C ? 1.f : 0.f);
          wacc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bb, wacc[mt],
                                                          0, 0, 0);
        }
      }
    }
    lh_wave_sync();                           // h tile free: reuse for gz1
#pragma unroll
    for (int c = 0; c < CC; ++c) {
      if (c < C) {
        const float gz1 = kv ? gh[c] * dfno_gelu::gelu_grad(z1[c]) : 0.f;
        pgb1 += gz1;
#pragma unroll
        for (int i = 0; i < TIC; ++i)
          pgW1[i] += gz1 * xw[(p * CC + c) * TIC + i];
        hw[c * GLD + lane] = gz1;
      }
    }
    lh_wave_sync();
#pragma unroll
    for (int j = 0; j < NPASS; ++j) {
      if (xo[j] >= 0) {
        const float* g1 = hw + sc[j] * GLD + sp[j] * LP;
        const float* wc = w1s + si[j];
        // four independent chains: the LDS reads of a step issue together
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        int kk = 0;
        for (; kk + 3 < To; kk += 4) {
          a0 += wc[kk * Ti] * g1[kk];
          a1 += wc[(kk + 1) * Ti] * g1[kk + 1];
          a2 += wc[(kk + 2) * Ti] * g1[kk + 2];
          a3 += wc[(kk + 3) * Ti] * g1[kk + 3];
        }
        for (; kk < To; ++kk) a0 += wc[kk * Ti] * g1[kk];
        st(gx + xo[j], (a0 + a1) + (a2 + a3));
      }
    }
    lh_wave_sync();                           // tiles free for the next point
  }

  // flush: sum the block's waves in LDS (aliasing the gz tiles, now dead),
  // then one global atomic per (block, destination)
  __syncthreads();
  float* red = &gzt[0][0];
  float* r_gW1 = red;                         // [To*Ti] <= 1024
  float* r_gb1 = red + 64 * 16;               // [To]    <= 64
  float* r_gW2 = r_gb1 + 64;                  // [W*C]   <= 96
  float* r_gb2 = r_gW2 + 24 * CC;             // [W]     <= 24
  static_assert(64 * 16 + 64 + 24 * CC + 24 <= NW * 24 * GLD, "flush tile");
  for (int j = threadIdx.x; j < 64 * 16 + 64 + 24 * CC + 24; j += kBlock)
    red[j] = 0.f;
  __syncthreads();
  if (kv) {
#pragma unroll
    for (int i = 0; i < TIC; ++i)
      if (i < Ti) atomicAdd(&r_gW1[k * Ti + i], pgW1[i]);
    atomicAdd(&r_gb1[k], pgb1);
  }
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int w = mt * 16 + kg * 4 + r;
      const float v = wacc[mt][r];
      if (w < W) {
        if (l16 < C) atomicAdd(&r_gW2[w * C + l16], v);
        else if (l16 == C) atomicAdd(&r_gb2[w], v);
      }
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < To * Ti; j += kBlock)
    if (r_gW1[j] != 0.f) atomicAdd(&gW1[j], r_gW1[j]);
  for (int j = threadIdx.x; j < To; j += kBlock)
    if (r_gb1[j] != 0.f) atomicAdd(&gb1[j], r_gb1[j]);
  for (int j = threadIdx.x; j < W * C; j += kBlock)
    if (r_gW2[j] != 0.f) atomicAdd(&gW2[j], r_gW2[j]);
  for (int j = threadIdx.x; j < W; j += kBlock)
    if (r_gb2[j] != 0.f) atomicAdd(&gb2[j], r_gb2[j]);
}

// fp64 (correctness path) variants of the general lift: one thread per
// point, time axis chunked KC columns at a time like the kernels at the top
// of this file; x is re-read through L1 instead of living in registers.
template <typename T>
__global__ __launch_bounds__(kBlock) void lift_head_fwd_gen_chunk_kernel(
    const T* __restrict__ x, const T* __restrict__ W1, const T* __restrict__ b1,
    const T* __restrict__ W2, const T* __restrict__ b2, T* __restrict__ out,
    int C, int W, int Ti, int To, int S, int N) {
  constexpr int CC = 4, KC = 8;
  __shared__ T w1[64 * 16], bb1[64], w2[24 * CC], bb2[24];
  for (int j = threadIdx.x; j < To * Ti; j += kBlock) w1[j] = W1[j];
  for (int j = threadIdx.x; j < To; j += kBlock) bb1[j] = b1[j];
  for (int j = threadIdx.x; j < W * C; j += kBlock) w2[j] = W2[j];
  for (int j = threadIdx.x; j < W; j += kBlock) bb2[j] = b2[j];
  __syncthreads();

  const int stride = (int)gridDim.x * kBlock;
  for (int e = (int)blockIdx.x * kBlock + (int)threadIdx.x; e < N; e += stride) {
    const int b = e / S;
    const int s = e - b * S;
    for (int k0 = 0; k0 < To; k0 += KC) {
      const int kn = min(KC, To - k0);
      T h[CC][KC];
#pragma unroll
      for (int c = 0; c < CC; ++c) {
        if (c < C) {
          const T* xp = x + ((long)(b * C + c) * S + s) * Ti;
#pragma unroll
          for (int kk = 0; kk < KC; ++kk) {
            if (kk < kn) {
              T z = bb1[k0 + kk];
              for (int i = 0; i < Ti; ++i) z += w1[(k0 + kk) * Ti + i] * xp[i];
              h[c][kk] = dfno_gelu::gelu(z);
            }
          }
        }
      }
      for (int w = 0; w < W; ++w) {
        T* dst = out + ((long)(b * W + w) * S + s) * To + k0;
#pragma unroll
        for (int kk = 0; kk < KC; ++kk) {
          if (kk < kn) {
            T acc = bb2[w];
#pragma unroll
            for (int c = 0; c < CC; ++c)
              if (c < C) acc += w2[w * C + c] * h[c][kk];
            dst[kk] = dfno_gelu::gelu(acc);
          }
        }
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void lift_head_bwd_gen_chunk_kernel(
    const T* __restrict__ gy, const T* __restrict__ x,
    const T* __restrict__ W1, const T* __restrict__ b1,
    const T* __restrict__ W2, const T* __restrict__ b2,
    T* __restrict__ gx, T* __restrict__ gW1, T* __restrict__ gb1,
    T* __restrict__ gW2, T* __restrict__ gb2,
    int C, int W, int Ti, int To, int S, int N) {
  constexpr int CC = 4, KC = 8;
  __shared__ T w1[64 * 16], bb1[64], w2[24 * CC], bb2[24];
  // block accumulators (lane 0 of each wave adds its wave's sum)
  __shared__ T a_gW1[64 * 16], a_gb1[64], a_gW2[24 * CC], a_gb2[24];
  for (int j = threadIdx.x; j < To * Ti; j += kBlock) { w1[j] = W1[j]; a_gW1[j] = T(0); }
  for (int j = threadIdx.x; j < To; j += kBlock) { bb1[j] = b1[j]; a_gb1[j] = T(0); }
  for (int j = threadIdx.x; j < W * C; j += kBlock) { w2[j] = W2[j]; a_gW2[j] = T(0); }
  for (int j = threadIdx.x; j < W; j += kBlock) { bb2[j] = b2[j]; a_gb2[j] = T(0); }
  __syncthreads();

  const int lane = (int)(threadIdx.x & 63);
  const int stride = (int)gridDim.x * kBlock;
  // block-uniform trip count: every lane takes part in the wave sums; a
  // lane past the end works on the last point with its gy zeroed
  for (int e0 = (int)blockIdx.x * kBlock; e0 < N; e0 += stride) {
    const bool ev = e0 + (int)threadIdx.x < N;
    const int e = ev ? e0 + (int)threadIdx.x : N - 1;
    const int b = e / S;
    const int s = e - b * S;
    for (int k0 = 0; k0 < To; k0 += KC) {
      const int kn = min(KC, To - k0);
      T z1[CC][KC], h[CC][KC], gh[CC][KC];
#pragma unroll
      for (int c = 0; c < CC; ++c) {
        if (c < C) {
          const T* xp = x + ((long)(b * C + c) * S + s) * Ti;
#pragma unroll
          for (int kk = 0; kk < KC; ++kk) {
            if (kk < kn) {
              T z = bb1[k0 + kk];
              for (int i = 0; i < Ti; ++i) z += w1[(k0 + kk) * Ti + i] * xp[i];
              z1[c][kk] = z;
              h[c][kk] = dfno_gelu::gelu(z);
              gh[c][kk] = T(0);
            }
          }
        }
      }
      for (int w = 0; w < W; ++w) {
        const T* gyp = gy + ((long)(b * W + w) * S + s) * To + k0;
        T gz2[KC];
        T gb2p = T(0);
#pragma unroll
        for (int kk = 0; kk < KC; ++kk) {
          if (kk < kn) {
            T z2 = bb2[w];
#pragma unroll
            for (int c = 0; c < CC; ++c)
              if (c < C) z2 += w2[w * C + c] * h[c][kk];
            gz2[kk] = ev ? gyp[kk] * dfno_gelu::gelu_grad(z2) : T(0);
            gb2p += gz2[kk];
          }
        }
#pragma unroll
        for (int c = 0; c < CC; ++c) {
          if (c < C) {
            const T wv = w2[w * C + c];
            T gw2p = T(0);
#pragma unroll
            for (int kk = 0; kk < KC; ++kk) {
              if (kk < kn) {
                gh[c][kk] += wv * gz2[kk];
                gw2p += gz2[kk] * h[c][kk];
              }
            }
            gw2p = wave_sum(gw2p);
            if (lane == 0) atomicAdd(&a_gW2[w * C + c], gw2p);
          }
        }
        gb2p = wave_sum(gb2p);
        if (lane == 0) atomicAdd(&a_gb2[w], gb2p);
      }
      // gz1 = gh * gelu'(z1) (kept in gh); gx/gW1/gb1 from it
#pragma unroll
      for (int c = 0; c < CC; ++c) {
        if (c < C) {
#pragma unroll
          for (int kk = 0; kk < KC; ++kk)
            if (kk < kn) gh[c][kk] *= dfno_gelu::gelu_grad(z1[c][kk]);
          if (ev) {
            T* gxp = gx + ((long)(b * C + c) * S + s) * Ti;
            for (int i = 0; i < Ti; ++i) {
              T v = k0 > 0 ? gxp[i] : T(0);
#pragma unroll
              for (int kk = 0; kk < KC; ++kk)
                if (kk < kn) v += w1[(k0 + kk) * Ti + i] * gh[c][kk];
              gxp[i] = v;
            }
          }
        }
      }
#pragma unroll
      for (int kk = 0; kk < KC; ++kk) {
        if (kk < kn) {
          T pb = T(0);
#pragma unroll
          for (int c = 0; c < CC; ++c)
            if (c < C) pb += gh[c][kk];
          pb = wave_sum(pb);
          if (lane == 0) atomicAdd(&a_gb1[k0 + kk], pb);
          for (int i = 0; i < Ti; ++i) {
            T pw = T(0);
#pragma unroll
            for (int c = 0; c < CC; ++c)
              if (c < C)
                pw += gh[c][kk] * x[((long)(b * C + c) * S + s) * Ti + i];
            pw = wave_sum(pw);
            if (lane == 0) atomicAdd(&a_gW1[(k0 + kk) * Ti + i], pw);
          }
        }
      }
    }
  }

  __syncthreads();
  for (int j = threadIdx.x; j < To * Ti; j += kBlock)
    if (a_gW1[j] != T(0)) atomicAdd(&gW1[j], a_gW1[j]);
  for (int j = threadIdx.x; j < To; j += kBlock)
    if (a_gb1[j] != T(0)) atomicAdd(&gb1[j], a_gb1[j]);
  for (int j = threadIdx.x; j < W * C; j += kBlock)
    if (a_gW2[j] != T(0)) atomicAdd(&gW2[j], a_gW2[j]);
  for (int j = threadIdx.x; j < W; j += kBlock)
    if (a_gb2[j] != T(0)) atomicAdd(&gb2[j], a_gb2[j]);
}

// ---- host side of the general lift: x [B, C, S, Ti] ----

struct LiftDims { int B, C, W, Ti, To, S, N; };

// Every cap below sizes an LDS array or a register tile of the kernels
// above: an out-of-range call must raise here, never launch.
LiftDims lift_gen_dims(const at::Tensor& x, const at::Tensor& W1,
                       const at::Tensor& b1, const at::Tensor& W2,
                       const at::Tensor& b2) {
  TORCH_CHECK(x.dim() == 4, "x must be [B,C,S,Ti]");
  TORCH_CHECK(x.is_cuda() && x.is_contiguous(), "x must be contiguous GPU");
  TORCH_CHECK(x.scalar_type() == at::kFloat || x.scalar_type() == at::kDouble ||
              x.scalar_type() == at::kBFloat16,
              "lift_head: x must be float32/float64/bfloat16");
  TORCH_CHECK(W1.dim() == 2 && W2.dim() == 2 && b1.dim() == 1 && b2.dim() == 1,
              "lift_head: W1 [To,Ti], b1 [To], W2 [W,C], b2 [W]");
  const long B = x.size(0), C = x.size(1), S = x.size(2), Ti = x.size(3);
  const long To = W1.size(0), W = W2.size(0);
  TORCH_CHECK(W1.size(1) == Ti && W2.size(1) == C && b1.size(0) == To &&
              b2.size(0) == W, "lift_head shapes");
  TORCH_CHECK(C >= 1 && C <= 4 && Ti >= 1 && Ti <= 16 && To >= 1 && To <= 64 &&
              W >= 1 && W <= 24, "lift_head: unsupported dims (C <= 4, "
              "T_in <= 16, T_out <= 64, width <= 24)");
  TORCH_CHECK(B * S < (1L << 30), "lift_head: too many grid points");
  for (const at::Tensor* t : {&W1, &b1, &W2, &b2}) {
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == x.scalar_type(),
                "lift_head: weights must be GPU tensors of x's dtype");
  }
  return {(int)B, (int)C, (int)W, (int)Ti, (int)To, (int)S, (int)(B * S)};
}

// blocks of 4 waves; a wave takes 64/LP points per iteration
int lift_gen_grid(const LiftDims& d, int lp, long cap) {
  const long pw = 64 / lp;
  const long nwork = (d.N + pw - 1) / pw;
  return launch_grid(nwork, kBlock / 64, cap);
}

// LP x TIC x WT dispatch shared by forward and backward
#define LH_GEN_DISPATCH(LAUNCH, TIO)                                          \
  do {                                                                        \
    if (d.To <= 32) {                                                         \
      if (d.Ti <= 4) { if (d.W == 20) LAUNCH(32, 4, 20, TIO);                 \
                       else LAUNCH(32, 4, 0, TIO); }                          \
      else { if (d.W == 20) LAUNCH(32, 16, 20, TIO);                          \
             else LAUNCH(32, 16, 0, TIO); }                                   \
    } else {                                                                  \
      if (d.Ti <= 4) { if (d.W == 20) LAUNCH(64, 4, 20, TIO);                 \
                       else LAUNCH(64, 4, 0, TIO); }                          \
      else { if (d.W == 20) LAUNCH(64, 16, 20, TIO);                          \
             else LAUNCH(64, 16, 0, TIO); }                                   \
    }                                                                         \
  } while (0)

at::Tensor lift_head_gen_fwd(const at::Tensor& x, const at::Tensor& W1,
                             const at::Tensor& b1, const at::Tensor& W2,
                             const at::Tensor& b2) {
  const LiftDims d = lift_gen_dims(x, W1, b1, W2, b2);
  auto out = at::empty({d.B, d.W, d.S, d.To}, x.options());
  if (x.numel() == 0) return out;
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  // weights are read in their storage dtype (bf16 ones widen on load)
  auto W1f = W1.contiguous(), b1f = b1.contiguous();
  auto W2f = W2.contiguous(), b2f = b2.contiguous();
  if (x.scalar_type() == at::kDouble) {
    hipLaunchKernelGGL((lift_head_fwd_gen_chunk_kernel<double>),
                       dim3(launch_grid(d.N, kBlock, 256L * 8)), dim3(kBlock), 0,
                       stream,
                       x.data_ptr<double>(), W1f.data_ptr<double>(),
                       b1f.data_ptr<double>(), W2f.data_ptr<double>(),
                       b2f.data_ptr<double>(), out.data_ptr<double>(),
                       d.C, d.W, d.Ti, d.To, d.S, d.N);
    DFNO_CHECK_LAUNCH("lift_head");
    return out;
  }
  const bool bf16 = x.scalar_type() == at::kBFloat16;
  const int grid = lift_gen_grid(d, d.To <= 32 ? 32 : 64, 256L * 8);
#define LH_GEN_FWD(LP, TIC, WT, TIO)                                          \
  hipLaunchKernelGGL((lift_head_fwd_gen_kernel<LP, TIC, WT, TIO>),            \
                     dim3(grid), dim3(kBlock), 0, stream,                     \
                     reinterpret_cast<const TIO*>(x.data_ptr()),              \
                     reinterpret_cast<const TIO*>(W1f.data_ptr()),            \
                     reinterpret_cast<const TIO*>(b1f.data_ptr()),            \
                     reinterpret_cast<const TIO*>(W2f.data_ptr()),            \
                     reinterpret_cast<const TIO*>(b2f.data_ptr()),            \
                     reinterpret_cast<TIO*>(out.data_ptr()),                  \
                     d.C, d.W, d.Ti, d.To, d.S, d.N)
  if (bf16) LH_GEN_DISPATCH(LH_GEN_FWD, unsigned short);
  else LH_GEN_DISPATCH(LH_GEN_FWD, float);
#undef LH_GEN_FWD
  DFNO_CHECK_LAUNCH("lift_head");
  return out;
}

std::vector<at::Tensor> lift_head_gen_bwd(
    const at::Tensor& gy, const at::Tensor& x, const at::Tensor& W1,
    const at::Tensor& b1, const at::Tensor& W2, const at::Tensor& b2) {
  const LiftDims d = lift_gen_dims(x, W1, b1, W2, b2);
  TORCH_CHECK(gy.dim() == 4 && gy.size(0) == d.B && gy.size(1) == d.W &&
              gy.size(2) == d.S && gy.size(3) == d.To, "lift_head_bwd: gy shape");
  auto gx = at::empty_like(x);
  // weight grads accumulate fp32 even for bf16 activations
  auto fopt = x.options().dtype(x.scalar_type() == at::kDouble
                                    ? at::kDouble : at::kFloat);
  // one zero fill for the four accumulators
  const long n1 = (long)d.To * d.Ti, n2 = (long)d.W * d.C;
  auto gw = at::zeros({n1 + d.To + n2 + d.W}, fopt);
  auto gW1 = gw.narrow(0, 0, n1).view({d.To, d.Ti});
  auto gb1 = gw.narrow(0, n1, d.To);
  auto gW2 = gw.narrow(0, n1 + d.To, n2).view({d.W, d.C});
  auto gb2 = gw.narrow(0, n1 + d.To + n2, d.W);
  if (x.numel() == 0) return {gx, gW1, gb1, gW2, gb2};
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  auto W1f = W1.contiguous(), b1f = b1.contiguous();
  auto W2f = W2.contiguous(), b2f = b2.contiguous();
  if (x.scalar_type() == at::kDouble) {
    hipLaunchKernelGGL((lift_head_bwd_gen_chunk_kernel<double>),
                       dim3(launch_grid(d.N, kBlock, 256L * 8)), dim3(kBlock), 0,
                       stream,
                       gy.data_ptr<double>(), x.data_ptr<double>(),
                       W1f.data_ptr<double>(), b1f.data_ptr<double>(),
                       W2f.data_ptr<double>(), b2f.data_ptr<double>(),
                       gx.data_ptr<double>(), gW1.data_ptr<double>(),
                       gb1.data_ptr<double>(), gW2.data_ptr<double>(),
                       gb2.data_ptr<double>(), d.C, d.W, d.Ti, d.To, d.S, d.N);
    DFNO_CHECK_LAUNCH("lift_head");
    return {gx, gW1, gb1, gW2, gb2};
  }
  const bool bf16 = x.scalar_type() == at::kBFloat16;
  // one resident round of blocks (3 per CU fit by VGPRs at the Ti cap of
  // 16, 4 by LDS): every block ends with its weight-grad atomics, so fewer,
  // longer-lived blocks are cheaper
  const int grid = lift_gen_grid(d, d.To <= 32 ? 32 : 64, 256L * 3);
#define LH_GEN_BWD(LP, TIC, WT, TIO)                                          \
  hipLaunchKernelGGL((lift_head_bwd_gen_kernel<LP, TIC, WT, TIO>),            \
                     dim3(grid), dim3(kBlock), 0, stream,                     \
                     reinterpret_cast<const TIO*>(gy.data_ptr()),             \
                     reinterpret_cast<const TIO*>(x.data_ptr()),              \
                     reinterpret_cast<const TIO*>(W1f.data_ptr()),            \
                     reinterpret_cast<const TIO*>(b1f.data_ptr()),            \
                     reinterpret_cast<const TIO*>(W2f.data_ptr()),            \
                     reinterpret_cast<const TIO*>(b2f.data_ptr()),            \
                     reinterpret_cast<TIO*>(gx.data_ptr()),                   \
                     gW1.data_ptr<float>(), gb1.data_ptr<float>(),            \
                     gW2.data_ptr<float>(), gb2.data_ptr<float>(),            \
                     d.C, d.W, d.Ti, d.To, d.S, d.N)
  if (bf16) LH_GEN_DISPATCH(LH_GEN_BWD, unsigned short);
  else LH_GEN_DISPATCH(LH_GEN_BWD, float);
#undef LH_GEN_BWD
  DFNO_CHECK_LAUNCH("lift_head");
  return {gx, gW1, gb1, gW2, gb2};
}
#undef LH_GEN_DISPATCH

}  // namespace

at::Tensor lift_head_fwd(const at::Tensor& x, const at::Tensor& W1,
                         const at::Tensor& b1, const at::Tensor& W2,
                         const at::Tensor& b2) {
  if (x.dim() == 4) return lift_head_gen_fwd(x, W1, b1, W2, b2);
  TORCH_CHECK(x.is_cuda() && x.is_contiguous(), "x must be contiguous GPU");
  if (x.scalar_type() != at::kBFloat16) { check_real(x, "x"); }
  TORCH_CHECK(x.dim() == 3, "x must be [B,C,S] or [B,C,S,Ti]");
  int B = (int)x.size(0), C = (int)x.size(1);
  long S = x.size(2);
  int Tn = (int)W1.size(0), W = (int)W2.size(0);
  TORCH_CHECK(W1.size(1) == 1 && (int)W2.size(1) == C, "lift_head shapes");
  TORCH_CHECK(C <= 4 && Tn <= 32 && W <= 24, "lift_head: unsupported dims");
  // fp64 (the gradient-check path) has no lane-per-k kernel: [B,C,S] runs
  // the chunked general lift as [B,C,S,1]
  if (x.scalar_type() == at::kDouble)
    return lift_head_gen_fwd(x.unsqueeze(-1), W1, b1, W2, b2);

  auto out = at::empty({B, W, S, (long)Tn}, x.options());
  if (x.numel() == 0) return out;
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  int grid2 = launch_grid(2 * (((long)B * S + 1) / 2) * 32, kBlock, 256L * 8);
  const bool bf16 = x.scalar_type() == at::kBFloat16;
  auto W1f = bf16 ? W1.to(at::kFloat).contiguous() : W1;
  auto b1f = bf16 ? b1.to(at::kFloat).contiguous() : b1;
  auto W2f = bf16 ? W2.to(at::kFloat).contiguous() : W2;
  auto b2f = bf16 ? b2.to(at::kFloat).contiguous() : b2;
#define LH_FWD(WT, TIO)                                                       \
  hipLaunchKernelGGL((lift_head_fwd_lk_kernel<WT, TIO>), dim3(grid2),         \
                     dim3(kBlock), 0, stream,                                 \
                     reinterpret_cast<const TIO*>(x.data_ptr()),              \
                     W1f.data_ptr<float>(), b1f.data_ptr<float>(),            \
                     W2f.data_ptr<float>(), b2f.data_ptr<float>(),            \
                     reinterpret_cast<TIO*>(out.data_ptr()), B, C, W, Tn, S)
  if (bf16) { if (W == 20) LH_FWD(20, unsigned short);
              else LH_FWD(0, unsigned short); }
  else { if (W == 20) LH_FWD(20, float); else LH_FWD(0, float); }
#undef LH_FWD
  DFNO_CHECK_LAUNCH("lift_head");
  return out;
}

std::vector<at::Tensor> lift_head_bwd(const at::Tensor& gy, const at::Tensor& x,
                                      const at::Tensor& W1, const at::Tensor& b1,
                                      const at::Tensor& W2, const at::Tensor& b2) {
  TORCH_CHECK(gy.is_cuda() && gy.is_contiguous() && x.is_contiguous() &&
              gy.scalar_type() == x.scalar_type(), "lift_head_bwd IO");
  if (x.dim() == 4) return lift_head_gen_bwd(gy, x, W1, b1, W2, b2);
  if (x.scalar_type() != at::kBFloat16) { check_real(gy, "gy"); check_real(x, "x"); }
  int B = (int)x.size(0), C = (int)x.size(1);
  long S = x.size(2);
  int Tn = (int)W1.size(0), W = (int)W2.size(0);
  TORCH_CHECK(C <= 4 && Tn <= 32 && W <= 24, "lift_head: unsupported dims");
  if (x.scalar_type() == at::kDouble) {   // as in lift_head_fwd
    auto g = lift_head_gen_bwd(gy, x.unsqueeze(-1), W1, b1, W2, b2);
    g[0] = g[0].view(x.sizes());
    return g;
  }

  auto gx = at::empty_like(x);
  // weight grads accumulate fp32 even for bf16 activations
  auto fopt = x.options().dtype(at::kFloat);
  auto gW1 = at::zeros({Tn, 1}, fopt);
  auto gb1 = at::zeros({Tn}, fopt);
  auto gW2 = at::zeros({W, C}, fopt);
  auto gb2 = at::zeros({W}, fopt);
  if (x.numel() == 0) return {gx, gW1, gb1, gW2, gb2};

  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  int grid2 = launch_grid(2 * (((long)B * S + 1) / 2) * 32, kBlock, 256L * 8);
  const bool bf16 = x.scalar_type() == at::kBFloat16;
  auto W1f = bf16 ? W1.to(at::kFloat).contiguous() : W1;
  auto b1f = bf16 ? b1.to(at::kFloat).contiguous() : b1;
  auto W2f = bf16 ? W2.to(at::kFloat).contiguous() : W2;
  auto b2f = bf16 ? b2.to(at::kFloat).contiguous() : b2;
#define LH_BWD(WT, TIO)                                                       \
  hipLaunchKernelGGL((lift_head_bwd_lk_kernel<WT, TIO>), dim3(grid2),         \
                     dim3(kBlock), 0, stream,                                 \
                     reinterpret_cast<const TIO*>(gy.data_ptr()),             \
                     reinterpret_cast<const TIO*>(x.data_ptr()),              \
                     W1f.data_ptr<float>(), b1f.data_ptr<float>(),            \
                     W2f.data_ptr<float>(), b2f.data_ptr<float>(),            \
                     reinterpret_cast<TIO*>(gx.data_ptr()),                   \
                     gW1.data_ptr<float>(), gb1.data_ptr<float>(),            \
                     gW2.data_ptr<float>(), gb2.data_ptr<float>(),            \
                     B, C, W, Tn, S)
  if (bf16) { if (W == 20) LH_BWD(20, unsigned short);
              else LH_BWD(0, unsigned short); }
  else { if (W == 20) LH_BWD(20, float); else LH_BWD(0, float); }
#undef LH_BWD
  DFNO_CHECK_LAUNCH("lift_head");
  return {gx, gW1, gb1, gW2, gb2};
}
