// gfx950 fused FNO lift head: y = gelu(W2 @ gelu(W1 @t x + b1) + b2).
//
// The reference runs this as a time-lift einsum (T_in -> T_out along the
// trailing dim), a GELU pass, a channel-lift einsum (C_in -> width) and
// another GELU (dfno.py:310-311,333-338).  rocBLAS
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
#include "launch_select.h"

namespace {

using namespace dfno_io;

constexpr int kBlock = 256;

// Width rows.  WCAP is the width cap that sizes the W2 / b2 LDS arrays: 24
// for the narrow row, 64 for widths 25..64.  The backward kernels walk the
// width in WCAP / SR slabs of SR rows: one 24-row slab in the narrow row, two
// 32-row slabs in the wide one, each slab with its own gy preload, its own
// fill of the per-wave gz tile and its own two 16-row MFMA m-tiles, so the
// tile and the preload stay near the narrow row's size at width 64.
template <int WCAP> struct LiftSlab {
  static_assert(WCAP == 24 || WCAP == 64, "width rows: 24 or 64");
  static constexpr int SR = WCAP > 32 ? 32 : WCAP;   // rows per slab
  static constexpr int NSLAB = WCAP / SR;
  static constexpr int NMT = 2 * NSLAB;              // 16-row MFMA m-tiles
};

// orders a wave's accesses to its private LDS tiles (no s_barrier)
__device__ __forceinline__ void lh_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// fp32 lane-per-k variants: each 64-lane wave covers TWO s-points with
// lanes 0..Tn-1 / 32..32+Tn-1 owning one time column each, so every gy
// read and out write is a contiguous Tn-dword run (a one-point-per-thread
// layout streams 30-float runs per lane -> fully scattered wave accesses;
// measured 699/843 us vs ~110/130 us of traffic).  Per-lane state is
// ~40 VGPRs; gW1/gb1 partials accumulate in registers (k fixed per lane).
template <int WT, int WCAP, typename TIO = float>
__global__ __launch_bounds__(kBlock) void lift_head_fwd_lk_kernel(
    const TIO* __restrict__ x, const float* __restrict__ W1,
    const float* __restrict__ b1, const float* __restrict__ W2,
    const float* __restrict__ b2, TIO* __restrict__ out,
    int B, int C, int W, int Tn, long S) {
  constexpr int CC = 4;
  __shared__ float w1[32], bb1[32], w2[WCAP * CC], bb2[WCAP];
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

template <int WT, int WCAP, typename TIO = float>
__global__ __launch_bounds__(kBlock) void lift_head_bwd_lk_kernel(
    const TIO* __restrict__ gy, const TIO* __restrict__ x,
    const float* __restrict__ W1, const float* __restrict__ b1,
    const float* __restrict__ W2, const float* __restrict__ b2,
    TIO* __restrict__ gx, float* __restrict__ gW1, float* __restrict__ gb1,
    float* __restrict__ gW2, float* __restrict__ gb2,
    int B, int C, int W, int Tn, long S) {
  constexpr int CC = 4;
  constexpr int GLD = 68;                     // gz/h tile row pad (banks)
  constexpr int SR = LiftSlab<WCAP>::SR, NSLAB = LiftSlab<WCAP>::NSLAB;
  constexpr int NMT = LiftSlab<WCAP>::NMT;
  // row-loop trip bound: the pin, a slab, or (one slab) "until w == W"
  constexpr int WL = WT > 0 ? WT : (NSLAB > 1 ? SR : 512);
  __shared__ float w1[32], bb1[32], w2[WCAP * CC], bb2[WCAP];
  // per-wave tiles: gz [SR w][64 lanes] and h [4 c][64 lanes]; the gW2 and
  // gb2 reductions run as v_mfma_f32_16x16x4 over these (B-operand column
  // 4 is a constant ones column giving gb2) with the C fragments carried
  // in registers across pairs — the per-pair 6-shuffle wave_sum chains of
  // the first cut were the whole kernel's latency.
  __shared__ float gzt[4][SR * GLD];
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
  f32x4 wacc[NMT];                         // gW2/gb2 frags (2 m-tiles a slab)
#pragma unroll
  for (int mt = 0; mt < NMT; ++mt) wacc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
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
    // per slab of SR rows (gh accumulates over the slabs): all of the slab's
    // gy columns preloaded back-to-back, one memory round trip per pair and
    // slab instead of one per unroll batch (the loads were the kernel's
    // whole latency — all reduction variants measured the same ~900 us)
#pragma unroll
    for (int sl = 0; sl < NSLAB; ++sl) {
      const int w0 = sl * SR;                 // wave-uniform
      if (NSLAB > 1 && w0 >= W) break;
      float gyv[WT > 0 ? WT : SR];
#pragma unroll
      for (int wl = 0; wl < (WT > 0 ? WT : SR); ++wl) {
        const int w = w0 + wl;
        gyv[wl] = (w < W && ev && kv)
                      ? ld(gy + ((b * W + w) * S + s) * Tn + k) : 0.f;
      }
      // the previous slab's MFMA reads of the gz tile come first
      if (NSLAB > 1) lh_wave_sync();
#pragma unroll 4
      for (int wl = 0; wl < WL; ++wl) {
        const int w = w0 + wl;
        if (WT == 0 && w >= W) break;
        float z2 = bb2[w];
#pragma unroll
        for (int c = 0; c < CC; ++c)
          if (c < C) z2 += w2[w * C + c] * h[c];
        const float gz2 = gyv[wl] * dfno_gelu::gelu_grad(z2);
        gzw[wl * GLD + lane] = gz2;
#pragma unroll
        for (int c = 0; c < CC; ++c)
          if (c < C) gh[c] += w2[w * C + c] * gz2;
      }
      if (NSLAB > 1) lh_wave_sync();
      // gW2/gb2 fragment update from this slab's tiles (wave-synchronous:
      // same wave wrote gzt/ht just above)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        if (NSLAB > 1 && w0 + mt * 16 >= W) break;
        const int wrow = w0 + mt * 16 + l16;
        const bool av = wrow < W;
#pragma unroll 4
        for (int k0 = 0; k0 < 64; k0 += 4) {
          const float a = av ? gzw[(mt * 16 + l16) * GLD + k0 + kg] : 0.f;
          const float bb = (l16 < C) ? hw[l16 * GLD + k0 + kg]
                                     : (l16 == C ? 1.f : 0.f);
          wacc[2 * sl + mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(
              a, bb, wacc[2 * sl + mt], 0, 0, 0);
        }
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
  for (int mt = 0; mt < NMT; ++mt) {
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
template <int LP, int TIC, int WT, int WCAP, typename TIO>
__global__ __launch_bounds__(kBlock) void lift_head_fwd_gen_kernel(
    const TIO* __restrict__ x, const TIO* __restrict__ W1,
    const TIO* __restrict__ b1, const TIO* __restrict__ W2,
    const TIO* __restrict__ b2, TIO* __restrict__ out,
    int C, int W, int Ti, int To, int S, int N) {
  constexpr int CC = 4;
  constexpr int PW = 64 / LP;                 // points per wave
  constexpr int XT = PW * CC * TIC;           // x tile floats per wave
  constexpr int NPASS = (XT + 63) / 64;
  __shared__ float w2[WCAP * CC], bb2[WCAP];
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
template <int LP, int TIC, int WT, int WCAP, typename TIO>
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
  constexpr int SR = LiftSlab<WCAP>::SR, NSLAB = LiftSlab<WCAP>::NSLAB;
  constexpr int NMT = LiftSlab<WCAP>::NMT;
  // row-loop trip bound: the pin, a slab, or (one slab) "until w == W"
  constexpr int WL = WT > 0 ? WT : (NSLAB > 1 ? SR : 512);
  __shared__ float w1s[64 * 16], w2[WCAP * CC], bb2[WCAP];
  __shared__ float gzt[NW][SR * GLD];
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
  f32x4 wacc[NMT];                         // gW2/gb2 frags (2 m-tiles a slab)
#pragma unroll
  for (int mt = 0; mt < NMT; ++mt) wacc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
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
    float z1[CC], h[CC], gh[CC];
    // per slab of SR rows; gh accumulates over the slabs
#pragma unroll
    for (int sl = 0; sl < NSLAB; ++sl) {
      const int w0 = sl * SR;                 // wave-uniform
      if (sl > 0 && w0 >= W) break;
      // the slab's gy columns preloaded back-to-back: one memory round trip
      float gyv[WT > 0 ? WT : SR];
#pragma unroll
      for (int wl = 0; wl < (WT > 0 ? WT : SR); ++wl) {
        const int w = w0 + wl;
        gyv[wl] = (w < W && ev && kv)
                      ? ld(gy + ((long)(b * W + w) * S + s) * To + k) : 0.f;
      }
      if (sl == 0) {
        // z1 / h of the point, under the first slab's loads
#pragma unroll
        for (int c = 0; c < CC; ++c) {
          if (c < C) {
            float z = b1k;
#pragma unroll
            for (int i = 0; i < TIC; ++i)
              z += w1r[i] * xw[(p * CC + c) * TIC + i];
            z1[c] = z;
            h[c] = kv ? dfno_gelu::gelu(z) : 0.f;
            gh[c] = 0.f;
            hw[c * GLD + lane] = h[c];
          }
        }
      } else {
        lh_wave_sync();                       // gz tile free: MFMA reads done
      }
#pragma unroll 4
      for (int wl = 0; wl < WL; ++wl) {
        const int w = w0 + wl;
        if (WT == 0 && w >= W) break;
        float z2 = bb2[w];
#pragma unroll
        for (int c = 0; c < CC; ++c)
          if (c < C) z2 += w2[w * C + c] * h[c];
        const float gz2 = gyv[wl] * dfno_gelu::gelu_grad(z2);
        gzw[wl * GLD + lane] = gz2;
#pragma unroll
        for (int c = 0; c < CC; ++c)
          if (c < C) gh[c] += w2[w * C + c] * gz2;
      }
      lh_wave_sync();
      // gW2/gb2 fragment update from this slab's tiles
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        if (w0 + mt * 16 < W) {
          const int wrow = w0 + mt * 16 + l16;
          const bool av = wrow < W;
#pragma unroll 4
          for (int k0 = 0; k0 < kend; k0 += 4) {
            const float a = av ? gzw[(mt * 16 + l16) * GLD + k0 + kg] : 0.f;
            const float bb = (l16 < C) ? hw[l16 * GLD + k0 + kg]
                                       : (l16 == C ? 1.f : 0.f);
            wacc[2 * sl + mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                a, bb, wacc[2 * sl + mt], 0, 0, 0);
          }
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
  float* r_gW2 = r_gb1 + 64;                  // [W*C]   <= WCAP * 4
  float* r_gb2 = r_gW2 + WCAP * CC;           // [W]     <= WCAP
  static_assert(64 * 16 + 64 + WCAP * CC + WCAP <= NW * SR * GLD, "flush tile");
  for (int j = threadIdx.x; j < 64 * 16 + 64 + WCAP * CC + WCAP; j += kBlock)
    red[j] = 0.f;
  __syncthreads();
  if (kv) {
#pragma unroll
    for (int i = 0; i < TIC; ++i)
      if (i < Ti) atomicAdd(&r_gW1[k * Ti + i], pgW1[i]);
    atomicAdd(&r_gb1[k], pgb1);
  }
#pragma unroll
  for (int mt = 0; mt < NMT; ++mt) {
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

// fp64 (correctness path) variants of the general lift, for every T_in, 1
// included: one thread per point, the time axis walked KC columns at a time
// so that the h tile [C][KC] stays in registers; x is re-read through L1
// instead of living in registers.
template <typename T, int WCAP>
__global__ __launch_bounds__(kBlock) void lift_head_fwd_gen_chunk_kernel(
    const T* __restrict__ x, const T* __restrict__ W1, const T* __restrict__ b1,
    const T* __restrict__ W2, const T* __restrict__ b2, T* __restrict__ out,
    int C, int W, int Ti, int To, int S, int N) {
  constexpr int CC = 4, KC = 8;
  __shared__ T w1[64 * 16], bb1[64], w2[WCAP * CC], bb2[WCAP];
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

template <typename T, int WCAP>
__global__ __launch_bounds__(kBlock) void lift_head_bwd_gen_chunk_kernel(
    const T* __restrict__ gy, const T* __restrict__ x,
    const T* __restrict__ W1, const T* __restrict__ b1,
    const T* __restrict__ W2, const T* __restrict__ b2,
    T* __restrict__ gx, T* __restrict__ gW1, T* __restrict__ gb1,
    T* __restrict__ gW2, T* __restrict__ gb2,
    int C, int W, int Ti, int To, int S, int N) {
  constexpr int CC = 4, KC = 8;
  __shared__ T w1[64 * 16], bb1[64], w2[WCAP * CC], bb2[WCAP];
  // block accumulators (lane 0 of each wave adds its wave's sum)
  __shared__ T a_gW1[64 * 16], a_gb1[64], a_gW2[WCAP * CC],
      a_gb2[WCAP];
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

// ---- host side ----

struct LiftDims { int B, C, W, Ti, To, S, N; };

// x is [B,C,S,Ti], or [B,C,S] for T_in == 1 with T_out up to this (the form
// the lane-per-k kernels take; ops/lifthead.py routes by the same constant)
constexpr int kLaneKMaxTo = 32;

// Every cap below sizes an LDS array or a register tile of the kernels
// above: an out-of-range call must raise here, never launch.  [B,C,S] is
// validated as [B,C,S,1]; gy (backward) is [B,W,S,To] for both forms.
LiftDims lift_dims(const at::Tensor& x, const at::Tensor& W1,
                   const at::Tensor& b1, const at::Tensor& W2,
                   const at::Tensor& b2, const at::Tensor* gy) {
  TORCH_CHECK(x.dim() == 3 || x.dim() == 4, "x must be [B,C,S] or [B,C,S,Ti]");
  TORCH_CHECK(x.is_cuda() && x.is_contiguous(), "x must be contiguous GPU");
  TORCH_CHECK(x.scalar_type() == at::kFloat || x.scalar_type() == at::kDouble ||
              x.scalar_type() == at::kBFloat16,
              "lift_head: x must be float32/float64/bfloat16");
  TORCH_CHECK(W1.dim() == 2 && W2.dim() == 2 && b1.dim() == 1 && b2.dim() == 1,
              "lift_head: W1 [To,Ti], b1 [To], W2 [W,C], b2 [W]");
  const long B = x.size(0), C = x.size(1), S = x.size(2);
  const long Ti = x.dim() == 4 ? x.size(3) : 1;
  const long To = W1.size(0), W = W2.size(0);
  TORCH_CHECK(W1.size(1) == Ti && W2.size(1) == C && b1.size(0) == To &&
              b2.size(0) == W, "lift_head shapes");
  TORCH_CHECK(C >= 1 && C <= 4 && Ti >= 1 && Ti <= 16 && To >= 1 && To <= 64 &&
              W >= 1 && W <= 64, "lift_head: unsupported dims (C <= 4, "
              "T_in <= 16, T_out <= 64, width <= 64)");
  TORCH_CHECK(x.dim() == 4 || To <= kLaneKMaxTo,
              "lift_head: unsupported dims ([B,C,S] takes T_out <= 32)");
  TORCH_CHECK(B * S < (1L << 30), "lift_head: too many grid points");
  for (const at::Tensor* t : {&W1, &b1, &W2, &b2}) {
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() &&
                t->scalar_type() == x.scalar_type(),
                "lift_head: weights must be contiguous GPU tensors of x's dtype");
  }
  if (gy != nullptr) {
    TORCH_CHECK(gy->is_cuda() && gy->is_contiguous() &&
                gy->scalar_type() == x.scalar_type(), "lift_head_bwd IO");
    TORCH_CHECK(gy->dim() == 4 && gy->size(0) == B && gy->size(1) == W &&
                gy->size(2) == S && gy->size(3) == To, "lift_head_bwd: gy shape");
  }
  return {(int)B, (int)C, (int)W, (int)Ti, (int)To, (int)S, (int)(B * S)};
}

// The tensors of one call: forward writes out; backward (gy set) writes gx
// and accumulates into the four zeroed weight grads.
struct LiftCall {
  LiftDims d;
  const at::Tensor &x, &W1, &b1, &W2, &b2;
  at::Tensor* out;
  const at::Tensor* gy;
  at::Tensor *gx, *gW1, *gb1, *gW2, *gb2;
  hipStream_t stream;
};

// Rows (fp32 and bf16 each; TIO is the storage type of x / out / gy / gx):
//   [B,C,S]       lane-per-k    <WT, WCAP>      WT 20 at width 20, else 0;
//                 WCAP 24 at width <= 24, else 64 (LiftSlab: the backward
//                 walks two 32-row slabs, four MFMA fragments)
//   [B,C,S,Ti]    general       <LP, TIC, WT, WCAP>   LP 32 lanes per point
//                 at T_out <= 32, else 64; TIC 4 x steps in registers at
//                 T_in <= 4, else 16; WT and WCAP as above
//   fp64          chunk kernels, both forms     <WCAP> as above
// The width rows are <20, 24>, <0, 24> and <0, 64>: no width above 24 is
// pinned.  Grids are blocks of 4 waves, grid-stride: lane-per-k one wave per pair of
// points, forward and backward at most 8 blocks per CU; general one wave per
// 64 / LP points, forward at most 8 per CU, backward 3 (one resident round:
// 3 fit by VGPRs at the T_in cap, and every block ends with its weight-grad
// atomics, so fewer, longer-lived blocks are cheaper); fp64 one thread per
// point, at most 8 per CU.
template <typename F>
void with_width(const LiftDims& d, F&& f) {
  if (d.W > 24) {
    f(int_c<0>{}, int_c<64>{});
  } else {
    select_bool(d.W == 20, [&](auto pin) {
      f(int_c<decltype(pin)::value ? 20 : 0>{}, int_c<24>{});
    });
  }
}
template <typename F>
void with_lift_row(const LiftDims& d, F&& f) {
  select_le<32, 64>(d.To, [&](auto lp) {
    select_le<4, 16>(d.Ti, [&](auto tic) {
      with_width(d, [&](auto wt, auto wcap) { f(lp, tic, wt, wcap); });
    });
  });
}

template <typename TIO>
const TIO* lift_in(const at::Tensor& t) {
  return static_cast<const TIO*>(t.data_ptr());
}

// fp32 staging copy of a bf16 weight (the tensor itself when it is fp32)
at::Tensor f32(const at::Tensor& t) { return t.to(at::kFloat); }

// lane-per-k kernels: fp32 weights, bf16 ones through a staging copy
template <typename TIO>
void launch_lift_lk(const LiftCall& c) {
  const LiftDims& d = c.d;
  const auto W1f = f32(c.W1), b1f = f32(c.b1), W2f = f32(c.W2), b2f = f32(c.b2);
  const int grid =
      launch_grid(2 * (((long)d.N + 1) / 2) * 32, kBlock, 256L * 8);
  with_width(d, [&](auto wt, auto wcap) {
    constexpr int WT = decltype(wt)::value, WCAP = decltype(wcap)::value;
    if (c.gy == nullptr) {
      hipLaunchKernelGGL((lift_head_fwd_lk_kernel<WT, WCAP, TIO>), dim3(grid),
                         dim3(kBlock), 0, c.stream, lift_in<TIO>(c.x),
                         W1f.data_ptr<float>(), b1f.data_ptr<float>(),
                         W2f.data_ptr<float>(), b2f.data_ptr<float>(),
                         static_cast<TIO*>(c.out->data_ptr()), d.B, d.C, d.W,
                         d.To, (long)d.S);
    } else {
      hipLaunchKernelGGL((lift_head_bwd_lk_kernel<WT, WCAP, TIO>), dim3(grid),
                         dim3(kBlock), 0, c.stream, lift_in<TIO>(*c.gy),
                         lift_in<TIO>(c.x), W1f.data_ptr<float>(),
                         b1f.data_ptr<float>(), W2f.data_ptr<float>(),
                         b2f.data_ptr<float>(),
                         static_cast<TIO*>(c.gx->data_ptr()),
                         c.gW1->data_ptr<float>(), c.gb1->data_ptr<float>(),
                         c.gW2->data_ptr<float>(), c.gb2->data_ptr<float>(),
                         d.B, d.C, d.W, d.To, (long)d.S);
    }
  });
}

// general kernels: weights read in their storage dtype (bf16 widens on load)
template <typename TIO>
void launch_lift_gen(const LiftCall& c) {
  const LiftDims& d = c.d;
  with_lift_row(d, [&](auto lp, auto tic, auto wt, auto wcap) {
    constexpr int LP = decltype(lp)::value, TIC = decltype(tic)::value;
    constexpr int WT = decltype(wt)::value, WCAP = decltype(wcap)::value;
    const long nwork = (d.N + 64 / LP - 1) / (64 / LP);
    if (c.gy == nullptr) {
      hipLaunchKernelGGL((lift_head_fwd_gen_kernel<LP, TIC, WT, WCAP, TIO>),
                         dim3(launch_grid(nwork, kBlock / 64, 256L * 8)),
                         dim3(kBlock), 0, c.stream, lift_in<TIO>(c.x),
                         lift_in<TIO>(c.W1), lift_in<TIO>(c.b1),
                         lift_in<TIO>(c.W2), lift_in<TIO>(c.b2),
                         static_cast<TIO*>(c.out->data_ptr()), d.C, d.W, d.Ti,
                         d.To, d.S, d.N);
    } else {
      hipLaunchKernelGGL((lift_head_bwd_gen_kernel<LP, TIC, WT, WCAP, TIO>),
                         dim3(launch_grid(nwork, kBlock / 64, 256L * 3)),
                         dim3(kBlock), 0, c.stream, lift_in<TIO>(*c.gy),
                         lift_in<TIO>(c.x), lift_in<TIO>(c.W1),
                         lift_in<TIO>(c.b1), lift_in<TIO>(c.W2),
                         lift_in<TIO>(c.b2), static_cast<TIO*>(c.gx->data_ptr()),
                         c.gW1->data_ptr<float>(), c.gb1->data_ptr<float>(),
                         c.gW2->data_ptr<float>(), c.gb2->data_ptr<float>(),
                         d.C, d.W, d.Ti, d.To, d.S, d.N);
    }
  });
}

void launch_lift_chunk(const LiftCall& c) {
  const LiftDims& d = c.d;
  const dim3 grid(launch_grid(d.N, kBlock, 256L * 8));
  select_le<24, 64>(d.W, [&](auto wcap) {
    constexpr int WCAP = decltype(wcap)::value;
    if (c.gy == nullptr) {
      hipLaunchKernelGGL((lift_head_fwd_gen_chunk_kernel<double, WCAP>), grid,
                         dim3(kBlock), 0, c.stream, c.x.data_ptr<double>(),
                         c.W1.data_ptr<double>(), c.b1.data_ptr<double>(),
                         c.W2.data_ptr<double>(), c.b2.data_ptr<double>(),
                         c.out->data_ptr<double>(), d.C, d.W, d.Ti, d.To, d.S,
                         d.N);
    } else {
      hipLaunchKernelGGL((lift_head_bwd_gen_chunk_kernel<double, WCAP>), grid,
                         dim3(kBlock), 0, c.stream, c.gy->data_ptr<double>(),
                         c.x.data_ptr<double>(), c.W1.data_ptr<double>(),
                         c.b1.data_ptr<double>(), c.W2.data_ptr<double>(),
                         c.b2.data_ptr<double>(), c.gx->data_ptr<double>(),
                         c.gW1->data_ptr<double>(), c.gb1->data_ptr<double>(),
                         c.gW2->data_ptr<double>(), c.gb2->data_ptr<double>(),
                         d.C, d.W, d.Ti, d.To, d.S, d.N);
    }
  });
}

// kernel family by dtype and entry form
void launch_lift(const LiftCall& c) {
  const auto st = c.x.scalar_type();
  const bool lane_k = c.x.dim() == 3;
  if (st == at::kDouble) {
    launch_lift_chunk(c);
  } else if (st == at::kBFloat16) {
    if (lane_k) launch_lift_lk<unsigned short>(c);
    else launch_lift_gen<unsigned short>(c);
  } else {
    if (lane_k) launch_lift_lk<float>(c); else launch_lift_gen<float>(c);
  }
  DFNO_CHECK_LAUNCH("lift_head");
}

}  // namespace

at::Tensor lift_head_fwd(const at::Tensor& x, const at::Tensor& W1,
                         const at::Tensor& b1, const at::Tensor& W2,
                         const at::Tensor& b2) {
  const LiftDims d = lift_dims(x, W1, b1, W2, b2, nullptr);
  auto out = at::empty({d.B, d.W, d.S, d.To}, x.options());
  if (x.numel() == 0) return out;
  launch_lift({d, x, W1, b1, W2, b2, &out, nullptr, nullptr, nullptr, nullptr,
               nullptr, nullptr,
               at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()});
  return out;
}

std::vector<at::Tensor> lift_head_bwd(const at::Tensor& gy, const at::Tensor& x,
                                      const at::Tensor& W1, const at::Tensor& b1,
                                      const at::Tensor& W2, const at::Tensor& b2) {
  const LiftDims d = lift_dims(x, W1, b1, W2, b2, &gy);
  auto gx = at::empty_like(x);
  // weight grads accumulate fp32 even for bf16 activations
  auto fopt = x.options().dtype(x.scalar_type() == at::kDouble
                                    ? at::kDouble : at::kFloat);
  at::Tensor gW1, gb1, gW2, gb2;
  if (x.dim() == 3 && x.scalar_type() != at::kDouble) {
    // lane-per-k: every wave ends with its atomics, so the four accumulators
    // stay separate allocations (packed into one buffer the flagship
    // backward measured 1.10 against 0.66 ms)
    gW1 = at::zeros({d.To, d.Ti}, fopt);
    gb1 = at::zeros({d.To}, fopt);
    gW2 = at::zeros({d.W, d.C}, fopt);
    gb2 = at::zeros({d.W}, fopt);
  } else {
    // blocks pre-reduce in LDS: one zero fill for the four accumulators
    const long n1 = (long)d.To * d.Ti, n2 = (long)d.W * d.C;
    auto gw = at::zeros({n1 + d.To + n2 + d.W}, fopt);
    gW1 = gw.narrow(0, 0, n1).view({d.To, d.Ti});
    gb1 = gw.narrow(0, n1, d.To);
    gW2 = gw.narrow(0, n1 + d.To, n2).view({d.W, d.C});
    gb2 = gw.narrow(0, n1 + d.To + n2, d.W);
  }
  if (x.numel() == 0) return {gx, gW1, gb1, gW2, gb2};
  launch_lift({d, x, W1, b1, W2, b2, nullptr, &gy, &gx, &gW1, &gb1, &gW2, &gb2,
               at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()});
  return {gx, gW1, gb1, gW2, gb2};
}
