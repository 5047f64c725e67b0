// gfx950 (CDNA4) wide channel mix: y = act(W x + bias + res) over [B, I, S]
// for 33 <= max(I, O) <= 128, fp32 and bf16 storage.
//
// The x-resident / accumulator-resident kernels of pointwise.hip keep one
// side of the contraction in registers and stop at 32 channels; past that
// the only route was the scalar LDS kernel (no residual, fp32/fp64 only).
// Here the contraction runs on the matrix cores.  fp32: v_mfma_f32_16x16x4_f32
// (fp32 in, fp32 accumulate: bitwise an i-ascending fmaf chain, so the
// numerics are those of the narrow kernels).  bf16 storage:
// v_mfma_f32_16x16x32_bf16 (mix_wide_bf16_kernel further down; exact
// products, fp32 accumulate, bias and residual added in fp32, one rounding at
// the store); the fp32 body also compiles for bf16 storage and is kept as the
// A/B partner (DFNO_WIDE_BF16_F32MFMA=1).
//
// One body serves the three forms:
//  * trunk epilogue  gelu(W x + res), z stored only when asked for,
//  * plain mix with bias, with or without GELU (linear3, 64 -> 128),
//  * transposed mix  gx = W^T gz with W left in its [O, I] storage (wt).
// A fourth form (SYN, fp32, at most 64 rows and 64 contracted channels, entry
// wide_irfft_mix) replaces the residual by the time-axis irfft of a kept-mode
// spectrum, synthesized in the second pass: the fused block epilogue
// gelu(W x + pad_irfft(Yt)) and its adjoint mode W^T gz + rfft_trunc_adj(G)
// of epilogue.hip past 32 channels.
//
// Layout per block (4 waves) and s-tile of TS = 64 columns:
//  * W never touches LDS: a wave owns the output row groups mt = wave + 4 j
//    (j < MW) and holds their A fragments in registers for the whole kernel
//    (MW * KCAP / 4 VGPRs),
//  * the x tile is staged as [K][TS + 16] fp32 (the +16 pad puts the four
//    k-rows of one B-fragment read on disjoint banks); the next tile's rows
//    are register-prefetched over the current tile's MFMA phase,
//  * a 16x16 C fragment would store 64-byte row segments; instead the output
//    tile goes through LDS ([M][TS + 4]) and leaves in a second pass where a
//    row's 64 columns are contiguous (256 B fp32 / 128 B bf16 per row), with
//    residual, z store, GELU and the bf16 rounding done in that pass.
// Ragged S, S below one tile and unaligned rows (B > 1 with odd S) take the
// per-element variant of the same body (VECTOR = false).

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <torch/extension.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <algorithm>
#include <vector>

#include "kernels.h"
#include "gelu_math.h"
#include "device_util.h"

namespace {

using namespace dfno_io;

constexpr int kBlock = 256;
constexpr int kTS = 64;            // s columns per tile
constexpr int kLDX = kTS + 16;     // x tile row stride (floats)
constexpr int kLDO = kTS + 4;      // output tile row stride (floats)
constexpr long kGridCap = 256L * 4;

typedef float f32x4_mw __attribute__((ext_vector_type(4)));

// Columns of the synthesis addend (see SynArgs below): the staged spectrum
// tile Yl[row * RS + line * 2m + 2k], the twiddle rows twl[t * TWS + 2k] and
// this thread's four (line, t) offsets, packed: the kernel has four
// registers to spare at four waves per SIMD.
struct SynCols {
  const float* Yl;
  const float* twl;
  int lt[4];      // line offset | twiddle row offset << 16 (both < 2^16)
  int m, RS;
};

// irfft of row's staged lines at the thread's four columns; lanes whose
// columns share a line read one address (an LDS broadcast)
__device__ __forceinline__ void wide_syn_row(const SynCols& sc, int row,
                                             float (&syn)[4]) {
  const float* yrow = sc.Yl + row * sc.RS;
#pragma unroll
  for (int e = 0; e < 4; ++e) syn[e] = 0.0f;
#pragma unroll 1
  for (int k = 0; k < sc.m; ++k) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float2 w = *reinterpret_cast<const float2*>(
          sc.twl + (sc.lt[e] >> 16) + 2 * k);
      const float2 yv = *reinterpret_cast<const float2*>(
          yrow + (sc.lt[e] & 0xffff) + 2 * k);
      syn[e] += yv.x * w.x - yv.y * w.y;
    }
  }
}

// Second pass over the output tile ot[M][kLDO]: a thread owns 4 consecutive
// columns of one row, so a row's 64 columns leave in one contiguous segment.
// v = tile (+ res); z = v (when asked for); y = act ? gelu(v) : v.
// SYN: the addend is the synthesis of sc (wide_syn_row) instead of res.
template <typename T, int MW, bool VECTOR, bool SYN = false>
__device__ __forceinline__ void wide_epilogue(
    const float* ot, const T* __restrict__ res, T* __restrict__ y,
    T* __restrict__ z, int b, int M, long S, long s0, bool act,
    const SynCols* sc = nullptr) {
#pragma unroll
  for (int q = 0; q < MW * 4; ++q) {
    const int u = (int)threadIdx.x + q * kBlock;
    const int row = u >> 4;
    const int c = (u & 15) * 4;
    if (row < M && s0 + c < S) {
      const float4 o4 = *reinterpret_cast<const float4*>(&ot[row * kLDO + c]);
      float v[4] = {o4.x, o4.y, o4.z, o4.w};
      if constexpr (SYN) {
        float syn[4];
        wide_syn_row(*sc, row, syn);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += syn[e];
      }
      const long off = ((long)b * M + row) * S + s0 + c;
      if constexpr (VECTOR) {
        if (res != nullptr) {
          float rv[4];
          ldv<4>(res + off, rv);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += rv[e];
        }
        if (z != nullptr) stv<4>(z + off, v);
        if (act) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = dfno_gelu::gelu(v[e]);
        }
        stv<4>(y + off, v);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (s0 + c + e < S) {
            float ve = v[e];
            if (res != nullptr) ve += ld(res + off + e);
            if (z != nullptr) st(z + off + e, ve);
            st(y + off + e, act ? dfno_gelu::gelu(ve) : ve);
          }
        }
      }
    }
  }
}

// Synthesis addend (SYN): the value added to ot[row][col] is the time-axis
// irfft of row's kept-mode spectrum line at that column, column s of the
// tile being (line l = s / N, time t = s % N):
//   sum_{k < m} Yr[l][k] cos(2 pi k t / N) - Yi[l][k] sin(2 pi k t / N)
// i.e. dft_c2r_last_kernel's arithmetic, as the narrow kernel of epilogue.hip
// does it.  A tile starts and ends mid-line in general; the block stages the
// lines its 64 columns touch ([M][RS] floats, at most 62 / N + 2 lines per
// row) with pad_irfft's factors applied at the staging write.
struct SynArgs {
  const float* Ys;    // [B, M, L, m] complex64 as floats
  const float* tw;    // [N, m, 2] synthesis twiddles (cos, sin)
  long L;
  int N, m;
  float scale;        // 1 / N with factors, 1 without
  bool factors;       // interior modes doubled, DC / Nyquist imaginary dropped
};

__host__ __device__ inline int syn_max_lines(int N) { return 62 / N + 2; }
// row strides: +2 floats moves consecutive rows / time steps off one bank pair
__host__ __device__ inline int syn_row_stride(int N, int m) {
  return syn_max_lines(N) * 2 * m + 2;
}
__host__ __device__ inline int syn_tw_stride(int m) { return 2 * m + 2; }

// Stage the nl lines from l0 on of every row of batch b: 16 lanes per row,
// one complex value each, so a row's run is read in contiguous segments.
template <int MW>
__device__ __forceinline__ void wide_stage_spectrum(
    float* Yl, const SynArgs& sa, int b, int M, long l0, int nl, int RS) {
  const int m = sa.m;
  const int l16 = (int)threadIdx.x & 15;
  const int run = nl * m;
  const float f2 = 2.0f * sa.scale;
#pragma unroll
  for (int q = 0; q < MW * 4; ++q) {
    const int row = ((int)threadIdx.x >> 4) + q * 16;
    if (row < M) {
      const float2* src = reinterpret_cast<const float2*>(
          sa.Ys + (((long)b * M + row) * sa.L + l0) * (2 * m));
      float2* dst = reinterpret_cast<float2*>(Yl + row * RS);
#pragma unroll 1
      for (int j = l16; j < run; j += 16) {
        float2 v = src[j];
        if (sa.factors) {
          const int k = j % m;
          const bool edge = (k == 0) || (2 * k == sa.N);
          const float f = edge ? sa.scale : f2;
          v.x = f * v.x;
          v.y = edge ? 0.0f : f * v.y;
        }
        dst[j] = v;
      }
    }
  }
}

// A thread's four columns are the same in every unit of wide_epilogue: their
// staged line and twiddle row offsets.  tstart = s0 % N, nl = staged lines.
__device__ __forceinline__ SynCols wide_syn_cols(
    const float* Yl, const float* twl, int N, int m, int RS, int TWS,
    int tstart, int nl) {
  SynCols sc;
  sc.Yl = Yl; sc.twl = twl; sc.m = m; sc.RS = RS;
  const int c = ((int)threadIdx.x & 15) * 4;
  int l = (tstart + c) / N;
  int t = tstart + c - l * N;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    // columns past S: any staged line
    sc.lt[e] = (min(l, nl - 1) * 2 * m) | ((t * TWS) << 16);
    if (++t == N) { t = 0; ++l; }
  }
  return sc;
}

// K = contraction depth, M = output rows; W(m, k) = wt ? W[k*M + m] : W[m*K + k].
// KCAP >= K rounded up to 4, MW * 64 >= M.  SYN: the addend is synthesized
// from sa (res unused).  The kernel streams at the rate its resident blocks
// allow (four per CU at 37.9 KB), so the spectrum tile ([M][syn_row_stride]
// floats) takes no LDS of its own where it fits the x tile, which is dead
// between the MFMA phase and the next tile's staging: it is staged there
// after the second barrier, at the price of two more barriers per tile.
// Dynamic LDS holds the twiddle table ([N][syn_tw_stride], 2.1 KB at N = 30,
// m = 8) and the spectrum tile only where the x tile is too small for it.
template <int KCAP>
__host__ __device__ inline bool syn_tile_in_xt(int M, int N, int m) {
  return M * syn_row_stride(N, m) <= KCAP * kLDX;
}

template <typename T, int KCAP, int MW, bool VECTOR, bool SYN = false>
__global__ __launch_bounds__(kBlock, SYN ? 4 : 1) void mix_wide_kernel(
    const T* __restrict__ x, const T* __restrict__ W, const T* __restrict__ bias,
    const T* __restrict__ res, T* __restrict__ y, T* __restrict__ z,
    int B, int K, int M, long S, bool wt, bool act, SynArgs sa) {
  __shared__ __align__(16) float xt[KCAP * kLDX];
  __shared__ __align__(16) float ot[MW * 64 * kLDO];
  extern __shared__ __align__(16) float syn_lds[];
  float* twl = nullptr;
  float* Yl = nullptr;
  int RS = 0, TWS = 0;
  if constexpr (SYN) {
    RS = syn_row_stride(sa.N, sa.m);
    TWS = syn_tw_stride(sa.m);
    twl = syn_lds;
    Yl = syn_tile_in_xt<KCAP>(M, sa.N, sa.m)
             ? xt : syn_lds + ((sa.N * TWS + 3) & ~3);
    // read first after the first tile's first barrier
    for (int i = (int)threadIdx.x; i < sa.N * sa.m; i += kBlock) {
      const int t = i / sa.m;
      *reinterpret_cast<float2*>(twl + t * TWS + 2 * (i - t * sa.m)) =
          *reinterpret_cast<const float2*>(sa.tw + 2 * i);
    }
  }

  const int lane = (int)(threadIdx.x & 63);
  const int wave = (int)(threadIdx.x >> 6);
  const int l16 = lane & 15;
  const int kg = lane >> 4;
  const int K4 = (K + 3) & ~3;

  // A fragments and the bias rows of this wave's row groups
  float a[MW][KCAP / 4];
  float bv[MW][4];
#pragma unroll
  for (int j = 0; j < MW; ++j) {
    const int m = (wave + 4 * j) * 16 + l16;
#pragma unroll
    for (int k4 = 0; k4 < KCAP / 4; ++k4) {
      const int k = k4 * 4 + kg;
      float v = 0.f;
      if (m < M && k < K) v = ld(W + (wt ? (long)k * M + m : (long)m * K + k));
      a[j][k4] = v;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int mo = (wave + 4 * j) * 16 + kg * 4 + r;
      bv[j][r] = (!SYN && bias != nullptr && mo < M) ? ld(bias + mo) : 0.f;
    }
  }

  const long stiles = (S + kTS - 1) / kTS;
  const long tend = (long)B * stiles;

  // register-prefetched staging: unit u = 4 consecutive columns of one row
  constexpr int NPF = KCAP * (kTS / 4) / kBlock;
  float pf[NPF][4];
  auto prefetch = [&](long tt) {
    if (tt >= tend) return;
    const int b = (int)(tt / stiles);
    const long s0 = (tt % stiles) * kTS;
#pragma unroll
    for (int q = 0; q < NPF; ++q) {
      const int u = (int)threadIdx.x + q * kBlock;
      const int row = u >> 4;
      const int c = (u & 15) * 4;
      pf[q][0] = pf[q][1] = pf[q][2] = pf[q][3] = 0.f;
      if (row < K) {
        const T* p = x + ((long)b * K + row) * S + s0 + c;
        if constexpr (VECTOR) {
          if (s0 + c < S) ldv<4>(p, pf[q]);    // S % 4 == 0: all four or none
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (s0 + c + e < S) pf[q][e] = ld(p + e);
        }
      }
    }
  };
  prefetch(blockIdx.x);

  for (long t = blockIdx.x; t < tend; t += gridDim.x) {
    const int b = (int)(t / stiles);
    const long s0 = (t % stiles) * kTS;
    // xt was last read before the previous tile's second barrier
#pragma unroll
    for (int q = 0; q < NPF; ++q) {
      const int u = (int)threadIdx.x + q * kBlock;
      const int row = u >> 4;
      const int c = (u & 15) * 4;
      if (row < K4)      // rows K..K4-1 are the zero padding of the last k-step
        *reinterpret_cast<float4*>(&xt[row * kLDX + c]) =
            make_float4(pf[q][0], pf[q][1], pf[q][2], pf[q][3]);
    }
    prefetch(t + gridDim.x);
    __syncthreads();

    // D[m][n] over n = 4 column tiles; accumulate order: bias, k ascending
    f32x4_mw acc[MW][4];
#pragma unroll
    for (int j = 0; j < MW; ++j)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        acc[j][nt] = f32x4_mw{bv[j][0], bv[j][1], bv[j][2], bv[j][3]};
#pragma unroll
    for (int k4 = 0; k4 < KCAP / 4; ++k4) {
      if (k4 * 4 < K) {
        float bb[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
          bb[nt] = xt[(k4 * 4 + kg) * kLDX + nt * 16 + l16];
#pragma unroll
        for (int j = 0; j < MW; ++j) {
          if ((wave + 4 * j) * 16 < M) {
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
              acc[j][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                  a[j][k4], bb[nt], acc[j][nt], 0, 0, 0);
          }
        }
      }
    }
    // ot was last read before this tile's first barrier
#pragma unroll
    for (int j = 0; j < MW; ++j) {
      if ((wave + 4 * j) * 16 < M) {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            ot[((wave + 4 * j) * 16 + kg * 4 + r) * kLDO + nt * 16 + l16] =
                acc[j][nt][r];
      }
    }
    __syncthreads();

    if constexpr (SYN) {
      // every wave is past the MFMA phase: the x tile is free for the
      // spectrum lines of this tile's columns
      const long l0 = s0 / sa.N;
      const int tstart = (int)(s0 - l0 * sa.N);
      const long send = s0 + kTS < S ? s0 + kTS : S;
      const int nl = (int)((send - 1) / sa.N - l0) + 1;
      wide_stage_spectrum<MW>(Yl, sa, b, M, l0, nl, RS);
      __syncthreads();
      const SynCols sc = wide_syn_cols(Yl, twl, sa.N, sa.m, RS, TWS, tstart, nl);
      wide_epilogue<T, MW, VECTOR, true>(ot, nullptr, y, z, b, M, S, s0, act, &sc);
      __syncthreads();      // Yl read out before the next tile's x rows land
    } else {
      wide_epilogue<T, MW, VECTOR>(ot, res, y, z, b, M, S, s0, act);
    }
  }
}

// bf16 storage on v_mfma_f32_16x16x32_bf16.  A bf16 model holds W in bf16 as
// well, the product of two bf16 values is exact in fp32 and the accumulate is
// fp32, so this meets the bf16 contract (fp32 arithmetic, one rounding at the
// store) at 16x the fp32 MFMA rate; the fp32-MFMA body above is compute-bound
// on bf16 traffic (same time as fp32 at half the bytes).  A lane's B fragment
// is 8 consecutive k of one column, so the x tile is staged transposed,
// [TS][K + 8] bf16, and a fragment is one 16-byte LDS read.  K is padded to
// the MFMA depth 32 with zero columns.  Output tile and epilogue as above.
typedef __bf16 bf16x8_mw __attribute__((ext_vector_type(8)));

template <int KCAP, int MW>
__global__ __launch_bounds__(kBlock) void mix_wide_bf16_kernel(
    const unsigned short* __restrict__ x, const unsigned short* __restrict__ W,
    const unsigned short* __restrict__ bias, const unsigned short* __restrict__ res,
    unsigned short* __restrict__ y, unsigned short* __restrict__ z,
    int B, int K, int M, long S, bool wt, bool act) {
  using T = unsigned short;
  constexpr int LDB = KCAP + 8;    // bf16 per staged column (16-byte multiple)
  __shared__ __align__(16) unsigned short xt[kTS * LDB];
  __shared__ __align__(16) float ot[MW * 64 * kLDO];

  const int lane = (int)(threadIdx.x & 63);
  const int wave = (int)(threadIdx.x >> 6);
  const int l16 = lane & 15;
  const int kg = lane >> 4;
  const int K32 = (K + 31) & ~31;

  bf16x8_mw a[MW][KCAP / 32];
  float bv[MW][4];
#pragma unroll
  for (int j = 0; j < MW; ++j) {
    const int m = (wave + 4 * j) * 16 + l16;
#pragma unroll
    for (int ks = 0; ks < KCAP / 32; ++ks) {
      unsigned short w8[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int k = ks * 32 + kg * 8 + e;
        w8[e] = (m < M && k < K) ? W[wt ? (long)k * M + m : (long)m * K + k]
                                 : (unsigned short)0;
      }
      __builtin_memcpy(&a[j][ks], w8, sizeof(w8));
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int mo = (wave + 4 * j) * 16 + kg * 4 + r;
      bv[j][r] = (bias != nullptr && mo < M) ? ld(bias + mo) : 0.f;
    }
  }

  const long stiles = (S + kTS - 1) / kTS;
  const long tend = (long)B * stiles;

  // unit u = 4 consecutive columns of one row, kept packed (S % 8 == 0)
  constexpr int NPF = KCAP * (kTS / 4) / kBlock;
  uint2 pf[NPF];
  auto prefetch = [&](long tt) {
    if (tt >= tend) return;
    const int b = (int)(tt / stiles);
    const long s0 = (tt % stiles) * kTS;
#pragma unroll
    for (int q = 0; q < NPF; ++q) {
      const int u = (int)threadIdx.x + q * kBlock;
      const int row = u >> 4;
      const int c = (u & 15) * 4;
      pf[q] = make_uint2(0u, 0u);
      if (row < K && s0 + c < S)
        pf[q] = *reinterpret_cast<const uint2*>(x + ((long)b * K + row) * S + s0 + c);
    }
  };
  prefetch(blockIdx.x);

  for (long t = blockIdx.x; t < tend; t += gridDim.x) {
    const int b = (int)(t / stiles);
    const long s0 = (t % stiles) * kTS;
    // xt was last read before the previous tile's second barrier
#pragma unroll
    for (int q = 0; q < NPF; ++q) {
      const int u = (int)threadIdx.x + q * kBlock;
      const int row = u >> 4;
      const int c = (u & 15) * 4;
      if (row < K32) {   // rows K..K32-1: zero padding of the last k-step
        xt[(c + 0) * LDB + row] = (unsigned short)(pf[q].x & 0xffffu);
        xt[(c + 1) * LDB + row] = (unsigned short)(pf[q].x >> 16);
        xt[(c + 2) * LDB + row] = (unsigned short)(pf[q].y & 0xffffu);
        xt[(c + 3) * LDB + row] = (unsigned short)(pf[q].y >> 16);
      }
    }
    prefetch(t + gridDim.x);
    __syncthreads();

    f32x4_mw acc[MW][4];
#pragma unroll
    for (int j = 0; j < MW; ++j)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        acc[j][nt] = f32x4_mw{bv[j][0], bv[j][1], bv[j][2], bv[j][3]};
#pragma unroll
    for (int ks = 0; ks < KCAP / 32; ++ks) {
      if (ks * 32 < K) {
        bf16x8_mw bb[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
          bb[nt] = *reinterpret_cast<const bf16x8_mw*>(
              &xt[(nt * 16 + l16) * LDB + ks * 32 + kg * 8]);
#pragma unroll
        for (int j = 0; j < MW; ++j) {
          if ((wave + 4 * j) * 16 < M) {
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
              acc[j][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  a[j][ks], bb[nt], acc[j][nt], 0, 0, 0);
          }
        }
      }
    }
    // ot was last read before this tile's first barrier
#pragma unroll
    for (int j = 0; j < MW; ++j) {
      if ((wave + 4 * j) * 16 < M) {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            ot[((wave + 4 * j) * 16 + kg * 4 + r) * kLDO + nt * 16 + l16] =
                acc[j][nt][r];
      }
    }
    __syncthreads();

    wide_epilogue<T, MW, true>(ot, res, y, z, b, M, S, s0, act);
  }
}

template <typename T>
struct WideArgs {
  const T* x; const T* W; const T* bias; const T* res; T* y; T* z;
  int B, K, M; long S; bool wt, act, vec;
  hipStream_t stream;
};

template <typename T, int KCAP, int MW>
void launch_wide_km(const WideArgs<T>& a) {
  const long tiles = (long)a.B * ((a.S + kTS - 1) / kTS);
  const int grid = (int)std::max(1L, std::min(tiles, kGridCap));
  if constexpr (std::is_same<T, unsigned short>::value) {
    static const bool f32_mfma = []() {
      const char* e = getenv("DFNO_WIDE_BF16_F32MFMA");   // A/B knob
      return e && e[0] == '1';
    }();
    if (!f32_mfma) {
      hipLaunchKernelGGL((mix_wide_bf16_kernel<KCAP, MW>), dim3(grid),
                         dim3(kBlock), 0, a.stream, a.x, a.W, a.bias, a.res, a.y,
                         a.z, a.B, a.K, a.M, a.S, a.wt, a.act);
      return;
    }
  }
  // bf16 is vector-only (the host requires S % 8 == 0)
  if (a.vec || std::is_same<T, unsigned short>::value) {
    hipLaunchKernelGGL((mix_wide_kernel<T, KCAP, MW, true>), dim3(grid),
                       dim3(kBlock), 0, a.stream, a.x, a.W, a.bias, a.res, a.y,
                       a.z, a.B, a.K, a.M, a.S, a.wt, a.act, SynArgs{});
  } else if constexpr (std::is_same<T, float>::value) {
    hipLaunchKernelGGL((mix_wide_kernel<T, KCAP, MW, false>), dim3(grid),
                       dim3(kBlock), 0, a.stream, a.x, a.W, a.bias, a.res, a.y,
                       a.z, a.B, a.K, a.M, a.S, a.wt, a.act, SynArgs{});
  }
}

template <typename T>
void launch_wide(const WideArgs<T>& a) {
  if (a.K <= 64) {
    if (a.M <= 64) launch_wide_km<T, 64, 1>(a);
    else launch_wide_km<T, 64, 2>(a);
  } else {
    if (a.M <= 64) launch_wide_km<T, 128, 1>(a);
    else launch_wide_km<T, 128, 2>(a);
  }
}

// The synthesis form runs at K, M <= 64 only (one row group per wave).
template <bool VECTOR>
void launch_wide_syn(const WideArgs<float>& a, const SynArgs& sa) {
  const long tiles = (long)a.B * ((a.S + kTS - 1) / kTS);
  const int grid = (int)std::max(1L, std::min(tiles, kGridCap));
  const size_t smem = sizeof(float) * (size_t)(
      ((sa.N * syn_tw_stride(sa.m) + 3) & ~3) +
      (syn_tile_in_xt<64>(a.M, sa.N, sa.m)
           ? 0 : a.M * syn_row_stride(sa.N, sa.m)));
  auto kern = mix_wide_kernel<float, 64, 1, VECTOR, true>;
  // static + dynamic LDS passes 64 KiB at the long-line corners only
  // (N = 62, m = 32, 64 rows: 37.9 + 66.6 KiB of the CU's 160); the limit is
  // a property of the function on the current device, so it is raised at
  // each such launch, not once per process
  if (smem > (size_t)24 * 1024) {
    const hipError_t attr = hipFuncSetAttribute(
        reinterpret_cast<const void*>(kern),
        hipFuncAttributeMaxDynamicSharedMemorySize, 72 * 1024);
    TORCH_CHECK(attr == hipSuccess,
                "wide_irfft_mix: cannot raise the LDS limit: ",
                hipGetErrorString(attr));
  }
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), smem, a.stream, a.x, a.W,
                     a.bias, a.res, a.y, a.z, a.B, a.K, a.M, a.S, a.wt, a.act, sa);
}

}  // namespace

void wide_irfft_mix(const at::Tensor& x, const at::Tensor& W, const at::Tensor& Ys,
                    const at::Tensor& tw, at::Tensor& y, at::Tensor& z, int N,
                    bool adj) {
  const int B = (int)x.size(0), K = (int)x.size(1);
  const long S = x.size(2);
  const int M = (int)y.size(1);
  const int m = (int)Ys.size(3);
  TORCH_CHECK(K >= 1 && K <= 64 && M >= 1 && M <= 64 && N >= 1 && N <= 64 &&
              m >= 1 && m <= 32 && Ys.size(1) == M && Ys.size(2) * N == S &&
              W.numel() == (long)K * M,
              "wide_irfft_mix: needs K, M <= 64, N <= 64, m <= 32");
  const bool need_z = z.numel() > 0;
  const bool vec = S % 4 == 0 && aligned16(x.data_ptr()) && aligned16(y.data_ptr()) &&
                   (!need_z || aligned16(z.data_ptr()));
  const WideArgs<float> a{x.data_ptr<float>(), W.data_ptr<float>(), nullptr, nullptr,
                          y.data_ptr<float>(),
                          need_z ? z.data_ptr<float>() : nullptr, B, K, M, S,
                          /*wt=*/adj, /*act=*/!adj, vec,
                          at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()};
  const SynArgs sa{reinterpret_cast<const float*>(Ys.data_ptr()),
                   tw.data_ptr<float>(), Ys.size(2), N, m,
                   adj ? 1.0f : (float)(1.0 / (double)N), !adj};
  if (vec) launch_wide_syn<true>(a, sa);
  else launch_wide_syn<false>(a, sa);
}

std::vector<at::Tensor> wide_channel_mix(const at::Tensor& x, const at::Tensor& W,
                                         const at::Tensor& b, const at::Tensor& res,
                                         bool act, bool wt, bool need_z) {
  const bool bf16 = x.scalar_type() == at::kBFloat16;
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && W.is_cuda() && W.is_contiguous() &&
              (bf16 || x.scalar_type() == at::kFloat) &&
              W.scalar_type() == x.scalar_type(),
              "wide_channel_mix: contiguous fp32/bf16 GPU tensors of one dtype");
  TORCH_CHECK(x.dim() == 3 && W.dim() == 2, "wide_channel_mix: x [B,I,S], W [O,I]");
  const int B = (int)x.size(0), K = (int)x.size(1);
  const long S = x.size(2);
  const int M = wt ? (int)W.size(1) : (int)W.size(0);
  TORCH_CHECK((wt ? W.size(0) : W.size(1)) == K, "wide_channel_mix: W/x mismatch");
  TORCH_CHECK(K >= 1 && M >= 1 && std::max(K, M) >= 33 && std::max(K, M) <= 128,
              "wide_channel_mix: needs 33 <= max(I, O) <= 128, got I=", K,
              " O=", M);
  TORCH_CHECK(!bf16 || S % 8 == 0,
              "wide_channel_mix: bf16 S must be a multiple of 8");
  const bool has_bias = b.defined() && b.numel() > 0;
  const bool has_res = res.defined() && res.numel() > 0;
  if (has_bias)
    TORCH_CHECK(b.is_cuda() && b.is_contiguous() && b.numel() == M &&
                b.scalar_type() == x.scalar_type(), "wide_channel_mix: bias");
  if (has_res)
    TORCH_CHECK(res.is_cuda() && res.is_contiguous() && res.dim() == 3 &&
                res.size(0) == B && res.size(1) == M && res.size(2) == S &&
                res.scalar_type() == x.scalar_type(), "wide_channel_mix: res");

  auto y = at::empty({B, M, S}, x.options());
  auto z = need_z ? at::empty({B, M, S}, x.options()) : at::empty({0}, x.options());
  if (x.numel() == 0 || y.numel() == 0) return {y, z};

  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  const bool vec = S % 4 == 0 && aligned16(x.data_ptr()) && aligned16(y.data_ptr()) &&
                   (!need_z || aligned16(z.data_ptr())) &&
                   (!has_res || aligned16(res.data_ptr()));
  TORCH_CHECK(!bf16 || vec, "wide_channel_mix: bf16 tensors must be 16-byte aligned");
  if (bf16) {
    launch_wide<unsigned short>(
        {usp(x), usp(W), has_bias ? usp(b) : nullptr, has_res ? usp(res) : nullptr,
         usp_mut(y), need_z ? usp_mut(z) : nullptr, B, K, M, S, wt, act, true,
         stream});
  } else {
    launch_wide<float>(
        {x.data_ptr<float>(), W.data_ptr<float>(),
         has_bias ? b.data_ptr<float>() : nullptr,
         has_res ? res.data_ptr<float>() : nullptr, y.data_ptr<float>(),
         need_z ? z.data_ptr<float>() : nullptr, B, K, M, S, wt, act, vec, stream});
  }
  DFNO_CHECK_LAUNCH("wide_channel_mix");
  return {y, z};
}
