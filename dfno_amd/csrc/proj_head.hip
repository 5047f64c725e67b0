// gfx950 fused FNO projection head: out = W4 @ gelu(W3 @ x + b3) + b4.
//
// The reference computes this as two BroadcastedLinear einsums with a
// separate GELU between (dfno.py:348-352), which at the
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
#include "launch_select.h"

namespace {

using namespace dfno_io;

constexpr int kBlock = 256;

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
//
// Per 64-column tile, 4 waves (lane = kg*16 + l16), block barriers between
// the phases:
//   stage  x / gy columns, prefetched into registers during the previous
//          tile, go to LDS (xt, gyt); gb4 partials accumulate on the way.
//   1a     z3 = W3 @ x.  Wave w owns m-tiles 2w and 2w+1 for all four
//          n-tiles: its ten W3 fragments sit in registers for the whole
//          kernel, each x fragment is read once per (n-tile, k-step) and
//          feeds both m-tiles, and the eight chains run independently.
//   1b     gz = (W4^T gy) * gelu'(z3 + b3) in place (VALU); gb3 / gW4
//          partials per thread pair.
//   2a     gx = W3^T @ gz, K = 128.  Wave w owns n-tile w for both m-tiles
//          (channels 0..15 and 16..19): one gz fragment per k-step feeds two
//          chains; the W3 fragments come as one ds_read_b128 per four
//          k-steps from an LDS image in fragment order (W3f, W3g).
//   2b     gW3 += gz @ x^T, K = 64 columns.  Wave w owns x n-tile w&1 and
//          gz m-tiles (w>>1) + 2p: one x fragment feeds four chains.  Both
//          operands run along the tile row, so lane group kg takes columns
//          16g + 4kg .. +3 in four successive MFMAs (the same k order for A
//          and B) and one ds_read_b128 each serves four k-steps.
// The order in which any gx element is summed (k ascending, one chain from
// zero) is the plain one; only the gW3 column order inside a tile is
// permuted, and gW3 is summed over tiles and blocks in atomic order anyway.
//
// MFMA operands are loaded unconditionally.  Output row m of an MFMA
// depends only on A row m, output column n only on B column n, and the
// padded rows and columns (channel i >= 20) are dropped at the gx store and
// at the gW3 flush.  So the padded lanes read some in-bounds LDS word (a
// clamped row, or a repeat of rows 16..19 in W3g) with no exec mask and no
// zero: a masked operand read puts every MFMA in a basic block of its own
// with a full lgkmcnt(0) wait in front of it.
// ---------------------------------------------------------------------------

template <int IT, int MT, int O2T, typename TIO = float>
__global__ __launch_bounds__(kBlock, 3) void proj_head_bwd_fused_kernel(
    const TIO* __restrict__ gy, const TIO* __restrict__ x,
    const float* __restrict__ W3, const float* __restrict__ b3,
    const float* __restrict__ W4,
    TIO* __restrict__ gx, float* __restrict__ gW3,
    float* __restrict__ gb3, float* __restrict__ gW4,
    float* __restrict__ gb4, int B, int O2, long S) {
  static_assert(IT == 20 && MT == 128,
                "fragment maps: 4 waves x 2 m-tiles, channels 16..19 padded");
  constexpr int TS = 64;           // s-columns per tile (16 MFMA K-steps)
  constexpr int LD = TS + 4;       // row pad (float4-aligned, 4-bank skew)
  // gz tile + staged x tile + weights in LDS (52 KB -> 3 blocks/CU; an
  // x/W3-from-global variant at 4 blocks/CU measured 2x slower: the cold
  // per-lane B-operand loads serialize inside the MFMA chains)
  extern __shared__ __align__(16) char smem_raw[];
  float* gzt = reinterpret_cast<float*>(smem_raw);   // [MT][LD]
  float* xt = gzt + (size_t)MT * LD;                 // [IT][LD]
  float* gyt = xt + (size_t)IT * LD;                 // [O2T][TS]
  float* W3f = gyt + O2T * TS;                       // [MT/16][64][4]
  float* W3g = W3f + (size_t)MT * 16;                // [MT/16][4][IT-16][4]
  float* b3l = W3g + (size_t)MT * (IT - 16);         // [MT]
  float* W4l = b3l + MT;                             // [O2T*MT]
  float* gb3s = W4l + O2T * MT;                      // [MT]
  float* gW4s = gb3s + MT;                           // [O2T*MT]
  // W3 in phase 2a's A-fragment order, k = j = 16*g + 4*e + kg: W3f holds
  // rows i < 16 as [g][lane = kg*16 + i][e], W3g rows 16..IT-1 as
  // [g][kg][i - 16][e]; one ds_read_b128 each serves four k-steps
#pragma clang loop unroll(disable)
  for (int k = threadIdx.x; k < MT * 16; k += kBlock) {
    const int e = k & 3, ln = (k >> 2) & 63, g = k >> 8;
    W3f[k] = W3[(16 * g + 4 * e + (ln >> 4)) * IT + (ln & 15)];
  }
#pragma clang loop unroll(disable)
  for (int k = threadIdx.x; k < MT * (IT - 16); k += kBlock) {
    const int e = k & 3, r = (k >> 2) & 3, q = (k >> 4) & 3, g = k >> 6;
    W3g[k] = W3[(16 * g + 4 * e + q) * IT + 16 + r];
  }
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

  f32x4 wacc[4];                // gW3 frags: 8 mt-tiles x 2 nt-tiles
#pragma unroll
  for (int p = 0; p < 4; ++p) wacc[p] = f32x4{0.f, 0.f, 0.f, 0.f};
  float gb4a0 = 0.f, gb4a1 = 0.f;
  // phase 1a A fragments: the wave's m-tiles 2*wave and 2*wave+1 of W3,
  // the same for every tile
  float w3a[2][IT / 4];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ks = 0; ks < IT / 4; ++ks)
      w3a[mi][ks] = W3[((2 * wave + mi) * 16 + l16) * IT + 4 * ks + kg];

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
    // 8 m-tiles x 4 n-tiles over K = IT = 20; the wave's two m-tiles x all
    // four n-tiles as eight independent chains, x fragments shared.
    {
      f32x4 z4[2][4];
#pragma unroll
      for (int q = 0; q < 8; ++q) z4[q >> 2][q & 3] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < IT / 4; ++ks) {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const float bb = xt[(4 * ks + kg) * LD + nt * 16 + l16];
#pragma unroll
          for (int mi = 0; mi < 2; ++mi)
            z4[mi][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                w3a[mi][ks], bb, z4[mi][nt], 0, 0, 0);
        }
      }
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            gzt[((2 * wave + mi) * 16 + kg * 4 + r) * LD + nt * 16 + l16] =
                z4[mi][nt][r];
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
    // phase 2a: gx tile = W3^T @ gz via MFMA.  A[m=i][k=j] = W3[k*IT+m],
    // B[n=c][k=j] = gzt[k*LD+n]; K = MT.  A wave's two pairs (m-tiles 0
    // and 1) share the n-tile: one gz fragment per k-step, two chains.
    {
      const int n = wave * 16 + l16;
      const float* a0p = W3f + lane * 4;
      const float* a1p = W3g + (kg * 4 + (l16 & 3)) * 4;
      f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
      for (int g = 0; g < MT / 16; ++g) {
        const float4 a0 = *reinterpret_cast<const float4*>(a0p + g * 256);
        const float4 a1 = *reinterpret_cast<const float4*>(a1p + g * 64);
        const float a0e[4] = {a0.x, a0.y, a0.z, a0.w};
        const float a1e[4] = {a1.x, a1.y, a1.z, a1.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float bb = gzt[(16 * g + 4 * e + kg) * LD + n];
          c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0e[e], bb, c0, 0, 0, 0);
          c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1e[e], bb, c1, 0, 0, 0);
        }
      }
      const long sc = s0 + n;
      if (sc < S) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          st(gx + ((long)b * IT + kg * 4 + r) * S + sc, c0[r]);
          if (16 + kg * 4 + r < IT)
            st(gx + ((long)b * IT + 16 + kg * 4 + r) * S + sc, c1[r]);
        }
      }
    }
    // phase 2b: gW3 fragments += gz_tile @ x_tile^T (reads only; the
    // tile loop's top sync fences the next staging pass).  A wave's four
    // pairs share the x n-tile: one x fragment per k-step, four chains.
    {
      const float* gr = gzt + ((wave >> 1) * 16 + l16) * LD + 4 * kg;
      const float* xr =
          xt + min((wave & 1) * 16 + l16, IT - 1) * LD + 4 * kg;
#pragma unroll 2
      for (int g = 0; g < TS / 16; ++g) {
        const float4 xb = *reinterpret_cast<const float4*>(xr + 16 * g);
        const float xe[4] = {xb.x, xb.y, xb.z, xb.w};
        float4 ga[4];
#pragma unroll
        for (int pp = 0; pp < 4; ++pp)
          ga[pp] = *reinterpret_cast<const float4*>(gr + pp * 32 * LD + 16 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
          for (int pp = 0; pp < 4; ++pp) {
            const float ge[4] = {ga[pp].x, ga[pp].y, ga[pp].z, ga[pp].w};
            wacc[pp] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                ge[e], xe[e], wacc[pp], 0, 0, 0);
          }
        }
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

// ---- host side ----

// x [B,I,S], W3 [M,I], b3 [M], W4 [O2,M] and b4 [O2] (forward) or gy [B,O2,S]
// (backward).  I and O2 size the per-thread register tiles, M the hidden
// walk and, with them, the LDS of proj_head_bwd_kernel: an out-of-range call
// raises in proj_dims, never launches.
struct ProjDims {
  int B, I, M, O2;
  long S;
  // the shape with compile-time M / I kernels, the bf16 forward and the
  // fused backward
  bool pinned() const { return I == 20 && M == 128 && O2 <= 2; }
  // dynamic LDS of proj_head_bwd_kernel, in its layout order: W3l [M*I],
  // b3l [M], W4l [O2*M], the per-wave partials gb3w [4*M] and gW4w [4*O2*M]
  // (ops/projhead.py, proj_head_bwd_lds, states the same sum)
  size_t bwd_lds(size_t elem) const {
    const size_t m = (size_t)M;
    return elem * (m * I + m + O2 * m + 4 * m + 4 * O2 * m);
  }
};
constexpr size_t kBwdLdsLimit = 160 * 1024;

ProjDims proj_dims(const at::Tensor& x, const at::Tensor& W3,
                   const at::Tensor& b3, const at::Tensor& W4,
                   const at::Tensor& last, bool last_is_gy) {
  const auto st = x.scalar_type();
  TORCH_CHECK(st == at::kFloat || st == at::kDouble || st == at::kBFloat16,
              "proj_head: x must be float32/float64/bfloat16");
  TORCH_CHECK(x.dim() == 3 && W3.dim() == 2 && b3.dim() == 1 && W4.dim() == 2,
              "proj_head: x [B,I,S], W3 [M,I], b3 [M], W4 [O2,M]");
  for (const at::Tensor* t : {&x, &W3, &b3, &W4, &last}) {
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() && t->scalar_type() == st,
                "proj_head: contiguous GPU tensors of one dtype");
  }
  const long B = x.size(0), I = x.size(1), S = x.size(2);
  const long M = W3.size(0), O2 = W4.size(0);
  TORCH_CHECK(W3.size(1) == I && b3.size(0) == M && W4.size(1) == M,
              "proj_head shapes");
  if (last_is_gy) {
    TORCH_CHECK(last.dim() == 3 && last.size(0) == B && last.size(1) == O2 &&
                last.size(2) == S, "proj_head: gy must be [B,O2,S]");
  } else {
    TORCH_CHECK(last.dim() == 1 && last.size(0) == O2, "proj_head shapes");
  }
  TORCH_CHECK(I >= 1 && I <= 32 && O2 >= 1 && O2 <= 8 && M >= 1 && M <= 512,
              "proj_head: unsupported dims (I <= 32, M <= 512, O2 <= 8)");
  TORCH_CHECK(B < (1L << 31), "proj_head: batch too large");
  return {(int)B, (int)I, (int)M, (int)O2, S};
}

// Rows of the per-thread kernels, first match wins:
//   pinned 20 -> 128 -> (<= 2)   <IMAX 24, O2MAX 2, MT 128, IT 20>
//   I <= 24, O2 <= 2             <24, 2>, runtime M / I
//   the rest, to the caps        <32, 8>, runtime M / I
// each with VECTOR (float4 IO: fp32, S % 4 == 0, 16-byte aligned bases) or
// element-wise; fp64 has the element-wise form only and bf16 IO only the
// pinned element-wise forward (its backward is proj_head_bwd_fused).
struct ProjRow { int imax, o2max, mt, it; };
constexpr ProjRow kProjRows[] = {{24, 2, 128, 20}, {24, 2, 0, 0}, {32, 8, 0, 0}};

template <typename F>
void with_proj_row(const ProjDims& d, F&& f) {
  const int row = d.pinned() ? 0 : (d.I <= 24 && d.O2 <= 2) ? 1 : 2;
  select_eq<0, 1, 2>(row, f);
}
template <typename T, typename F>
void with_vector(bool vec, F&& f) {
  if constexpr (std::is_same_v<T, float>) select_bool(vec, f);
  else f(std::false_type{});
}

// both per-thread kernels: one thread per 4 s-columns, at most 8 blocks per CU
int proj_grid(const ProjDims& d) {
  return launch_grid((long)d.B * ((d.S + 3) / 4), kBlock, 256L * 8);
}

// T: math and weight type, TIO: storage type of x / out
template <typename T, typename TIO>
void launch_proj_fwd(const ProjDims& d, const at::Tensor& x,
                     const at::Tensor& W3, const at::Tensor& b3,
                     const at::Tensor& W4, const at::Tensor& b4,
                     at::Tensor& out) {
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  auto launch = [&](auto r, auto v) {
    constexpr ProjRow R = kProjRows[decltype(r)::value];
    hipLaunchKernelGGL(
        (proj_head_fwd_kernel<T, R.imax, R.o2max, 4, decltype(v)::value, R.mt,
                              R.it, TIO>),
        dim3(proj_grid(d)), dim3(kBlock), 0, stream,
        static_cast<const TIO*>(x.data_ptr()), W3.data_ptr<T>(),
        b3.data_ptr<T>(), W4.data_ptr<T>(), b4.data_ptr<T>(),
        static_cast<TIO*>(out.data_ptr()), d.B, d.I, d.M, d.O2, d.S);
  };
  if constexpr (!std::is_same_v<T, TIO>) {
    launch(int_c<0>{}, std::false_type{});     // bf16 IO: the pinned row
  } else {
    const bool vec = d.S % 4 == 0 && aligned16(x.data_ptr()) &&
                     aligned16(out.data_ptr());
    with_proj_row(d, [&](auto r) {
      with_vector<T>(vec, [&](auto v) { launch(r, v); });
    });
  }
  DFNO_CHECK_LAUNCH("proj_head");
}

template <typename T>
void launch_proj_bwd(const ProjDims& d, const at::Tensor& gy,
                     const at::Tensor& x, const at::Tensor& W3,
                     const at::Tensor& b3, const at::Tensor& W4,
                     at::Tensor& gz3, at::Tensor& gb3, at::Tensor& gW4,
                     at::Tensor& gb4) {
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  const bool vec = d.S % 4 == 0 && aligned16(x.data_ptr()) &&
                   aligned16(gy.data_ptr()) && aligned16(gz3.data_ptr());
  with_proj_row(d, [&](auto r) {
    with_vector<T>(vec, [&](auto v) {
      constexpr ProjRow R = kProjRows[decltype(r)::value];
      hipLaunchKernelGGL(
          (proj_head_bwd_kernel<T, R.imax, R.o2max, 4, decltype(v)::value, R.mt,
                                R.it>),
          dim3(proj_grid(d)), dim3(kBlock), d.bwd_lds(sizeof(T)), stream,
          gy.data_ptr<T>(), x.data_ptr<T>(), W3.data_ptr<T>(),
          b3.data_ptr<T>(), W4.data_ptr<T>(), gz3.data_ptr<T>(),
          gb3.data_ptr<T>(), gW4.data_ptr<T>(), gb4.data_ptr<T>(), d.B, d.I,
          d.M, d.O2, d.S);
    });
  });
  DFNO_CHECK_LAUNCH("proj_head");
}

// fp32 staging copy of a bf16 weight (the tensor itself when it is fp32)
at::Tensor f32(const at::Tensor& t) { return t.to(at::kFloat); }

}  // namespace

at::Tensor proj_head_fwd(const at::Tensor& x, const at::Tensor& W3,
                         const at::Tensor& b3, const at::Tensor& W4,
                         const at::Tensor& b4) {
  const ProjDims d = proj_dims(x, W3, b3, W4, b4, false);
  const bool bf16 = x.scalar_type() == at::kBFloat16;
  TORCH_CHECK(!bf16 || d.pinned(), "proj_head_fwd: flagship shape only");
  auto out = at::empty({d.B, d.O2, d.S}, x.options());
  if (x.numel() == 0) return out;
  if (bf16)     // bf16 activations, fp32 weights and math
    launch_proj_fwd<float, unsigned short>(d, x, f32(W3), f32(b3), f32(W4),
                                           f32(b4), out);
  else if (x.scalar_type() == at::kDouble)
    launch_proj_fwd<double, double>(d, x, W3, b3, W4, b4, out);
  else
    launch_proj_fwd<float, float>(d, x, W3, b3, W4, b4, out);
  return out;
}

std::vector<at::Tensor> proj_head_bwd(const at::Tensor& gy, const at::Tensor& x,
                                      const at::Tensor& W3, const at::Tensor& b3,
                                      const at::Tensor& W4) {
  check_real(x, "x");
  const ProjDims d = proj_dims(x, W3, b3, W4, gy, true);
  TORCH_CHECK(d.bwd_lds(x.element_size()) <= kBwdLdsLimit,
              "proj_head_bwd: LDS overflow");
  auto gz3 = at::empty({d.B, d.M, d.S}, x.options());
  auto gb3 = at::zeros({d.M}, x.options());
  auto gW4 = at::zeros({d.O2, d.M}, x.options());
  auto gb4 = at::zeros({d.O2}, x.options());
  if (x.numel() == 0) return {gz3, gb3, gW4, gb4};
  if (x.scalar_type() == at::kDouble)
    launch_proj_bwd<double>(d, gy, x, W3, b3, W4, gz3, gb3, gW4, gb4);
  else
    launch_proj_bwd<float>(d, gy, x, W3, b3, W4, gz3, gb3, gW4, gb4);
  return {gz3, gb3, gW4, gb4};
}

std::vector<at::Tensor> proj_head_bwd_fused(const at::Tensor& gy,
                                            const at::Tensor& x,
                                            const at::Tensor& W3,
                                            const at::Tensor& b3,
                                            const at::Tensor& W4) {
  const ProjDims d = proj_dims(x, W3, b3, W4, gy, true);
  const bool bf16 = x.scalar_type() == at::kBFloat16;
  TORCH_CHECK(d.pinned() && (bf16 || x.scalar_type() == at::kFloat),
              "proj_head_bwd_fused: flagship shape only");
  auto W3f = f32(W3), b3f = f32(b3), W4f = f32(W4);
  auto fopt = x.options().dtype(at::kFloat);   // weight grads accumulate fp32
  auto gx = at::empty({d.B, d.I, d.S}, x.options());
  auto gW3 = at::zeros({d.M, d.I}, fopt);
  auto gb3 = at::zeros({d.M}, fopt);
  auto gW4 = at::zeros({d.O2, d.M}, fopt);
  auto gb4 = at::zeros({d.O2}, fopt);
  if (x.numel() == 0) return {gx, gW3, gb3, gW4, gb4};

  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  // 64-column tiles, grid-stride with at most 3 blocks per CU (by LDS)
  const long stiles = (d.S + 63) / 64;
  const int grid = (int)std::min((long)d.B * stiles, 768L);
  auto go = [&](auto elem, auto o2t) {     // storage type by example, O2T
    using TIO = decltype(elem);
    constexpr int IT = 20, MT = 128, O2T = decltype(o2t)::value;
    constexpr int TS = 64, LD = TS + 4;
    // the kernel's layout order: gzt [MT][LD], xt [IT][LD], gyt [O2T][TS],
    // W3f + W3g [MT*IT], b3l [MT], W4l [O2T*MT], gb3s [MT], gW4s [O2T*MT]
    constexpr size_t smem = sizeof(float) *
        (MT * LD + IT * LD + O2T * TS + MT * IT + MT + O2T * MT + MT + O2T * MT);
    hipLaunchKernelGGL(
        (proj_head_bwd_fused_kernel<IT, MT, O2T, TIO>), dim3(grid),
        dim3(kBlock), smem, stream, static_cast<const TIO*>(gy.data_ptr()),
        static_cast<const TIO*>(x.data_ptr()), W3f.data_ptr<float>(),
        b3f.data_ptr<float>(), W4f.data_ptr<float>(),
        static_cast<TIO*>(gx.data_ptr()), gW3.data_ptr<float>(),
        gb3.data_ptr<float>(), gW4.data_ptr<float>(), gb4.data_ptr<float>(),
        d.B, d.O2, d.S);
  };
  select_eq<1, 2>(d.O2, [&](auto o2t) {
    if (bf16) go((unsigned short)0, o2t); else go(0.f, o2t);
  });
  DFNO_CHECK_LAUNCH("proj_head_bwd_fused");
  return {gx, gW3, gb3, gW4, gb4};
}
