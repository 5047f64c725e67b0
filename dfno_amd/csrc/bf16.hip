// gfx950 bf16-storage grad-W kernels (the bf16 compute config,
// BASELINE.json config #2 / VERDICT.md round-1 item 3).
//
// Storage is bf16, arithmetic and the gW/gb accumulators are fp32 (atomics
// on an fp32 staging buffer).  The bf16 channel mixes and elementwise
// epilogues are instantiations of the kernels in pointwise.hip.
//
// Kernels:
//  * bf16_gw: split-s grad-W/grad-bias outer-product reduction.
//  * bf16_gw_mfma: the same contraction on the matrix cores.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <torch/extension.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include "kernels.h"
#include "device_util.h"

namespace {

using namespace dfno_io;

constexpr int kBlock = 256;
constexpr int kVec = 8;   // bf16 per lane per vector op (16 B)

// ---------------------------------------------------------------------------
// grad-W (+grad-bias): gW[o,i] = sum_{b,s} gz[b,o,s] x[b,i,s], fp32 accum.
// LDS-tiled outer product: each s-tile of TS elements is staged (converted
// to fp32, row stride TS+1 so lanes with consecutive i hit distinct banks),
// then every thread owns ceil(O*I/256) fixed (o,i) pairs and accumulates in
// REGISTERS over the tile — no atomics in the hot loop (the first version's
// per-element LDS atomics serialized to 14 ms/launch); one global atomicAdd
// per pair at thread end.
// ---------------------------------------------------------------------------

template <int NP, int XR = 32>
__global__ __launch_bounds__(kBlock) void bf16_gw_kernel(
    const unsigned short* __restrict__ gz, const unsigned short* __restrict__ x,
    float* __restrict__ gW, float* __restrict__ gb,
    int B, int I, int O, long S, bool want_bias) {
  constexpr int TS = 128;          // s-elements per tile
  constexpr int LD = TS + 4;       // row stride: float4 reads stay 16 B-
                                   // aligned, banks spread (132 % 64 = 4)
  constexpr int OSL = 32;          // O-slab per blockIdx.y: caps the LDS
                                   // footprint at (32+32)*132*4 = 33 KiB so
                                   // 4 blocks/CU stay resident (the O=128
                                   // single-slab version ran 1 block/CU)
  extern __shared__ __align__(16) char smem_raw[];
  float* xs = reinterpret_cast<float*>(smem_raw);    // [I <= XR][LD]
  float* gs = xs + (size_t)XR * LD;                  // [O_sl][LD]

  const int o0 = (int)blockIdx.y * OSL;
  const int O_sl = min(OSL, O - o0);

  // fixed (o, i) pairs of this thread within the slab
  int po[NP], pi[NP];
  float acc[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int idx = (int)threadIdx.x + p * kBlock;
    po[p] = idx / I;
    pi[p] = idx - po[p] * I;
    acc[p] = 0.f;
  }
  float accb = 0.f;                // bias partial (thread o = threadIdx.x)

  const long ntiles = (S / TS) * (long)B;   // host guarantees S % TS == 0
  for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int b = (int)(t / (S / TS));
    const long s0 = (t % (S / TS)) * TS;
    // stage: 8 bf16 per thread per instruction, convert to fp32
    for (int r = threadIdx.x; r < (I + O_sl) * (TS / kVec); r += kBlock) {
      const int row = r / (TS / kVec);
      const int col = (r - row * (TS / kVec)) * kVec;
      float v[kVec];
      if (row < I) {
        load8(x + ((long)b * I + row) * S + s0 + col, v);
#pragma unroll
        for (int k = 0; k < kVec; ++k) xs[row * LD + col + k] = v[k];
      } else {
        const int ro = row - I;
        load8(gz + ((long)b * O + o0 + ro) * S + s0 + col, v);
#pragma unroll
        for (int k = 0; k < kVec; ++k) gs[ro * LD + col + k] = v[k];
      }
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      if (po[p] < O_sl) {
        const float* gr = gs + po[p] * LD;
        const float* xr = xs + pi[p] * LD;
#pragma unroll
        for (int k = 0; k < TS; k += 4) {
          const float4 g4 = *reinterpret_cast<const float4*>(gr + k);
          const float4 x4 = *reinterpret_cast<const float4*>(xr + k);
          acc[p] += g4.x * x4.x + g4.y * x4.y + g4.z * x4.z + g4.w * x4.w;
        }
      }
    }
    if (want_bias && (int)threadIdx.x < O_sl) {
      const float* gr = gs + threadIdx.x * LD;
#pragma unroll
      for (int k = 0; k < TS; k += 4) {
        const float4 g4 = *reinterpret_cast<const float4*>(gr + k);
        accb += g4.x + g4.y + g4.z + g4.w;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int p = 0; p < NP; ++p)
    if (po[p] < O_sl) atomicAdd(&gW[(size_t)(o0 + po[p]) * I + pi[p]], acc[p]);
  if (want_bias && (int)threadIdx.x < O_sl)
    atomicAdd(&gb[o0 + threadIdx.x], accb);
}

// ---------------------------------------------------------------------------
// MFMA grad-W: gW[o,i] = sum_s gz[o,s] x[i,s] on v_mfma_f32_16x16x32_bf16.
// The one truly GEMM-shaped hot op of the model (K = S ~ 10^7): the VALU
// version above is arithmetic-limited (~10 flop per bf16-byte at width 20,
// right at the fp32 VALU roofline); the matrix cores run the same contraction
// at the 2.5 PF bf16 rate, making it memory-bound.  Fragment loads need no
// LDS: for both A (gz) and B (x) a lane's 8 k-elements are 8 CONSECUTIVE
// s-positions of one channel row — one 16-byte load each, rows spread over
// lanes (lane groups at k-offsets 0/8/16/24 tile 64 B per row).  Bias falls
// out of one extra MFMA against a ones-column B fragment.
// ---------------------------------------------------------------------------

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bf16x8 load_frag(const unsigned short* row_base,
                                            long k0) {
  // 8 consecutive bf16 at s = k0 (16 B)
  return *reinterpret_cast<const bf16x8*>(row_base + k0);
}

template <int NPAIR>
__global__ __launch_bounds__(kBlock) void bf16_gw_mfma_kernel(
    const unsigned short* __restrict__ gz, const unsigned short* __restrict__ x,
    float* __restrict__ gW, float* __restrict__ gb,
    int B, int I, int O, long S, bool want_bias) {
  constexpr int TS = 256;          // s per grid tile (8 MFMA steps of K=32)
  const int lane = (int)(threadIdx.x & 63);
  const int wave = (int)(threadIdx.x >> 6);
  const int row16 = lane & 15;     // A row / B col within the 16-tile
  const int kgrp = lane >> 4;      // k-group (8 k each)

  const int oT = (O + 15) / 16, iT = (I + 15) / 16;
  const int npairs = oT * iT;      // host guarantees npairs <= 4 * NPAIR

  f32x4 acc[NPAIR];
  f32x4 accb[NPAIR];               // bias (only i-tile 0 pairs contribute)
#pragma unroll
  for (int p = 0; p < NPAIR; ++p) {
    acc[p] = f32x4{0.f, 0.f, 0.f, 0.f};
    accb[p] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  bf16x8 ones = bf16x8{};
  if (kgrp >= 0) {                 // B[k][0] = 1 for the bias column
#pragma unroll
    for (int j = 0; j < 8; ++j) ones[j] = (row16 == 0) ? (__bf16)1.f : (__bf16)0.f;
  }

  const long ntiles = (S / TS) * (long)B;
  for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int b = (int)(t / (S / TS));
    const long s0 = (t % (S / TS)) * TS;
    for (int pp = 0; pp < NPAIR; ++pp) {
      const int p = wave + 4 * pp;
      if (p >= npairs) break;
      const int ot = p / iT, it = p - ot * iT;
      const int o = ot * 16 + row16;
      const int i = it * 16 + row16;
      const unsigned short* gr =
          (o < O) ? gz + ((long)b * O + o) * S + s0 : nullptr;
      const unsigned short* xr =
          (i < I) ? x + ((long)b * I + i) * S + s0 : nullptr;
#pragma unroll
      for (int ks = 0; ks < TS; ks += 32) {
        const long k0 = ks + kgrp * 8;
        bf16x8 a = gr ? load_frag(gr, k0) : bf16x8{};
        bf16x8 bb = xr ? load_frag(xr, k0) : bf16x8{};
        acc[pp] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bb, acc[pp], 0, 0, 0);
        if (want_bias && it == 0)
          accb[pp] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, ones, accb[pp], 0, 0, 0);
      }
    }
  }

  // writeback: D[row][col], row = (lane>>4)*4 + r, col = lane&15
#pragma unroll
  for (int pp = 0; pp < NPAIR; ++pp) {
    const int p = wave + 4 * pp;
    if (p >= npairs) continue;
    const int ot = p / iT, it = p - ot * iT;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = ot * 16 + kgrp * 4 + r;
      const int i = it * 16 + row16;
      if (o < O && i < I) atomicAdd(&gW[(size_t)o * I + i], acc[pp][r]);
      if (want_bias && it == 0 && o < O && row16 == 0)
        atomicAdd(&gb[o], accb[pp][r]);
    }
  }
}

}  // namespace

std::vector<at::Tensor> bf16_channel_mix_bwd_w(const at::Tensor& gz,
                                               const at::Tensor& x,
                                               bool want_bias) {
  check_bf16(gz, "gz"); check_bf16(x, "x");
  const int B = (int)x.size(0);
  const int I = (int)x.size(1);
  const long S = x.size(2);
  const int O = (int)gz.size(1);
  TORCH_CHECK(I <= 64, "bf16 grad-W: I must be <= 64");
  TORCH_CHECK(O <= 128, "bf16 grad-W: O must be <= 128");
  TORCH_CHECK(S % 128 == 0, "bf16 grad-W: S must be a multiple of 128");

  auto opts = x.options().dtype(at::kFloat);
  auto gW = at::zeros({O, I}, opts);
  auto gb = at::zeros({want_bias ? O : 0}, opts);
  if (x.numel() == 0) return {gW, gb};

  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  static const bool no_mfma = []() {
    const char* e = getenv("DFNO_BF16_GW_NO_MFMA");  // A/B knob
    return e && e[0] == '1';
  }();
  const int mfma_pairs = ((O + 15) / 16) * ((I + 15) / 16);
  if (!no_mfma && S % 256 == 0 && mfma_pairs <= 32) {
    long ntiles = (S / 256) * (long)B;
    int grid = (int)std::min(ntiles, 2048L);
    if (mfma_pairs <= 4) {
      hipLaunchKernelGGL((bf16_gw_mfma_kernel<1>), dim3(grid), dim3(kBlock), 0,
                         stream, usp(gz), usp(x), gW.data_ptr<float>(),
                         gb.numel() ? gb.data_ptr<float>() : nullptr, B, I, O,
                         S, want_bias);
    } else if (mfma_pairs <= 16) {
      hipLaunchKernelGGL((bf16_gw_mfma_kernel<4>), dim3(grid), dim3(kBlock), 0,
                         stream, usp(gz), usp(x), gW.data_ptr<float>(),
                         gb.numel() ? gb.data_ptr<float>() : nullptr, B, I, O,
                         S, want_bias);
    } else {   // 33..64 x rows against up to 128 gz rows
      hipLaunchKernelGGL((bf16_gw_mfma_kernel<8>), dim3(grid), dim3(kBlock), 0,
                         stream, usp(gz), usp(x), gW.data_ptr<float>(),
                         gb.numel() ? gb.data_ptr<float>() : nullptr, B, I, O,
                         S, want_bias);
    }
    DFNO_CHECK_LAUNCH("bf16_gw_mfma");
    return {gW, gb};
  }
  constexpr int LD = 132;
  const int nslab = (O + 31) / 32;
  const int o_sl = std::min(O, 32);
  const int xr = I <= 32 ? 32 : 64;
  size_t smem = sizeof(float) * (size_t)(xr + o_sl) * LD;
  long ntiles = (S / 128) * (long)B;
  int grid = (int)std::min(ntiles, 2048L);
  const int pairs = o_sl * I;
#define BGW(NP)                                                                \
  hipLaunchKernelGGL((bf16_gw_kernel<NP>), dim3(grid, nslab), dim3(kBlock),    \
                     smem, stream, usp(gz), usp(x), gW.data_ptr<float>(),      \
                     gb.numel() ? gb.data_ptr<float>() : nullptr, B, I, O, S,  \
                     want_bias);
  if (I > 32) {
    hipLaunchKernelGGL((bf16_gw_kernel<8, 64>), dim3(grid, nslab), dim3(kBlock),
                       smem, stream, usp(gz), usp(x), gW.data_ptr<float>(),
                       gb.numel() ? gb.data_ptr<float>() : nullptr, B, I, O, S,
                       want_bias);
  } else if (pairs <= 256) { BGW(1) } else if (pairs <= 512) { BGW(2) }
  else { BGW(4) }
#undef BGW
  DFNO_CHECK_LAUNCH("bf16_gw");
  return {gW, gb};
}
