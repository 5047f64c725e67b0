// Fused backward for the trunk 20x20 channel mixes (gfx950, fp32).
//
// The unfused chain per mix-backward is three full-activation kernels:
// gelu_bwd (read gy+z, write gz), channel_mix_fwd_t (read gz, write gx)
// and gw_outer (read gz+x) — ~4.4 GB of HBM traffic at the flagship
// (z/gy/x are [1,20,64^3*30] fp32).  Here gz exists only as a [20 x 64]
// LDS tile computed while staging gy/z; gx = W^T @ gz and
// gW = gz @ x^T (+ gb via a constant ones column) run as
// v_mfma_f32_16x16x4 over the tile, with the gW fragments carried in
// registers across tiles and flushed once per block (atomicAdd, the
// same fp32 reduction-order caveat as every gw kernel here).  When the
// gz tensor itself is a needed gradient (linear_res_gelu's residual
// input), WG=true streams the tile back coalesced — still one pass.
//
// Reference semantics: dfno.py:348-352 (the per-block linear+GELU pair
// around the spectral conv).

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

constexpr int kTile = 64;          // s-columns per tile (16 MFMA K-steps)

// TIO = unsigned short selects bf16 activations (fp32 compute; W and the
// gW/gb accumulators stay fp32).  WG streams the gz tile back to gzout.
// WX = false compiles phase A (gx = W^T gz and its store) out: the caller
// applies W^T to the streamed-back gz itself (rfft_adj_mix, epilogue.hip);
// gx is never touched.
template <typename TIO, bool WG, bool WX>
__global__ __launch_bounds__(kBlock, 4) void mix_bwd_fused_kernel(
    const TIO* __restrict__ gy, const TIO* __restrict__ z,
    const TIO* __restrict__ x, const float* __restrict__ W,
    TIO* __restrict__ gx, float* __restrict__ gW, float* __restrict__ gb,
    TIO* __restrict__ gzout, int B, long S) {
  constexpr int TS = kTile;
  constexpr int C = 20;            // in = out channels (trunk width)
  constexpr int LD = TS + 4;
  extern __shared__ __align__(16) char smem_raw[];
  float* gzt = reinterpret_cast<float*>(smem_raw);   // [C][LD]
  float* xt = gzt + (size_t)C * LD;                  // [C + 1][LD]
  // row C of xt is all ones (phase B's gb column); staging never writes it
  if (threadIdx.x < TS) xt[C * LD + threadIdx.x] = 1.f;

  const int lane = (int)(threadIdx.x & 63);
  const int wave = (int)(threadIdx.x >> 6);
  const int l16 = lane & 15;
  const int kg = lane >> 4;

  // MFMA operands are loaded unconditionally.  Output row m of an MFMA
  // depends only on A row m and output column n only on B column n, and
  // the padded rows and columns (>= C, or > C with the ones row) are
  // dropped at the gx store and at the flush: their lanes read a clamped,
  // in-bounds row instead of a masked zero.
  // phase A's A fragments, W^T for the wave's two m-tiles: tile-invariant
  float wa[2][C / 4];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int ks = 0; ks < C / 4; ++ks)
      wa[mt][ks] = WX ? W[(4 * ks + kg) * C + min(mt * 16 + l16, C - 1)] : 0.f;

  // gW/gb fragments: M = 2 o-tiles, N = 2 tiles (i channels + ones col)
  f32x4 wacc;
  wacc = f32x4{0.f, 0.f, 0.f, 0.f};

  const long stiles = (S + TS - 1) / TS;
  const long tend = (long)B * stiles;
  // register-prefetched staging (proj_head pattern): next tile's gy/z/x
  // fly over this tile's MFMA phases
  constexpr int NPF = (2 * C * TS + kBlock - 1) / kBlock;
  float pfa[NPF], pfb[NPF];        // pfa: x or gy row; pfb: z row
  auto prefetch = [&](long tt) {
    if (tt >= tend) return;
    const int b = (int)(tt / stiles);
    const long s0 = (tt % stiles) * TS;
    const int nv = (int)min((long)TS, S - s0);
#pragma unroll
    for (int q = 0; q < NPF; ++q) {
      const int r = (int)threadIdx.x + q * kBlock;
      const int row = r / TS;
      const int c = r - row * TS;
      float a = 0.f, bb = 0.f;
      if (c < nv) {
        if (row < C) {
          a = ld(x + ((long)b * C + row) * S + s0 + c);
        } else {
          const long off = ((long)b * C + (row - C)) * S + s0 + c;
          a = ld(gy + off);
          bb = ld(z + off);
        }
      }
      pfa[q] = a;
      pfb[q] = bb;
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
      const int row = r / TS;
      const int c = r - row * TS;
      if (row < C) {
        xt[row * LD + c] = pfa[q];
      } else {
        const float gzv = pfa[q] * dfno_gelu::gelu_grad(pfb[q]);
        gzt[(row - C) * LD + c] = gzv;
        if (WG && c < nv)
          st(gzout + ((long)b * C + (row - C)) * S + s0 + c, gzv);
      }
    }
    prefetch(t + gridDim.x);
    __syncthreads();
    // phase A: gx = W^T @ gz.  A[m=i][k=o] = W[o*C+i] (wa, registers),
    // B[n=c][k=o] = gzt[o][c]; K = C (4-aligned).  The wave's two pairs
    // (m-tiles 0 and 1) share n-tile `wave`: one gz fragment per k-step.
    if constexpr (WX) {
      const int n = wave * 16 + l16;
      f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < C / 4; ++ks) {
        const float bb = gzt[(4 * ks + kg) * LD + n];
        c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[0][ks], bb, c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[1][ks], bb, c1, 0, 0, 0);
      }
      const long sc = s0 + n;
      if (sc < S) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          st(gx + ((long)b * C + kg * 4 + r) * S + sc, c0[r]);
          if (16 + kg * 4 + r < C)
            st(gx + ((long)b * C + 16 + kg * 4 + r) * S + sc, c1[r]);
        }
      }
    }
    // phase B: gW fragments += gz @ [x; ones]^T.  One (mt, nt) pair per
    // wave: mt = wave>>1 (o-tiles), nt = wave&1 (i-tiles; col C = the ones
    // row, for gb).  Both operands run along the tile row: lane group kg
    // takes columns 16*g + 4*kg .. +3 in four successive MFMAs, the same k
    // order for A and B, so one ds_read_b128 each serves four k-steps.
    {
      const int mt = wave >> 1, nt = wave & 1;
      const float* gr = gzt + min(mt * 16 + l16, C - 1) * LD + 4 * kg;
      const float* xr = xt + min(nt * 16 + l16, C) * LD + 4 * kg;
#pragma unroll
      for (int g = 0; g < TS / 16; ++g) {
        const float4 a = *reinterpret_cast<const float4*>(gr + 16 * g);
        const float4 bb = *reinterpret_cast<const float4*>(xr + 16 * g);
        wacc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, bb.x, wacc, 0, 0, 0);
        wacc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, bb.y, wacc, 0, 0, 0);
        wacc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, bb.z, wacc, 0, 0, 0);
        wacc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, bb.w, wacc, 0, 0, 0);
      }
    }
  }

  // flush gW/gb fragments.  D[m = o][n]: n < C -> gW[o][n], n == C -> gb[o]
  {
    const int mt = wave >> 1, nt = wave & 1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = mt * 16 + kg * 4 + r;
      const int n = nt * 16 + l16;
      const float v = wacc[r];
      if (o < C && v != 0.f) {
        if (n < C) atomicAdd(&gW[(size_t)o * C + n], v);
        else if (n == C && gb != nullptr) atomicAdd(&gb[o], v);
      }
    }
  }
}

// One launch of mix_bwd_fused_kernel<TIO, WG, WX>: grid-stride over the
// B * ceil(S / 64) tiles with at most 1024 blocks (4 per CU), the gz tile
// [20][68] and the x tile plus its ones row [21][68] fp32 in dynamic LDS.  An output the instantiation never
// stores (gz without WG, gx without WX) goes in as null.
template <typename TIO, bool WG, bool WX>
void launch_mix_bwd(const at::Tensor& gy, const at::Tensor& z,
                    const at::Tensor& x, const at::Tensor& W, at::Tensor& gx,
                    at::Tensor& gW, float* gb, at::Tensor& gz, int B, long S) {
  const long stiles = (S + kTile - 1) / kTile;
  const int grid = (int)std::min((long)B * stiles, 1024L);
  const size_t smem = sizeof(float) * (2 * 20 + 1) * (kTile + 4);
  hipLaunchKernelGGL((mix_bwd_fused_kernel<TIO, WG, WX>), dim3(grid),
                     dim3(kBlock), smem,
                     at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream(),
                     static_cast<const TIO*>(gy.data_ptr()),
                     static_cast<const TIO*>(z.data_ptr()),
                     static_cast<const TIO*>(x.data_ptr()), W.data_ptr<float>(),
                     WX ? static_cast<TIO*>(gx.data_ptr()) : nullptr,
                     gW.data_ptr<float>(), gb,
                     WG ? static_cast<TIO*>(gz.data_ptr()) : nullptr, B, S);
}

}  // namespace

std::vector<at::Tensor> channel_mix_bwd_fused(const at::Tensor& gy,
                                              const at::Tensor& z,
                                              const at::Tensor& x,
                                              const at::Tensor& W,
                                              bool want_bias, bool want_gz,
                                              bool want_gx) {
  const bool bf16 = gy.scalar_type() == at::kBFloat16;
  TORCH_CHECK(gy.is_cuda() && gy.is_contiguous() && z.is_contiguous() &&
              x.is_contiguous() && W.is_contiguous() &&
              (bf16 || gy.scalar_type() == at::kFloat) &&
              x.scalar_type() == gy.scalar_type() &&
              z.scalar_type() == gy.scalar_type() &&
              W.scalar_type() == at::kFloat,
              "mix_bwd_fused: fp32/bf16 activations, fp32 W");
  int B = (int)x.size(0), I = (int)x.size(1);
  long S = x.size(2);
  int O = (int)W.size(0);
  TORCH_CHECK(I == 20 && O == 20, "mix_bwd_fused: trunk 20x20 only");
  TORCH_CHECK(gy.numel() == x.numel() && z.numel() == x.numel(),
              "mix_bwd_fused: shape mismatch");

  TORCH_CHECK(want_gx || want_gz,
              "mix_bwd_fused: want_gx=false needs want_gz (grad-x is then "
              "the caller's W^T gz)");
  auto gx = want_gx ? at::empty({B, I, S}, x.options())
                    : at::empty({0}, x.options());
  auto fopt = x.options().dtype(at::kFloat);   // gW/gb accumulate fp32
  auto gW = at::zeros({O, I}, fopt);
  auto gb = want_bias ? at::zeros({O}, fopt) : at::empty({0}, fopt);
  auto gz = want_gz ? at::empty({B, O, S}, x.options())
                    : at::empty({0}, x.options());
  if (x.numel() == 0) return {gx, gW, gb, gz};

  // Rows: {fp32, bf16} x (gz and gx | gx only | gz only); gz only is the
  // WX = false kernel without phase A.
  float* gbp = want_bias ? gb.data_ptr<float>() : nullptr;
  auto go = [&](auto elem) {            // storage type, by example
    using TIO = decltype(elem);
    select_bool(want_gz, [&](auto wg) {
      select_bool(want_gx, [&](auto wx) {
        constexpr bool WG = decltype(wg)::value, WX = decltype(wx)::value;
        if constexpr (WG || WX)
          launch_mix_bwd<TIO, WG, WX>(gy, z, x, W, gx, gW, gbp, gz, B, S);
      });
    });
  };
  if (bf16) go((unsigned short)0); else go(0.f);
  DFNO_CHECK_LAUNCH("mix_bwd_fused");
  return {gx, gW, gb, gz};
}

