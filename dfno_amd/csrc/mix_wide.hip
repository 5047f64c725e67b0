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

// Second pass over the output tile ot[M][kLDO]: a thread owns 4 consecutive
// columns of one row, so a row's 64 columns leave in one contiguous segment.
// v = tile (+ res); z = v (when asked for); y = act ? gelu(v) : v.
template <typename T, int MW, bool VECTOR>
__device__ __forceinline__ void wide_epilogue(
    const float* ot, const T* __restrict__ res, T* __restrict__ y,
    T* __restrict__ z, int b, int M, long S, long s0, bool act) {
#pragma unroll
  for (int q = 0; q < MW * 4; ++q) {
    const int u = (int)threadIdx.x + q * kBlock;
    const int row = u >> 4;
    const int c = (u & 15) * 4;
    if (row < M && s0 + c < S) {
      const float4 o4 = *reinterpret_cast<const float4*>(&ot[row * kLDO + c]);
      float v[4] = {o4.x, o4.y, o4.z, o4.w};
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

// K = contraction depth, M = output rows; W(m, k) = wt ? W[k*M + m] : W[m*K + k].
// KCAP >= K rounded up to 4, MW * 64 >= M.
template <typename T, int KCAP, int MW, bool VECTOR>
__global__ __launch_bounds__(kBlock) void mix_wide_kernel(
    const T* __restrict__ x, const T* __restrict__ W, const T* __restrict__ bias,
    const T* __restrict__ res, T* __restrict__ y, T* __restrict__ z,
    int B, int K, int M, long S, bool wt, bool act) {
  __shared__ __align__(16) float xt[KCAP * kLDX];
  __shared__ __align__(16) float ot[MW * 64 * kLDO];

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
      bv[j][r] = (bias != nullptr && mo < M) ? ld(bias + mo) : 0.f;
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

    wide_epilogue<T, MW, VECTOR>(ot, res, y, z, b, M, S, s0, act);
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
                       a.z, a.B, a.K, a.M, a.S, a.wt, a.act);
  } else if constexpr (std::is_same<T, float>::value) {
    hipLaunchKernelGGL((mix_wide_kernel<T, KCAP, MW, false>), dim3(grid),
                       dim3(kBlock), 0, a.stream, a.x, a.W, a.bias, a.res, a.y,
                       a.z, a.B, a.K, a.M, a.S, a.wt, a.act);
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

}  // namespace

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
