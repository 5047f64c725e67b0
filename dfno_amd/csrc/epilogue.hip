// gfx950 fused block epilogue: time-axis irfft synthesized on the fly.
//
//   z[b,o,l,t] = sum_i W[o,i] x[b,i,l,t] + pad_irfft(Yt[b,o,l,:])[t]
//   y = gelu_erf(z)
//
// The two-kernel form (dft_c2r_last_kernel writing the full activation, then
// channel_mix_xres_kernel reading it back as the addend) moves the
// activation through HBM twice for nothing: the spectrum line is 2m floats
// where the real line is N (16 vs 30 at the flagship).  Here the block
// stages the kept-mode lines of its tile in LDS (pad_irfft's factors and
// 1/N applied at the staging write, so the arithmetic below is the c2r
// kernel's) and every thread synthesizes its own columns: 2m FMAs per output
// next to the I FMAs of the mix.
//
// Thread mapping: a tile is LT whole lines; thread -> (line, column chunk)
// is FIXED for the kernel's lifetime, so the per-column twiddles are loaded
// once (registers on the pinned path, an LDS table otherwise) and the tile
// is one contiguous run of LT*N floats per channel — consecutive lanes read
// consecutive addresses.  The pinned flagship shape (I=O=20, N=30, m=8) uses
// 2 columns per thread (N even: a float2 never straddles a line) and 17
// lines = 255 of 256 threads.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <algorithm>
#include <vector>

#include "kernels.h"
#include "gelu_math.h"

namespace {

constexpr int kBlock = 256;

// IT/OT/NT/MT > 0 pin I, O, N, m at compile time (full unroll, register
// twiddles, float4 LDS reads); 0 = runtime extents, scalar accesses.
//
// ADJ selects the adjoint mode (rfft_adj_mix below): the register-resident
// columns are gz, W is staged TRANSPOSED, the spectrum is the rfft adjoint's
// input (unit scale, no interior doubling, DC / Nyquist imaginary parts
// kept — dft_c2r_last_kernel with factors=false), and the single output is
// the plain sum: no GELU, no second store.
template <int IMAX, int VEC, int IT, int OT, int NT, int MT, bool ADJ = false>
__global__ __launch_bounds__(kBlock) void irfft_mix_gelu_kernel(
    const float* __restrict__ x, const float* __restrict__ W,
    const float* __restrict__ Yt, const float* __restrict__ tw,
    float* __restrict__ y, float* __restrict__ z,
    int B, int I_, int O_, long L, int N_, int m_, int LT, float scale,
    bool write_z) {
  constexpr bool PIN = NT > 0;
  const int I = IT > 0 ? IT : I_;
  const int O = OT > 0 ? OT : O_;
  const int N = PIN ? NT : N_;
  const int m = PIN ? MT : m_;
  const int M2 = 2 * m;                 // floats per spectrum line
  const long S = L * N;

  extern __shared__ __align__(16) char smem_raw[];
  float* Wl = reinterpret_cast<float*>(smem_raw);          // [O*I]
  float* twl = Wl + (((size_t)O * I + 3) & ~(size_t)3);    // [N*m*2] (!PIN)
  float* Yl = twl + (PIN ? 0 : (((size_t)N * M2 + 3) & ~(size_t)3));
                                                           // [O][LT][2m]
  if constexpr (ADJ) {
    // W is [I, O] in this kernel's roles (the mix's [O, I]): Wl = W^T
    for (int k = threadIdx.x; k < O * I; k += kBlock) {
      const int o = k / I;
      Wl[k] = W[(size_t)(k - o * I) * O + o];
    }
  } else {
    for (int k = threadIdx.x; k < O * I; k += kBlock) Wl[k] = W[k];
  }
  if constexpr (!PIN)
    for (int k = threadIdx.x; k < N * M2; k += kBlock) twl[k] = tw[k];

  // fixed (line, column) role of this thread inside every tile
  const int CPL = N / VEC;              // column chunks per line
  const int line = (int)threadIdx.x / CPL;
  const int t0 = ((int)threadIdx.x - line * CPL) * VEC;
  const bool role = line < LT;

  float twc[PIN ? VEC : 1][PIN ? MT : 1], tws[PIN ? VEC : 1][PIN ? MT : 1];
  if constexpr (PIN) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const float* twj = tw + (size_t)(role ? t0 + v : 0) * M2;
#pragma unroll
      for (int k = 0; k < MT; ++k) {
        twc[v][k] = twj[2 * k];
        tws[v][k] = twj[2 * k + 1];
      }
    }
  }

  const long ntl = (L + LT - 1) / LT;
  for (long tile = blockIdx.x; tile < (long)B * ntl; tile += gridDim.x) {
    const int b = (int)(tile / ntl);
    const long l0 = (tile - (long)b * ntl) * LT;
    const int nl = (int)min((long)LT, L - l0);

    __syncthreads();                    // last tile's readers are done
    // stage the tile's spectrum lines: per channel one contiguous run of
    // nl*2m floats, scaled as dft_c2r_last_kernel scales its registers
    // (interior modes doubled, imaginary part of DC / Nyquist dropped;
    // ADJ: copied as they are, its factors=false)
    const int run = nl * M2;
    if constexpr (PIN) {
      const int run4 = run / 4;         // MT even: float4 = modes (k, k+1)
      for (int idx = threadIdx.x; idx < O * run4; idx += kBlock) {
        const int o = idx / run4;
        const int r4 = idx - o * run4;
        float4 v = *reinterpret_cast<const float4*>(
            Yt + (((long)b * O + o) * L + l0) * M2 + (long)r4 * 4);
        if constexpr (!ADJ) {
          const int k = (r4 * 2) % MT;
          const bool e0 = (k == 0) || (2 * k == NT);
          const bool e1 = (2 * (k + 1) == NT);
          const float f0 = e0 ? scale : 2.0f * scale;
          const float f1 = e1 ? scale : 2.0f * scale;
          v.x = f0 * v.x; v.y = e0 ? 0.0f : f0 * v.y;
          v.z = f1 * v.z; v.w = e1 ? 0.0f : f1 * v.w;
        }
        *reinterpret_cast<float4*>(Yl + (size_t)o * LT * M2 + (size_t)r4 * 4) = v;
      }
    } else {
      for (int idx = threadIdx.x; idx < O * run; idx += kBlock) {
        const int o = idx / run;
        const int r = idx - o * run;
        float v = Yt[(((long)b * O + o) * L + l0) * M2 + r];
        if constexpr (!ADJ) {
          const int k = (r >> 1) % m;
          const bool edge = (k == 0) || (2 * k == N);
          const float f = edge ? scale : 2.0f * scale;
          v = f * v;
          if (edge && (r & 1)) v = 0.0f;
        }
        Yl[(size_t)o * LT * M2 + r] = v;
      }
    }
    __syncthreads();

    if (!role || line >= nl) continue;  // (barriers above are loop-uniform)

    const long s = (l0 + line) * N + t0;
    const float* xb = x + ((long)b * I) * S + s;
    float xr[IMAX][VEC];
#pragma unroll
    for (int i = 0; i < IMAX; ++i) {
      if (i < I) {
        if constexpr (VEC == 2) {
          const float2 v = *reinterpret_cast<const float2*>(xb + (long)i * S);
          xr[i][0] = v.x; xr[i][1] = v.y;
        } else {
#pragma unroll
          for (int v = 0; v < VEC; ++v) xr[i][v] = xb[(long)i * S + v];
        }
      }
    }

    float* yb = y + ((long)b * O) * S + s;
    float* zb = z + ((long)b * O) * S + s;   // dereferenced only if write_z
    const float* yline = Yl + (size_t)line * M2;
#pragma unroll 2
    for (int o = 0; o < (OT > 0 ? OT : 1 << 20); ++o) {
      if (OT == 0 && o >= O) break;
      float acc[VEC], syn[VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) { acc[v] = 0.0f; syn[v] = 0.0f; }
#pragma unroll
      for (int i = 0; i < IMAX; ++i) {
        if (i < I) {
          const float wv = Wl[(size_t)o * I + i];
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc[v] += wv * xr[i][v];
        }
      }
      const float* yo = yline + (size_t)o * LT * M2;
      if constexpr (PIN) {
        float yk[2 * MT];
#pragma unroll
        for (int q = 0; q < MT / 2; ++q) {
          const float4 v = *reinterpret_cast<const float4*>(yo + 4 * q);
          yk[4 * q] = v.x; yk[4 * q + 1] = v.y;
          yk[4 * q + 2] = v.z; yk[4 * q + 3] = v.w;
        }
#pragma unroll
        for (int k = 0; k < MT; ++k) {
#pragma unroll
          for (int v = 0; v < VEC; ++v)
            syn[v] += yk[2 * k] * twc[v][k] - yk[2 * k + 1] * tws[v][k];
        }
      } else {
        for (int k = 0; k < m; ++k) {
          const float yr_ = yo[2 * k], yi_ = yo[2 * k + 1];
#pragma unroll
          for (int v = 0; v < VEC; ++v) {
            const float* twj = twl + (size_t)(t0 + v) * M2;
            syn[v] += yr_ * twj[2 * k] - yi_ * twj[2 * k + 1];
          }
        }
      }
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[v] += syn[v];
      if constexpr (ADJ) {
        if constexpr (VEC == 2) {
          *reinterpret_cast<float2*>(yb + (long)o * S) =
              make_float2(acc[0], acc[1]);
        } else {
#pragma unroll
          for (int v = 0; v < VEC; ++v) yb[(long)o * S + v] = acc[v];
        }
      } else if constexpr (VEC == 2) {
        if (write_z)
          *reinterpret_cast<float2*>(zb + (long)o * S) =
              make_float2(acc[0], acc[1]);
        *reinterpret_cast<float2*>(yb + (long)o * S) =
            make_float2(dfno_gelu::gelu(acc[0]), dfno_gelu::gelu(acc[1]));
      } else {
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          if (write_z) zb[(long)o * S + v] = acc[v];
          yb[(long)o * S + v] = dfno_gelu::gelu(acc[v]);
        }
      }
    }
  }
}

// One dispatch for both modes.  I/O are the KERNEL's roles: I register-
// resident input channels, O output channels (= spectrum channels).
template <bool ADJ>
void launch_irfft_mix(const float* xp, const float* Wp, const float* Yp,
                      const float* twp, float* yp, float* zp, int B, int I,
                      int O, long L, int N, int m, float scale, bool write_z,
                      hipStream_t stream) {
  auto pad4 = [](size_t n) { return (n + 3) & ~(size_t)3; };
  if (I == 20 && O == 20 && N == 30 && m == 8) {
    constexpr int LT = 17;              // 17 lines x 15 float2 = 255 threads
    const long ntiles = (long)B * ((L + LT - 1) / LT);
    const int grid = (int)std::min(ntiles, 256L * 8);
    const size_t smem = sizeof(float) * (pad4(400) + (size_t)20 * LT * 16);
    hipLaunchKernelGGL((irfft_mix_gelu_kernel<20, 2, 20, 20, 30, 8, ADJ>),
                       dim3(grid), dim3(kBlock), smem, stream, xp, Wp, Yp, twp,
                       yp, zp, B, I, O, L, N, m, LT, scale, write_z);
  } else {
    // whole lines per tile, one column per thread; the spectrum tile is
    // capped at 32 KiB so several blocks stay resident per CU
    int LT = kBlock / N;
    const size_t line_bytes = sizeof(float) * (size_t)O * 2 * m;
    LT = (int)std::max<size_t>(1, std::min<size_t>(LT, (32 * 1024) / line_bytes));
    const long ntiles = (long)B * ((L + LT - 1) / LT);
    const int grid = (int)std::min(ntiles, 256L * 8);
    const size_t smem = sizeof(float) * (pad4((size_t)O * I) +
                                         pad4((size_t)N * 2 * m) +
                                         (size_t)O * LT * 2 * m);
#define EPI_GENERIC(CAP)                                                       \
    hipLaunchKernelGGL((irfft_mix_gelu_kernel<CAP, 1, 0, 0, 0, 0, ADJ>),       \
                       dim3(grid), dim3(kBlock), smem, stream, xp, Wp, Yp,     \
                       twp, yp, zp, B, I, O, L, N, m, LT, scale, write_z);
    if (I <= 8) { EPI_GENERIC(8) }
    else if (I <= 16) { EPI_GENERIC(16) }
    else if (I <= 24) { EPI_GENERIC(24) }
    else { EPI_GENERIC(32) }
#undef EPI_GENERIC
  }
}

}  // namespace

std::vector<at::Tensor> irfft_linear_res_gelu_fwd(const at::Tensor& x,
                                                  const at::Tensor& W,
                                                  const at::Tensor& Yt,
                                                  int64_t n_out, bool need_z) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.scalar_type() == at::kFloat,
              "irfft_linear_res_gelu: x must be contiguous fp32 on GPU");
  TORCH_CHECK(W.is_cuda() && W.is_contiguous() && W.scalar_type() == at::kFloat,
              "irfft_linear_res_gelu: W must be contiguous fp32 on GPU");
  TORCH_CHECK(Yt.is_cuda() && Yt.is_contiguous() &&
              Yt.scalar_type() == at::kComplexFloat,
              "irfft_linear_res_gelu: Yt must be contiguous complex64 on GPU");
  TORCH_CHECK(x.dim() == 3 && W.dim() == 2 && Yt.dim() == 4,
              "irfft_linear_res_gelu: x [B,I,S], W [O,I], Yt [B,O,L,m]");
  const int B = (int)x.size(0), I = (int)x.size(1);
  const long S = x.size(2);
  const int O = (int)W.size(0);
  const long L = Yt.size(2);
  const int m = (int)Yt.size(3);
  const int N = (int)n_out;
  TORCH_CHECK((int)W.size(1) == I, "irfft_linear_res_gelu: W/I mismatch");
  TORCH_CHECK(Yt.size(0) == B && (int)Yt.size(1) == O && L * N == S,
              "irfft_linear_res_gelu: Yt shape mismatch");
  TORCH_CHECK(I >= 1 && I <= 64 && O >= 1 && O <= 64 && N >= 1 && N <= 64 &&
              m >= 1 && m <= 32 && m <= N / 2 + 1,
              "irfft_linear_res_gelu: needs I<=64, O<=64, N<=64, m<=min(32,N/2+1)");

  auto y = at::empty({B, O, S}, x.options());
  auto z = need_z ? at::empty({B, O, S}, x.options())
                  : at::empty({0}, x.options());
  if (x.numel() == 0) return {y, z};

  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  auto tw = dfno_twiddle_table(N, m, /*analysis=*/false, x.options());
  const float scale = (float)(1.0 / (double)N);
  if (I > 32) {   // past the register-resident columns: the MFMA wide mix
    wide_irfft_mix(x, W, Yt, tw, y, z, N, /*adj=*/false);
    DFNO_CHECK_LAUNCH("irfft_linear_res_gelu");
    return {y, z};
  }
  float* yp = y.data_ptr<float>();
  float* zp = need_z ? z.data_ptr<float>() : yp;   // never stored through
  launch_irfft_mix<false>(x.data_ptr<float>(), W.data_ptr<float>(),
                          reinterpret_cast<const float*>(Yt.data_ptr()),
                          tw.data_ptr<float>(), yp, zp, B, I, O, L, N, m,
                          scale, need_z, stream);
  DFNO_CHECK_LAUNCH("irfft_linear_res_gelu");
  return {y, z};
}

at::Tensor rfft_adj_mix(const at::Tensor& gz, const at::Tensor& W,
                        const at::Tensor& G, int64_t n) {
  TORCH_CHECK(gz.is_cuda() && gz.is_contiguous() &&
              gz.scalar_type() == at::kFloat,
              "rfft_adj_mix: gz must be contiguous fp32 on GPU");
  TORCH_CHECK(W.is_cuda() && W.is_contiguous() && W.scalar_type() == at::kFloat,
              "rfft_adj_mix: W must be contiguous fp32 on GPU");
  TORCH_CHECK(G.is_cuda() && G.is_contiguous() &&
              G.scalar_type() == at::kComplexFloat,
              "rfft_adj_mix: G must be contiguous complex64 on GPU");
  TORCH_CHECK(gz.dim() == 3 && W.dim() == 2 && G.dim() == 4,
              "rfft_adj_mix: gz [B,O,S], W [O,I], G [B,I,L,m]");
  const int B = (int)gz.size(0), O = (int)gz.size(1);
  const long S = gz.size(2);
  const int I = (int)W.size(1);
  const long L = G.size(2);
  const int m = (int)G.size(3);
  const int N = (int)n;
  TORCH_CHECK((int)W.size(0) == O, "rfft_adj_mix: W/O mismatch");
  TORCH_CHECK(G.size(0) == B && (int)G.size(1) == I && L * N == S,
              "rfft_adj_mix: G shape mismatch");
  // the roles swap against the forward mode: the mix's O channels are the
  // contracted ones (register-resident up to 32, the MFMA wide mix past
  // that), its I channels the outputs
  TORCH_CHECK(O >= 1 && O <= 64 && I >= 1 && I <= 64 && N >= 1 && N <= 64 &&
              m >= 1 && m <= 32 && m <= N / 2 + 1,
              "rfft_adj_mix: needs O<=64, I<=64, N<=64, m<=min(32,N/2+1)");

  auto gx = at::empty({B, I, S}, gz.options());
  if (gz.numel() == 0) return gx;

  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  auto tw = dfno_twiddle_table(N, m, /*analysis=*/false, gz.options());
  if (O > 32) {
    at::Tensor none = at::empty({0}, gz.options());
    wide_irfft_mix(gz, W, G, tw, gx, none, N, /*adj=*/true);
    DFNO_CHECK_LAUNCH("rfft_adj_mix");
    return gx;
  }
  float* gp = gx.data_ptr<float>();
  launch_irfft_mix<true>(gz.data_ptr<float>(), W.data_ptr<float>(),
                         reinterpret_cast<const float*>(G.data_ptr()),
                         tw.data_ptr<float>(), gp, gp, B, /*I=*/O, /*O=*/I, L,
                         N, m, 1.0f, false, stream);
  DFNO_CHECK_LAUNCH("rfft_adj_mix");
  return gx;
}
