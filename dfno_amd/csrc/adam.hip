// gfx950 fused Adam kernels for dfno_amd: the single-tensor step and the
// batched multi-tensor steps (fp32, bf16 parameters, fp8 side table).

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp8.h>
#include <torch/extension.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <map>
#include <vector>

#include "kernels.h"
#include "device_util.h"
#include "adam_update.h"

// ---------------------------------------------------------------------------
// fused Adam step (flat real view; complex params are elementwise-identical
// to their real views under torch's Adam). One vec4 pass over p/g/m/v.
// ---------------------------------------------------------------------------

namespace {

using namespace dfno_io;

constexpr int kBlock = 256;
constexpr long kGridCap = 256L * 8;   // a few blocks per CU, as in pointwise.hip

template <typename T, bool VECTOR>
__global__ void adam_step_kernel(T* __restrict__ p, const T* __restrict__ g,
                                 T* __restrict__ m, T* __restrict__ v,
                                 long n, T lr, T b1, T b2, T eps, T wd,
                                 T c1, T c2) {
  long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  if constexpr (VECTOR && std::is_same<T, float>::value) {
    for (long i = i0; i * 4 < n; i += stride) {
      float4 pv = *reinterpret_cast<float4*>(p + i * 4);
      const float4 gv = *reinterpret_cast<const float4*>(g + i * 4);
      float4 mv = *reinterpret_cast<float4*>(m + i * 4);
      float4 vv = *reinterpret_cast<float4*>(v + i * 4);
      float pr[4] = {pv.x, pv.y, pv.z, pv.w};
      float gr[4] = {gv.x, gv.y, gv.z, gv.w};
      float mr[4] = {mv.x, mv.y, mv.z, mv.w};
      float vr[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float gg = gr[k] + wd * pr[k];
        mr[k] = b1 * mr[k] + (1.f - b1) * gg;
        vr[k] = b2 * vr[k] + (1.f - b2) * gg * gg;
        float mh = mr[k] / c1;
        float vh = vr[k] / c2;
        pr[k] -= lr * mh / (sqrtf(vh) + eps);
      }
      *reinterpret_cast<float4*>(p + i * 4) = make_float4(pr[0], pr[1], pr[2], pr[3]);
      *reinterpret_cast<float4*>(m + i * 4) = make_float4(mr[0], mr[1], mr[2], mr[3]);
      *reinterpret_cast<float4*>(v + i * 4) = make_float4(vr[0], vr[1], vr[2], vr[3]);
    }
  } else {
    for (long i = i0; i < n; i += stride) {
      T gg = g[i] + wd * p[i];
      T mi = b1 * m[i] + (T(1) - b1) * gg;
      T vi = b2 * v[i] + (T(1) - b2) * gg * gg;
      m[i] = mi;
      v[i] = vi;
      T mh = mi / c1;
      T vh = vi / c2;
      p[i] -= lr * mh / (sqrt(vh) + eps);
    }
  }
}

// Multi-tensor Adam: the whole parameter set updates in ONE launch.  The
// pointer/size table travels by value in kernargs (fits: 40 tensors x 48 B
// < the 4 KB kernarg segment); blocks grid-stride over the concatenated
// vec4 index space and locate their tensor with a short uniform search.
constexpr int kAdamMaxT = 40;
struct AdamTab {
  float* p[kAdamMaxT];
  const float* g[kAdamMaxT];
  float* m[kAdamMaxT];
  float* v[kAdamMaxT];
  long end4[kAdamMaxT];   // exclusive prefix sum of n/4 per tensor
  float c1[kAdamMaxT], c2[kAdamMaxT];
  int nt;
};

// fp8 quantize-in-Adam side table (the spectral-weight group): the update
// pass emits the e4m3 copy for the NEXT forward using the PREVIOUS step's
// amax (delayed scaling; e4m3 conversion saturates), and reduces the new
// amax into am_out — re-quantization costs nothing beyond the bytes the
// optimizer already streams (docs/ROADMAP.md item 5).
struct AdamFp8Tab {
  unsigned char* q[kAdamMaxT];
  const float* am_in[kAdamMaxT];
  float* am_out[kAdamMaxT];
};

__global__ __launch_bounds__(kBlock) void adam_multi_kernel(
    AdamTab tab, long total4, float lr, float b1, float b2, float eps,
    float wd) {
  long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  int t = 0;
  for (long i = i0; i < total4; i += stride) {
    while (i >= tab.end4[t]) ++t;          // monotone: i increases
    long base = (t == 0) ? 0 : tab.end4[t - 1];
    long j = (i - base) * 4;
    float4 pv = *reinterpret_cast<float4*>(tab.p[t] + j);
    const float4 gv = *reinterpret_cast<const float4*>(tab.g[t] + j);
    float4 mv = *reinterpret_cast<float4*>(tab.m[t] + j);
    float4 vv = *reinterpret_cast<float4*>(tab.v[t] + j);
    float pr[4] = {pv.x, pv.y, pv.z, pv.w};
    float gr[4] = {gv.x, gv.y, gv.z, gv.w};
    float mr[4] = {mv.x, mv.y, mv.z, mv.w};
    float vr[4] = {vv.x, vv.y, vv.z, vv.w};
    const float c1 = tab.c1[t], c2 = tab.c2[t];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      adam_update(pr[k], gr[k], mr[k], vr[k], lr, b1, b2, eps, wd, c1, c2);
    }
    *reinterpret_cast<float4*>(tab.p[t] + j) = make_float4(pr[0], pr[1], pr[2], pr[3]);
    *reinterpret_cast<float4*>(tab.m[t] + j) = make_float4(mr[0], mr[1], mr[2], mr[3]);
    *reinterpret_cast<float4*>(tab.v[t] + j) = make_float4(vr[0], vr[1], vr[2], vr[3]);
  }
}

// bf16 multi-tensor variant (the bf16 config's linear parameters): bf16
// storage for p/g/m/v (matching torch's state dtype for bf16 params), fp32
// arithmetic, 8-wide vector IO.  Replaces the stock-torch fallback's ~100
// tiny eager launches per step.
struct AdamTabB {
  unsigned short* p[kAdamMaxT];
  const unsigned short* g[kAdamMaxT];
  unsigned short* m[kAdamMaxT];
  unsigned short* v[kAdamMaxT];
  long end8[kAdamMaxT];   // exclusive prefix sum of ceil(n/8) per tensor
  long nn[kAdamMaxT];     // exact element count (ragged-tail guard)
  float c1[kAdamMaxT], c2[kAdamMaxT];
  int nt;
};

__global__ __launch_bounds__(kBlock) void adam_multi_bf16_kernel(
    AdamTabB tab, long total8, float lr, float b1, float b2, float eps,
    float wd) {
  long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  int t = 0;
  for (long i = i0; i < total8; i += stride) {
    while (i >= tab.end8[t]) ++t;
    long base = (t == 0) ? 0 : tab.end8[t - 1];
    long j = (i - base) * 8;
    const float c1 = tab.c1[t], c2 = tab.c2[t];
    if (j + 8 <= tab.nn[t]) {
      float pr[8], gr[8], mr[8], vr[8];
      load8(tab.p[t] + j, pr);
      load8(tab.g[t] + j, gr);
      load8(tab.m[t] + j, mr);
      load8(tab.v[t] + j, vr);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        adam_update(pr[k], gr[k], mr[k], vr[k], lr, b1, b2, eps, wd, c1, c2);
      }
      store8(tab.p[t] + j, pr);
      store8(tab.m[t] + j, mr);
      store8(tab.v[t] + j, vr);
    } else {
      for (long e = j; e < tab.nn[t]; ++e) {   // ragged tail, scalar
        float pv = __uint_as_float(((unsigned int)tab.p[t][e]) << 16);
        float gv = __uint_as_float(((unsigned int)tab.g[t][e]) << 16);
        float mv = __uint_as_float(((unsigned int)tab.m[t][e]) << 16);
        float vv = __uint_as_float(((unsigned int)tab.v[t][e]) << 16);
        adam_update(pv, gv, mv, vv, lr, b1, b2, eps, wd, c1, c2);
        __hip_bfloat16 hp = __float2bfloat16(pv);
        __hip_bfloat16 hm = __float2bfloat16(mv);
        __hip_bfloat16 hv = __float2bfloat16(vv);
        tab.p[t][e] = *reinterpret_cast<unsigned short*>(&hp);
        tab.m[t][e] = *reinterpret_cast<unsigned short*>(&hm);
        tab.v[t][e] = *reinterpret_cast<unsigned short*>(&hv);
      }
    }
  }
}

// Uniform-size variant: a group of SAME-length tensors (the 32 spectral
// corner weights dominate the parameter set) updates with blockIdx.y as the
// tensor index — no per-iteration tensor search / end4 kernarg loads at all
// (docs/ROADMAP.md item 4: runtime-trip-count folding for the Adam loop).
template <bool QOUT>
__global__ __launch_bounds__(kBlock) void adam_multi_uniform_kernel(
    AdamTab tab, AdamFp8Tab qt, long n4, float lr, float b1, float b2,
    float eps, float wd) {
  const int t = blockIdx.y;
  float* __restrict__ p = tab.p[t];
  const float* __restrict__ g = tab.g[t];
  float* __restrict__ m = tab.m[t];
  float* __restrict__ v = tab.v[t];
  const float c1 = tab.c1[t], c2 = tab.c2[t];
  float inv = 0.f, amax = 0.f;
  if constexpr (QOUT) inv = 448.f / fmaxf(*qt.am_in[t], 1e-30f);
  long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (long i = i0; i < n4; i += stride) {
    long j = i * 4;
    float4 pv = *reinterpret_cast<float4*>(p + j);
    const float4 gv = *reinterpret_cast<const float4*>(g + j);
    float4 mv = *reinterpret_cast<float4*>(m + j);
    float4 vv = *reinterpret_cast<float4*>(v + j);
    float pr[4] = {pv.x, pv.y, pv.z, pv.w};
    float gr[4] = {gv.x, gv.y, gv.z, gv.w};
    float mr[4] = {mv.x, mv.y, mv.z, mv.w};
    float vr[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      adam_update(pr[k], gr[k], mr[k], vr[k], lr, b1, b2, eps, wd, c1, c2);
    }
    *reinterpret_cast<float4*>(p + j) = make_float4(pr[0], pr[1], pr[2], pr[3]);
    *reinterpret_cast<float4*>(m + j) = make_float4(mr[0], mr[1], mr[2], mr[3]);
    *reinterpret_cast<float4*>(v + j) = make_float4(vr[0], vr[1], vr[2], vr[3]);
    if constexpr (QOUT) {
      uchar4 qb;
      __hip_fp8_e4m3 h0(pr[0] * inv), h1(pr[1] * inv), h2(pr[2] * inv),
          h3(pr[3] * inv);
      qb.x = h0.__x; qb.y = h1.__x; qb.z = h2.__x; qb.w = h3.__x;
      *reinterpret_cast<uchar4*>(qt.q[t] + j) = qb;
#pragma unroll
      for (int k = 0; k < 4; ++k) amax = fmaxf(amax, fabsf(pr[k]));
    }
  }
  if constexpr (QOUT) {
    // block-reduce the new amax, one device atomicMax per block
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
      amax = fmaxf(amax, __shfl_down(amax, off, 64));
    __shared__ float wred[4];
    if ((threadIdx.x & 63) == 0) wred[threadIdx.x >> 6] = amax;
    __syncthreads();
    if (threadIdx.x == 0) {
      amax = fmaxf(fmaxf(wred[0], wred[1]), fmaxf(wred[2], wred[3]));
      atomicMax(reinterpret_cast<unsigned int*>(qt.am_out[t]),
                __float_as_uint(amax));
    }
  }
}

}  // namespace

static std::vector<int64_t> adam_step_batch_impl(
    std::vector<at::Tensor>& ps, std::vector<at::Tensor>& gs,
    std::vector<at::Tensor>& ms, std::vector<at::Tensor>& vs,
    double lr, double beta1, double beta2, double eps,
    double weight_decay, std::vector<int64_t>& steps,
    std::vector<at::Tensor>* qs, std::vector<at::Tensor>* am_ins,
    std::vector<at::Tensor>* am_outs) {
  TORCH_CHECK(ps.size() == gs.size() && ps.size() == ms.size() &&
              ps.size() == vs.size() && ps.size() == steps.size(),
              "adam batch: length mismatch");
  std::vector<int64_t> quantized;
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();

  // bucket vec4-eligible tensors by length: same-size groups (>= 2) take
  // the uniform kernel, the ragged rest the searched multi-tensor kernel;
  // bf16 tensors batch into the bf16 multi-tensor kernel
  std::vector<size_t> vec_idx;
  std::map<long, std::vector<size_t>> by_len;
  AdamTabB btab;
  btab.nt = 0;
  long btotal8 = 0;
  auto flush_bf16 = [&]() {
    if (btab.nt == 0) return;
    int grid = launch_grid(btotal8, kBlock, kGridCap);
    hipLaunchKernelGGL(adam_multi_bf16_kernel, dim3(grid), dim3(kBlock), 0,
                       stream, btab, btotal8, (float)lr, (float)beta1,
                       (float)beta2, (float)eps, (float)weight_decay);
    btab.nt = 0;
    btotal8 = 0;
  };
  for (size_t i = 0; i < ps.size(); ++i) {
    long n = ps[i].numel();
    bool aligned = ((reinterpret_cast<uintptr_t>(ps[i].data_ptr()) & 15) == 0) &&
                   ((reinterpret_cast<uintptr_t>(gs[i].data_ptr()) & 15) == 0) &&
                   ((reinterpret_cast<uintptr_t>(ms[i].data_ptr()) & 15) == 0) &&
                   ((reinterpret_cast<uintptr_t>(vs[i].data_ptr()) & 15) == 0);
    if (ps[i].scalar_type() == at::kBFloat16 && n > 0 && aligned) {
      int t = btab.nt++;
      btab.p[t] = reinterpret_cast<unsigned short*>(ps[i].data_ptr());
      btab.g[t] = reinterpret_cast<const unsigned short*>(gs[i].data_ptr());
      btab.m[t] = reinterpret_cast<unsigned short*>(ms[i].data_ptr());
      btab.v[t] = reinterpret_cast<unsigned short*>(vs[i].data_ptr());
      btotal8 += (n + 7) / 8;
      btab.end8[t] = btotal8;
      btab.nn[t] = n;
      btab.c1[t] = (float)(1.0 - std::pow(beta1, (double)steps[i]));
      btab.c2[t] = (float)(1.0 - std::pow(beta2, (double)steps[i]));
      if (btab.nt == kAdamMaxT) flush_bf16();
      continue;
    }
    bool vec = ps[i].scalar_type() == at::kFloat && (n % 4 == 0) && n > 0 &&
               aligned;
    if (!vec) {  // rare: odd-sized or fp64 tensor keeps the single-tensor path
      adam_step_(ps[i], gs[i], ms[i], vs[i], lr, beta1, beta2, eps,
                 weight_decay, steps[i]);
      continue;
    }
    by_len[n].push_back(i);
  }
  flush_bf16();

  auto fill = [&](AdamTab& tab, size_t i, int t) {
    tab.p[t] = ps[i].data_ptr<float>();
    tab.g[t] = gs[i].data_ptr<float>();
    tab.m[t] = ms[i].data_ptr<float>();
    tab.v[t] = vs[i].data_ptr<float>();
    tab.c1[t] = (float)(1.0 - std::pow(beta1, (double)steps[i]));
    tab.c2[t] = (float)(1.0 - std::pow(beta2, (double)steps[i]));
  };

  AdamTab rag;
  rag.nt = 0;
  long total4 = 0;
  auto flush_ragged = [&]() {
    if (rag.nt == 0) return;
    int grid = launch_grid(total4, kBlock, kGridCap);
    hipLaunchKernelGGL(adam_multi_kernel, dim3(grid), dim3(kBlock), 0, stream,
                       rag, total4, (float)lr, (float)beta1, (float)beta2,
                       (float)eps, (float)weight_decay);
    rag.nt = 0;
    total4 = 0;
  };

  for (auto& [n, idxs] : by_len) {
    if (idxs.size() < 2) {
      for (size_t i : idxs) {
        int t = rag.nt++;
        fill(rag, i, t);
        total4 += n / 4;
        rag.end4[t] = total4;
        if (rag.nt == kAdamMaxT) flush_ragged();
      }
      continue;
    }
    long n4 = n / 4;
    for (size_t off = 0; off < idxs.size(); off += kAdamMaxT) {
      AdamTab tab;
      AdamFp8Tab qt{};
      int cnt = (int)std::min<size_t>(kAdamMaxT, idxs.size() - off);
      bool all_q = qs != nullptr;
      for (int t = 0; t < cnt; ++t) {
        size_t i = idxs[off + t];
        fill(tab, i, t);
        if (all_q && (*qs)[i].defined() && (*qs)[i].numel() > 0) {
          qt.q[t] = reinterpret_cast<unsigned char*>((*qs)[i].data_ptr());
          qt.am_in[t] = (*am_ins)[i].data_ptr<float>();
          qt.am_out[t] = (*am_outs)[i].data_ptr<float>();
        } else {
          all_q = false;
        }
      }
      tab.nt = cnt;
      // size grid.x so that grid.x * cnt covers the chip at ~8 blocks/CU
      long gx = (n4 + kBlock - 1) / kBlock;
      long cap = std::max(1L, (256L * 8) / cnt);
      if (gx > cap) gx = cap;
      if (all_q) {
        for (int t = 0; t < cnt; ++t) quantized.push_back((int64_t)idxs[off + t]);
        hipLaunchKernelGGL(adam_multi_uniform_kernel<true>, dim3((int)gx, cnt),
                           dim3(kBlock), 0, stream, tab, qt, n4, (float)lr,
                           (float)beta1, (float)beta2, (float)eps,
                           (float)weight_decay);
      } else {
        hipLaunchKernelGGL(adam_multi_uniform_kernel<false>, dim3((int)gx, cnt),
                           dim3(kBlock), 0, stream, tab, qt, n4, (float)lr,
                           (float)beta1, (float)beta2, (float)eps,
                           (float)weight_decay);
      }
    }
  }
  flush_ragged();
  hipError_t lerr = hipGetLastError();
  TORCH_CHECK(lerr == hipSuccess, "adam_multi launch failed: ",
              hipGetErrorString(lerr));
  return quantized;
}

void adam_step_batch_(std::vector<at::Tensor> ps, std::vector<at::Tensor> gs,
                      std::vector<at::Tensor> ms, std::vector<at::Tensor> vs,
                      double lr, double beta1, double beta2, double eps,
                      double weight_decay, std::vector<int64_t> steps) {
  adam_step_batch_impl(ps, gs, ms, vs, lr, beta1, beta2, eps, weight_decay,
                       steps, nullptr, nullptr, nullptr);
}

std::vector<int64_t> adam_step_batch_fp8_(
    std::vector<at::Tensor> ps, std::vector<at::Tensor> gs,
    std::vector<at::Tensor> ms, std::vector<at::Tensor> vs,
    double lr, double beta1, double beta2, double eps, double weight_decay,
    std::vector<int64_t> steps, std::vector<at::Tensor> qs,
    std::vector<at::Tensor> am_ins, std::vector<at::Tensor> am_outs) {
  TORCH_CHECK(qs.size() == ps.size() && am_ins.size() == ps.size() &&
              am_outs.size() == ps.size(), "adam fp8: list size mismatch");
  // returns the indices whose e4m3 copies were refreshed in-kernel
  return adam_step_batch_impl(ps, gs, ms, vs, lr, beta1, beta2, eps,
                              weight_decay, steps, &qs, &am_ins, &am_outs);
}

void adam_step_(at::Tensor& p, const at::Tensor& g, at::Tensor& m, at::Tensor& v,
                double lr, double beta1, double beta2, double eps,
                double weight_decay, int64_t step) {
  check_real(p, "p"); check_real(g, "g"); check_real(m, "m"); check_real(v, "v");
  long n = p.numel();
  TORCH_CHECK(g.numel() == n && m.numel() == n && v.numel() == n, "adam: size mismatch");
  if (n == 0) return;
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  double c1 = 1.0 - std::pow(beta1, (double)step);
  double c2 = 1.0 - std::pow(beta2, (double)step);
  AT_DISPATCH_FLOATING_TYPES(p.scalar_type(), "adam_step_", [&] {
    bool vec = std::is_same<scalar_t, float>::value && (n % 4 == 0) &&
               ((reinterpret_cast<uintptr_t>(p.data_ptr()) & 15) == 0) &&
               ((reinterpret_cast<uintptr_t>(g.data_ptr()) & 15) == 0) &&
               ((reinterpret_cast<uintptr_t>(m.data_ptr()) & 15) == 0) &&
               ((reinterpret_cast<uintptr_t>(v.data_ptr()) & 15) == 0);
    int grid = launch_grid(vec ? (n + 3) / 4 : n, kBlock, kGridCap);
    if (vec) {
      hipLaunchKernelGGL((adam_step_kernel<scalar_t, true>), dim3(grid), dim3(kBlock),
                         0, stream, p.data_ptr<scalar_t>(), g.data_ptr<scalar_t>(),
                         m.data_ptr<scalar_t>(), v.data_ptr<scalar_t>(), n,
                         (scalar_t)lr, (scalar_t)beta1, (scalar_t)beta2,
                         (scalar_t)eps, (scalar_t)weight_decay,
                         (scalar_t)c1, (scalar_t)c2);
    } else {
      hipLaunchKernelGGL((adam_step_kernel<scalar_t, false>), dim3(grid), dim3(kBlock),
                         0, stream, p.data_ptr<scalar_t>(), g.data_ptr<scalar_t>(),
                         m.data_ptr<scalar_t>(), v.data_ptr<scalar_t>(), n,
                         (scalar_t)lr, (scalar_t)beta1, (scalar_t)beta2,
                         (scalar_t)eps, (scalar_t)weight_decay,
                         (scalar_t)c1, (scalar_t)c2);
    }
  });
}
