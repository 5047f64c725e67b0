// gfx950 grad-W kernels of the channel mix:
//   gW[o,i] = sum_{b,s} gz[b,o,s] x[b,i,s],  optionally gb[o] = sum_{b,s} gz[b,o,s]
// a GEMM with M, N <= 128 and K = B * S ~ 10^7.  Two entry points:
//  * channel_mix_bwd_w: fp32 / fp64 storage, accumulators and gW in the
//    storage type.  Kernels: gw_outer (generic split-s outer product, also
//    with i-slabs), gw_outer_glds3 (the same behind an LDS DMA ring, fp32),
//    gw_mfma_f32 (fp32 matrix cores, big O * I).
//  * bf16_channel_mix_bwd_w: bf16 storage (BASELINE.json config #2), fp32
//    arithmetic, gW / gb returned in fp32.  Kernels: bf16_gw_mfma (matrix
//    cores, fragments straight from global), bf16_gw (LDS-tiled VALU).
// The host half of each entry point is a decision list over the rows of its
// launch table (docs/DESIGN.md, "Grad-W launch table").

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <torch/extension.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "kernels.h"
#include "device_util.h"
#include "launch_select.h"

namespace {

using namespace dfno_io;

constexpr int kBlock = 256;
constexpr int kVec = 8;   // bf16 per lane per vector op (16 B)

// ---------------------------------------------------------------------------
// grad-W outer-product reduction: gW[o,i] = sum_{b,s} A[b,o,s] B[b,i,s]
// (optionally gb[o] = sum A[b,o,s]).
//
// rocBLAS picks a no-split-K schedule for these M,N<=128 / K~10^7 GEMMs
// (observed: ~2 workgroups on 256 CUs, 3.2 ms for a 1.3 GB reduction); here
// the s axis is split across blocks (grid ordered s-chunk-major so the
// o-tiles sweeping one s-chunk hit L2/L3 on the B re-reads), each wave owns
// one A row with the <=32 B rows accumulated in registers, and partials are
// wave-shuffle-reduced then atomically added into gW once per block.
// ---------------------------------------------------------------------------

template <typename T, int ICAP, int OW, bool BIAS, bool VECTOR, bool ISLAB>
__global__ __launch_bounds__(kBlock) void gw_outer_kernel(
    const T* __restrict__ A, const T* __restrict__ Bm,
    T* __restrict__ gW, T* __restrict__ gb,
    int B, int O, int I_, long S, int n_schunk) {
  static_assert(!VECTOR || std::is_same<T, float>::value, "float4 access is fp32");
  // grid: blockIdx.x = schunk * o_tiles + o_tile (s-chunk-major); each wave
  // owns OW consecutive output rows (cuts B re-reads by OW and raises the
  // fma:load ratio).  ISLAB (I_ > ICAP): blockIdx.y picks the slab of ICAP
  // B rows this block reduces; slab 0 owns the bias.
  const int i0 = ISLAB ? (int)blockIdx.y * ICAP : 0;
  const int I = ISLAB ? min(ICAP, I_ - i0) : I_;   // rows of this slab
  const bool do_bias = BIAS && (!ISLAB || blockIdx.y == 0);
  const int o_tiles = (O + 4 * OW - 1) / (4 * OW);
  const int schunk = blockIdx.x / o_tiles;
  const int o_tile = blockIdx.x % o_tiles;
  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  const int o0 = (o_tile * 4 + wave) * OW;

  // chunk boundaries on 256-element grain so the float4 lanes stay aligned
  long chunk_sz = ((S + n_schunk - 1) / n_schunk + 255) & ~255L;
  long s0 = (long)schunk * chunk_sz;
  long s1 = min(S, s0 + chunk_sz);

  T acc[OW][ICAP];
#pragma unroll
  for (int w = 0; w < OW; ++w)
#pragma unroll
    for (int i = 0; i < ICAP; ++i) acc[w][i] = T(0);
  T bacc[OW];
#pragma unroll
  for (int w = 0; w < OW; ++w) bacc[w] = T(0);

  if (o0 < O) {
    for (int b = 0; b < B; ++b) {
      const T* Ab = A + ((long)b * O + o0) * S;
      const T* Bb = Bm + ((long)b * I_ + i0) * S;
      long se = s0;   // start of the element-by-element part
      if constexpr (VECTOR) {
        const long tail0 = s0 + ((s1 - s0) / (64 * 4)) * (64 * 4);
        for (long s = s0 + (long)lane * 4; s < tail0; s += 64 * 4) {
          float4 av[OW];
#pragma unroll
          for (int w = 0; w < OW; ++w) {
            if (o0 + w < O) {
              av[w] = *reinterpret_cast<const float4*>(Ab + (long)w * S + s);
              if (do_bias) bacc[w] += av[w].x + av[w].y + av[w].z + av[w].w;
            }
          }
#pragma unroll
          for (int i = 0; i < ICAP; ++i) {
            if (i < I) {
              const float4 bv = *reinterpret_cast<const float4*>(Bb + (long)i * S + s);
#pragma unroll
              for (int w = 0; w < OW; ++w) {
                if (o0 + w < O)
                  acc[w][i] += av[w].x * bv.x + av[w].y * bv.y +
                               av[w].z * bv.z + av[w].w * bv.w;
              }
            }
          }
        }
        se = tail0;
      }
      for (long s = se + lane; s < s1; s += 64) {
#pragma unroll
        for (int w = 0; w < OW; ++w) {
          if (o0 + w < O) {
            T av = Ab[(long)w * S + s];
            if (do_bias) bacc[w] += av;
#pragma unroll
            for (int i = 0; i < ICAP; ++i)
              if (i < I) acc[w][i] += av * Bb[(long)i * S + s];
          }
        }
      }
    }
  }

  // flush: wave-reduce each acc, lane 0 atomically accumulates
#pragma unroll
  for (int w = 0; w < OW; ++w) {
    if (o0 + w < O) {
#pragma unroll
      for (int i = 0; i < ICAP; ++i) {
        if (i < I) {
          T v = wave_sum(acc[w][i]);
          if (lane == 0 && v != T(0)) atomicAdd(&gW[(size_t)(o0 + w) * I_ + i0 + i], v);
        }
      }
      if (do_bias) {
        T v = wave_sum(bacc[w]);
        if (lane == 0 && v != T(0)) atomicAdd(&gb[o0 + w], v);
      }
    }
  }
}

// All-glds pipelined variant (fp32).  Both operand tiles (the I<=32 narrow B
// rows AND this block's 4*OW A rows) are staged into a 3-deep LDS ring by
// global_load_lds DMA; the loop keeps exactly one tile's DMA in flight and
// waits for the current tile with a COUNTED s_waitcnt vmcnt(NG) + raw
// s_barrier.  The previous version kept A in registers via ordinary loads:
// hipcc then inserted s_waitcnt vmcnt(0) before every A use (76 of them in
// the unrolled body), draining the in-flight next-tile DMA each step and
// serializing the ring at ~1.8 TB/s.  Counted vmcnt needs a compile-time
// exact per-wave instruction count, so the issue loops are padded to fixed
// trip counts (NB = ICAP/4 for B, OW for A) with out-of-range rows clamped
// to a valid source row; compute masks those lanes out as before.  3
// buffers (not 2) so a tile's DMA lands in a buffer whose last readers are
// two barriers back.  LDS = 3*(ICAP+4*OW)*1KB -> 1-2 blocks/CU; the low
// occupancy is by design, latency hides in the pipeline depth.
template <int ICAP, int OW, int TS>
__global__ __launch_bounds__(kBlock) void gw_outer_glds3_kernel(
    const float* __restrict__ A, const float* __restrict__ Bm,
    float* __restrict__ gW, float* __restrict__ gb,
    int B, int O, int I, long S, int n_schunk, bool want_bias) {
  // TS = floats per s-tile row: bigger rows read longer contiguous HBM
  // bursts per stream (TS=512 -> 2 KB sequential per row per tile).
  static_assert((ICAP * TS) % (kBlock * 4) == 0, "B image must tile evenly");
  static_assert((OW * TS) % 256 == 0, "A image must tile evenly");
  constexpr int NBUF = 3;                       // ring depth
  constexpr int NB = ICAP * TS / (kBlock * 4);  // B glds instrs per wave
  constexpr int NA = OW * TS / 256;             // A glds instrs per wave
  constexpr int NG = NB + NA;                   // per wave per tile
  constexpr int AROWS = 4 * OW;     // A rows staged per block
  constexpr int PASS = TS >= 256 ? TS / 256 : 1;  // compute passes per tile
  __shared__ float ring[NBUF][(ICAP + AROWS) * TS];

  const int o_tiles = (O + 4 * OW - 1) / (4 * OW);
  // XCD-aware decode: workgroups are dealt round-robin to the 8 XCDs, each
  // with its own L2.  All o-tiles of one s-chunk share the B rows, so place
  // them on ONE XCD (ids congruent mod 8): the 2nd..Nth o-tile then reads B
  // from that XCD's L2 instead of re-fetching HBM (gW3's O=128 shape was 16x
  // amplified).  Identity when o_tiles == 1; host rounds n_schunk up to a
  // multiple of 8 when o_tiles > 1 so the decode stays a bijection.
  const int xr = blockIdx.x % 8;
  const int xq = blockIdx.x / 8;
  const int o_tile = xq % o_tiles;
  const int schunk = (xq / o_tiles) * 8 + xr;
  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  const int o0 = (o_tile * 4 + wave) * OW;
  const int ob0 = o_tile * 4 * OW;  // first A row of the whole block

  long chunk_sz = ((S + n_schunk - 1) / n_schunk + (TS - 1)) & ~((long)TS - 1);
  long s0 = (long)schunk * chunk_sz;
  long s1 = min(S, s0 + chunk_sz);
  long full_end = (s0 < s1) ? s0 + ((s1 - s0) / TS) * TS : s0;

  float acc[OW][ICAP];
#pragma unroll
  for (int w = 0; w < OW; ++w)
#pragma unroll
    for (int i = 0; i < ICAP; ++i) acc[w][i] = 0.f;
  float bacc[OW];
#pragma unroll
  for (int w = 0; w < OW; ++w) bacc[w] = 0.f;

  for (int b = 0; b < B; ++b) {
    const float* Ab = A + ((long)b * O + o0) * S;
    const float* Abl = A + ((long)b * O) * S;
    const float* Bb = Bm + ((long)b * I) * S;

    // one tile's DMA: exactly NG glds instructions per wave, every wave.
    auto issue_tile = [&](int buf, long st) {
      float* dst = ring[buf];
#pragma unroll
      for (int k = 0; k < NB; ++k) {            // B rows, lane-linear image
        int slot = wave * 64 + k * kBlock + lane;
        int fo = slot * 4;
        int row = fo / TS, col = fo % TS;
        int srow = row < I ? row : I - 1;       // pad: clamp to a valid row
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)
                (Bb + (long)srow * S + st + col),
            (__attribute__((address_space(3))) void*)&dst[slot * 4],
            16, 0, 0);
      }
#pragma unroll
      for (int k = 0; k < NA; ++k) {            // this wave's own A rows
        int fa = k * 256 + lane * 4;            // flat offset in OW*TS image
        int w = fa / TS, col = fa % TS;
        int row = ob0 + wave * OW + w;
        int srow = row < O ? row : O - 1;
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)
                (Abl + (long)srow * S + st + col),
            (__attribute__((address_space(3))) void*)
                &dst[(ICAP + wave * OW + w) * TS + col],
            16, 0, 0);
      }
    };

    if (s0 < full_end) {
      const long nt = (full_end - s0) / TS;
      issue_tile(0, s0);
      for (long t = 0; t < nt; ++t) {
        if (t + 1 < nt) {
          issue_tile((int)((t + 1) % NBUF), s0 + (t + 1) * TS);
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NG) : "memory");
        } else {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        // raw barrier (no implicit vmcnt drain), fenced so the compiler
        // cannot hoist the LDS reads above it
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const float* cur = ring[t % NBUF];
        if (o0 < O) {
          if constexpr (TS >= 256) {
#pragma unroll
            for (int p = 0; p < PASS; ++p) {
              float4 av[OW];
#pragma unroll
              for (int w = 0; w < OW; ++w) {
                if (o0 + w < O) {
                  av[w] = *reinterpret_cast<const float4*>(
                      &cur[(ICAP + wave * OW + w) * TS + p * 256 + lane * 4]);
                  if (want_bias)
                    bacc[w] += av[w].x + av[w].y + av[w].z + av[w].w;
                }
              }
#pragma unroll
              for (int i = 0; i < ICAP; ++i) {
                if (i < I) {
                  const float4 bv = *reinterpret_cast<const float4*>(
                      &cur[i * TS + p * 256 + lane * 4]);
#pragma unroll
                  for (int w = 0; w < OW; ++w) {
                    if (o0 + w < O)
                      acc[w][i] += av[w].x * bv.x + av[w].y * bv.y +
                                   av[w].z * bv.z + av[w].w * bv.w;
                  }
                }
              }
            }
          } else {                              // TS == 128: float2 per lane
            float2 av[OW];
#pragma unroll
            for (int w = 0; w < OW; ++w) {
              if (o0 + w < O) {
                av[w] = *reinterpret_cast<const float2*>(
                    &cur[(ICAP + wave * OW + w) * TS + lane * 2]);
                if (want_bias) bacc[w] += av[w].x + av[w].y;
              }
            }
#pragma unroll
            for (int i = 0; i < ICAP; ++i) {
              if (i < I) {
                const float2 bv = *reinterpret_cast<const float2*>(
                    &cur[i * TS + lane * 2]);
#pragma unroll
                for (int w = 0; w < OW; ++w) {
                  if (o0 + w < O)
                    acc[w][i] += av[w].x * bv.x + av[w].y * bv.y;
                }
              }
            }
          }
        }
      }
      __syncthreads();  // next b (or tail) may overwrite ring buffers
    }

    // ragged tail of the last (partial) tile, direct from global
    if (o0 < O) {
      for (long s = full_end + lane; s < s1; s += 64) {
#pragma unroll
        for (int w = 0; w < OW; ++w) {
          if (o0 + w < O) {
            float av = Ab[(long)w * S + s];
            if (want_bias) bacc[w] += av;
#pragma unroll
            for (int i = 0; i < ICAP; ++i)
              if (i < I) acc[w][i] += av * Bb[(long)i * S + s];
          }
        }
      }
    }
  }

#pragma unroll
  for (int w = 0; w < OW; ++w) {
    if (o0 + w < O) {
#pragma unroll
      for (int i = 0; i < ICAP; ++i) {
        if (i < I) {
          float v = wave_sum(acc[w][i]);
          if (lane == 0 && v != 0.f) atomicAdd(&gW[(size_t)(o0 + w) * I + i], v);
        }
      }
      if (want_bias) {
        float v = wave_sum(bacc[w]);
        if (lane == 0 && v != 0.f) atomicAdd(&gb[o0 + w], v);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// fp32-MFMA grad-W for big-O shapes (the projection lift's gW3 [128, 20]).
// gW[o,i] = sum_s gz[o,s] x[i,s] is GEMM-shaped with K = S ~ 10^7; the VALU
// glds3 kernel sits at the round-1 "0.9 TB/s per resident block" ceiling
// (2.8 ms at this shape).  v_mfma_f32_16x16x4_f32 runs the identical-
// numerics contraction at the f32 matrix rate with one f32 operand register
// per lane (cdna_hip_programming.md section 3: an untuned f32-MFMA tile
// outruns a VALU f32 GEMM 122 vs 52 TF) — LDS-staged [rows][TS] tiles,
// wave-per-(16x16)-output-tile, fp32 accumulate, atomic flush.
// ---------------------------------------------------------------------------

typedef float f32x4_pw __attribute__((ext_vector_type(4)));

template <int NPAIR, int XR = 32, int OSL = 64, bool BIAS = false>
__global__ __launch_bounds__(kBlock) void gw_mfma_f32_kernel(
    const float* __restrict__ gz, const float* __restrict__ x,
    float* __restrict__ gW, int B, int O, int I, long S,
    float* __restrict__ gb = nullptr) {
  constexpr int TS = 128;          // s per tile (32 MFMA K-steps)
  constexpr int LD = TS + 4;       // float4-aligned row pad
  // OSL: o-rows per blockIdx.y slab; XR: x-row capacity (I <= XR).  The
  // I <= 64 instantiation halves the slab, keeping the tile pair near 50 KB.
  // BIAS: B column I is a constant one, so D column I is gb (as in
  // mix_bwd_fused); o-slabs partition the rows, each gb[o] has one owner.
  extern __shared__ __align__(16) char smem_raw[];
  float* xs = reinterpret_cast<float*>(smem_raw);    // [I<=XR][LD]
  float* gs = xs + (size_t)XR * LD;                  // [O_sl][LD]

  const int o0 = (int)blockIdx.y * OSL;
  const int O_sl = min(OSL, O - o0);
  const int iT = (I + (BIAS ? 1 : 0) + 15) / 16;
  const int npairs = ((O_sl + 15) / 16) * iT;

  const int lane = (int)(threadIdx.x & 63);
  const int wave = (int)(threadIdx.x >> 6);
  const int l16 = lane & 15;
  const int kg = lane >> 4;        // k-group within the MFMA K=4

  f32x4_pw acc[NPAIR];
#pragma unroll
  for (int p = 0; p < NPAIR; ++p) acc[p] = f32x4_pw{0.f, 0.f, 0.f, 0.f};

  const long ntiles = (S / TS) * (long)B;
  for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int b = (int)(t / (S / TS));
    const long s0 = (t % (S / TS)) * TS;
    for (int r = threadIdx.x; r < (I + O_sl) * (TS / 4); r += kBlock) {
      const int row = r / (TS / 4);
      const int col = (r - row * (TS / 4)) * 4;
      if (row < I) {
        *reinterpret_cast<float4*>(&xs[row * LD + col]) =
            *reinterpret_cast<const float4*>(x + ((long)b * I + row) * S + s0 + col);
      } else {
        const int ro = row - I;
        *reinterpret_cast<float4*>(&gs[ro * LD + col]) =
            *reinterpret_cast<const float4*>(gz + ((long)b * O + o0 + ro) * S + s0 + col);
      }
    }
    __syncthreads();
#pragma unroll
    for (int pp = 0; pp < NPAIR; ++pp) {
      const int p = wave + 4 * pp;
      if (p < npairs) {
        const int mt = p / iT, nt = p - mt * iT;
        const float* gr = gs + (mt * 16 + l16) * LD;         // A row
        const float* xr = xs + (nt * 16 + l16) * LD;         // B col's row
        const bool av = (mt * 16 + l16) < O_sl;
        const bool bv = (nt * 16 + l16) < I;
#pragma unroll
        for (int k = 0; k < TS; k += 4) {
          const float a = av ? gr[k + kg] : 0.f;
          const float bb = bv ? xr[k + kg]
                              : ((BIAS && nt * 16 + l16 == I) ? 1.f : 0.f);
          acc[pp] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bb, acc[pp], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

#pragma unroll
  for (int pp = 0; pp < NPAIR; ++pp) {
    const int p = wave + 4 * pp;
    if (p >= npairs) continue;
    const int mt = p / iT, nt = p - mt * iT;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = o0 + mt * 16 + kg * 4 + r;   // D row
      const int i = nt * 16 + l16;               // D col
      if (o < O && (mt * 16 + kg * 4 + r) < O_sl) {
        if (i < I) atomicAdd(&gW[(size_t)o * I + i], acc[pp][r]);
        else if (BIAS && i == I) atomicAdd(&gb[o], acc[pp][r]);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// bf16 grad-W (+grad-bias): gW[o,i] = sum_{b,s} gz[b,o,s] x[b,i,s], fp32 accum.
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

// Launch layer.  Every compile-time parameter of a kernel is named at the one
// place that launches it, so a kernel is instantiated exactly where it runs.

// A/B and sweep knobs (docs/instructions_mi355x.md), read once per process
struct GwKnobs {
  bool no_glds;        // DFNO_GW_NO_GLDS=1: glds3 rows fall to the generic ones
  bool no_mfma;        // DFNO_GW_NO_MFMA=1: no fp32 MFMA rows
  bool bf16_no_mfma;   // DFNO_BF16_GW_NO_MFMA=1: bf16 takes the LDS-tiled kernel
  long nschunk;        // DFNO_GW_NSCHUNK=n > 0: s-chunks before the caps below
};

const GwKnobs& gw_knobs() {
  auto flag = [](const char* name) {
    const char* e = getenv(name);
    return e && e[0] == '1';
  };
  static const char* ns = getenv("DFNO_GW_NSCHUNK");
  static const GwKnobs knobs{flag("DFNO_GW_NO_GLDS"), flag("DFNO_GW_NO_MFMA"),
                             flag("DFNO_BF16_GW_NO_MFMA"), ns ? atol(ns) : 0L};
  return knobs;
}

// operands and outputs of one channel_mix_bwd_w call
struct GwCall {
  const at::Tensor &gz, &x;
  at::Tensor &gW, &gb;
  bool want_bias;
  int B, O, I;
  long S;
  hipStream_t stream;
  template <typename T> T* gb_ptr() const { return want_bias ? gb.data_ptr<T>() : nullptr; }
};

// Grid rule of the split-s rows: s-chunks for a row of o_tiles o-tiles that
// keeps bpc blocks per CU resident.  Every block atomically flushes its whole
// O*I accumulator, so the flush cost scales with grid and serializes per
// cache line (measured: 4096 s-chunks -> 1.84 ms, 256 -> 0.52 ms on the 20x20
// S=7.9M flagship shape): one grid-wave of 256 * bpc blocks, chunks of at
// least 1024 elements.  swizzle: the glds3 XCD decode takes schunk mod 8, so
// the count is rounded up to a multiple of 8 (padded chunks are empty).
// n_islab: i-slabs are a second grid dimension and share the chunks out.
int gw_schunks(long S, int o_tiles, int bpc, bool swizzle, int n_islab) {
  const long by_len = S / (64 * 16);
  const long want = gw_knobs().nschunk > 0 ? gw_knobs().nschunk
                                           : (long)(256 * bpc / o_tiles);
  long n = std::max(1L, std::min(want, by_len));
  if (swizzle && o_tiles > 1) n = (n + 7) & ~7L;
  return (int)std::max(1L, n / n_islab);
}

// generic row <ICAP, OW>, ISLAB with ceil(I / ICAP) i-slabs in grid.y; fp64
// has the element-wise form only
template <int ICAP, int OW, bool ISLAB>
void launch_gw_outer(const GwCall& c, bool vec, int bpc, bool swizzle) {
  const int o_tiles = (c.O + 4 * OW - 1) / (4 * OW);
  const int n_islab = ISLAB ? (c.I + ICAP - 1) / ICAP : 1;
  const int n_schunk = gw_schunks(c.S, o_tiles, bpc, swizzle, n_islab);
  auto go = [&](auto elem, auto v) {   // element type (by example), VECTOR
    using T = decltype(elem);
    select_bool(c.want_bias, [&](auto bias) {
      hipLaunchKernelGGL(
          (gw_outer_kernel<T, ICAP, OW, decltype(bias)::value, decltype(v)::value, ISLAB>),
          dim3(n_schunk * o_tiles, n_islab), dim3(kBlock), 0, c.stream,
          c.gz.data_ptr<T>(), c.x.data_ptr<T>(), c.gW.data_ptr<T>(),
          c.template gb_ptr<T>(), c.B, c.O, c.I, c.S, n_schunk);
    });
  };
  if (c.gz.scalar_type() == at::kDouble) go(0.0, std::false_type{});
  else select_bool(vec, [&](auto v) { go(0.f, v); });
  DFNO_CHECK_LAUNCH("channel_mix_bwd_w");
}

// glds3 row <ICAP, OW, TS> (fp32, 16-byte aligned rows).  The kernels carry
// 72-120 KB static LDS: a refused launch must not return the zeroed gW.
template <int ICAP, int OW, int TS>
void launch_gw_glds3(const GwCall& c, int bpc) {
  const int o_tiles = (c.O + 4 * OW - 1) / (4 * OW);
  const int n_schunk = gw_schunks(c.S, o_tiles, bpc, true, 1);
  hipLaunchKernelGGL((gw_outer_glds3_kernel<ICAP, OW, TS>),
                     dim3(n_schunk * o_tiles), dim3(kBlock), 0, c.stream,
                     c.gz.data_ptr<float>(), c.x.data_ptr<float>(),
                     c.gW.data_ptr<float>(), c.gb_ptr<float>(), c.B, c.O, c.I,
                     c.S, n_schunk, c.want_bias);
  DFNO_CHECK_LAUNCH("channel_mix_bwd_w");
}

// fp32 MFMA row: o-slabs of OSL rows in grid.y, three grid-waves of 128-wide
// s-tiles in grid.x, the [XR + OSL][132] tile pair in dynamic LDS
template <int NPAIR, int XR, int OSL, bool BIAS>
void launch_gw_mfma(const GwCall& c) {
  const long ntiles = (c.S / 128) * (long)c.B;
  const int nslab = (c.O + OSL - 1) / OSL;
  const int gx = (int)std::min(ntiles, (long)(256 * 3 / std::max(nslab, 1)));
  const size_t smem = sizeof(float) * (size_t)(XR + std::min(c.O, OSL)) * 132;
  hipLaunchKernelGGL((gw_mfma_f32_kernel<NPAIR, XR, OSL, BIAS>),
                     dim3(gx, nslab), dim3(kBlock), smem, c.stream,
                     c.gz.data_ptr<float>(), c.x.data_ptr<float>(),
                     c.gW.data_ptr<float>(), c.B, c.O, c.I, c.S,
                     BIAS ? c.gb.data_ptr<float>() : nullptr);
  DFNO_CHECK_LAUNCH("gw_mfma");
}

}  // namespace

std::vector<at::Tensor> channel_mix_bwd_w(const at::Tensor& gz, const at::Tensor& x,
                                          bool want_bias) {
  check_real(gz, "gz"); check_real(x, "x");
  TORCH_CHECK(gz.dim() == 3 && x.dim() == 3, "gz/x must be [B,*,S]");
  int B = (int)gz.size(0), O = (int)gz.size(1), I = (int)x.size(1);
  long S = gz.size(2);
  TORCH_CHECK(x.size(0) == B && x.size(2) == S, "shape mismatch");
  TORCH_CHECK(I <= 64, "channel_mix_bwd_w: I must be <= 64");

  auto gW = at::zeros({O, I}, gz.options());
  auto gb = want_bias ? at::zeros({O}, gz.options())
                      : at::empty({0}, gz.options());
  if (gz.numel() == 0) return {gW, gb};

  const GwKnobs& knobs = gw_knobs();
  const GwCall c{gz, x, gW, gb, want_bias, B, O, I, S,
                 at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()};

  // vec: fp32 with whole, 16-byte aligned float4s in every row
  const bool vec = gz.scalar_type() == at::kFloat && S % 4 == 0 &&
                   aligned16(gz.data_ptr()) && aligned16(x.data_ptr());
  // big-O shapes (the projection lift's gW3 [128, 20]) take the f32-MFMA tile
  // kernel; identical numerics (f32-in MFMA is a bitwise fmaf chain,
  // cdna_hip_programming.md section 3).  Bias only where the ones column
  // has a free i-tile slot (33..64 x rows).
  const bool mfma = vec && !knobs.no_mfma && (!want_bias || I > 32) &&
                    (long)O * I >= 1024 && S % 128 == 0;
  const bool use_glds = vec && !knobs.no_glds && O >= 8;
  // rows per wave: wider cuts B re-reads but costs registers/occupancy.
  // The glds3 OW=5 variant covers O<=20 in ONE o-tile so B is read once.
  // For big-O shapes (gW3: O=128), wider OW (4: 9 GB, 6: 7.8 GB vs OW=2's
  // 14 GB of o-tile-amplified traffic) measured NO faster: per-block
  // throughput here scales with resident blocks (3/CU at the 48 KB OW=2
  // ring vs 2/CU at 60-72 KB), which exactly offsets the traffic cut.
  const bool ow5 = use_glds && I > 8 && I <= 20 && O <= 20;
  const int OW = ow5 ? 5 : (O >= 8 ? (I <= 8 ? 4 : 2) : 1);
  const int o_tiles = (O + 4 * OW - 1) / (4 * OW);

  // Rows, first match wins (bpc = resident blocks per CU the grid is sized
  // for, see gw_schunks):
  //   mfma                 gw_mfma_f32<2,32,64>            I <= 32, no bias
  //                        gw_mfma_f32<3,64,32,bias>       I > 32, bias
  //                        gw_mfma_f32<2,64,32>            I > 32, no bias
  //   I > 32               gw_outer<32, OW 2|1, i-slab>    bpc of its glds3 row
  //   use_glds             glds3<20,5,256>  bpc 1          ow5
  //                        glds3<8,4,256>   bpc 2          I <= 8
  //                        glds3<24|32,2,128> bpc 3        o_tiles >= 8
  //                        glds3<24|32,2,256> bpc 1
  //   otherwise            gw_outer<8,4> <24,2> <32,2> <32,1>  bpc 4
  // Each gw_outer row exists per bias and, in fp32, per vec.
  if (mfma) {
    if (I <= 32) launch_gw_mfma<2, 32, 64, false>(c);
    // 33..64 x rows: 2 o-tiles x 4 i-tiles (+ the ones column's) per 32-row slab
    else if (want_bias) launch_gw_mfma<3, 64, 32, true>(c);
    else launch_gw_mfma<2, 64, 32, false>(c);
  } else if (I > 32) {
    // 33..64 x rows off the MFMA conditions (ragged or unaligned S, small
    // O * I, fp64): the generic kernel with a second grid dimension over
    // 32-row i-slabs, no channel-slice copies.  Its chunk count is that of
    // the glds3 row the same O would take, divided among the slabs.
    const int bpc = use_glds ? (o_tiles >= 8 ? 3 : 1) : 4;
    if (OW == 2) launch_gw_outer<32, 2, true>(c, vec, bpc, use_glds);
    else launch_gw_outer<32, 1, true>(c, vec, bpc, use_glds);
  } else if (use_glds) {
    // 1-2 blocks/CU by LDS, so one grid-wave exactly fills the 256 CUs
    if (ow5) launch_gw_glds3<20, 5, 256>(c, 1);
    else if (I <= 8) launch_gw_glds3<8, 4, 256>(c, 2);
    // big-O shapes (gW3: O=128) re-read B o_tiles times; occupancy (3
    // blocks/CU at a 48 KB TS=128 ring) beats per-stream burst length
    // there (measured 2.7 ms vs 4.4 ms at 1 block/CU, matmul 3.8 ms)
    else if (o_tiles >= 8) {
      if (I <= 24) launch_gw_glds3<24, 2, 128>(c, 3);
      else launch_gw_glds3<32, 2, 128>(c, 3);
    } else {
      if (I <= 24) launch_gw_glds3<24, 2, 256>(c, 1);
      else launch_gw_glds3<32, 2, 256>(c, 1);
    }
  } else {
    // the generic kernel gets a few more blocks per CU for latency-hiding
    if (OW == 4) launch_gw_outer<8, 4, false>(c, vec, 4, false);
    else if (OW == 1) launch_gw_outer<32, 1, false>(c, vec, 4, false);
    else if (I <= 24) launch_gw_outer<24, 2, false>(c, vec, 4, false);
    else launch_gw_outer<32, 2, false>(c, vec, 4, false);
  }
  return {gW, gb};
}

std::vector<at::Tensor> bf16_channel_mix_bwd_w(const at::Tensor& gz,
                                               const at::Tensor& x,
                                               bool want_bias) {
  check_bf16(gz, "gz"); check_bf16(x, "x");
  const int B = (int)x.size(0), I = (int)x.size(1), O = (int)gz.size(1);
  const long S = x.size(2);
  TORCH_CHECK(I <= 64, "bf16 grad-W: I must be <= 64");
  TORCH_CHECK(O <= 128, "bf16 grad-W: O must be <= 128");
  TORCH_CHECK(S % 128 == 0, "bf16 grad-W: S must be a multiple of 128");

  auto opts = x.options().dtype(at::kFloat);
  auto gW = at::zeros({O, I}, opts);
  auto gb = at::zeros({want_bias ? O : 0}, opts);
  if (x.numel() == 0) return {gW, gb};

  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  auto launch = [&](auto kernel, dim3 grid, size_t smem) {
    hipLaunchKernelGGL(kernel, grid, dim3(kBlock), smem, stream, usp(gz), usp(x),
                       gW.data_ptr<float>(),
                       gb.numel() ? gb.data_ptr<float>() : nullptr, B, I, O, S,
                       want_bias);
  };

  // Rows, first match wins:
  //   S % 256 == 0, <= 32 tile pairs   bf16_gw_mfma<NPAIR 1|4|8> at <= 4 | 16 |
  //                                    32 16x16 tile pairs (4 waves x NPAIR)
  //   I > 32                           bf16_gw<8, 64>
  //   otherwise                        bf16_gw<NP 1|2|4> at <= 256 | 512 | 1024
  //                                    (o, i) pairs per 32-row o-slab
  const int mfma_pairs = ((O + 15) / 16) * ((I + 15) / 16);
  if (!gw_knobs().bf16_no_mfma && S % 256 == 0 && mfma_pairs <= 32) {
    const long ntiles = (S / 256) * (long)B;
    const dim3 grid((int)std::min(ntiles, 2048L));
    select_le<4, 16, 32>(mfma_pairs, [&](auto cap) {
      launch(bf16_gw_mfma_kernel<decltype(cap)::value / 4>, grid, 0);
    });
    DFNO_CHECK_LAUNCH("bf16_gw_mfma");
    return {gW, gb};
  }
  const int nslab = (O + 31) / 32;
  const int o_sl = std::min(O, 32);
  const int xr = I <= 32 ? 32 : 64;
  const size_t smem = sizeof(float) * (size_t)(xr + o_sl) * 132;   // [rows][LD]
  const long ntiles = (S / 128) * (long)B;
  const dim3 grid((int)std::min(ntiles, 2048L), nslab);
  if (I > 32) {
    launch(bf16_gw_kernel<8, 64>, grid, smem);
  } else {
    select_le<256, 512, 1024>(o_sl * I, [&](auto cap) {
      launch(bf16_gw_kernel<decltype(cap)::value / 256>, grid, smem);
    });
  }
  DFNO_CHECK_LAUNCH("bf16_gw");
  return {gW, gb};
}
