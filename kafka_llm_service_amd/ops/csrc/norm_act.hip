// RMSNorm, fused residual-add + RMSNorm, and SwiGLU activation for gfx950.
//
// All three are HBM-bound streaming ops: one workgroup per token row, 16-byte (bf16x8) loads per lane, the
// row kept in registers between the reduction and the scale pass (one HBM read + one write per element),
// fp32 accumulation. The residual add is fused into the norm so the decoder layer reads the residual
// stream once per sub-block instead of three times.
//
// Split-K slab inputs: the decode GEMM (wstream_gemm.hip) leaves its output as S fp32 partial slabs
// P[S][T][n]; every kernel here can take such a slab instead of a bf16 input and sums the S partials while
// loading (load_in8 in common.h), so the split-K combine costs no launch of its own.
#include <cstdlib>

#include "common.h"
#include "mx_quant.h"

namespace kafka {

// y = x * rsqrt(mean(x^2) + eps) * w     (x: [T, d] with row stride, out: [T, d] contiguous)
// If RESID: r = x + r (rounded to bf16, written back to r), y = norm(r) * w.
template <int NV, bool RESID, int NT = 256, bool SC1 = false>
__global__ __launch_bounds__(NT) void rmsnorm_kernel(bf16* __restrict__ out, int64_t out_stride,
                                                       const bf16* __restrict__ x, const float* __restrict__ xp,
                                                       int S, int64_t ps, int64_t x_stride,
                                                       bf16* __restrict__ resid, int64_t r_stride,
                                                       const bf16* __restrict__ w, int d, float eps) {
  __shared__ float red[NT / 64];
  const int64_t row = blockIdx.x;
  const int nvec = d >> 3;
  float v[NV][8];
  float ss = 0.f;
  // the weight loads go out with the row loads (not after the reduction: one HBM round trip instead of two)
  bf16x8 wv[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int vi = threadIdx.x + i * NT;
    if (vi < nvec) wv[i] = load_bf16x8(w + vi * 8);
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int vi = threadIdx.x + i * NT;
    if (vi < nvec) {
      load_in8(v[i], x, xp, S, ps, row * x_stride + vi * 8);
      if constexpr (RESID) {
        const bf16x8 b = load_bf16x8(resid + row * r_stride + vi * 8);
        bf16x8 s;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          s[j] = (bf16)(v[i][j] + (float)b[j]);
          v[i][j] = (float)s[j];
        }
        if constexpr (SC1)
          store16_slab(reinterpret_cast<float*>(resid + row * r_stride + vi * 8), __builtin_bit_cast(f32x4, s));
        else
          store_bf16x8(resid + row * r_stride + vi * 8, s);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) ss += v[i][j] * v[i][j];
    }
  }
  ss = block_sum<NT>(ss, red);
  const float r = rsqrtf(ss / (float)d + eps);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int vi = threadIdx.x + i * NT;
    if (vi < nvec) {
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (bf16)(v[i][j] * r * (float)wv[i][j]);
      if constexpr (SC1)
        store16_slab(reinterpret_cast<float*>(out + row * out_stride + vi * 8), __builtin_bit_cast(f32x4, o));
      else
        store_bf16x8(out + row * out_stride + vi * 8, o);
    }
  }
}

// out[t, :] = silu(x[t, :F]) * x[t, F:]   (x: [T, 2F] row stride xs (bf16 or slabs), out: [T, F] contiguous)
__global__ __launch_bounds__(256) void silu_mul_kernel(bf16* __restrict__ out, const bf16* __restrict__ x,
                                                        const float* __restrict__ xp, int S, int64_t ps,
                                                        int64_t xs, int F) {
  const int64_t row = blockIdx.y;
  const int nvec = F >> 3;
  for (int vi = blockIdx.x * 256 + threadIdx.x; vi < nvec; vi += gridDim.x * 256) {
    float g[8], u[8];
    load_in8(g, x, xp, S, ps, row * xs + vi * 8);
    load_in8(u, x, xp, S, ps, row * xs + F + vi * 8);
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (bf16)(g[j] / (1.0f + __expf(-g[j])) * u[j]);
    store_bf16x8(out + row * (int64_t)F + vi * 8, o);
  }
}

// ---- RMSNorm whose output leaves quantised for the dense tile GEMMs (tile_gemm_mx.hip / tile_gemm_f8.hip) ----------
// The same row ownership as rmsnorm_kernel (one workgroup per row, thread t owning the 16-B vectors t, t + NT, ...;
// loads, residual update and reduction are its code line for line), but the normalised row never reaches HBM as bf16:
// each vector is rounded to bf16 exactly as rmsnorm_kernel would have stored it, kept as 4 dwords in registers, and
// quantised by the stand-alone quantisers' own per-lane bodies (mx_quant.h), so bytes and exponents equal
// act_quant_*(rmsnorm(..)) bit for bit. d % 256 == 0: a half-wave's 32 vectors are live or dead together.
//   Q_MXFP8: a 32-column block is the 4 consecutive lanes 4 q .. 4 q + 3 of a vector group: amax over the quad by two
//     DPP shuffles, 8 B of e4m3 per lane in natural K order, the 8 exponent bytes of a half-wave (256 columns) as one
//     8-B store. No second block reduction.
//   Q_FP8: the row amax (bf16 bit patterns, integer max) is a second block reduction through red[] behind the sum of
//     squares; one int32 exponent per row; 8 B of e4m3 per lane in fp8-tile K order (the 8-B runs 1 and 2 of every 32
//     columns trade places: lane c of a quad stores at run c ^ 3 for c = 1, 2).
// Outputs are ordinary vector stores (the GEMM reads them by LDS-DMA; see common.h "Store / load scopes").
enum { Q_MXFP8 = 1, Q_FP8 = 2 };

template <int NT>
__device__ __forceinline__ uint32_t block_max_u32(uint32_t v, uint32_t* red) {
#pragma unroll
  for (int d = 1; d < 64; d *= 2) v = max(v, (uint32_t)__shfl_xor((int)v, d, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t t = 0;
#pragma unroll
  for (int i = 0; i < NT / 64; ++i) t = max(t, red[i]);
  return t;
}

template <int NV, bool RESID, int NT, int Q>
__global__ __launch_bounds__(NT) void rmsnorm_quant_kernel(uint8_t* __restrict__ xq, uint8_t* __restrict__ xe8,
                                                             int* __restrict__ xe32, const bf16* __restrict__ x,
                                                             const float* __restrict__ xp, int S, int64_t ps,
                                                             int64_t x_stride, bf16* __restrict__ resid,
                                                             int64_t r_stride, const bf16* __restrict__ w, int d,
                                                             float eps) {
  __shared__ float red[NT / 64];
  const int64_t row = blockIdx.x;
  const int nvec = d >> 3;
  const int lane = threadIdx.x & 63;
  float v[NV][8];
  float ss = 0.f;
  bf16x8 wv[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int vi = threadIdx.x + i * NT;
    if (vi < nvec) wv[i] = load_bf16x8(w + vi * 8);
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int vi = threadIdx.x + i * NT;
    if (vi < nvec) {
      load_in8(v[i], x, xp, S, ps, row * x_stride + vi * 8);
      if constexpr (RESID) {
        const bf16x8 b = load_bf16x8(resid + row * r_stride + vi * 8);
        bf16x8 s;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          s[j] = (bf16)(v[i][j] + (float)b[j]);
          v[i][j] = (float)s[j];
        }
        store_bf16x8(resid + row * r_stride + vi * 8, s);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) ss += v[i][j] * v[i][j];
    }
  }
  ss = block_sum<NT>(ss, red);
  const float r = rsqrtf(ss / (float)d + eps);
  // the bf16 row rmsnorm_kernel would have stored, 4 dwords per vector; dead vectors are zero (they take part in the
  // shuffles below and store nothing)
  u32x4 raw[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int vi = threadIdx.x + i * NT;
    raw[i] = u32x4{0, 0, 0, 0};
    if (vi < nvec) {
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (bf16)(v[i][j] * r * (float)wv[i][j]);
      raw[i] = __builtin_bit_cast(u32x4, o);
    }
  }
  if constexpr (Q == Q_MXFP8) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int vi = threadIdx.x + i * NT;
      uint32_t o[2];
      const int eb = mxfp8_quant_lane(raw[i], o);
      const uint2 ev = mxfp8_exps_halfwave(eb, lane);
      if (vi < nvec) {
        *reinterpret_cast<uint2*>(xq + row * d + 8 * vi) = make_uint2(o[0], o[1]);
        if ((lane & 31) == 0) *reinterpret_cast<uint2*>(xe8 + row * (d >> 5) + (vi >> 2)) = ev;
      }
    }
  } else {
    uint32_t am = 0;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) am = max(am, max(raw[i][j] & 0x7fffu, (raw[i][j] >> 16) & 0x7fffu));
    am = block_max_u32<NT>(am, reinterpret_cast<uint32_t*>(red));  // (block_sum ends with a barrier: red is free)
    const int e = fp8_row_exp(am);
    const float inv = exp2i(-e);
    if (threadIdx.x == 0) xe32[row] = e;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int vi = threadIdx.x + i * NT;
      if (vi < nvec) {
        uint32_t o[2];
        fp8_quant8(raw[i], inv, o);
        const int c = vi & 3, cp = (c == 1 || c == 2) ? c ^ 3 : c;
        *reinterpret_cast<uint2*>(xq + row * d + 32 * (vi >> 2) + 8 * cp) = make_uint2(o[0], o[1]);
      }
    }
  }
}

template <bool RESID, int Q>
static hipError_t launch_rmsnorm_quant_t(uint8_t* xq, void* xe, const bf16* x, const float* xp, int S, int64_t ps,
                                         int64_t xs, bf16* r, int64_t rs, const bf16* w, int T, int d, float eps,
                                         hipStream_t st) {
  const int nvec = d / 8;
  const int nv = (nvec + 255) / 256;
  dim3 grid(T);
  uint8_t* e8 = static_cast<uint8_t*>(xe);
  int* e32 = static_cast<int*>(xe);
#define KAFKA_RQ(NV, NT) \
  rmsnorm_quant_kernel<NV, RESID, NT, Q><<<grid, NT, 0, st>>>(xq, e8, e32, x, xp, S, ps, xs, r, rs, w, d, eps)
  if (nvec <= 512 && nvec > 256) {  // as launch_rmsnorm_t: one vector per thread of 512
    KAFKA_RQ(1, 512);
    return hipGetLastError();
  }
  switch (nv) {
    case 1: KAFKA_RQ(1, 256); break;
    case 2: KAFKA_RQ(2, 256); break;
    case 3:
    case 4: KAFKA_RQ(4, 256); break;
    default: KAFKA_RQ(8, 256); break;
  }
#undef KAFKA_RQ
  return hipGetLastError();
}

extern "C" hipError_t kafka_launch_rmsnorm_quant(int quant, uint8_t* xq, void* xe, const bf16* x, int64_t xs,
                                                const float* xp, int S, int64_t ps, bf16* resid, int64_t rs,
                                                const bf16* w, int T, int d, float eps, hipStream_t st) {
  auto al16 = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
  if (T < 0 || d <= 0 || d % 256 != 0 || d > 16384 || (quant != Q_MXFP8 && quant != Q_FP8)) return hipErrorInvalidValue;
  if (xq == nullptr || xe == nullptr || w == nullptr || !al16(xq) || !al16(xe) || !al16(w)) return hipErrorInvalidValue;
  if (xp != nullptr) {  // slabs [S][T][d]: only as the delta of a fused add
    if (x != nullptr || resid == nullptr || S < 1 || !al16(xp) || ps % 4 != 0) return hipErrorInvalidValue;
    xs = d;
  } else if (x == nullptr || !al16(x) || xs % 8 != 0 || xs < d) {
    return hipErrorInvalidValue;
  }
  if (resid != nullptr && (!al16(resid) || rs % 8 != 0 || rs < d)) return hipErrorInvalidValue;
  if (T == 0) return hipSuccess;
  if (resid != nullptr)
    return quant == Q_MXFP8 ? launch_rmsnorm_quant_t<true, Q_MXFP8>(xq, xe, x, xp, S, ps, xs, resid, rs, w, T, d, eps, st)
                            : launch_rmsnorm_quant_t<true, Q_FP8>(xq, xe, x, xp, S, ps, xs, resid, rs, w, T, d, eps, st);
  return quant == Q_MXFP8 ? launch_rmsnorm_quant_t<false, Q_MXFP8>(xq, xe, x, xp, S, ps, xs, resid, rs, w, T, d, eps, st)
                          : launch_rmsnorm_quant_t<false, Q_FP8>(xq, xe, x, xp, S, ps, xs, resid, rs, w, T, d, eps, st);
}

template <bool RESID>
static hipError_t launch_rmsnorm_t(bf16* out, int64_t os, const bf16* x, const float* xp, int S, int64_t ps,
                                   int64_t xs, bf16* r, int64_t rs, const bf16* w, int T, int d, float eps,
                                   hipStream_t st) {
  const int nvec = d / 8;
  const int nv = (nvec + 255) / 256;
  dim3 grid(T), block(256);
  if (T == 0) return hipSuccess;
  // outputs (normalised rows and the in-place residual) as 16-B sc1 stores — the lines leave this XCD's L2, so the
  // launch ends with none of them dirty (+2.1 % on the headline with RoPE's, profiles/r06/ab/). Needs 16-B aligned
  // rows; others keep plain stores. common.h "Store / load scopes"
  if (nvec <= 512 && nvec > 256) {  // e.g. d = 4096: one 16-B vector per thread, twice the loads in flight per row
    if (os % 8 == 0 && rs % 8 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0 &&
        (!RESID || reinterpret_cast<uintptr_t>(r) % 16 == 0))
      rmsnorm_kernel<1, RESID, 512, true><<<grid, 512, 0, st>>>(out, os, x, xp, S, ps, xs, r, rs, w, d, eps);
    else
      rmsnorm_kernel<1, RESID, 512><<<grid, 512, 0, st>>>(out, os, x, xp, S, ps, xs, r, rs, w, d, eps);
    return hipGetLastError();
  }
  switch (nv) {
    case 1: rmsnorm_kernel<1, RESID><<<grid, block, 0, st>>>(out, os, x, xp, S, ps, xs, r, rs, w, d, eps); break;
    case 2: rmsnorm_kernel<2, RESID><<<grid, block, 0, st>>>(out, os, x, xp, S, ps, xs, r, rs, w, d, eps); break;
    case 3:
    case 4: rmsnorm_kernel<4, RESID><<<grid, block, 0, st>>>(out, os, x, xp, S, ps, xs, r, rs, w, d, eps); break;
    default: rmsnorm_kernel<8, RESID><<<grid, block, 0, st>>>(out, os, x, xp, S, ps, xs, r, rs, w, d, eps); break;
  }
  return hipGetLastError();
}

extern "C" hipError_t kafka_launch_rmsnorm(bf16* out, int64_t os, const bf16* x, int64_t xs, const bf16* w, int T, int d,
                          float eps, hipStream_t st) {
  return launch_rmsnorm_t<false>(out, os, x, nullptr, 0, 0, xs, nullptr, 0, w, T, d, eps, st);
}

extern "C" hipError_t kafka_launch_fused_add_rmsnorm(bf16* out, int64_t os, const bf16* x, int64_t xs, bf16* resid, int64_t rs,
                                    const bf16* w, int T, int d, float eps, hipStream_t st) {
  return launch_rmsnorm_t<true>(out, os, x, nullptr, 0, 0, xs, resid, rs, w, T, d, eps, st);
}

// fused add + RMSNorm whose x input is S fp32 split-K slabs [S][T][d] (row stride d, slab stride ps)
extern "C" hipError_t kafka_launch_fused_add_rmsnorm_slab(bf16* out, int64_t os, const float* xp, int S, int64_t ps,
                                                         bf16* resid, int64_t rs, const bf16* w, int T, int d,
                                                         float eps, hipStream_t st) {
  return launch_rmsnorm_t<true>(out, os, nullptr, xp, S, ps, d, resid, rs, w, T, d, eps, st);
}

extern "C" hipError_t kafka_launch_silu_mul(bf16* out, const bf16* x, int64_t xs, int T, int F, hipStream_t st) {
  if (T == 0) return hipSuccess;
  const int nvec = F / 8;
  int gx = (nvec + 255) / 256;
  if (gx > 64) gx = 64;
  silu_mul_kernel<<<dim3(gx, T), dim3(256), 0, st>>>(out, x, nullptr, 0, 0, xs, F);
  return hipGetLastError();
}

// SwiGLU over S fp32 split-K slabs [S][T][2F]
extern "C" hipError_t kafka_launch_silu_mul_slab(bf16* out, const float* xp, int S, int64_t ps, int T, int F,
                                                hipStream_t st) {
  if (T == 0) return hipSuccess;
  const int nvec = F / 8;
  int gx = (nvec + 255) / 256;
  if (gx > 64) gx = 64;
  silu_mul_kernel<<<dim3(gx, T), dim3(256), 0, st>>>(out, nullptr, xp, S, ps, 2 * (int64_t)F, F);
  return hipGetLastError();
}

}  // namespace kafka
