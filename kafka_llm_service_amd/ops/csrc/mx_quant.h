// The per-lane bodies of the activation quantisers. MXFP8: shared by act_quant_mxfp8_kernel (tile_gemm_mx.hip), the
// quantising GLU epilogue of the dense and grouped scaled kernels (tile_epilogue.h) and the quantising RMSNorm
// (norm_act.hip); per-row fp8 at the end of the file. The MXFP8 rule is ops.reference.mxfp8_quant's: per 32-column block e = the frexp
// exponent of amax / 448 (so amax / 2^e lies in [224, 448): never clipped), stored biased by 127 and clamped to
// [7, 247], 127 for an all-zero block; elements x / 2^e rounded to nearest-even by v_cvt_scalef32_pk_fp8_f32.
#pragma once
#include "common.h"

namespace kafka {

// raw: this lane's 8 bf16 values (16 B) of a block whose 32 columns lie in the 4 consecutive lanes 4 q .. 4 q + 3, all
// of them active. The block's amax is taken on the bf16 bit patterns (e follows from the exponent field and whether the
// mantissa reaches 1.75 = 448 / 256, no division). Returns the biased block exponent (the same in the 4 lanes); o = the
// lane's 8 e4m3 bytes in column order.
__device__ __forceinline__ int mxfp8_quant_lane(const u32x4 raw, uint32_t (&o)[2]) {
  uint32_t am = 0;  // the largest |x| as a bf16 bit pattern
#pragma unroll
  for (int j = 0; j < 4; ++j) am = max(am, max(raw[j] & 0x7fffu, (raw[j] >> 16) & 0x7fffu));
  am = max(am, (uint32_t)__shfl_xor((int)am, 1, 64));
  am = max(am, (uint32_t)__shfl_xor((int)am, 2, 64));
  // amax = 1.f * 2^(E - 127): amax / 448 = (1.f / 1.75) * 2^(E - 135), whose frexp exponent is E - 135 + (1.f >= 1.75)
  int eb = am == 0 ? 127 : (int)(am >> 7) - 8 + ((am & 0x7f) >= 0x60 ? 1 : 0);
  eb = min(max(eb, 7), 247);
  const float sc = __uint_as_float((uint32_t)eb << 23);
  typedef short i16x2 __attribute__((ext_vector_type(2)));
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const float f0 = __uint_as_float(raw[2 * j] << 16), f1 = __uint_as_float(raw[2 * j] & 0xffff0000u);
    const float f2 = __uint_as_float(raw[2 * j + 1] << 16), f3 = __uint_as_float(raw[2 * j + 1] & 0xffff0000u);
    i16x2 v = {0, 0};
    v = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(v, f0, f1, sc, false);
    v = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(v, f2, f3, sc, true);
    o[j] = __builtin_bit_cast(uint32_t, v);
  }
  return eb;
}

// The exponent bytes of a half-wave whose 32 lanes hold 256 consecutive columns of one row (8 blocks, eb as
// mxfp8_quant_lane returns it): a dword per 16 lanes, then the pair, so lane 0 of the half-wave stores 8 B at once.
// Every lane of the wave takes part.
__device__ __forceinline__ uint2 mxfp8_exps_halfwave(int eb, int lane) {
  uint32_t ev = (lane & 3) == 0 ? (uint32_t)eb << (8 * ((lane >> 2) & 3)) : 0u;
  ev |= (uint32_t)__shfl_xor((int)ev, 4, 64);
  ev |= (uint32_t)__shfl_xor((int)ev, 8, 64);
  const uint32_t ev2 = (uint32_t)__shfl_xor((int)ev, 16, 64);
  return make_uint2(ev, ev2);  // (in byte order for the half-wave's lanes 0-15)
}

// ---- per-row fp8 (ops.reference.fp8_quant over a whole row): shared by act_quant_fp8_kernel (tile_gemm_f8.hip) and the
// quantising RMSNorm (norm_act.hip)
// am: the row's largest |x| as a bf16 bit pattern. e = the frexp exponent of amax / 448, clamped to [-100, 100], 0 for
// an all-zero row. amax = 1.f * 2^(E - 127): amax / 448 = (1.f / 1.75) * 2^(E - 135), whose frexp exponent is
// E - 135 + (1.f >= 1.75)
__device__ __forceinline__ int fp8_row_exp(uint32_t am) {
  const int e = am == 0 ? 0 : (int)(am >> 7) - 135 + ((am & 0x7f) >= 0x60 ? 1 : 0);
  return min(max(e, -100), 100);
}

// raw: 8 bf16 values (16 B); o = their 8 e4m3 bytes in the same order: x * inv (inv = 2^-e) saturated to +-448 and
// rounded to nearest-even by v_cvt_pk_fp8_f32
__device__ __forceinline__ void fp8_quant8(const u32x4 raw, float inv, uint32_t (&o)[2]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const uint32_t d0 = raw[2 * j], d1 = raw[2 * j + 1];
    const float f0 = __builtin_amdgcn_fmed3f(__uint_as_float(d0 << 16) * inv, 448.f, -448.f);
    const float f1 = __builtin_amdgcn_fmed3f(__uint_as_float(d0 & 0xffff0000u) * inv, 448.f, -448.f);
    const float f2 = __builtin_amdgcn_fmed3f(__uint_as_float(d1 << 16) * inv, 448.f, -448.f);
    const float f3 = __builtin_amdgcn_fmed3f(__uint_as_float(d1 & 0xffff0000u) * inv, 448.f, -448.f);
    const int v = __builtin_amdgcn_cvt_pk_fp8_f32(f0, f1, 0, false);
    o[j] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(f2, f3, v, true);
  }
}

}  // namespace kafka
