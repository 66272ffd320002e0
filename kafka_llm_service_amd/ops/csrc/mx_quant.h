// The per-lane body of the MXFP8 quantiser, shared by act_quant_mxfp8_kernel (tile_gemm_mx.hip) and the quantising GLU
// epilogue of grouped_tile_gemm_mx.hip. The rule is ops.reference.mxfp8_quant's: per 32-column block e = the frexp
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

}  // namespace kafka
