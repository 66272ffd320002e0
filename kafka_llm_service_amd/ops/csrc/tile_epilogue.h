// The epilogues of the dense tile GEMMs (three shared by all, and EPI_GLU_MX of the scaled kernels below;tile_gemm.hip: bf16 MFMA; tile_gemm_mx.hip: scaled fp8 x fp4 MFMA;
// tile_gemm_f8.hip: fp8 x fp8 MFMA, which scales its accumulators first). The kernels end with the same picture: 8 waves over a 256 x 256 tile, wave w = row half w & 1 (128 rows) x column group
// w >> 1 (64 columns), a 4 x 2 block of 32 x 32 fp32 accumulators per wave, and an LDS ring that is dead by now.
#pragma once
#include "common.h"
#include "mx_quant.h"

namespace kafka {
namespace tlg {
enum { EPI_PLAIN = 0, EPI_GLU = 1, EPI_SLAB = 2, EPI_GLU_MX = 3 };

// C lane layout (lanes along N): acc[a][b][i] -> row mw + 32 a + (i & 3) + 8 (i >> 2) + 4 h of the tile, column nw +
// 32 b + r of W. Each 32-row group a goes through the wave's own 8 KB LDS tile tp (the ring is dead once every wave is
// past its last stage: the caller has put a barrier behind the main loop; one wave's LDS accesses complete in order, so
// its reads see its writes and the next group's writes follow the reads) and leaves as 16-B ordinary vector stores:
// plain bf16 a whole 128-B line per row and wave, GLU 64 B, slabs 256 B. row0 + rows: the tile's rows of Y / P that
// exist; split: the slab of EPI_SLAB.
template <int EPI>
__device__ __forceinline__ void tile_epilogue(const f32x16 (&acc)[4][2], char* tp, int lane, int mw, int nw, int row0,
                                              int rows, int M, int N, int split, bf16* __restrict__ Y, int64_t ldy,
                                              float* __restrict__ P) {
  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    if constexpr (EPI == EPI_GLU) {
      // (gate, up) = (tile 2 cg, 2 cg + 1): 32 output columns at nw / 2; [32 rows][32] bf16, 4 lanes a row
      bf16* t = reinterpret_cast<bf16*>(tp);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float g = acc[a][0][i], u = acc[a][1][i];
        t[((i & 3) + 8 * (i >> 2) + 4 * h) * 32 + r] = (bf16)(g / (1.0f + __expf(-g)) * u);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int qi = j * 64 + lane, row = qi >> 2, c8 = qi & 3;
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(t + row * 32 + 8 * c8);
        const int m = mw + 32 * a + row;
        if (m < rows) store_bf16x8(Y + (int64_t)(row0 + m) * ldy + (nw >> 1) + 8 * c8, v);
      }
    } else if constexpr (EPI == EPI_PLAIN) {
      // [32 rows][64] bf16, 8 lanes a row: one 128-B line per row
      bf16* t = reinterpret_cast<bf16*>(tp);
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int i = 0; i < 16; ++i) t[((i & 3) + 8 * (i >> 2) + 4 * h) * 64 + 32 * b + r] = (bf16)acc[a][b][i];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int qi = j * 64 + lane, row = qi >> 3, c8 = qi & 7;
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(t + row * 64 + 8 * c8);
        const int m = mw + 32 * a + row;
        if (m < rows) store_bf16x8(Y + (int64_t)(row0 + m) * ldy + nw + 8 * c8, v);
      }
    } else {
      // [32 rows][64] fp32, 16 lanes a row, into this split's slab
      float* t = reinterpret_cast<float*>(tp);
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int i = 0; i < 16; ++i) t[((i & 3) + 8 * (i >> 2) + 4 * h) * 64 + 32 * b + r] = acc[a][b][i];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int qi = j * 64 + lane, row = qi >> 4, c4 = qi & 15;
        const f32x4 v = *reinterpret_cast<const f32x4*>(t + row * 64 + 4 * c4);
        const int m = mw + 32 * a + row;
        if (m < rows) *reinterpret_cast<f32x4*>(P + ((int64_t)split * M + row0 + m) * N + nw + 4 * c4) = v;
      }
    }
  }
}

// The fourth epilogue, EPI_GLU_MX (the scaled kernels tile_gemm_mx.hip and grouped_tile_gemm_mx.hip): silu(g) * u in
// MXFP8 form for the down projection, no bf16 [M, F] written. (gate, up) = (tile 2 cg, 2 cg + 1): the 32 output columns
// at nw / 2 are MX block nw / 64 of the row. Per 32-row group a the wave's LDS tile holds [32 rows][32] bf16 exactly as
// EPI_GLU rounds it; in the read-back 4 lanes hold a row, 8 columns each = one block: they run the quantiser's body
// (mx_quant.h) and store 8 B of e4m3 each to Aq [., F] and one e8m0 byte to Ae [., F / 32], both contiguous. The bytes
// are ops.reference.mxfp8_quant of the bf16 GLU output bit for bit. Row and N-tail rules as above.
__device__ __forceinline__ void tile_epilogue_glu_mx(const f32x16 (&acc)[4][2], char* tp, int lane, int mw, int nw,
                                                     int row0, int rows, int F, uint8_t* __restrict__ Aq,
                                                     uint8_t* __restrict__ Ae) {
  const int r = lane & 31, h = lane >> 5;
  bf16* t = reinterpret_cast<bf16*>(tp);
#pragma unroll
  for (int a = 0; a < 4; ++a) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float g = acc[a][0][i], u = acc[a][1][i];
      t[((i & 3) + 8 * (i >> 2) + 4 * h) * 32 + r] = (bf16)(g / (1.0f + __expf(-g)) * u);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int qi = j * 64 + lane, row = qi >> 2, c8 = qi & 3;
      const u32x4 raw = *reinterpret_cast<const u32x4*>(t + row * 32 + 8 * c8);
      uint32_t o[2];
      const int eb = mxfp8_quant_lane(raw, o);  // (every lane takes part: rows past the tile's are not stored)
      const int m = mw + 32 * a + row;
      if (m < rows) {
        const int64_t gr = (int64_t)row0 + m;
        *reinterpret_cast<uint2*>(Aq + gr * F + (nw >> 1) + 8 * c8) = make_uint2(o[0], o[1]);
        if (c8 == 0) Ae[gr * (F >> 5) + (nw >> 6)] = (uint8_t)eb;
      }
    }
  }
}

typedef __attribute__((address_space(3))) void lds_t;
__device__ __forceinline__ void dma16(const void* g, char* lds) {
  __builtin_amdgcn_global_load_lds(g, (lds_t*)lds, 16, 0, 0);
}
__device__ __forceinline__ void dma4(const void* g, char* lds) {
  __builtin_amdgcn_global_load_lds(g, (lds_t*)lds, 4, 0, 0);
}
}  // namespace tlg
}  // namespace kafka
