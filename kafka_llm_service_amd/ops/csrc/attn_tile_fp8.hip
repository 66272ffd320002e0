// Tile attention v3 on an fp8 KV cache: the e4m3-page instantiations of attn_tile_kernel (attn_tile.h, "fp8 KV cache"
// in its header) and their launch. A unit of its own because it is built with packed-fp32 VALU selection off
// (ops/build.py NO_PK_F32, as the quantised GEMM units), which the bf16 instantiations in attn_tile.hip are not: their
// device code stays what it was.
#include "attn_tile.h"

namespace kafka {

hipError_t launch_attn_tile_fp8(const AttnWorkItem* items, int n_items, const bf16* q, int64_t q_stride,
                                const void* k_cache, const void* v_cache, int Hkv, int G, const int* block_tables,
                                int bt_stride, const int* q_limit, bf16* out, int64_t out_stride, float* out_part,
                                float* lse_part, int S_total, float scale_log2, int part_bf16, AltPart ap,
                                hipStream_t st) {
  // the cascade launch (bf16 partials) streams its pages nt and stores its partials sc1, as the bf16 kernel's
  auto kern = part_bf16 ? attn_tile_kernel<0, 2, 1, true> : attn_tile_kernel<0, 0, 0, true>;
  kern<<<dim3(Hkv, n_items), 512, 0, st>>>(items, q, q_stride, static_cast<const bf16*>(k_cache),
                                           static_cast<const bf16*>(v_cache), Hkv, G, block_tables, bt_stride, q_limit,
                                           out, out_stride, out_part, lse_part, S_total, scale_log2, part_bf16, ap);
  return hipGetLastError();
}

}  // namespace kafka
