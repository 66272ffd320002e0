// Tile attention v3 (attn_tile.h): the bf16-page instantiations and the host launcher.
#include "attn_tile.h"

namespace kafka {

// Host launcher. Items: int32 [n, 8] AttnWorkItem records; fp8: k_cache / v_cache are e4m3 pages (uint8
// [blocks, Hkv, KPAGE8] / [blocks, Hkv, VPAGE8]).
extern "C" hipError_t kafka_launch_attn_tile(const void* items, int n_items, const bf16* q, int64_t q_stride,
                                            const void* k_cache, const void* v_cache, int fp8, int Hkv, int G, int D,
                                            const int* block_tables, int bt_stride, const int* q_limit, bf16* out,
                                            int64_t out_stride, float* out_part, float* lse_part, int S_total,
                                            float scale, int part_bf16, float* alt_part, float* alt_lse, int alt_S,
                                            int alt_tok_off, hipStream_t st) {
  if (n_items == 0) return hipSuccess;
  if (D != 128 || G < 1 || G > 32 || (256 % G) != 0 || n_items > 65535) return hipErrorInvalidValue;
  const float scale_log2 = scale * 1.4426950408889634f;
  const AltPart ap{alt_part, alt_lse, alt_S, alt_tok_off};
  // (the stamp build below is bf16-only: an fp8 cache runs its production kernels)
  if (fp8)
    return launch_attn_tile_fp8(reinterpret_cast<const AttnWorkItem*>(items), n_items, q, q_stride, k_cache, v_cache,
                                Hkv, G, block_tables, bt_stride, q_limit, out, out_stride, out_part, lse_part, S_total,
                                scale_log2, part_bf16, ap, st);
  static const bool stamps = [] {  // diagnostic build (benchmarks/attn_tile_stamps.py)
    const char* e = getenv("KAFKA_TILE_ABL");
    return e && atoi(e) == 8;
  }();
  // The cascade prefix pass (bf16 partials) reads each K / V tile of the shared prefix once per KV head and 256 query
  // rows (one workgroup at the headline's 64 streams): its DMAs go nt (aux = 2), +0.9 % on the headline
  // (profiles/r05/cascade/bench_ab_kv_nt.jsonl). Prefill launches keep the default policy: their query tiles re-read
  // the same keys.
  // Its bf16 partials are stored sc1 (16-B stores that leave this XCD's L2: +0.2..0.6 %, bench_ab_part_sc1.jsonl).
  auto kern = stamps ? attn_tile_kernel<8> : part_bf16 ? attn_tile_kernel<0, 2, 1> : attn_tile_kernel<0>;
  kern<<<dim3(Hkv, n_items), 512, 0, st>>>(reinterpret_cast<const AttnWorkItem*>(items), q, q_stride,
                                           static_cast<const bf16*>(k_cache), static_cast<const bf16*>(v_cache), Hkv,
                                           G, block_tables, bt_stride, q_limit, out, out_stride, out_part, lse_part,
                                           S_total, scale_log2, part_bf16, ap);
  return hipGetLastError();
}

}  // namespace kafka
