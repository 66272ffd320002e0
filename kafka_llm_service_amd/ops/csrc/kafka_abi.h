// The contract between the kernel units (csrc/*.hip, hipcc) and their host callers (csrc/bindings.cpp, g++; other
// .hip units): every `extern "C"` launcher's prototype, the structs that cross the seam and the layout constants
// more than one unit relies on. Both sides include this file (the .hip units through common.h), so a definition that
// disagrees with its prototype here is a compile error (conflicting `extern "C"` declaration) instead of a call
// with shifted arguments. No device code and no torch in here.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

// bf16 storage: the clang scalar type in the kernel units, its raw 16 bits on the g++ side
#ifdef __HIPCC__
typedef __bf16 bf16;
#else
typedef unsigned short bf16;
#endif

namespace kafka {

// ---- paged KV cache layout (rope_kv.hip writes it, attention.hip / attn_tile.hip read it) ------------------------
constexpr int PAGE = 16;                 // tokens per page
// fp8 (e4m3) pages of head dim 128, per (block, kv head) — layout in rope_kv.hip
constexpr int KPAGE8 = PAGE * 128 + 32;  // K page bytes: data + K/V exponents
constexpr int VPAGE8 = PAGE * 128;       // V page bytes
constexpr int KEXP8 = PAGE * 128;        // int8 K exponent of key o at byte KEXP8 + o of the K page
constexpr int VEXP8 = PAGE * 128 + 16;   // int8 V exponent of key o at byte VEXP8 + vt_pos(o) of the K page

// ---- attention work items: rows of the int32 [n, ITEM_INTS] device tensors the host planner uploads --------------
constexpr int ITEM_INTS = 8;

// One tile of query rows against a paged key range (attn_prefill_kernel, attn_tile_kernel)
struct AttnWorkItem {
  int q_start;  // first query token (row of q / out)
  int q_count;  // tokens in this tile
  int bt_row;   // block-table row used for the keys
  int kv_lo;    // first key position (inclusive)
  int kv_hi;    // last key position (exclusive)
  int split;    // -1: write normalized bf16 to out; >= 0: write partial #split
  int alt;      // tile kernel: != 0 writes the partial to the launch's alt buffer (attn_tile.hip AltPart); the
                // register-staged prefill kernel ignores it
  int pad1;
};

// One decode row's key range [lo, hi): the whole per-thread suffix, or piece `split` of `nsplit` (attention.hip
// "Decode"). Row b's partials live at slots [0, npre) (cascade prefix) and npre + split (this piece).
struct DecodeItem {
  int b, lo, hi, split, nsplit, npre, pad0, pad1;
};

static_assert(sizeof(AttnWorkItem) == ITEM_INTS * sizeof(int), "AttnWorkItem is one row of the items tensor");
static_assert(sizeof(DecodeItem) == ITEM_INTS * sizeof(int), "DecodeItem is one row of the items tensor");

// ---- sampler logit bias (sampling.hip RowProc; engine/logits_proc.py) ---------------------------------------------
// bias_tab int32 [rows, >= 2 * LOGIT_BIAS_MAX]: per row the token ids in strictly ascending order at [0, n), the fp32
// bits of their biases at [LOGIT_BIAS_MAX, LOGIT_BIAS_MAX + n); proc[5] names the row, proc[6] is n (0: no bias)
constexpr int LOGIT_BIAS_MAX = 300;  // OpenAI's bound on the entries of one request's logit_bias

// ---- sampler count table (sampling.hip RowProc; engine/logits_proc.py) --------------------------------------------
// counts[slot][token]: the generated-token count in the low 30 bits (presence / frequency penalties) and this flag
// where the slot's sequence holds the token in its prompt (seeded by the host for repetition-penalty slots only). A
// token is "seen" by the repetition penalty when the word is non-zero.
constexpr int COUNT_SEEN_PROMPT = 1 << 30;

// ---- JSON mode (json_mask.hip; engine/json_mode.py holds the automaton and its transition table) ---------------------
// A row's state record in the device state table is int32 [JSON_STATE_INTS]: (state id, depth, stack bits, 0). The
// kernels name the few states the walk itself assigns; every other id only ever comes out of the table.
constexpr int JSON_STATE_INTS = 4;
constexpr int JSON_MAX_DEPTH = 32;  // open containers; the stack is one bit per level (1 = object) in one word
constexpr int JSON_MAX_EOS = 8;     // EOS ids the mask kernel compares a token with in DONE
constexpr int JSON_EXPECT_KEY = 2, JSON_EXPECT_VALUE = 4, JSON_DONE = 7;

// ---- structured outputs (table_grammar.hip; engine/json_schema.py compiles a schema to cls uint8 [256] + trans uint16
// [S, C]) ---------------------------------------------------------------------------------------------------------------
// A schema row's record in the same state table is (state, 0, 0, table index + 1): word 3 is 0 for a JSON-mode row.
constexpr int SCHEMA_MAX_STATES = 8192;        // states of one compiled automaton
constexpr int SCHEMA_TAB_BYTES = 256 * 1024;   // one table of the device pool: S * C * 2 bytes at most
// up to here the mask kernel stages the table in LDS: with the 256 B of cls, 160 KiB / 8, so eight 256-thread workgroups
// (the CU's 32 waves) stay resident; at 32 KiB (four per CU) the LDS path measured slower than the global-memory walk
constexpr int SCHEMA_LDS_BYTES = 20 * 1024 - 256;
constexpr int SCHEMA_DEAD = 0xFFFF, SCHEMA_DONE = 1;  // (START is 0)

// ---- automaton tool grammar (table_grammar.hip; engine/tool_automaton.py compiles a call's body to a schema table) ---
// A tool row's record in the same state table is (state, phase, 0, table index + 1); a row of the launch is int32
// [TOOL_ROW_INTS] = (sampled row, slot, table, open id, close id).
constexpr int TOOL_ROW_INTS = 5;
constexpr int TOOL_FREE = 0, TOOL_OPEN = 1, TOOL_BODY = 2, TOOL_TEXT = 3, TOOL_CLOSED = 4, TOOL_PHASES = 5;

// ---- weight tile formats of the streaming GEMMs (wstream_gemm.hip WFMT; ops.WEIGHT_FORMATS) ----------------------
// bf16 tiles [N/32][K/16][64 lanes][8]; fp8: e4m3 bytes [N/32][K/32][64][16] + fp32 row scales [N]; MXFP4: e2m1 bytes
// [N/32][K/64][64][16] + e8m0 block exponents [N/32][K/64][32][2]
enum { WF_BF16 = 0, WF_FP8 = 1, WF_MXFP4 = 2 };

// ---- arguments of the fused decode-layer GEMM epilogues (wstream_gemm.hip FIN_*) ---------------------------------
struct FinArgs {
  int* tickets;                 // [N / 128] zeroed once, re-armed by each column block's finisher
  union {
    const float* ss_in;         // [nss][ss_ld] partial sums of h^2 of X's rows (nullptr: X is already normalised)
    const void* wscale;         // FIN_NONE on quantised tiles: their scales (fp8 row scales / mxfp4 exponent image)
  };
  int nss, ss_ld;
  float inv_d, eps;
  bf16* resid;                  // FIN_RES: residual stream [M, N] (row stride ldr), updated in place
  int64_t ldr;
  const bf16* nw;               // FIN_RES: the next RMSNorm's weight [N]
  bf16* xn;                     // FIN_RES: bf16(h (.) nw) [M, N] (row stride ldxn): the next GEMM's A operand
  int64_t ldxn;
  float* ss_out;                // FIN_RES: [N / 128][ss_out_ld]
  int ss_out_ld;
  const int64_t* positions;     // FIN_ROPE
  const float* cos_sin;         // [max_pos, 128]: cos in [0, 64), sin in [64, 128)
  bf16* q_out;                  // [M, Hq, 128] (row stride q_stride)
  int64_t q_stride;
  bf16* k_cache;                // [blocks, Hkv, 16, 128] in D/8 chunk planes (rope_kv.hip)
  bf16* v_cache;                // [blocks, Hkv, 128, 16] V^T, key o at vt_pos(o)
  const int64_t* slots;         // [M] (-1: no KV write) or nullptr
  int Hq, Hkv;
  uint64_t* stamps;             // optional phase stamps [grid][8] (100 MHz clock; benchmarks/fused_bench.py)
  int* err;                     // bit 0 set if a finisher could not reach a split's slab (wstream_gemm.hip "home XCD")
};
static_assert(sizeof(FinArgs) == 168 && offsetof(FinArgs, ss_in) == 8, "the union must not move the kernels' arguments");

}  // namespace kafka

extern "C" {

// ---- norm_act.hip
hipError_t kafka_launch_rmsnorm(bf16* out, int64_t os, const bf16* x, int64_t xs, const bf16* w, int T, int d,
                                float eps, hipStream_t st);
hipError_t kafka_launch_fused_add_rmsnorm(bf16* out, int64_t os, const bf16* x, int64_t xs, bf16* resid, int64_t rs,
                                          const bf16* w, int T, int d, float eps, hipStream_t st);
// fused add + RMSNorm whose x input is S fp32 split-K slabs [S][T][d] (row stride d, slab stride ps)
hipError_t kafka_launch_fused_add_rmsnorm_slab(bf16* out, int64_t os, const float* xp, int S, int64_t ps, bf16* resid,
                                               int64_t rs, const bf16* w, int T, int d, float eps, hipStream_t st);
hipError_t kafka_launch_silu_mul(bf16* out, const bf16* x, int64_t xs, int T, int F, hipStream_t st);
// SwiGLU over S fp32 split-K slabs [S][T][2F]
hipError_t kafka_launch_silu_mul_slab(bf16* out, const float* xp, int S, int64_t ps, int T, int F, hipStream_t st);

// ---- rope_kv.hip
// qp != nullptr: the input is S fp32 slabs [S][T][(Hq + 2 Hkv) D] (slab stride ps) instead of bf16 qkv
hipError_t kafka_launch_rope_kv(const bf16* qkv, const float* qp, int S, int64_t ps, int64_t qkv_stride,
                                const int64_t* positions, const float* cos_sin, bf16* q_out, int64_t q_stride,
                                bf16* k_cache, bf16* v_cache, const int64_t* slot_mapping, int T, int Hq, int Hkv,
                                int D, int block_size, hipStream_t st);
hipError_t kafka_launch_rope_kv_fp8(const bf16* qkv, const float* qp, int S, int64_t ps, int64_t qkv_stride,
                                    const int64_t* positions, const float* cos_sin, bf16* q_out, int64_t q_stride,
                                    uint8_t* k_cache, uint8_t* v_cache, const int64_t* slot_mapping, int T, int Hq,
                                    int Hkv, int D, hipStream_t st);

// ---- attention.hip
// items: int32 [n_items, ITEM_INTS] DecodeItem records (host-checked: npre + nsplit <= S_total, and <= 64 with `out`
// — the fused merge gives one wave lane per partial; items with nsplit > 1 merge through the ticket counters
// ([B * Hkv] int32, zero, re-armed by the kernel)).
hipError_t kafka_launch_attn_decode(const bf16* q, int64_t q_stride, const void* k_cache, const void* v_cache, int fp8,
                                    int n_items, int B, int Hkv, int G, int D, const int* block_tables, int bt_stride,
                                    const int* items, float* out_part, float* lse_part, int S_total, float scale,
                                    bf16* out, int64_t out_stride, int* tickets, const bf16* pre_bf16,
                                    const float* m_part, const float* m_lse, int m_S, int m_rows, bf16* m_out,
                                    int64_t m_out_stride, hipStream_t st);
// items: int32 [n_items, ITEM_INTS] AttnWorkItem records; variant 3 forwards to kafka_launch_attn_tile
hipError_t kafka_launch_attn_prefill(const void* items, int n_items, const bf16* q, int64_t q_stride,
                                     const void* k_cache, const void* v_cache, int fp8, int Hkv, int G, int D,
                                     const int* block_tables, int bt_stride, const int* q_limit, bf16* out,
                                     int64_t out_stride, float* out_part, float* lse_part, int S_total, float scale,
                                     int variant, int part_bf16, float* alt_part, float* alt_lse, int alt_S,
                                     int alt_tok_off, hipStream_t st);
hipError_t kafka_launch_attn_merge(const float* part, const float* lse, int rows, int Hq, int S, int D, bf16* out,
                                   int64_t out_stride, float* lse_out, const bf16* pre, int npre, hipStream_t st);

// ---- attn_tile.hip (called by kafka_launch_attn_prefill)
// Host launcher (bf16 KV only; the fp8 cache keeps tile variant 0). Items: int32 [n, ITEM_INTS] AttnWorkItem records.
hipError_t kafka_launch_attn_tile(const void* items, int n_items, const bf16* q, int64_t q_stride,
                                  const void* k_cache, const void* v_cache, int Hkv, int G, int D,
                                  const int* block_tables, int bt_stride, const int* q_limit, bf16* out,
                                  int64_t out_stride, float* out_part, float* lse_part, int S_total, float scale,
                                  int part_bf16, float* alt_part, float* alt_lse, int alt_S, int alt_tok_off,
                                  hipStream_t st);

// ---- sampling.hip
// ws (optional): int32 workspace of >= SAMPLE_MAX_ROWS + 2 * B * nsplit entries whose first SAMPLE_MAX_ROWS are zero
// (tickets, re-armed by the kernel); without it every row is one workgroup. proc (optional, int32 [B, 8], see
// RowProc) selects the logits-processing instantiation; mask_tab uint32 [rows, mask_ld] and counts int32
// [slots, cnt_ld] (cnt_ld >= V rounded up to 8) are only read for rows that name them; bias_tab (optional, int32
// [rows, bias_ld], bias_ld >= 2 * LOGIT_BIAS_MAX and a multiple of 4) likewise — without it no row is biased.
// proc[7] carries min_p as the fp32 bits of float32(ln(min_p)) (0: off, min_p = 1 is -0.0): a row under temperature
// keeps the tokens with x / T >= max(x / T) + that value. The same workspace serves min_p rows (two ints per split).
// rep_tab (optional, fp32 [slots, 2] with the rows of counts): (r, 1 / r) of each penalty slot's repetition penalty;
// a row with r != 1 multiplies its seen tokens' logits (counts word != 0) before the other penalties.
hipError_t kafka_launch_sample(const void* logits, bool is_bf16, int64_t stride, int B, int V, const float* temperature,
                               const float* top_p, const int* top_k, const int64_t* seeds, const int64_t* step,
                               int64_t* out_tokens, int* ws, int nsplit, const int* proc, const uint32_t* mask_tab,
                               int64_t mask_ld, int* counts, int64_t cnt_ld, const int* bias_tab, int64_t bias_ld,
                               const float* rep_tab, hipStream_t st);

// ---- json_mask.hip
// The vocabulary masks of the step's JSON rows, written into rows json_row0 + slot of mask_tab from the slots' state
// records, and (behind the sampler) the records' advance over the sampled ids. trans: uint8 [64 * 256]; tok_off int32
// [V + 1] / tok_bytes: the tokens' bytes (CSR); eos: n_eos <= JSON_MAX_EOS ids; jrows int32 [n_rows, 2]: (sampled row,
// slot) pairs; jstate int32 [n_slots, JSON_STATE_INTS]; mask_tab uint32 [mask_rows, mask_ld] with mask_ld * 32 >= V
// and json_row0 + n_slots <= mask_rows; sampled int64 [n_sampled]. Nothing is launched for n_rows == 0.
hipError_t kafka_launch_json_mask(const uint8_t* trans, const int* tok_off, const uint8_t* tok_bytes, int V,
                                  const int* eos, int n_eos, const int* jrows, int n_rows, const int* jstate,
                                  int n_slots, uint32_t* mask_tab, int64_t mask_ld, int64_t mask_rows, int json_row0,
                                  hipStream_t st);
hipError_t kafka_launch_json_advance(const uint8_t* trans, const int* tok_off, const uint8_t* tok_bytes, int V,
                                     const int* jrows, int n_rows, const int64_t* sampled, int n_sampled, int* jstate,
                                     int n_slots, hipStream_t st);

// ---- table_grammar.hip: schema rows
// The masks and the advance of the step's schema rows, as the two JSON-mode launches above but over per-request
// tables: strans uint16 [n_tabs, SCHEMA_TAB_BYTES / 2], scls uint8 [n_tabs, 256], sdim int32 [n_tabs, 2] = (S, C);
// srows int32 [n_rows, 3]: (sampled row, slot, table). tok_bytes needs 4 readable bytes behind the last token and a
// 4-byte aligned address. kinds: bit 0 launches the instantiation with the table in LDS (S * C * 2 <= lds_bytes <=
// SCHEMA_LDS_BYTES, a multiple of 16: what the launch allocates), bit 1 the one that walks it in global memory; each
// skips the other's rows, and a launch of one of them leaves the other's rows untouched. tokens: tokens of one
// workgroup (a multiple of 256); dword: read token bytes through aligned 4-byte loads.
hipError_t kafka_launch_schema_mask(const uint16_t* strans, const uint8_t* scls, const int* sdim, int n_tabs,
                                    const int* tok_off, const uint8_t* tok_bytes, int V, const int* eos, int n_eos,
                                    const int* srows, int n_rows, int n_sampled, const int* jstate, int n_slots,
                                    uint32_t* mask_tab, int64_t mask_ld, int64_t mask_rows, int json_row0, int kinds,
                                    int lds_bytes, int tokens, int dword, hipStream_t st);
hipError_t kafka_launch_schema_advance(const uint16_t* strans, const uint8_t* scls, const int* sdim, int n_tabs,
                                       const int* tok_off, const uint8_t* tok_bytes, int V, const int* srows,
                                       int n_rows, const int64_t* sampled, int n_sampled, int* jstate, int n_slots,
                                       hipStream_t st);

// ---- table_grammar.hip: tool rows
// The masks and the advance of the step's tool rows over the schema pool's tables: the same two kernels as above with
// the envelope of a tool call around the walk: trows int32 [n_rows, TOOL_ROW_INTS]. kinds (1..3), lds_bytes, tokens and
// dword as for kafka_launch_schema_mask; a row that needs no walk is written by the first instantiation launched.
hipError_t kafka_launch_tool_mask(const uint16_t* strans, const uint8_t* scls, const int* sdim, int n_tabs,
                                  const int* tok_off, const uint8_t* tok_bytes, int V, const int* trows, int n_rows,
                                  int n_sampled, const int* jstate, int n_slots, uint32_t* mask_tab, int64_t mask_ld,
                                  int64_t mask_rows, int json_row0, int kinds, int lds_bytes, int tokens, int dword,
                                  hipStream_t st);
hipError_t kafka_launch_tool_advance(const uint16_t* strans, const uint8_t* scls, const int* sdim, int n_tabs,
                                     const int* tok_off, const uint8_t* tok_bytes, int V, const int* trows,
                                     int n_rows, const int64_t* sampled, int n_sampled, int* jstate, int n_slots,
                                     hipStream_t st);

// ---- logprobs.hip
// Log softmax of the RAW logits (no temperature / penalties / mask) at each scored row's sampled token, and the row's
// K (0..20) largest entries in the order (value descending, index ascending). rows (optional): int32 [R] rows of
// `logits` (nullptr: rows 0..R-1; the kernel trusts them); tokens: int64 [>= max row + 1], the sampled id of each
// LOGITS row. Record r lands at tok_lp[r * ld], top_lp[r * ld + j], top_id[r * ld + j] (three views of one packed
// buffer). ws (optional): int32 workspace of >= 8192 + R * nsplit * 42 entries whose first 8192 are zero (tickets,
// re-armed by the kernel); without it, or for V < 16384, every row is one workgroup. R <= 8192, nsplit <= 64.
hipError_t kafka_launch_token_logprobs(const void* logits, bool is_bf16, int64_t stride, int V, const int* rows, int R,
                                       const int64_t* tokens, int K, float* tok_lp, float* top_lp, int* top_id,
                                       int64_t ld, int* ws, int nsplit, hipStream_t st);

// ---- wstream_gemm.hip
// Host plan: row tiles MT, K chunk KC and split count S for a shape; returns 0 if supported (mirrored by
// ops.stream_plan). max_splits caps S (1 forces a direct bf16 output).
int kafka_wstream_plan(int M, int N, int K, int max_splits, int* mt, int* kc, int* splits);
// wfmt (WF_*) names the layout of Wt and scale: bf16 tiles and no scale; fp8 tiles (ops.tile_weight_fp8: a lane's
// 16 B are the B fragments of two k-steps) with St [N] fp32 power-of-two row scales in tile order; MXFP4 tiles
// (ops.tile_weight_mxfp4: four k-steps per 16 B, low nibble first) with Se, the e8m0 block exponents (bias 127, in
// [7, 247]). Same plans, configurations and outputs; the quantised formats need nt.
hipError_t kafka_launch_wstream_gemm(const bf16* X, int64_t ldx, int wfmt, const void* Wt, const void* scale, int M,
                                     int N, int K, int mt, int kc, int splits, int nt, int kw, int pin, int glu,
                                     bf16* Y, int64_t ldy, float* P, hipStream_t st);
// Fused decode-layer GEMMs (FIN_RES / FIN_ROPE / FIN_GLU): one row tile (M <= 128), N % 128 == 0, S in
// {1, 2, 4, 8}; P = [S][M][N] fp32 scratch (unused for S == 1); FIN_GLU needs S == 1.
hipError_t kafka_launch_wstream_fin(int fin, const bf16* X, int64_t ldx, const bf16* Wt, int M, int N, int K, int mt,
                                    int kc, int splits, int kw, int pin, bf16* Y, int64_t ldy, float* P,
                                    const kafka::FinArgs* fa, hipStream_t st);
hipError_t kafka_launch_slab_reduce(const float* P, int S, int M, int N, bf16* Y, int64_t ldy, hipStream_t st);
// Grouped streaming GEMM for the expert MLP (see wstream_grouped_kernel). max_rows bounds any expert's segment
// (the token count T: a token picks an expert at most once); glu: gate_up with fused SwiGLU into Y [n_ent, N/2];
// else combine into out_f32 [T, N].
// wfmt: WF_BF16 (Wt [E_local][N/32][K/16][64 lanes][8], no scale), WF_FP8 (e4m3 bytes [E_local][N/32][K/32][64][16]
// and St [E_local][N] fp32 power-of-two row scales in tile order, ops.tile_experts_fp8) or WF_MXFP4 (e2m1 bytes
// [E_local][N/32][K/64][64][16] and Se [E_local][N/32][K/64][32][2] e8m0 block exponents, ops.tile_experts_mxfp4: the
// dense images per expert), tiles and scales indexed by the local expert.
hipError_t kafka_launch_wstream_grouped(const bf16* X, int64_t ldx, int wfmt, const void* Wt, const void* scale,
                                        int e_local, int N, int K, const int* perm_tok, const float* perm_w,
                                        const int* expert_off, int e_lo, int max_rows, int gather, bf16* Y,
                                        int64_t ldy, float* out, int64_t ldo, int pin, hipStream_t st);

// ---- skinny_gemm.hip
// Split plan for a shape (mirrored by ops.skinny_plan): the fewest power-of-two splits that give >= 192 workgroups
// while every split keeps >= 4 K stages of 64.
int kafka_skinny_plan(int M, int N, int K, int max_splits, int* splits);
hipError_t kafka_launch_skinny_gemm(const bf16* X, int64_t ldx, const bf16* Wt, int M, int N, int K, int splits,
                                    int glu, bf16* Y, int64_t ldy, float* P, hipStream_t st);

// ---- moe.hip
hipError_t kafka_launch_moe_route(const bf16* logits, int64_t ld, int T, int E, int K, int BM, float* topk_w,
                                  int* topk_e, int* perm_tok, float* perm_w, int* expert_off, int* tile_off,
                                  hipStream_t st);
hipError_t kafka_launch_grouped_gemm(const bf16* X, int64_t ldx, const bf16* W, int N, int Kd, const int* perm_tok,
                                     const float* perm_w, const int* expert_off, const int* tile_off, int e_lo,
                                     int e_n, int max_tiles, int gather, bf16* Y, int64_t ldy, float* out,
                                     int64_t ldo, hipStream_t st);
hipError_t kafka_launch_ep_dispatch(const bf16* x, int64_t ldx, const int* topk_e, int lo, int n_pairs, int k, int El,
                                    int ep, int C, int MR, int d, bf16* img, int* slot_map, hipStream_t st);
hipError_t kafka_launch_ep_recv_route(const bf16* img, int ep, int C, int MR, int d, int El, int BM, int* perm_tok,
                                      float* perm_w, int* expert_off, int* tile_off, hipStream_t st);
hipError_t kafka_launch_ep_combine(const bf16* back, const int* slot_map, const float* topk_w, int lo, int n_own,
                                   int k, int d, bf16* out, int64_t ldo, hipStream_t st);

// ---- allreduce.hip
hipError_t kafka_car_alloc(int64_t bytes, void** out);
// Host copy of the timing ring ([AR_TIME_SLOTS][2] uint64 = 2 KB) and of block 0's epoch (the call count), on a
// private stream so a /metrics request never waits behind the engine's queued steps.
hipError_t kafka_car_timing(const void* own, uint64_t* ring_out, int* epoch_out);
hipError_t kafka_car_ipc_handle(void* p, hipIpcMemHandle_t* h);
hipError_t kafka_car_open(const hipIpcMemHandle_t* h, void** out);
hipError_t kafka_car_close(void* p);
hipError_t kafka_car_free(void* p);
// x: bf16 input (or nullptr with xp = S fp32 slabs of stride ps elements); y: bf16 output (may alias x).
// Every call of a group must use the same nblocks (the per-block epochs advance together).
hipError_t kafka_launch_car_allreduce(char* const* bases, int nranks, int rank, const bf16* x, const float* xp, int S,
                                      int64_t ps, bf16* y, int64_t n8, int64_t max_bytes, int nblocks,
                                      hipStream_t st);
hipError_t kafka_launch_car_allreduce_add_rmsnorm(char* const* bases, int nranks, int rank, const bf16* x,
                                                  const float* xp, int S, int64_t ps, int T, int d, bf16* resid,
                                                  int64_t rs, const bf16* w, float eps, bf16* out, int64_t os,
                                                  int64_t max_bytes, int nblocks, const bf16* pre, int64_t pre_s,
                                                  int dpre, hipStream_t st);
hipError_t kafka_launch_car_a2a(char* const* bases, int nranks, int rank, const void* send, int64_t nbytes, void* recv,
                                int64_t bpd, int bcast, int64_t max_bytes, int nblocks, hipStream_t st);

}  // extern "C"
