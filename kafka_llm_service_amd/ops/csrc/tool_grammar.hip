// The automaton tool grammar for gfx950: the vocabulary mask of a tool row, and the row's advance over the token the
// sampler drew. engine/tool_automaton.py compiles the body of a tool call to a table of the schema pool
// (json_schema.hip: strans / scls / sdim); what these kernels add is the envelope around it, two special tokens
// without bytes: `open` begins a call, `close` ends it. ops/reference.py holds the definition (tool_mask_ref /
// tool_advance_ref); both kernels agree with it bit for bit — everything here is integer work.
//
// A tool row is int32 [5]: (sampled row, slot, table, open id, close id). Its state is the int32 [4] record (state,
// phase, 0, table + 1) of its slot in `jstate`:
//   TOOL_FREE   nothing drawn yet under tool_choice "auto": every id is allowed; `open` -> (START, TOOL_BODY), any
//               other id -> TOOL_TEXT
//   TOOL_OPEN   a call is required: only `open`; `open` -> (START, TOOL_BODY), any other id -> DEAD
//   TOOL_BODY   state != DONE: the ids with bytes whose walk over the table stays below S (schema_mask_kernel's rule),
//               and the state walks; state == DONE: only `close`; `close` -> TOOL_CLOSED, any other id -> DEAD
//   TOOL_TEXT   free text: every id, the record stays
//   TOOL_CLOSED only `close`, the record stays
//
// tool_mask_kernel<LDS, DWORD>   grid (ceil(V / (256 * iters)), tool rows), 256 threads. A BODY row before DONE whose
//   state is below S is a WALK row: schema_mask_kernel's work, the table in LDS when it fits the launch's lds_bytes
//   and in global memory otherwise, one instantiation each, the other one leaves. Every other row is a FILL row: all
//   ones below V, the single bit of `open` or `close`, or (a BODY state at or above S that is not DONE) zeros. A fill
//   stages nothing and does not look at the table's size; the launch hands it to exactly one instantiation (`fill`).
//   The ballot-to-mask store is json_mask.hip's (schema_walk.h: mask_store64).
// tool_advance_kernel   one thread per row, behind the sampler: the table above; word 3 stays table + 1.
// Skipped, nothing written: a row whose sampled row, slot or table lies outside its array, a table whose (S, C) is
// outside the limits, a record whose word 3 names another table, a phase outside 0..4, an `open` or `close` outside
// [0, V).
#include "common.h"
#include "schema_walk.h"

namespace kafka {

constexpr int TM_NT = 256;

struct ToolRow {
  int r, slot, tab, open, close;
};

__device__ __forceinline__ ToolRow tool_row(const int* __restrict__ trows, int i) {
  const int* p = trows + (int64_t)i * TOOL_ROW_INTS;
  ToolRow t;
  t.r = p[0], t.slot = p[1], t.tab = p[2], t.open = p[3], t.close = p[4];
  return t;
}

__device__ __forceinline__ bool tool_row_ok(const ToolRow& t, int n_sampled, int n_slots, int n_tabs, int V) {
  return t.r >= 0 && t.r < n_sampled && t.slot >= 0 && t.slot < n_slots && t.tab >= 0 && t.tab < n_tabs &&
         t.open >= 0 && t.open < V && t.close >= 0 && t.close < V;
}

template <bool LDS, bool DWORD>
__global__ void __launch_bounds__(TM_NT) tool_mask_kernel(const uint16_t* __restrict__ strans,
                                                          const uint8_t* __restrict__ scls,
                                                          const int* __restrict__ sdim, int n_tabs,
                                                          const int* __restrict__ tok_off,
                                                          const uint8_t* __restrict__ tok_bytes, int V,
                                                          const int* __restrict__ trows, int n_sampled,
                                                          const int* __restrict__ jstate, int n_slots,
                                                          uint32_t* __restrict__ mask_tab, int64_t mask_ld,
                                                          int json_row0, int iters, int lds_bytes, int fill) {
  // dynamic LDS as schema_mask_kernel's: cls [256], then (LDS) lds_bytes of table
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint8_t* cl = smem;
  uint16_t* tr_lds = reinterpret_cast<uint16_t*>(smem + 256);
  const ToolRow tw = tool_row(trows, blockIdx.y);
  // (uniform: the whole workgroup leaves)
  if (!tool_row_ok(tw, n_sampled, n_slots, n_tabs, V)) return;
  const SchemaTab dim = schema_dim(sdim, tw.tab);
  if (dim.S == 0) return;
  const uint32_t S = dim.S, C = dim.C;
  const int4 rec4 = *reinterpret_cast<const int4*>(jstate + (int64_t)tw.slot * JSON_STATE_INTS);
  if (rec4.w != tw.tab + 1 || rec4.y < 0 || rec4.y >= TOOL_PHASES) return;
  const uint32_t rec = (uint32_t)rec4.x;
  const int phase = rec4.y;
  const bool walk = phase == TOOL_BODY && rec != (uint32_t)SCHEMA_DONE && rec < S;
  if (walk ? (dim.S * dim.C * 2 <= lds_bytes) != LDS : !fill) return;
  // a fill row: every id (one = -1), one id, or none (one = -2)
  int one = -2;
  if (!walk) {
    if (phase == TOOL_FREE || phase == TOOL_TEXT) one = -1;
    else if (phase == TOOL_OPEN) one = tw.open;
    else if (phase == TOOL_CLOSED || rec == (uint32_t)SCHEMA_DONE) one = tw.close;
  }
  const uint16_t* __restrict__ tr_g = strans + (int64_t)tw.tab * (SCHEMA_TAB_BYTES / 2);
  if (walk) {
    cl[threadIdx.x] = (uint8_t)min((uint32_t)scls[(int64_t)tw.tab * 256 + threadIdx.x], C - 1);
    if (LDS) {
      const int n16 = (int)(S * C * 2 + 15) >> 4;  // <= lds_bytes / 16 (a multiple of 16); the pool row is longer
      const uint4* src = reinterpret_cast<const uint4*>(tr_g);
      uint4* dst = reinterpret_cast<uint4*>(tr_lds);
      for (int i = threadIdx.x; i < n16; i += TM_NT) dst[i] = src[i];
    }
    __syncthreads();
  }
  uint32_t* row = mask_tab + (int64_t)(json_row0 + tw.slot) * mask_ld;
  const int W = (V + 31) >> 5;
  const int lane = threadIdx.x & 63;
#pragma unroll 1
  for (int it = 0; it < iters; ++it) {
    const int64_t t64 = ((int64_t)blockIdx.x * iters + it) * TM_NT + (threadIdx.x & ~63);  // the wave's first token
    if (t64 >= V) break;  // (uniform per wave; later iterations lie further out)
    const int t0 = (int)t64, t = t0 + lane;
    unsigned long long bal;
    if (walk) {
      bool ok = false;
      if (t < V) {
        const int lo = tok_off[t], hi = tok_off[t + 1];
        uint32_t s;
        if (LDS)
          s = schema_token<DWORD>(rec, tr_lds, cl, S, C, tok_bytes, lo, hi);
        else
          s = schema_token<DWORD>(rec, tr_g, cl, S, C, tok_bytes, lo, hi);
        ok = hi > lo && s < S;
      }
      bal = __ballot(ok);
    } else if (one == -1) {
      const int n = V - t0;  // >= 1
      bal = n >= 64 ? ~0ull : (1ull << n) - 1ull;
    } else {
      const int d = one - t0;  // (one == -2: below zero)
      bal = d >= 0 && d < 64 ? 1ull << d : 0ull;
    }
    if (lane == 0) mask_store64(row, W, t0, bal);
  }
}

__global__ void __launch_bounds__(64) tool_advance_kernel(const uint16_t* __restrict__ strans,
                                                          const uint8_t* __restrict__ scls,
                                                          const int* __restrict__ sdim, int n_tabs,
                                                          const int* __restrict__ tok_off,
                                                          const uint8_t* __restrict__ tok_bytes, int V,
                                                          const int* __restrict__ trows, int n_rows,
                                                          const int64_t* __restrict__ sampled, int n_sampled,
                                                          int* __restrict__ jstate, int n_slots) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n_rows) return;
  const ToolRow tw = tool_row(trows, i);
  if (!tool_row_ok(tw, n_sampled, n_slots, n_tabs, V)) return;
  const SchemaTab dim = schema_dim(sdim, tw.tab);
  if (dim.S == 0) return;
  const uint32_t S = dim.S, C = dim.C;
  int* rec = jstate + (int64_t)tw.slot * JSON_STATE_INTS;
  const int phase = rec[1];
  if (rec[3] != tw.tab + 1 || phase < 0 || phase >= TOOL_PHASES) return;
  if (phase == TOOL_TEXT || phase == TOOL_CLOSED) return;
  uint32_t s = (uint32_t)rec[0];
  int ph = phase;
  const int64_t t = sampled[tw.r];
  if (phase == TOOL_FREE) {
    if (t == tw.open) s = 0, ph = TOOL_BODY;  // (START)
    else ph = TOOL_TEXT;
  } else if (phase == TOOL_OPEN) {
    if (t == tw.open) s = 0, ph = TOOL_BODY;
    else s = SCHEMA_DEAD;
  } else if (s == (uint32_t)SCHEMA_DONE) {
    if (t == tw.close) ph = TOOL_CLOSED;
    else s = SCHEMA_DEAD;
  } else if (s >= S || t < 0 || t >= V) {
    s = SCHEMA_DEAD;
  } else {
    const int lo = tok_off[t], hi = tok_off[t + 1];
    if (hi <= lo) {
      s = SCHEMA_DEAD;
    } else {
      const uint16_t* __restrict__ tr = strans + (int64_t)tw.tab * (SCHEMA_TAB_BYTES / 2);
      const uint8_t* __restrict__ cl = scls + (int64_t)tw.tab * 256;
      for (int j = lo; j < hi && s < S; ++j) s = tr[s * C + min((uint32_t)cl[tok_bytes[j]], C - 1)];
      if (s >= S) s = SCHEMA_DEAD;
    }
  }
  rec[0] = (int)s;  // (word 2 stays 0, word 3 stays table + 1)
  rec[1] = ph;
}

template <bool LDS, bool DWORD>
static void tool_mask_launch(dim3 grid, hipStream_t st, const uint16_t* strans, const uint8_t* scls, const int* sdim,
                             int n_tabs, const int* tok_off, const uint8_t* tok_bytes, int V, const int* trows,
                             int n_sampled, const int* jstate, int n_slots, uint32_t* mask_tab, int64_t mask_ld,
                             int json_row0, int iters, int lds_bytes, int fill) {
  tool_mask_kernel<LDS, DWORD><<<grid, TM_NT, 256 + (LDS ? lds_bytes : 0), st>>>(
      strans, scls, sdim, n_tabs, tok_off, tok_bytes, V, trows, n_sampled, jstate, n_slots, mask_tab, mask_ld,
      json_row0, iters, lds_bytes, fill);
}

// The arrays are kafka_launch_schema_mask's; trows int32 [n_rows, TOOL_ROW_INTS]. kinds: bit 0 launches the LDS
// instantiation, bit 1 the global-memory one; at least one. The first one launched also writes the fill rows.
extern "C" hipError_t kafka_launch_tool_mask(const uint16_t* strans, const uint8_t* scls, const int* sdim, int n_tabs,
                                             const int* tok_off, const uint8_t* tok_bytes, int V, const int* trows,
                                             int n_rows, int n_sampled, const int* jstate, int n_slots,
                                             uint32_t* mask_tab, int64_t mask_ld, int64_t mask_rows, int json_row0,
                                             int kinds, int lds_bytes, int tokens, int dword, hipStream_t st) {
  if (n_rows == 0) return hipSuccess;
  if (V < 1 || n_rows < 0 || n_rows > 65535 || mask_ld * 32 < V || json_row0 < 0 ||
      (int64_t)json_row0 + n_slots > mask_rows || n_tabs < 1 || n_sampled < 0 || tokens < TM_NT ||
      tokens % TM_NT != 0 || tokens > (1 << 20) || kinds < 1 || kinds > 3 || lds_bytes < 0 ||
      lds_bytes > SCHEMA_LDS_BYTES || lds_bytes % 16 != 0)
    return hipErrorInvalidValue;
  const dim3 grid((V + tokens - 1) / tokens, n_rows);
  const int iters = tokens / TM_NT;
#define TM_LAUNCH(L, D, F)                                                                                          \
  tool_mask_launch<L, D>(grid, st, strans, scls, sdim, n_tabs, tok_off, tok_bytes, V, trows, n_sampled, jstate,      \
                         n_slots, mask_tab, mask_ld, json_row0, iters, lds_bytes, F)
  if (kinds & 1) {
    if (dword) TM_LAUNCH(true, true, 1); else TM_LAUNCH(true, false, 1);
  }
  if (kinds & 2) {
    const int fill = (kinds & 1) ? 0 : 1;
    if (dword) TM_LAUNCH(false, true, fill); else TM_LAUNCH(false, false, fill);
  }
#undef TM_LAUNCH
  return hipGetLastError();
}

extern "C" hipError_t kafka_launch_tool_advance(const uint16_t* strans, const uint8_t* scls, const int* sdim,
                                                int n_tabs, const int* tok_off, const uint8_t* tok_bytes, int V,
                                                const int* trows, int n_rows, const int64_t* sampled, int n_sampled,
                                                int* jstate, int n_slots, hipStream_t st) {
  if (n_rows == 0) return hipSuccess;
  if (V < 1 || n_rows < 0 || n_sampled < 0 || n_tabs < 1) return hipErrorInvalidValue;
  tool_advance_kernel<<<(n_rows + 63) / 64, 64, 0, st>>>(strans, scls, sdim, n_tabs, tok_off, tok_bytes, V, trows,
                                                         n_rows, sampled, n_sampled, jstate, n_slots);
  return hipGetLastError();
}

}  // namespace kafka
