// The table-walk grammars for gfx950, structured outputs and the automaton tool grammar: the vocabulary mask of a row's
// automaton state, built on the device from the request's own transition table, and the state's advance over the token
// the sampler drew. engine/json_schema.py compiles a schema (engine/tool_automaton.py: the body of a tool call) to
// `cls` uint8 [256] (byte -> class) and `trans` uint16 [S, C] (next state; START 0, DONE 1, DEAD 0xFFFF);
// ops/reference.py holds the definitions (schema_walk / schema_mask_ref / schema_advance_ref, tool_mask_ref /
// tool_advance_ref). Both kernels agree with those bit for bit — everything here is integer work.
//
// Tables live in a device pool: strans uint16 [n_tabs, SCHEMA_TAB_BYTES / 2], scls uint8 [n_tabs, 256], sdim int32
// [n_tabs, 2] = (S, C). A launch carries rows of one width, `row_ints`:
//   3  a schema row (sampled row, slot, table). Its state is the record (state, 0, 0, table + 1) of its slot in the
//      state table JSON mode owns too (`jstate`; word 3 is 0 for a JSON-mode row). Word 1 is not read: the row is a
//      BODY row without an envelope, and once the state is DONE the allowed ids are the launch's EOS ids.
//   5  a tool row (sampled row, slot, table, open id, close id) with the record (state, phase, 0, table + 1). `open`
//      and `close` are two special tokens without bytes around the body:
//        TOOL_FREE   nothing drawn yet under tool_choice "auto": every id is allowed; `open` -> (START, TOOL_BODY), any
//                    other id -> TOOL_TEXT
//        TOOL_OPEN   a call is required: only `open`; `open` -> (START, TOOL_BODY), any other id -> DEAD
//        TOOL_BODY   state != DONE: the ids with bytes whose walk over the table stays below S, and the state walks;
//                    state == DONE: only `close`; `close` -> TOOL_CLOSED, any other id -> DEAD
//        TOOL_TEXT   free text: every id, the record stays
//        TOOL_CLOSED only `close`, the record stays
//
// table_mask_kernel<LDS, DWORD>   grid (ceil(V / (256 * iters)), rows), 256 threads. A BODY row before DONE whose state
//   is below S is a WALK row. The workgroup stages `cls` in LDS (every class clamped below C) and, when LDS is set, the
//   table's S * C * 2 bytes with 16-byte copies; the other instantiation walks the table in global memory (read-only,
//   L2 resident). The launch says up to which size tables go to LDS (at most SCHEMA_LDS_BYTES) and allocates that much
//   dynamically. SCHEMA_LDS_BYTES + 256 is 160 KiB / 8: eight workgroups per CU whatever the pool holds (a 32 KiB
//   array left 4 per CU and made the LDS path slower than the global one). A launch runs over all rows and a workgroup
//   whose table belongs to the other instantiation leaves at once, so one step may mix both. Every lane walks one
//   token: s = trans[s * C + cls[b]] until the token ends or s >= S (DEAD is 0xFFFF >= S). DWORD reads the token's
//   bytes through aligned 4-byte loads (the byte table is padded by 16 bytes). One wave ballot is 64 mask bits, stored
//   by lane 0 (common.h: mask_store64); a token past V contributes a zero bit and a token without bytes is never
//   allowed.
//   Every other row is a FILL row: all ones below V (FREE, TEXT), zeros (a BODY state at or above S that is not
//   DONE), or a set of at most JSON_MAX_EOS ids: `open` (OPEN), `close` (CLOSED, a tool row in DONE), the EOS ids (a
//   schema row in DONE). A fill stages nothing. Which instantiation writes it is the launch's `fill` argument:
//   FILL_NONE no fill row, FILL_ALL every fill row, FILL_SIZED the fill rows whose table has this instantiation's size
//   class. The launcher hands FILL_ALL to the first instantiation it launches and FILL_NONE to the second, so every
//   row is written exactly once. The exception is a schema launch of one instantiation only (kinds 1 or 2), which gets
//   FILL_SIZED: a row of the size class the caller left out stays untouched, walk or fill.
// table_advance_kernel   one thread per row, behind the sampler: the phases above, a schema row entering at BODY. It
//   walks the sampled id's bytes over the table in global memory; an id without bytes or outside the vocabulary gives
//   DEAD. Word 3 stays table + 1; a schema row writes only word 0 and stays DONE once there.
// Skipped, nothing written: a row whose sampled row, slot or table lies outside its array, a table whose (S, C) is
// outside the limits, a record whose word 3 names another table (or a JSON-mode row), and for a tool row a phase outside
// 0..4 or an `open` or `close` outside [0, V): a bad index never becomes an out-of-range access or a walk of one
// table's state over another table.
#include "common.h"

namespace kafka {

constexpr int TG_NT = 256;
constexpr int FILL_NONE = 0, FILL_ALL = 1, FILL_SIZED = 2;

// a row's indices inside their arrays; a tool row's `open` and `close` inside the vocabulary
__device__ __forceinline__ bool table_row_ok(const int* __restrict__ p, int row_ints, int n_sampled, int n_slots,
                                             int n_tabs, int V) {
  if (p[0] < 0 || p[0] >= n_sampled || p[1] < 0 || p[1] >= n_slots || p[2] < 0 || p[2] >= n_tabs) return false;
  return row_ints != TOOL_ROW_INTS || (p[3] >= 0 && p[3] < V && p[4] >= 0 && p[4] < V);
}

// a pool table's S, or 0 where (S, C) is outside the limits
__device__ __forceinline__ int table_states(int S, int C) {
  const bool ok = S >= 2 && S <= SCHEMA_MAX_STATES && C >= 1 && C <= 256 && S * C * 2 <= SCHEMA_TAB_BYTES;
  return ok ? S : 0;
}

// the state after the bytes [lo, hi) of the token table; `tr` and `cl` in LDS or in global memory
template <bool DWORD, typename PT, typename PC>
__device__ __forceinline__ uint32_t schema_token(uint32_t s, PT tr, PC cl, uint32_t S, uint32_t C,
                                                 const uint8_t* __restrict__ tok_bytes, int lo, int hi) {
  if (DWORD) {
    const uint32_t* __restrict__ words = reinterpret_cast<const uint32_t*>(tok_bytes);
    uint32_t w = lo < hi ? words[lo >> 2] : 0u;
    for (int j = lo; j < hi && s < S; ++j) {
      if ((j & 3) == 0 && j != lo) w = words[j >> 2];
      const uint32_t b = (w >> ((j & 3) * 8)) & 0xFFu;
      s = tr[s * C + cl[b]];
    }
  } else {
    for (int j = lo; j < hi && s < S; ++j) s = tr[s * C + cl[tok_bytes[j]]];
  }
  return s;
}

template <bool LDS, bool DWORD>
__global__ void __launch_bounds__(TG_NT) table_mask_kernel(const uint16_t* __restrict__ strans,
                                                           const uint8_t* __restrict__ scls,
                                                           const int* __restrict__ sdim, int n_tabs,
                                                           const int* __restrict__ tok_off,
                                                           const uint8_t* __restrict__ tok_bytes, int V,
                                                           const int* __restrict__ rows, int row_ints, int n_sampled,
                                                           const int* __restrict__ eos, int n_eos,
                                                           const int* __restrict__ jstate, int n_slots,
                                                           uint32_t* __restrict__ mask_tab, int64_t mask_ld,
                                                           int json_row0, int iters, int lds_bytes, int fill) {
  // dynamic LDS: cls [256], then (LDS) lds_bytes of table — sized by the launch, not by SCHEMA_LDS_BYTES, so small
  // tables leave the CU's LDS to more workgroups
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint8_t* cl = smem;
  uint16_t* tr_lds = reinterpret_cast<uint16_t*>(smem + 256);
  const int* __restrict__ rw = rows + (int64_t)blockIdx.y * row_ints;
  const bool tool = row_ints == TOOL_ROW_INTS;
  // (everything up to the loop is uniform: the whole workgroup leaves)
  if (!table_row_ok(rw, row_ints, n_sampled, n_slots, n_tabs, V)) return;
  const int slot = rw[1], tab = rw[2];
  const uint32_t C = (uint32_t)sdim[2 * tab + 1], S = (uint32_t)table_states(sdim[2 * tab], (int)C);
  if (S == 0) return;
  const int4 rec4 = *reinterpret_cast<const int4*>(jstate + (int64_t)slot * JSON_STATE_INTS);
  if (rec4.w != tab + 1) return;  // the slot's record belongs to another table (or to a JSON-mode row): not this row's
  if (tool && (rec4.y < 0 || rec4.y >= TOOL_PHASES)) return;
  const uint32_t rec = (uint32_t)rec4.x;
  const int phase = tool ? rec4.y : TOOL_BODY;
  const bool done = rec == (uint32_t)SCHEMA_DONE;
  const bool walk = phase == TOOL_BODY && !done && rec < S;
  const bool sized = ((int)(S * C * 2) <= lds_bytes) == LDS;  // (lds_bytes <= SCHEMA_LDS_BYTES)
  if (walk ? !sized : fill == FILL_NONE || (fill == FILL_SIZED && !sized)) return;
  // a fill row: every id (n_ids = -1) or the n_ids ids at `ids` (none: a BODY state at or above S that is not DONE)
  const int* __restrict__ ids = eos;
  int n_ids = 0;
  if (phase == TOOL_FREE || phase == TOOL_TEXT) n_ids = -1;
  else if (phase == TOOL_OPEN) ids = rw + 3, n_ids = 1;
  else if (phase == TOOL_CLOSED || (tool && done)) ids = rw + 4, n_ids = 1;
  else if (done) n_ids = n_eos;
  const uint16_t* __restrict__ tr_g = strans + (int64_t)tab * (SCHEMA_TAB_BYTES / 2);
  if (walk) {
    cl[threadIdx.x] = (uint8_t)min((uint32_t)scls[(int64_t)tab * 256 + threadIdx.x], C - 1);
    if (LDS) {
      const int n16 = (int)(S * C * 2 + 15) >> 4;  // <= lds_bytes / 16 (a multiple of 16); the pool row is longer
      const uint4* src = reinterpret_cast<const uint4*>(tr_g);
      uint4* dst = reinterpret_cast<uint4*>(tr_lds);
      for (int i = threadIdx.x; i < n16; i += TG_NT) dst[i] = src[i];
    }
    __syncthreads();
  }
  uint32_t* row = mask_tab + (int64_t)(json_row0 + slot) * mask_ld;
  const int W = (V + 31) >> 5;
  const int lane = threadIdx.x & 63;
#pragma unroll 1
  for (int it = 0; it < iters; ++it) {
    const int64_t t64 = ((int64_t)blockIdx.x * iters + it) * TG_NT + (threadIdx.x & ~63);  // the wave's first token
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
    } else if (n_ids < 0) {
      const int n = V - t0;  // >= 1
      bal = n >= 64 ? ~0ull : (1ull << n) - 1ull;
    } else {
      bal = 0ull;
      for (int k = 0; k < n_ids; ++k) {  // (n_ids <= JSON_MAX_EOS; an id outside [0, V) sets nothing)
        const uint32_t id = (uint32_t)ids[k], d = id - (uint32_t)t0;
        if (id < (uint32_t)V && d < 64u) bal |= 1ull << d;
      }
    }
    if (lane == 0) mask_store64(row, W, t0, bal);
  }
}

__global__ void __launch_bounds__(64) table_advance_kernel(const uint16_t* __restrict__ strans,
                                                           const uint8_t* __restrict__ scls,
                                                           const int* __restrict__ sdim, int n_tabs,
                                                           const int* __restrict__ tok_off,
                                                           const uint8_t* __restrict__ tok_bytes, int V,
                                                           const int* __restrict__ rows, int row_ints, int n_rows,
                                                           const int64_t* __restrict__ sampled, int n_sampled,
                                                           int* __restrict__ jstate, int n_slots) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n_rows) return;
  const int* __restrict__ rw = rows + (int64_t)i * row_ints;
  const bool tool = row_ints == TOOL_ROW_INTS;
  if (!table_row_ok(rw, row_ints, n_sampled, n_slots, n_tabs, V)) return;
  const int tab = rw[2];
  const uint32_t C = (uint32_t)sdim[2 * tab + 1], S = (uint32_t)table_states(sdim[2 * tab], (int)C);
  if (S == 0) return;
  int* rec = jstate + (int64_t)rw[1] * JSON_STATE_INTS;
  if (rec[3] != tab + 1) return;  // (as the mask kernel: the record is another table's)
  const int phase = tool ? rec[1] : TOOL_BODY;
  if (phase < 0 || phase >= TOOL_PHASES || phase == TOOL_TEXT || phase == TOOL_CLOSED) return;
  uint32_t s = (uint32_t)rec[0];
  int ph = phase;
  const int64_t t = sampled[rw[0]];
  if (phase == TOOL_FREE) {
    if (t == rw[3]) s = 0, ph = TOOL_BODY;  // (START)
    else ph = TOOL_TEXT;
  } else if (phase == TOOL_OPEN) {
    if (t == rw[3]) s = 0, ph = TOOL_BODY;
    else s = SCHEMA_DEAD;
  } else if (s == (uint32_t)SCHEMA_DONE) {
    if (!tool) return;  // (a schema row stays DONE)
    if (t == rw[4]) ph = TOOL_CLOSED;
    else s = SCHEMA_DEAD;
  } else if (s >= S || t < 0 || t >= V) {
    s = SCHEMA_DEAD;
  } else {
    const int lo = tok_off[t], hi = tok_off[t + 1];
    if (hi <= lo) {
      s = SCHEMA_DEAD;
    } else {
      const uint16_t* __restrict__ tr = strans + (int64_t)tab * (SCHEMA_TAB_BYTES / 2);
      const uint8_t* __restrict__ cl = scls + (int64_t)tab * 256;
      for (int j = lo; j < hi && s < S; ++j) s = tr[s * C + min((uint32_t)cl[tok_bytes[j]], C - 1)];
      if (s >= S) s = SCHEMA_DEAD;
    }
  }
  rec[0] = (int)s;  // (word 2 stays 0, word 3 stays table + 1)
  if (tool) rec[1] = ph;
}

template <bool LDS, bool DWORD>
static void table_mask_run(dim3 grid, hipStream_t st, const uint16_t* strans, const uint8_t* scls, const int* sdim,
                           int n_tabs, const int* tok_off, const uint8_t* tok_bytes, int V, const int* rows,
                           int row_ints, int n_sampled, const int* eos, int n_eos, const int* jstate, int n_slots,
                           uint32_t* mask_tab, int64_t mask_ld, int json_row0, int iters, int lds_bytes, int fill) {
  table_mask_kernel<LDS, DWORD><<<grid, TG_NT, 256 + (LDS ? lds_bytes : 0), st>>>(
      strans, scls, sdim, n_tabs, tok_off, tok_bytes, V, rows, row_ints, n_sampled, eos, n_eos, jstate, n_slots,
      mask_tab, mask_ld, json_row0, iters, lds_bytes, fill);
}

// strans / scls / sdim: the table pool (n_tabs tables); tok_off int32 [V + 1] with tok_off[V] bytes in tok_bytes, which
// is padded by at least 4 readable bytes; rows int32 [n_rows, row_ints]; jstate int32 [n_slots, 4]; the mask of slot s
// is row json_row0 + s of mask_tab (uint32 [mask_rows, mask_ld], mask_ld * 32 >= V). kinds (kinds_min..3): bit 0
// launches the LDS instantiation, bit 1 the global-memory one (the caller knows which sizes its pool holds; 3 is always
// right). lds_bytes (a multiple of 16, at most SCHEMA_LDS_BYTES): tables up to this size are staged in LDS, larger ones
// are walked in global memory — the LDS instantiation allocates exactly this much, so a pool of small tables keeps the
// occupancy of a small allocation. tokens: tokens of one workgroup, a multiple of 256; dword: aligned 4-byte token
// loads.
static hipError_t table_mask_launch(const uint16_t* strans, const uint8_t* scls, const int* sdim, int n_tabs,
                                    const int* tok_off, const uint8_t* tok_bytes, int V, const int* rows, int row_ints,
                                    int n_rows, int n_sampled, const int* eos, int n_eos, const int* jstate,
                                    int n_slots, uint32_t* mask_tab, int64_t mask_ld, int64_t mask_rows, int json_row0,
                                    int kinds_min, int kinds, int lds_bytes, int tokens, int dword, hipStream_t st) {
  if (n_rows == 0) return hipSuccess;
  if (V < 1 || n_rows < 0 || n_rows > 65535 || n_eos < 0 || n_eos > JSON_MAX_EOS || mask_ld * 32 < V ||
      json_row0 < 0 || (int64_t)json_row0 + n_slots > mask_rows || n_tabs < 1 || n_sampled < 0 || tokens < TG_NT ||
      tokens % TG_NT != 0 || tokens > (1 << 20) || kinds < kinds_min || kinds > 3 || lds_bytes < 0 ||
      lds_bytes > SCHEMA_LDS_BYTES || lds_bytes % 16 != 0)
    return hipErrorInvalidValue;
  const dim3 grid((V + tokens - 1) / tokens, n_rows);
  const int iters = tokens / TG_NT;
#define TG_RUN(L, D, F)                                                                                               \
  table_mask_run<L, D>(grid, st, strans, scls, sdim, n_tabs, tok_off, tok_bytes, V, rows, row_ints, n_sampled, eos,    \
                       n_eos, jstate, n_slots, mask_tab, mask_ld, json_row0, iters, lds_bytes, F)
  // (the kernel's header: who writes the fill rows)
  int fill = row_ints != TOOL_ROW_INTS && kinds != 3 ? FILL_SIZED : FILL_ALL;
  if (kinds & 1) {
    if (dword) TG_RUN(true, true, fill); else TG_RUN(true, false, fill);
    fill = FILL_NONE;
  }
  if (kinds & 2) {
    if (dword) TG_RUN(false, true, fill); else TG_RUN(false, false, fill);
  }
#undef TG_RUN
  return hipGetLastError();
}

static hipError_t table_advance_launch(const uint16_t* strans, const uint8_t* scls, const int* sdim, int n_tabs,
                                       const int* tok_off, const uint8_t* tok_bytes, int V, const int* rows,
                                       int row_ints, int n_rows, const int64_t* sampled, int n_sampled, int* jstate,
                                       int n_slots, hipStream_t st) {
  if (n_rows == 0) return hipSuccess;
  if (V < 1 || n_rows < 0 || n_sampled < 0 || n_tabs < 1) return hipErrorInvalidValue;
  table_advance_kernel<<<(n_rows + 63) / 64, 64, 0, st>>>(strans, scls, sdim, n_tabs, tok_off, tok_bytes, V, rows,
                                                          row_ints, n_rows, sampled, n_sampled, jstate, n_slots);
  return hipGetLastError();
}

extern "C" hipError_t kafka_launch_schema_mask(const uint16_t* strans, const uint8_t* scls, const int* sdim,
                                               int n_tabs, const int* tok_off, const uint8_t* tok_bytes, int V,
                                               const int* eos, int n_eos, const int* srows, int n_rows,
                                               int n_sampled, const int* jstate, int n_slots, uint32_t* mask_tab,
                                               int64_t mask_ld, int64_t mask_rows, int json_row0, int kinds,
                                               int lds_bytes, int tokens, int dword, hipStream_t st) {
  return table_mask_launch(strans, scls, sdim, n_tabs, tok_off, tok_bytes, V, srows, 3, n_rows, n_sampled, eos, n_eos,
                           jstate, n_slots, mask_tab, mask_ld, mask_rows, json_row0, 0, kinds, lds_bytes, tokens,
                           dword, st);
}

extern "C" hipError_t kafka_launch_tool_mask(const uint16_t* strans, const uint8_t* scls, const int* sdim, int n_tabs,
                                             const int* tok_off, const uint8_t* tok_bytes, int V, const int* trows,
                                             int n_rows, int n_sampled, const int* jstate, int n_slots,
                                             uint32_t* mask_tab, int64_t mask_ld, int64_t mask_rows, int json_row0,
                                             int kinds, int lds_bytes, int tokens, int dword, hipStream_t st) {
  return table_mask_launch(strans, scls, sdim, n_tabs, tok_off, tok_bytes, V, trows, TOOL_ROW_INTS, n_rows, n_sampled,
                           nullptr, 0, jstate, n_slots, mask_tab, mask_ld, mask_rows, json_row0, 1, kinds, lds_bytes,
                           tokens, dword, st);
}

extern "C" hipError_t kafka_launch_schema_advance(const uint16_t* strans, const uint8_t* scls, const int* sdim,
                                                  int n_tabs, const int* tok_off, const uint8_t* tok_bytes, int V,
                                                  const int* srows, int n_rows, const int64_t* sampled,
                                                  int n_sampled, int* jstate, int n_slots, hipStream_t st) {
  return table_advance_launch(strans, scls, sdim, n_tabs, tok_off, tok_bytes, V, srows, 3, n_rows, sampled, n_sampled,
                              jstate, n_slots, st);
}

extern "C" hipError_t kafka_launch_tool_advance(const uint16_t* strans, const uint8_t* scls, const int* sdim,
                                                int n_tabs, const int* tok_off, const uint8_t* tok_bytes, int V,
                                                const int* trows, int n_rows, const int64_t* sampled, int n_sampled,
                                                int* jstate, int n_slots, hipStream_t st) {
  return table_advance_launch(strans, scls, sdim, n_tabs, tok_off, tok_bytes, V, trows, TOOL_ROW_INTS, n_rows, sampled,
                              n_sampled, jstate, n_slots, st);
}

}  // namespace kafka
