// Structured outputs for gfx950: the vocabulary mask of a row's schema automaton state, built on the device from the
// request's own transition table, and the state's advance over the token the sampler drew. engine/json_schema.py
// compiles a schema to `cls` uint8 [256] (byte -> class) and `trans` uint16 [S, C] (next state; START 0, DONE 1, DEAD
// 0xFFFF); ops/reference.py holds the walk (schema_walk / schema_mask_ref / schema_advance_ref). Both kernels agree
// with those bit for bit — everything here is integer work.
//
// Tables live in a device pool: strans uint16 [n_tabs, SCHEMA_TAB_BYTES / 2], scls uint8 [n_tabs, 256], sdim int32
// [n_tabs, 2] = (S, C). A row's state is the int32 [4] record (state, 0, 0, table index + 1) of its slot in the state
// table JSON mode owns too (`jstate`; word 3 is 0 for a JSON-mode row).
//
// schema_mask_kernel<LDS, DWORD>   grid (ceil(V / (256 * iters)), schema rows), 256 threads. A row is (sampled row,
//   slot, table). The workgroup stages `cls` in LDS (every class clamped below C) and, when LDS is set, the table's
//   S * C * 2 bytes with 16-byte copies; the other instantiation walks the table in global memory (read-only, L2
//   resident). The launch says up to which size tables go to LDS (at most SCHEMA_LDS_BYTES) and allocates that much
//   dynamically. SCHEMA_LDS_BYTES + 256 is 160 KiB / 8: eight workgroups per CU whatever the pool holds (a 32 KiB
//   array left 4 per CU and made the LDS path slower than the global one). A
//   launch runs over all rows and a workgroup whose table belongs to the other instantiation leaves at once, so one
//   step may mix both. Every lane walks one token: s = trans[s * C + cls[b]] until the token ends or
//   s >= S (DEAD is 0xFFFF >= S; a record whose state is >= S and not DONE walks as DEAD). DWORD reads the token's
//   bytes through aligned 4-byte loads (the byte table is padded by 16 bytes). One wave ballot is 64 mask bits, stored
//   by lane 0 as in json_mask.hip: one 8-byte store, two 4-byte stores where the row's words are not 8-byte aligned,
//   one where the last word of the row is the ballot's low half; a token past V contributes a zero bit. In DONE the
//   allowed tokens are the EOS ids; a token without bytes is never allowed.
// schema_advance_kernel   one thread per schema row, behind the sampler: walks the sampled id's bytes over the table
//   in global memory and writes the record back (word 3 as it was). DONE stays DONE; elsewhere an id without bytes or
//   outside the vocabulary gives DEAD.
// A row naming a slot, a sampled row or a table outside its array, a table whose (S, C) is outside the limits, or a
// slot whose record names another table (word 3 != table + 1), is skipped: a bad index never becomes an out-of-range
// access or a walk of one table's state over another table.
#include "common.h"
#include "schema_walk.h"

namespace kafka {

constexpr int SM_NT = 256;

template <bool LDS, bool DWORD>
__global__ void __launch_bounds__(SM_NT) schema_mask_kernel(const uint16_t* __restrict__ strans,
                                                            const uint8_t* __restrict__ scls,
                                                            const int* __restrict__ sdim, int n_tabs,
                                                            const int* __restrict__ tok_off,
                                                            const uint8_t* __restrict__ tok_bytes, int V,
                                                            const int* __restrict__ eos, int n_eos,
                                                            const int* __restrict__ srows, int n_sampled,
                                                            const int* __restrict__ jstate, int n_slots,
                                                            uint32_t* __restrict__ mask_tab, int64_t mask_ld,
                                                            int json_row0, int iters, int lds_bytes) {
  // dynamic LDS: cls [256], then (LDS) lds_bytes of table — sized by the launch, not by SCHEMA_LDS_BYTES, so small
  // tables leave the CU's LDS to more workgroups
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint8_t* cl = smem;
  uint16_t* tr_lds = reinterpret_cast<uint16_t*>(smem + 256);
  const int r = srows[3 * blockIdx.y], slot = srows[3 * blockIdx.y + 1], tab = srows[3 * blockIdx.y + 2];
  // (uniform: the whole workgroup leaves)
  if (r < 0 || r >= n_sampled || slot < 0 || slot >= n_slots || tab < 0 || tab >= n_tabs) return;
  const SchemaTab dim = schema_dim(sdim, tab);
  if (dim.S == 0 || (dim.S * dim.C * 2 <= lds_bytes) != LDS) return;  // (lds_bytes <= SCHEMA_LDS_BYTES)
  const uint32_t S = dim.S, C = dim.C;
  const int4 rec4 = *reinterpret_cast<const int4*>(jstate + (int64_t)slot * JSON_STATE_INTS);
  if (rec4.w != tab + 1) return;  // the slot's record belongs to another table (or to a JSON-mode row): not this row's
  const uint32_t rec = (uint32_t)rec4.x;
  const bool done = rec == (uint32_t)SCHEMA_DONE;
  const bool walk = !done && rec < S;
  const uint16_t* __restrict__ tr_g = strans + (int64_t)tab * (SCHEMA_TAB_BYTES / 2);
  if (walk) {
    cl[threadIdx.x] = (uint8_t)min((uint32_t)scls[(int64_t)tab * 256 + threadIdx.x], C - 1);
    if (LDS) {
      const int n16 = (int)(S * C * 2 + 15) >> 4;  // <= lds_bytes / 16 (a multiple of 16); the pool row is longer
      const uint4* src = reinterpret_cast<const uint4*>(tr_g);
      uint4* dst = reinterpret_cast<uint4*>(tr_lds);
      for (int i = threadIdx.x; i < n16; i += SM_NT) dst[i] = src[i];
    }
    __syncthreads();
  }
  int e0 = -1, e1 = -1, e2 = -1, e3 = -1, e4 = -1, e5 = -1, e6 = -1, e7 = -1;
  if (done) {
    if (n_eos > 0) e0 = eos[0];
    if (n_eos > 1) e1 = eos[1];
    if (n_eos > 2) e2 = eos[2];
    if (n_eos > 3) e3 = eos[3];
    if (n_eos > 4) e4 = eos[4];
    if (n_eos > 5) e5 = eos[5];
    if (n_eos > 6) e6 = eos[6];
    if (n_eos > 7) e7 = eos[7];
  }
  uint32_t* row = mask_tab + (int64_t)(json_row0 + slot) * mask_ld;
  const int W = (V + 31) >> 5;
  const int lane = threadIdx.x & 63;
#pragma unroll 1
  for (int it = 0; it < iters; ++it) {
    const int64_t t64 = ((int64_t)blockIdx.x * iters + it) * SM_NT + (threadIdx.x & ~63);  // the wave's first token
    if (t64 >= V) break;  // (uniform per wave; later iterations lie further out)
    const int t0 = (int)t64, t = t0 + lane;
    bool ok = false;
    if (t < V) {
      if (walk) {
        const int lo = tok_off[t], hi = tok_off[t + 1];
        uint32_t s;
        if (LDS)
          s = schema_token<DWORD>(rec, tr_lds, cl, S, C, tok_bytes, lo, hi);
        else
          s = schema_token<DWORD>(rec, tr_g, cl, S, C, tok_bytes, lo, hi);
        ok = hi > lo && s < S;
      } else if (done) {
        ok = t == e0 || t == e1 || t == e2 || t == e3 || t == e4 || t == e5 || t == e6 || t == e7;
      }
    }
    const unsigned long long bal = __ballot(ok);
    if (lane == 0) {
      const int w = t0 >> 5;  // even; w < W because t0 < V
      uint32_t* p = row + w;
      if (w + 1 < W && (reinterpret_cast<uintptr_t>(p) & 7) == 0) {
        *reinterpret_cast<unsigned long long*>(p) = bal;
      } else {
        p[0] = (uint32_t)bal;
        if (w + 1 < W) p[1] = (uint32_t)(bal >> 32);
      }
    }
  }
}

__global__ void __launch_bounds__(64) schema_advance_kernel(const uint16_t* __restrict__ strans,
                                                            const uint8_t* __restrict__ scls,
                                                            const int* __restrict__ sdim, int n_tabs,
                                                            const int* __restrict__ tok_off,
                                                            const uint8_t* __restrict__ tok_bytes, int V,
                                                            const int* __restrict__ srows, int n_rows,
                                                            const int64_t* __restrict__ sampled, int n_sampled,
                                                            int* __restrict__ jstate, int n_slots) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n_rows) return;
  const int r = srows[3 * i], slot = srows[3 * i + 1], tab = srows[3 * i + 2];
  if (r < 0 || r >= n_sampled || slot < 0 || slot >= n_slots || tab < 0 || tab >= n_tabs) return;
  const SchemaTab dim = schema_dim(sdim, tab);
  if (dim.S == 0) return;
  const uint32_t S = dim.S, C = dim.C;
  int* rec = jstate + (int64_t)slot * JSON_STATE_INTS;
  if (rec[3] != tab + 1) return;  // (as the mask kernel: the record is another table's)
  uint32_t s = (uint32_t)rec[0];
  if (s == (uint32_t)SCHEMA_DONE) return;
  const int64_t t = sampled[r];
  if (s >= S || t < 0 || t >= V) {
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
  rec[0] = (int)s;  // (words 1 and 2 stay 0, word 3 stays table + 1)
}

template <bool LDS, bool DWORD>
static void schema_mask_launch(dim3 grid, hipStream_t st, const uint16_t* strans, const uint8_t* scls,
                               const int* sdim, int n_tabs, const int* tok_off, const uint8_t* tok_bytes, int V,
                               const int* eos, int n_eos, const int* srows, int n_sampled, const int* jstate,
                               int n_slots, uint32_t* mask_tab, int64_t mask_ld, int json_row0, int iters,
                               int lds_bytes) {
  schema_mask_kernel<LDS, DWORD><<<grid, SM_NT, 256 + (LDS ? lds_bytes : 0), st>>>(
      strans, scls, sdim, n_tabs, tok_off, tok_bytes, V, eos, n_eos, srows, n_sampled, jstate, n_slots, mask_tab,
      mask_ld, json_row0, iters, lds_bytes);
}

// strans / scls / sdim: the table pool (n_tabs tables); tok_off int32 [V + 1] with tok_off[V] bytes in tok_bytes, which
// is padded by at least 4 readable bytes; srows int32 [n_rows, 3] (sampled row, slot, table); jstate int32 [n_slots,
// 4]; the mask of slot s is row json_row0 + s of mask_tab (uint32 [mask_rows, mask_ld], mask_ld * 32 >= V). kinds:
// bit 0 launches the LDS instantiation, bit 1 the global-memory one (the caller knows which sizes its pool holds; 3 is
// always right). lds_bytes (a multiple of 16, at most SCHEMA_LDS_BYTES): tables up to this size are staged in LDS, larger
// ones are walked in global memory — the LDS instantiation allocates exactly this much, so a pool of small tables keeps
// the occupancy of a small allocation. tokens: tokens of one workgroup, a multiple of 256; dword: aligned 4-byte token
// loads.
extern "C" hipError_t kafka_launch_schema_mask(const uint16_t* strans, const uint8_t* scls, const int* sdim,
                                               int n_tabs, const int* tok_off, const uint8_t* tok_bytes, int V,
                                               const int* eos, int n_eos, const int* srows, int n_rows,
                                               int n_sampled, const int* jstate, int n_slots, uint32_t* mask_tab,
                                               int64_t mask_ld, int64_t mask_rows, int json_row0, int kinds,
                                               int lds_bytes, int tokens, int dword, hipStream_t st) {
  if (n_rows == 0) return hipSuccess;
  if (V < 1 || n_rows < 0 || n_rows > 65535 || n_eos < 0 || n_eos > JSON_MAX_EOS || mask_ld * 32 < V ||
      json_row0 < 0 || (int64_t)json_row0 + n_slots > mask_rows || n_tabs < 1 || n_sampled < 0 || tokens < SM_NT ||
      tokens % SM_NT != 0 || tokens > (1 << 20) || (kinds & ~3) != 0 || lds_bytes < 0 ||
      lds_bytes > SCHEMA_LDS_BYTES || lds_bytes % 16 != 0)
    return hipErrorInvalidValue;
  const dim3 grid((V + tokens - 1) / tokens, n_rows);
  const int iters = tokens / SM_NT;
#define SM_LAUNCH(L, D)                                                                                              \
  schema_mask_launch<L, D>(grid, st, strans, scls, sdim, n_tabs, tok_off, tok_bytes, V, eos, n_eos, srows, n_sampled, \
                           jstate, n_slots, mask_tab, mask_ld, json_row0, iters, lds_bytes)
  if (kinds & 1) {
    if (dword) SM_LAUNCH(true, true); else SM_LAUNCH(true, false);
  }
  if (kinds & 2) {
    if (dword) SM_LAUNCH(false, true); else SM_LAUNCH(false, false);
  }
#undef SM_LAUNCH
  return hipGetLastError();
}

extern "C" hipError_t kafka_launch_schema_advance(const uint16_t* strans, const uint8_t* scls, const int* sdim,
                                                  int n_tabs, const int* tok_off, const uint8_t* tok_bytes, int V,
                                                  const int* srows, int n_rows, const int64_t* sampled,
                                                  int n_sampled, int* jstate, int n_slots, hipStream_t st) {
  if (n_rows == 0) return hipSuccess;
  if (V < 1 || n_rows < 0 || n_sampled < 0 || n_tabs < 1) return hipErrorInvalidValue;
  schema_advance_kernel<<<(n_rows + 63) / 64, 64, 0, st>>>(strans, scls, sdim, n_tabs, tok_off, tok_bytes, V, srows,
                                                           n_rows, sampled, n_sampled, jstate, n_slots);
  return hipGetLastError();
}

}  // namespace kafka
