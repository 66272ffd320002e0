// JSON mode for gfx950: the vocabulary mask of a row's JSON automaton state, built on the device, and the state's
// advance over the token the sampler drew. engine/json_mode.py holds the automaton (TRANS uint8 [64, 256]: next state
// in the low six bits, operation in the top two) and ops/reference.py its walk (json_walk / json_mask_ref /
// json_advance_ref); both kernels agree with those bit for bit — everything here is integer work.
//
// A row's state is the int32 [4] record (state, depth, stack bits, 0) of its slot in `jstate`; it never leaves the
// device after the host seeded it, so a step can be planned and launched before the previous step's token is known.
//
// json_mask_kernel   grid (ceil(V / JM_TOKENS), JSON rows), 256 threads. The workgroup stages TRANS in LDS (16 KB);
//   every lane walks one token's bytes from a private copy of the row's state; one wave ballot is 64 mask bits,
//   stored by lane 0 into the slot's row of `mask_tab` (common.h: mask_store64). A token past V reads
//   nothing and contributes a zero bit, so the surplus bits of the last word are clear. In DONE the allowed tokens
//   are the EOS ids; a token without bytes is never allowed.
// json_advance_kernel   one thread per JSON row, launched behind the sampler: reads the row's sampled id, walks its
//   bytes and writes the slot's new record. DONE stays DONE whatever the id; elsewhere an id without bytes (or
//   outside the vocabulary) is a rejected byte: DEAD.
// Rows come as (sampled row, slot) pairs from the step's packed upload; a pair naming a slot outside the state table
// (or a row outside the sampler's output) is skipped.
#include "common.h"

namespace kafka {

constexpr int JM_NT = 256;
constexpr int JM_ITERS = 4;
constexpr int JM_TOKENS = JM_NT * JM_ITERS;  // tokens of one workgroup
constexpr int JM_DEAD = 63;
constexpr int JM_OP_OPEN = 1, JM_OP_CLOSE = 2, JM_OP_COMMA = 3;

struct JsonState {
  int s, d;
  uint32_t stk;
};

__device__ __forceinline__ JsonState json_load(const int* __restrict__ jstate, int slot) {
  const int4 r = *reinterpret_cast<const int4*>(jstate + (int64_t)slot * JSON_STATE_INTS);
  JsonState st;
  st.s = r.x & 63;
  st.d = min(max(r.y, 0), JSON_MAX_DEPTH);
  st.stk = (uint32_t)r.z;
  return st;
}

// one byte (ops/reference.py json_walk); `tr` is TRANS in LDS or in global memory
template <typename P>
__device__ __forceinline__ void json_step(JsonState& st, P tr, uint32_t b) {
  const uint32_t e = tr[st.s * 256 + b];
  const int op = e >> 6, nxt = e & 63;
  if (nxt == JM_DEAD) {
    st.s = JM_DEAD;
  } else if (op == 0) {
    st.s = nxt;
  } else if (op == JM_OP_OPEN) {
    if (st.d >= JSON_MAX_DEPTH) {
      st.s = JM_DEAD;
    } else {
      if (b == 0x7B) st.stk |= 1u << st.d;
      st.d += 1;
      st.s = nxt;
    }
  } else if (st.d <= 0) {
    st.s = JM_DEAD;
  } else {
    const uint32_t top = (st.stk >> (st.d - 1)) & 1u;
    if (op == JM_OP_COMMA) {
      st.s = top ? JSON_EXPECT_KEY : JSON_EXPECT_VALUE;
    } else if (top != (b == 0x7D ? 1u : 0u)) {
      st.s = JM_DEAD;
    } else {
      st.d -= 1;
      st.stk &= ~(1u << st.d);
      st.s = st.d == 0 ? JSON_DONE : nxt;
    }
  }
}

__global__ void __launch_bounds__(JM_NT) json_mask_kernel(const uint8_t* __restrict__ trans,
                                                          const int* __restrict__ tok_off,
                                                          const uint8_t* __restrict__ tok_bytes, int V,
                                                          const int* __restrict__ eos, int n_eos,
                                                          const int* __restrict__ jrows,
                                                          const int* __restrict__ jstate, int n_slots,
                                                          uint32_t* __restrict__ mask_tab, int64_t mask_ld,
                                                          int json_row0) {
  __shared__ __attribute__((aligned(16))) uint8_t tr[64 * 256];
  const int slot = jrows[2 * blockIdx.y + 1];
  if (slot < 0 || slot >= n_slots) return;  // (uniform: the whole workgroup)
  const JsonState st0 = json_load(jstate, slot);
  const bool walk = st0.s != JSON_DONE && st0.s != JM_DEAD;
  if (walk) {
    const uint4* src = reinterpret_cast<const uint4*>(trans);
    uint4* dst = reinterpret_cast<uint4*>(tr);
#pragma unroll
    for (int i = 0; i < 64 * 256 / 16 / JM_NT; ++i) dst[threadIdx.x + i * JM_NT] = src[threadIdx.x + i * JM_NT];
    __syncthreads();
  }
  int e0 = -1, e1 = -1, e2 = -1, e3 = -1, e4 = -1, e5 = -1, e6 = -1, e7 = -1;
  if (st0.s == JSON_DONE) {
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
  for (int it = 0; it < JM_ITERS; ++it) {
    const int t0 = blockIdx.x * JM_TOKENS + it * JM_NT + (threadIdx.x & ~63);  // the wave's first token
    if (t0 >= V) break;  // (uniform per wave; later iterations lie further out)
    const int t = t0 + lane;
    bool ok = false;
    if (t < V) {
      if (walk) {
        const int lo = tok_off[t], hi = tok_off[t + 1];
        JsonState st = st0;
        for (int j = lo; j < hi && st.s != JM_DEAD; ++j) json_step(st, tr, tok_bytes[j]);
        ok = hi > lo && st.s != JM_DEAD;
      } else if (st0.s == JSON_DONE) {
        ok = t == e0 || t == e1 || t == e2 || t == e3 || t == e4 || t == e5 || t == e6 || t == e7;
      }
    }
    const unsigned long long bal = __ballot(ok);
    if (lane == 0) mask_store64(row, W, t0, bal);
  }
}

__global__ void __launch_bounds__(64) json_advance_kernel(const uint8_t* __restrict__ trans,
                                                          const int* __restrict__ tok_off,
                                                          const uint8_t* __restrict__ tok_bytes, int V,
                                                          const int* __restrict__ jrows, int n_rows,
                                                          const int64_t* __restrict__ sampled, int n_sampled,
                                                          int* __restrict__ jstate, int n_slots) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n_rows) return;
  const int r = jrows[2 * i], slot = jrows[2 * i + 1];
  if (r < 0 || r >= n_sampled || slot < 0 || slot >= n_slots) return;
  JsonState st = json_load(jstate, slot);
  if (st.s == JSON_DONE) return;
  const int64_t t = sampled[r];
  if (st.s != JM_DEAD) {
    if (t < 0 || t >= V) {
      st.s = JM_DEAD;
    } else {
      const int lo = tok_off[t], hi = tok_off[t + 1];
      if (hi <= lo) st.s = JM_DEAD;
      for (int j = lo; j < hi && st.s != JM_DEAD; ++j) json_step(st, trans, tok_bytes[j]);
    }
  }
  *reinterpret_cast<int4*>(jstate + (int64_t)slot * JSON_STATE_INTS) = make_int4(st.s, st.d, (int)st.stk, 0);
}

// trans: uint8 [64 * 256]; tok_off int32 [V + 1] with tok_off[V] bytes in tok_bytes; eos: n_eos <= JSON_MAX_EOS ids;
// jrows int32 [n_rows, 2] (sampled row, slot); jstate int32 [n_slots, 4]; the mask of slot s is row json_row0 + s of
// mask_tab (uint32 [mask_rows, mask_ld], mask_ld * 32 >= V).
extern "C" hipError_t kafka_launch_json_mask(const uint8_t* trans, const int* tok_off, const uint8_t* tok_bytes, int V,
                                             const int* eos, int n_eos, const int* jrows, int n_rows,
                                             const int* jstate, int n_slots, uint32_t* mask_tab, int64_t mask_ld,
                                             int64_t mask_rows, int json_row0, hipStream_t st) {
  if (n_rows == 0) return hipSuccess;
  if (V < 1 || n_rows < 0 || n_rows > 65535 || n_eos < 0 || n_eos > JSON_MAX_EOS || mask_ld * 32 < V ||
      json_row0 < 0 || (int64_t)json_row0 + n_slots > mask_rows)
    return hipErrorInvalidValue;
  const dim3 grid((V + JM_TOKENS - 1) / JM_TOKENS, n_rows);
  json_mask_kernel<<<grid, JM_NT, 0, st>>>(trans, tok_off, tok_bytes, V, eos, n_eos, jrows, jstate, n_slots, mask_tab,
                                           mask_ld, json_row0);
  return hipGetLastError();
}

extern "C" hipError_t kafka_launch_json_advance(const uint8_t* trans, const int* tok_off, const uint8_t* tok_bytes,
                                                int V, const int* jrows, int n_rows, const int64_t* sampled,
                                                int n_sampled, int* jstate, int n_slots, hipStream_t st) {
  if (n_rows == 0) return hipSuccess;
  if (V < 1 || n_rows < 0 || n_sampled < 0) return hipErrorInvalidValue;
  json_advance_kernel<<<(n_rows + 63) / 64, 64, 0, st>>>(trans, tok_off, tok_bytes, V, jrows, n_rows, sampled,
                                                         n_sampled, jstate, n_slots);
  return hipGetLastError();
}

}  // namespace kafka
