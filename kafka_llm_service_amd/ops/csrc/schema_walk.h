// The device helpers the schema kernels (json_schema.hip) and the tool grammar kernels (tool_grammar.hip) share: a pool
// table's checked dimensions, the walk of one token's bytes over a table, and lane 0's store of a wave ballot into a
// mask row.
#pragma once
#include "common.h"

namespace kafka {

struct SchemaTab {
  int S, C;  // S == 0: not usable
};

__device__ __forceinline__ SchemaTab schema_dim(const int* __restrict__ sdim, int tab) {
  const int S = sdim[2 * tab], C = sdim[2 * tab + 1];
  SchemaTab t;
  const bool ok = S >= 2 && S <= SCHEMA_MAX_STATES && C >= 1 && C <= 256 && S * C * 2 <= SCHEMA_TAB_BYTES;
  t.S = ok ? S : 0;
  t.C = C;
  return t;
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

// 64 mask bits of the tokens [t0, t0 + 64) (t0 a multiple of 64 below V) into the row of W words: one 8-byte store,
// two 4-byte stores where the row's words are not 8-byte aligned, one where the row's last word is the low half
__device__ __forceinline__ void mask_store64(uint32_t* __restrict__ row, int W, int t0, unsigned long long bal) {
  const int w = t0 >> 5;  // even; w < W because t0 < V
  uint32_t* p = row + w;
  if (w + 1 < W && (reinterpret_cast<uintptr_t>(p) & 7) == 0) {
    *reinterpret_cast<unsigned long long*>(p) = bal;
  } else {
    p[0] = (uint32_t)bal;
    if (w + 1 < W) p[1] = (uint32_t)(bal >> 32);
  }
}

}  // namespace kafka
