// One pass over a row of logits, shared by the sampler (sampling.hip) and the log-probabilities (logprobs.hip): the
// 8-entry loader, the candidate order, the partition of a row over the workgroups of a split launch, and the walk of
// one workgroup's slice. Device-only: no launchers, nothing of it in kafka_abi.h.
#pragma once
#include "common.h"

namespace kafka {

// 8 consecutive logits as fp32. AL: the address is 16-byte aligned (every row is: base and row stride) -> 16-byte
// loads; otherwise (a view with an odd row stride) element loads — correct, not fast.
template <typename T, bool AL = true>
struct Vec8 {
  static __device__ __forceinline__ void load(const T* p, float (&v)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)p[j];
  }
};
template <>
struct Vec8<bf16, true> {
  static __device__ __forceinline__ void load(const bf16* p, float (&v)[8]) {
    bf16x8 a = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)a[j];
  }
};
template <>
struct Vec8<float, true> {
  static __device__ __forceinline__ void load(const float* p, float (&v)[8]) {
    f32x4 a = *reinterpret_cast<const f32x4*>(p);
    f32x4 b = *reinterpret_cast<const f32x4*>(p + 4);
    v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
    v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
  }
};

// A candidate (value, index) in the order value descending, index ascending: among equal values the first index wins.
// CAND_NONE is the index of "no candidate": it loses every tie.
struct Cand {
  float v;
  int i;
};
constexpr int CAND_NONE = 0x7fffffff;

__device__ __forceinline__ Cand better(Cand a, Cand b) {
  if (b.v > a.v || (b.v == a.v && b.i < a.i)) return b;
  return a;
}

// c comes strictly after b in the order
__device__ __forceinline__ bool cand_after(Cand c, Cand b) { return c.v < b.v || (c.v == b.v && c.i > b.i); }

__device__ __forceinline__ Cand wave_best(Cand a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a = better(a, Cand{__shfl_xor(a.v, o, 64), __shfl_xor(a.i, o, 64)});
  return a;
}

// Best candidate of a workgroup of NT threads, on every thread. sv / si hold NT / 64 entries.
template <int NT>
__device__ __forceinline__ Cand block_argmax(Cand a, float* sv, int* si) {
  a = wave_best(a);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sv[w] = a.v;
    si[w] = a.i;
  }
  __syncthreads();
  Cand r{sv[0], si[0]};
  for (int k = 1; k < NT / 64; ++k) r = better(r, Cand{sv[k], si[k]});
  __syncthreads();
  return r;
}

// Split sp of nsplit over a row of V entries: the 8-entry vectors [v0, v1) — ceil(nvec / nsplit) each, the late splits
// of a short row none — and the scalar entries [t0, t1): the row's tail [nvec * 8, V) for the last split, which owns
// it, empty for the others. ops/reference.py sample_replay partitions the same way.
struct RowSlice {
  int v0, v1, t0, t1;
};
__device__ __forceinline__ RowSlice row_slice(int V, int sp, int nsplit) {
  const int nvec = V >> 3;
  const int per = (nvec + nsplit - 1) / nsplit;
  const int v0 = sp * per;
  return RowSlice{v0, min(nvec, v0 + per), nvec << 3, sp == nsplit - 1 ? V : nvec << 3};
}

// f(value, index) for every entry of the slice that this thread of an NT-thread workgroup owns: its vectors in
// ascending order (load8(i0, v): the 8 entries from index i0), then its tail entries (load1(i)). Per-thread fp32 sums
// depend on this order.
template <int NT, typename L8, typename L1, typename F>
__device__ __forceinline__ void scan_slice(const RowSlice& s, L8&& load8, L1&& load1, F&& f) {
  for (int vi = s.v0 + threadIdx.x; vi < s.v1; vi += NT) {
    float v[8];
    load8(vi * 8, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) f(v[j], vi * 8 + j);
  }
  for (int i = s.t0 + threadIdx.x; i < s.t1; i += NT) f(load1(i), i);
}

}  // namespace kafka
