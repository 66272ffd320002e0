// The routing phases of one MoE step, shared by moe_route_kernel (moe.hip: logits from a router GEMM) and
// moe_gate_route_kernel (moe_router.hip: its finisher, on the logits it has just summed). One workgroup of MOE_NT
// threads; thread tid owns the tokens [t0, t1) of route_span.
#pragma once
#include "common.h"

namespace kafka {

constexpr int MOE_MAXE = 16;
constexpr int MOE_MAXK = 4;
constexpr int MOE_NT = 1024;

__device__ __forceinline__ void route_span(int T, int& t0, int& t1) {
  const int per = (T + MOE_NT - 1) / MOE_NT;
  t0 = min(T, (int)threadIdx.x * per);
  t1 = min(T, t0 + per);
}

// ---- phase 1: softmax + top-k + renormalise for the owned tokens
// (logits is not __restrict__: the fused router's finisher reads what other threads of its workgroup stored before a
// barrier)
__device__ __forceinline__ void route_topk(const bf16* logits, int64_t ld, int t0, int t1, int E, int K,
                                           float* __restrict__ topk_w, int* __restrict__ topk_e) {
  for (int t = t0; t < t1; ++t) {
    float p[MOE_MAXE];
    float m = -INFINITY;
    for (int e = 0; e < E; ++e) {
      p[e] = (float)logits[(int64_t)t * ld + e];
      m = fmaxf(m, p[e]);
    }
    float s = 0.f;
    for (int e = 0; e < E; ++e) {
      p[e] = __expf(p[e] - m);
      s += p[e];
    }
    float tot = 0.f;
    int sel[MOE_MAXK];
    float sw[MOE_MAXK];
    for (int j = 0; j < K; ++j) {
      int best = 0;
      float bv = -1.f;
      for (int e = 0; e < E; ++e)
        if (p[e] > bv) {  // strict: lowest index wins ties (torch.topk order on equal values is unspecified)
          bv = p[e];
          best = e;
        }
      sel[j] = best;
      sw[j] = bv / s;
      tot += sw[j];
      p[best] = -2.f;
    }
    for (int j = 0; j < K; ++j) {
      topk_w[(int64_t)t * K + j] = sw[j] / tot;
      topk_e[(int64_t)t * K + j] = sel[j];
    }
  }
}

// ---- phase 2: stable sort of the entries [t0*K, t1*K) by expert (each thread re-reads its own writes).
// wsum: MOE_NT / 64 ints of LDS.
__device__ __forceinline__ void route_sort(int t0, int t1, int E, int K, int BM, const float* topk_w, const int* topk_e,
                                           int* __restrict__ perm_tok, float* __restrict__ perm_w,
                                           int* __restrict__ expert_off, int* __restrict__ tile_off, int* wsum) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int base = 0, tbase = 0;
  for (int e = 0; e < E; ++e) {
    int c = 0;
    for (int i = t0 * K; i < t1 * K; ++i) c += topk_e[i] == e;
    // block exclusive scan of c
    int incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o, 64);
      if (lane >= o) incl += v;
    }
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    int wpre = 0, total = 0;
    for (int i = 0; i < MOE_NT / 64; ++i) {
      const int v = wsum[i];
      wpre += i < w ? v : 0;
      total += v;
    }
    int pos = base + wpre + incl - c;
    for (int i = t0 * K; i < t1 * K; ++i)
      if (topk_e[i] == e) {
        perm_tok[pos] = i / K;
        perm_w[pos] = topk_w[i];
        ++pos;
      }
    base += total;
    tbase += (total + BM - 1) / BM;
    if (tid == 0) {
      expert_off[e + 1] = base;
      tile_off[e + 1] = tbase;
    }
    __syncthreads();  // wsum is reused by the next expert
  }
  if (tid == 0) {
    expert_off[0] = 0;
    tile_off[0] = 0;
  }
}

}  // namespace kafka
