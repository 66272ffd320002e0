// Fused MoE router for gfx950: gate GEMM + softmax / top-k + stable expert sort in ONE launch (ops.moe_gate_route).
//   logits[T, E] = X[T, d] . W[E, d]^T   (bf16 in, fp32 accumulate, bf16 RNE out: what F.linear's bf16 output holds,
//                                          up to accumulation order)
//   then exactly moe_route_kernel's outputs on those logits (moe_route.h: the same two device functions).
// E <= 16, k <= 4, d % 64 == 0, X rows 16-B aligned with any row stride, W contiguous.
//
// The gate product is N = E <= 16 wide and memory-bound on X (T d 2 bytes against 16 T d 2 / 16 flops per byte): a
// general GEMM tile wastes its columns and, at decode sizes, runs on two to ten CUs. Here:
//
//   * grid = (row tiles of 64 tokens) x (K splits). A workgroup is 1024 threads = 16 waves because the LAST workgroup
//     to finish becomes the finisher and the routing phases are written for 1024 threads. For the gate phase the 16
//     waves are 4 row groups (16 tokens: one MFMA M) x 4 K groups: wave (rg, kg) multiplies rows [16 rg, +16) of the tile
//     by the 64-column K chunks kg, kg + 4, kg + 8, ... of the workgroup's K slice. MFMA = v_mfma_f32_16x16x32_bf16,
//     the experts zero-padded (in effect: see below) to N = 16: E = 8 wastes half of a unit that is idle anyway, and a
//     32x32x16 tile would waste three quarters and need 32-token row groups; 16 x 16 also makes the C tile one f32x4
//     per lane.
//   * X goes through LDS by LDS-DMA (global_load_lds_dwordx4, coalesced 16-B lanes, 128 B per row) into a ring that is
//     PRIVATE to the wave: 4 stages of 16 rows x 64 columns (2 KB; 8 KB a wave, 128 KB a workgroup). A wave reads back
//     only what it loaded, so the K loop has no barrier at all: a counted s_waitcnt vmcnt per stage is the whole
//     synchronisation, and up to three stages per wave (96 KB per CU) are in flight — in the prologue; in the loop
//     hipcc adds a vmcnt(0) in front of each stage's MFMAs for the B fragments (register loads next to LDS-DMA loads:
//     skinny_gemm.hip's header has the same finding), so a wave with more than three chunks then has one stage in
//     flight. Decode-sized steps have one to three chunks per wave. LDS is the layout change: the
//     16-B chunk c of row m sits at slot c ^ (m & 7), permuted on the source side (the DMA writes lane-linear), and the
//     A fragment of a k-step (lane l: row l & 15, K columns [8 (l >> 4), +8)) is one conflict-free ds_read_b128.
//   * W never touches LDS: its B fragment (lane l: expert l & 15, K columns [8 (l >> 4), +8)) is one 16-B global load
//     per k-step from the L2-resident [E, d] rows, issued with the stage's DMAs. Lanes of experts >= E re-read expert
//     E - 1: an MFMA output column depends on its own B column only, so columns >= E hold a copy of column E - 1 that
//     nothing reads — the padding costs no branch and no zero fill.
//   * the 4 K groups of a workgroup are summed through LDS in kg order (each wave parks its 16 x 16 fp32 tile in its
//     own, by then dead, ring), 256 threads store the 64 x 16 fp32 partial of the split to the workspace slab
//     [split][T][16] with 16-B sc1 stores. No float atomics anywhere: kg order, then split order, so the logits — and
//     the routing — are bit-reproducible from run to run.
//   * election (common.h's ticket protocol): every wave waits for vmcnt 0, barrier, one thread takes a ticket on the
//     workspace's counter. The last of the gridDim.x * gridDim.y arrivals re-arms the counter (hipGraph replay needs no
//     memset) and its workgroup becomes the finisher; everybody else exits. Nobody spins, so nothing depends on
//     workgroups being co-resident.
//   * finisher: 1024 threads sum the splits in split order with 16-B sc1 loads (never a plain load of a partial: the
//     writer may sit on another XCD), round to bf16 (RNE), store logits_out, barrier, and run route_topk / route_sort
//     on logits_out as moe_route_kernel does on its input.
// K splits (kafka_moe_gate_route_plan): as many as bring the grid to one workgroup per CU, at most one per 4 chunks (so
// every wave of a workgroup has a chunk), one once the row tiles alone fill the machine.
// Registers / LDS / occupancy: profiles/moe_router/resource_usage.txt.
#include <algorithm>

#include "common.h"
#include "moe_route.h"

namespace kafka {

namespace mgr {
constexpr int BM = 64;            // tokens of a row tile
constexpr int CK = 64;            // K columns of a chunk (one ring stage of a wave)
constexpr int NS = 4;             // ring stages per wave
constexpr int STAGE = 16 * CK * 2;  // 2 KB: 16 rows x 128 B
constexpr int RING = NS * STAGE;    // 8 KB per wave
constexpr int OPS = 4;              // vector-memory operations a wave issues per stage: 2 DMA + 2 B fragments
constexpr int HDR = 64;             // workspace header in 4-byte words (word 0: the ticket); the slabs follow

typedef __attribute__((address_space(3))) void lds_t;
__device__ __forceinline__ void dma16(const void* g, char* lds) {
  __builtin_amdgcn_global_load_lds(g, (lds_t*)lds, 16, 0, 0);
}
__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
// s_waitcnt vmcnt(OPS * n) for a wave-uniform n in [0, NS - 2]
__device__ __forceinline__ void wait_later_stages(int n) {
  static_assert(NS == 4, "one case per possible count of later stages in flight");
  if (n >= 2) wait_vmcnt<2 * OPS>();
  else if (n == 1) wait_vmcnt<OPS>();
  else wait_vmcnt<0>();
}
}  // namespace mgr

// X and W are not __restrict__: their register loads must stay between the counted waits they were written between
// (an asm with a memory clobber does not order loads from no-alias memory).
// cps: 64-column chunks of one K split (the last split may have fewer); ws: [HDR words][splits][T][16] fp32
__global__ __launch_bounds__(MOE_NT) void moe_gate_route_kernel(const bf16* X, int64_t ldx, const bf16* W, int T, int d,
                                                                 int E, int K, int BMr, int cps, int* __restrict__ ws,
                                                                 bf16* logits, int64_t ldl, float* __restrict__ topk_w,
                                                                 int* __restrict__ topk_e, int* __restrict__ perm_tok,
                                                                 float* __restrict__ perm_w,
                                                                 int* __restrict__ expert_off,
                                                                 int* __restrict__ tile_off) {
  using namespace mgr;
  __shared__ __attribute__((aligned(1024))) char smem[(MOE_NT / 64) * RING];
  __shared__ int wsum[MOE_NT / 64];
  __shared__ int elected;

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rg = w & 3, kg = w >> 2;
  const int row0 = blockIdx.x * BM;
  const int S = gridDim.y, split = blockIdx.y;
  const int nch = d / CK;
  const int cbeg = split * cps, cend = min(nch, cbeg + cps);
  float* slabs = reinterpret_cast<float*>(ws + HDR);
  char* ring = smem + w * RING;

  // ---- gate phase: this wave's 16 rows x its chunks cbeg + kg + 4 j
  const bool live = row0 + 16 * rg < T;                       // wave-uniform: the row group holds a token
  const int n = live ? (cend - cbeg - kg + 3) / 4 : 0;        // chunks of this wave (cend - cbeg - kg may be <= 0)
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (n > 0) {
    // DMA instruction u covers ring bytes [1024 u, +1024) = rows 8 u .. 8 u + 7; lane -> (row, slot); rows past T
    // re-read row T - 1 and are never stored
    const bf16* xsrc[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int row = 8 * u + (lane >> 3), slot = lane & 7;
      const int64_t gr = min(row0 + 16 * rg + row, T - 1);
      xsrc[u] = X + gr * ldx + (int64_t)(cbeg + kg) * CK + 8 * (slot ^ (row & 7));
    }
    const bf16* bsrc = W + (int64_t)min(lane & 15, E - 1) * d + (int64_t)(cbeg + kg) * CK + 8 * (lane >> 4);
    const int m = lane & 15, h = lane >> 4;
    const int aoff[2] = {m * 128 + 16 * (h ^ (m & 7)), m * 128 + 16 * ((4 + h) ^ (m & 7))};
    bf16x8 bq[NS][2];
    auto issue = [&](int j, int slot) {  // chunk j of this wave into ring stage `slot` (both compile-time after unroll)
      dma16(xsrc[0] + (int64_t)j * 4 * CK, ring + slot * STAGE);
      dma16(xsrc[1] + (int64_t)j * 4 * CK, ring + slot * STAGE + 1024);
      bq[slot][0] = load_bf16x8(bsrc + (int64_t)j * 4 * CK);
      bq[slot][1] = load_bf16x8(bsrc + (int64_t)j * 4 * CK + 32);
    };
#pragma unroll
    for (int u = 0; u < NS - 1; ++u)
      if (u < n) issue(u, u);
    for (int j0 = 0; j0 < n; j0 += NS) {
#pragma unroll
      for (int u = 0; u < NS; ++u) {
        const int j = j0 + u;
        if (j < n) {
          // stage j has landed (up to NS - 2 later ones may still be in flight); this wave's reads of stage j - 1,
          // whose slot the next DMA overwrites, have returned
          wait_later_stages(min(NS - 2, n - 1 - j));
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          if (j + NS - 1 < n) issue(j + NS - 1, (u + NS - 1) % NS);
          const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(ring + u * STAGE + aoff[0]);
          const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(ring + u * STAGE + aoff[1]);
          acc = mfma16(a0, bq[u][0], acc);
          acc = mfma16(a1, bq[u][1], acc);
        }
      }
    }
  }
  // ---- the 4 K groups of the workgroup, summed in kg order through LDS. C layout: lane l, register i -> row
  // 4 (l >> 4) + i of the wave's 16, column l & 15. Every DMA of this wave has landed (the loop's last wait is vmcnt 0).
  {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    float* tile = reinterpret_cast<float*>(ring);  // [16 rows][16 columns]
#pragma unroll
    for (int i = 0; i < 4; ++i) tile[(4 * (lane >> 4) + i) * 16 + (lane & 15)] = acc[i];
  }
  __syncthreads();
  if (tid < 256) {
    const int row = tid >> 2, q = tid & 3;  // token row of the tile, column quad
    if (row0 + row < T) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int g = 0; g < 4; ++g)
        v += *reinterpret_cast<const f32x4*>(smem + (4 * g + (row >> 4)) * RING + ((row & 15) * 16 + 4 * q) * 4);
      store16_slab(slabs + ((int64_t)split * T + row0 + row) * 16 + 4 * q, v);
    }
  }
  // ---- election: the last workgroup to arrive is the finisher (no partial store after this wait)
  wait_vmcnt<0>();
  __syncthreads();
  if (tid == 0) elected = take_ticket(ws, gridDim.x * gridDim.y) ? 1 : 0;
  __syncthreads();
  if (!elected) return;

  // ---- finisher: logits = bf16(sum over the splits, in split order); item = (token, column quad)
  {
    const __amdgpu_buffer_rsrc_t rs = buf_rsrc(slabs);
    const int nq = (E + 3) >> 2;
    for (int it = tid; it < T * nq; it += MOE_NT) {
      const int t = it / nq, q = it - t * nq;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      for (int s = 0; s < S; s += 4) {  // four slab loads in flight before the first add
        f32x4 p[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) p[u] = load16_sc1(rs, ((min(s + u, S - 1) * T + t) * 16 + 4 * q) * 4);
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (s + u < S) v += p[u];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (4 * q + u < E) logits[(int64_t)t * ldl + 4 * q + u] = (bf16)v[u];
    }
  }
  __syncthreads();  // the logits are read back by the threads that own their tokens
  int t0, t1;
  route_span(T, t0, t1);
  route_topk(logits, ldl, t0, t1, E, K, topk_w, topk_e);
  route_sort(t0, t1, E, K, BMr, topk_w, topk_e, perm_tok, perm_w, expert_off, tile_off, wsum);
}

// K splits for a step of T tokens at width d on a device of `cus` compute units; *ws_words = the 4-byte words of
// workspace the launch needs (header + slabs). 0 if the shape is supported.
extern "C" int kafka_moe_gate_route_plan(int T, int d, int cus, int* splits, int64_t* ws_words) {
  using namespace mgr;
  if (T < 1 || d < CK || d % CK != 0 || cus < 1) return 1;
  const int nch = d / CK;
  const int64_t rts = ((int64_t)T + BM - 1) / BM;
  int64_t s = (cus + rts - 1) / rts;                  // one workgroup per CU
  s = std::max<int64_t>(1, std::min<int64_t>(s, nch / 4));  // every wave of a workgroup has a chunk
  const int cps = (int)((nch + s - 1) / s);
  s = (nch + cps - 1) / cps;                          // no empty split
  if (s * T * 64 >= (1LL << 31)) return 1;            // the finisher's 32-bit slab offsets
  *splits = (int)s;
  if (ws_words) *ws_words = HDR + s * T * 16;
  return 0;
}

extern "C" hipError_t kafka_launch_moe_gate_route(const bf16* X, int64_t ldx, const bf16* W, int T, int d, int E, int K,
                                                 int BM, int splits, int* ws, bf16* logits, int64_t ldl,
                                                 float* topk_w, int* topk_e, int* perm_tok, float* perm_w,
                                                 int* expert_off, int* tile_off, hipStream_t st) {
  using namespace mgr;
  if (T < 1 || E < 1 || E > MOE_MAXE || K < 1 || K > MOE_MAXK || K > E || BM < 1) return hipErrorInvalidValue;
  if (d < CK || d % CK != 0 || ldx % 8 != 0 || ldx < d || ldl < E) return hipErrorInvalidValue;
  if (!X || !W || !ws || !logits || (reinterpret_cast<uintptr_t>(X) & 15) || (reinterpret_cast<uintptr_t>(W) & 15) ||
      (reinterpret_cast<uintptr_t>(ws) & 15))
    return hipErrorInvalidValue;
  const int nch = d / CK;
  if (splits < 1 || splits > nch || (int64_t)splits * T * 64 >= (1LL << 31)) return hipErrorInvalidValue;
  const int cps = (nch + splits - 1) / splits;
  if ((int64_t)(splits - 1) * cps >= nch) return hipErrorInvalidValue;  // an empty split
  const dim3 grid((unsigned)((T + mgr::BM - 1) / mgr::BM), (unsigned)splits);
  moe_gate_route_kernel<<<grid, MOE_NT, 0, st>>>(X, ldx, W, T, d, E, K, BM, cps, ws, logits, ldl, topk_w, topk_e,
                                                 perm_tok, perm_w, expert_off, tile_off);
  return hipGetLastError();
}

}  // namespace kafka
