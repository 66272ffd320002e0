// Grouped MFMA GEMM over the wave-tiled expert weights, for prefill-sized MoE steps (gfx950).
//     per local expert el and its routing segment [expert_off[e_lo + el], expert_off[e_lo + el + 1]):
//     GLU:      Y[entry, :N/2] = silu(gate) * up of X[perm_tok[entry]] . W_el^T   (bf16, GLU-interleaved w13 tiles)
//     COMBINE:  out[perm_tok[entry], n] += perm_w[entry] * (X[entry] . W_el^T)     (fp32 atomics, out zeroed by the caller)
// W in any tile format of kafka_abi.h (WF_BF16 / WF_FP8 / WF_MXFP4; layouts in wstream_gemm.hip "WFMT"), tiles and
// scales indexed by the LOCAL expert. N % 64 == 0, K % 256 == 0 (ops.stream_moe_supported): every tiled expert.
//
// The streaming grouped kernel (wstream_grouped_kernel) is built for segments of tens of rows: a wave spans all rows of
// 32 columns, takes B from global memory and reads one A fragment from LDS per MFMA, so an expert's weights are
// streamed once per 128 of its rows. With hundreds to thousands of rows per expert the step is compute-bound and that
// split re-reads W and starves the MFMAs; ops.grouped_gemm (moe.hip) has the right shape but reads row-major bf16 only,
// which is why a quantised Mixtral kept a dequantised bf16 copy of every expert. This kernel reads the tiles.
//
//   * workgroup = 8 waves owns one (expert, row tile of BM = 256 entries, column block of 128): wave w has rows
//     64 (w & 3) .. + 64 and the column-tile pair (4 cb + 2 (w >> 2), + 1), a 2 x 2 block of 32 x 32 x 16 bf16 MFMAs, so
//     every A and every B fragment read from LDS feeds two MFMAs (the skinny GEMM's block, here per expert segment);
//   * no host sync after the router: the grid is (ceil(n_ent / BM) + E_local) row tiles x N / 128 column blocks, a
//     bound on sum_e ceil(cnt_e / BM); a workgroup finds its (expert, row tile) by a prefix over ceil(cnt_e / BM) read
//     from expert_off (E_local <= 16 scalar loads) and exits at once past the last tile;
//   * grid order: the ROW TILE is the fastest index, the column block the slowest, so the workgroups resident together
//     (one per CU: ~256 of them = all row tiles x ~10 column blocks) are the row tiles of a few column blocks, and the
//     row tiles of one expert, neighbours in launch order, read the same W column block (128 x K: 1 MB of bf16 at
//     K = 4096) while it is in L2 / MALL. W is the large operand (1.9 GB per Mixtral-8x7B layer in bf16 against 16-64 MB
//     of gathered X, which stays in the MALL whatever the order), so it is the one worth reading from HBM once; with
//     the column block fastest an expert's W would be streamed once per row tile (8 times at 8,192 tokens);
//   * both operands go by LDS-DMA (global_load_lds) into a ring of 64-deep K stages, a counted `s_waitcnt vmcnt` and one
//     raw `s_barrier` per stage. X rows are GATHERED: each lane's source row comes from perm_tok (GLU) or is the entry
//     itself (COMBINE), with the 16-B chunk c of row m kept at chunk c ^ (m & 7) by permuting on the source side (the DMA
//     writes lane-linear). Rows past the segment reload the segment's last row and are never stored;
//   * W travels as raw bytes; each wave dequantises its fragments between the ds_read and the MFMAs (dq8 / dq4 of
//     common.h: the exact bf16 values), activations are not quantised and the MFMA stays bf16. fp8: 8 blocks of 1 KB
//     per stage, one 16-B DMA instruction per wave; the fp32 row scales are loaded once per wave next to stage 0.
//     mxfp4: waves 0..3 fetch the 1 KB block of tile w, waves 4..7 the 64 B of e8m0 exponents of tile w - 4 (a 4-B DMA
//     into a 256-B slot) — a wave-uniform choice of WHAT the one extra instruction fetches, so every wave issues
//     DX + DW loads per stage on every path, the counted wait is one constant and "stage landed" covers the exponents;
//   * a column block past N (N % 128 == 64: the last block has one tile pair) re-reads the block's first pair into
//     the other pair's slots (same load count) and waves 4..7 store nothing;
//   * whole K in ascending order, no split-K: the fp8 / mxfp4 GLU outputs are bit-equal to the bf16 instantiation on
//     the dequantised tiles;
//   * GLU epilogue: a wave's two column tiles are the gate and the up of 32 output columns (its own accumulators); it
//     writes bf16 through a 4 KB LDS tile of its own and stores 16 B per lane, 64 B per row. COMBINE: fp32 atomics from
//     the accumulators (lanes along N), exactly k contributions per token.
// LDS: 3 x 48 KB (bf16), 3 x 40 KB (fp8), 4 x 37 KB (mxfp4): one workgroup per CU, as the skinny GEMM's ring depths.
// Registers and occupancy per instantiation: profiles/moe_tiles/resource_usage.txt.
#include "common.h"

namespace kafka {

namespace gtg {
constexpr int BM = 256, BN = 128, BK = 64;
constexpr int NW = 8;  // waves
template <int WF>
struct Cfg {
  static constexpr bool WQ = WF != WF_BF16;
  static constexpr int NS = WF == WF_MXFP4 ? 4 : 3;  // ring stages
  static constexpr int XB = BM * BK * 2;             // X bytes per stage (32 KB)
  static constexpr int WB = BN * BK * 2 / (WF == WF_MXFP4 ? 4 : (WF == WF_FP8 ? 2 : 1));  // 16 / 8 / 4 KB
  static constexpr int SB = WF == WF_MXFP4 ? 1024 : 0;  // mxfp4: four 256-B block-exponent slots per stage
  static constexpr int STAGE = XB + WB + SB;
  static constexpr int DX = XB / 1024 / NW;             // X DMA instructions per wave per stage
  static constexpr int DW = WQ ? 1 : WB / 1024 / NW;    // W (mxfp4: W or exponent) instructions per wave per stage
  static constexpr int DPS = DX + DW;
  // bytes of one column tile's K run per K column: bf16 [K/16][64][16 B], fp8 [K/32][64][16 B], mxfp4 [K/64][64][16 B]
  static constexpr int TKB = WF == WF_MXFP4 ? 16 : (WF == WF_FP8 ? 32 : 64);
};
// the scales' argument type per format (a specialisation, not std::conditional: see wstream_gemm.hip WfScales)
struct NoScale {};
template <int WF>
struct Scale {
  typedef NoScale type;
};
template <>
struct Scale<WF_FP8> {
  typedef const float* type;  // St [E_local][N], tile order
};
template <>
struct Scale<WF_MXFP4> {
  typedef const char* type;   // Se [E_local][N/32][K/64][32][2] e8m0 bytes
};

typedef __attribute__((address_space(3))) void lds_t;
__device__ __forceinline__ void dma16(const void* g, char* lds) {
  __builtin_amdgcn_global_load_lds(g, (lds_t*)lds, 16, 0, 0);
}
__device__ __forceinline__ void dma4(const void* g, char* lds) {
  __builtin_amdgcn_global_load_lds(g, (lds_t*)lds, 4, 0, 0);
}
}  // namespace gtg

// rt_max: row tiles of the grid (blockIdx.x = cb * rt_max + row tile)
template <int WF, bool GLU>
__global__ __launch_bounds__(512, 1) void grouped_tile_gemm_kernel(
    const bf16* __restrict__ X, int64_t ldx, const char* __restrict__ Wt, int N, int K,
    const int* __restrict__ perm_tok, const float* __restrict__ perm_w, const int* __restrict__ expert_off, int e_lo,
    int e_local, int rt_max, bf16* __restrict__ Y, int64_t ldy, float* __restrict__ out, int64_t ldo,
    typename gtg::Scale<WF>::type St) {
  using namespace gtg;
  using C = Cfg<WF>;
  constexpr int NS = C::NS, XB = C::XB, WB = C::WB, STAGE = C::STAGE, DX = C::DX, DW = C::DW, DPS = C::DPS;
  constexpr bool W8 = WF == WF_FP8, W4 = WF == WF_MXFP4, WQ = C::WQ;
  constexpr int RB = BK * 2, CPR = BK / 8, KB = BK / 16;  // X row bytes / 16-B chunks / k-steps per stage
  static_assert(DX == 4 && DW >= 1 && CPR == 8 && NS >= 3 && NS <= 4, "stage shape");
  static_assert(NS * STAGE <= 160 * 1024 && NS * STAGE >= NW * 64 * 32 * 2, "LDS of one gfx950 workgroup");
  __shared__ __attribute__((aligned(1024))) char smem[NS * STAGE];

  // (expert, row tile) of this workgroup: a prefix over the local experts' tile counts (all scalar, workgroup-uniform)
  const int cb = blockIdx.x / rt_max;
  int rt = blockIdx.x - cb * rt_max;
  int el = 0, seg0 = 0, cnt = 0;
  for (; el < e_local; ++el) {
    seg0 = expert_off[e_lo + el];
    cnt = expert_off[e_lo + el + 1] - seg0;
    const int tiles = (cnt + BM - 1) / BM;
    if (rt < tiles) break;
    rt -= tiles;
  }
  if (el == e_local) return;  // past the last tile
  const int row0 = rt * BM;
  const int rows = min(BM, cnt - row0);  // >= 1

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int rg = w & 3, cg = w >> 2;
  const int NT = N >> 5;                // column tiles of an expert
  const bool pair1 = cb * 4 + 2 < NT;   // the block's second tile pair exists (else N % 128 == 64, last block)
  // column tile t of the block, or where it is past N the tile two before it (its loads land in t's slots, unused)
  auto tile_of = [&](int t) { return cb * 4 + t - ((t >= 2 && !pair1) ? 2 : 0); };
  const int nst = K / BK;
  const char* We = Wt + (int64_t)el * NT * K * C::TKB;

  // per-lane DMA sources of this wave's share of a stage (stage s adds s * BK K columns)
  // X: instruction j = DX w + u covers LDS bytes [1024 j, +1024) = 8 rows; lane -> (row, slot), chunk c of row m at
  // slot c ^ (m % 8)
  const bf16* xsrc[DX];
#pragma unroll
  for (int u = 0; u < DX; ++u) {
    const int row = 8 * (DX * w + u) + lane / CPR, slot = lane % CPR;
    const int ent = seg0 + row0 + min(row, rows - 1);
    const int64_t src = GLU ? (int64_t)perm_tok[ent] : (int64_t)ent;
    xsrc[u] = X + src * ldx + 8 * (slot ^ (row % CPR));
  }
  // W. bf16: instruction j = DW w + u = (tile t = j / KB, k-step kk = j % KB), one 1 KB B fragment. fp8: block
  // (t = w / 2, kb2 = w % 2), the fragments of two k-steps. mxfp4: waves 0..3 the block of tile w (four k-steps), waves
  // 4..7 the 64 B of exponents of tile w - 4 (lanes >= 16 re-read them into the slot's unused 192 B). wq is w as a
  // scalar: the role branch is wave-uniform
  const char* wsrc[DW];
  int wq = 0;
  if constexpr (W8) {
    wsrc[0] = We + ((int64_t)tile_of(w >> 1) * (K >> 5) + (w & 1)) * 1024 + lane * 16;
  } else if constexpr (W4) {
    wq = __builtin_amdgcn_readfirstlane(w);
    const int64_t v = (int64_t)tile_of(wq & 3) * (K >> 6);  // (tile, kb4 = 0) of the expert
    wsrc[0] = wq < 4 ? We + v * 1024 + lane * 16
                     : St + ((int64_t)el * NT * (K >> 6) + v) * 64 + (lane & 15) * 4;
  } else {
#pragma unroll
    for (int u = 0; u < DW; ++u) {
      const int j = DW * w + u, t = j / KB, kk = j % KB;
      wsrc[u] = We + ((int64_t)tile_of(t) * (K >> 4) + kk) * 1024 + lane * 16;
    }
  }
  auto issue = [&](int s) {
    char* base = smem + (s % NS) * STAGE;
#pragma unroll
    for (int u = 0; u < DX; ++u) dma16(xsrc[u] + s * BK, base + (DX * w + u) * 1024);
    if constexpr (W8) {
      dma16(wsrc[0] + (int64_t)s * 2048, base + XB + w * 1024);
    } else if constexpr (W4) {
      if (wq < 4)
        dma16(wsrc[0] + (int64_t)s * 1024, base + XB + wq * 1024);
      else
        dma4(wsrc[0] + (int64_t)s * 64, base + XB + WB + (wq - 4) * 256);
    } else {
#pragma unroll
      for (int u = 0; u < DW; ++u) dma16(wsrc[u] + (int64_t)s * KB * 1024, base + XB + (DW * w + u) * 1024);
    }
  };

  float wsc[2] = {1.f, 1.f};  // fp8: 2^e of this lane's row in the wave's two column tiles
  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;

  // s_waitcnt vmcnt(n * DPS) for a wave-uniform n in [0, NS - 2] (the count is an immediate)
  auto wait_stage = [&](int n) {
    if (NS > 3 && n >= 2) wait_vmcnt<(NS > 3 ? 2 : 0) * DPS>();
    else if (n >= 1) wait_vmcnt<DPS>();
    else wait_vmcnt<0>();
  };
  if constexpr (W8) {
    // the row scales are consumed here, between stage 0's issue and the rest of the prologue: hipcc waits for a register
    // load next to LDS-DMA loads with vmcnt(0), which left to the first dq8 would sit in the loop and drain the ring
    wsc[0] = St[(int64_t)el * N + 32 * tile_of(2 * cg) + r];
    wsc[1] = St[(int64_t)el * N + 32 * tile_of(2 * cg + 1) + r];
    issue(0);
    asm volatile("" : "+v"(wsc[0]), "+v"(wsc[1]));
    for (int s = 1; s < NS - 1; ++s) issue(s);  // (nst >= 4: K % 256 == 0)
  } else {
    for (int s = 0; s < NS - 1; ++s) issue(s);
  }
  for (int s = 0; s < nst; ++s) {
    // this wave's DMAs of stage s have landed (the NS - 2 later stages may be in flight), then every wave's have, and
    // every wave is done reading slot (s + NS - 1) % NS (stage s - 1)
    wait_stage(min(NS - 2, nst - 1 - s));
    asm volatile("s_barrier" ::: "memory");
    if (s + NS - 1 < nst) issue(s + NS - 1);
    const char* xs = smem + (s % NS) * STAGE;
    const char* ws = xs + XB;
    // quantised: the raw vectors of the wave's two tiles (fp8: two per tile, k-steps 0, 1 and 2, 3; mxfp4: one, dword kk
    // = k-step kk) and, mxfp4, the lane's row's exponent pair (byte 0: k-steps 0, 1; byte 1: k-steps 2, 3)
    constexpr int NV = W8 ? 2 : 1;
    u32x4 q[2][NV];
    uint32_t e2[2] = {0, 0};
    if constexpr (WQ) {
#pragma unroll
      for (int b = 0; b < 2; ++b) {
#pragma unroll
        for (int v = 0; v < NV; ++v)
          q[b][v] = *reinterpret_cast<const u32x4*>(ws + ((2 * cg + b) * NV + v) * 1024 + lane * 16);
        if constexpr (W4) e2[b] = *reinterpret_cast<const uint16_t*>(ws + WB + (2 * cg + b) * 256 + 2 * r);
      }
    }
    auto wfrag = [&](int b, int kk) -> bf16x8 {  // B fragment of tile 2 cg + b, k-step kk of the stage
      if constexpr (W8) {
        const u32x4 v = q[b][kk >> 1];
        return (kk & 1) ? dq8(v[2], v[3], wsc[b]) : dq8(v[0], v[1], wsc[b]);
      } else if constexpr (W4) {
        const uint32_t eb = (kk & 2) ? e2[b] >> 8 : e2[b] & 0xffu;
        return dq4(q[b][0][kk], __builtin_bit_cast(float, eb << 23));
      } else {
        return *reinterpret_cast<const bf16x8*>(ws + ((2 * cg + b) * KB + kk) * 1024 + lane * 16);
      }
    };
#pragma unroll
    for (int kk = 0; kk < KB; ++kk) {
      const int c = 2 * kk + h;
      const int m0 = 64 * rg + r, m1 = m0 + 32;
      const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(xs + m0 * RB + 16 * (c ^ (m0 % CPR)));
      const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(xs + m1 * RB + 16 * (c ^ (m1 % CPR)));
      const bf16x8 b0 = wfrag(0, kk);
      const bf16x8 b1 = wfrag(1, kk);
      acc[0][0] = mfma32(a0, b0, acc[0][0]);
      acc[0][1] = mfma32(a0, b1, acc[0][1]);
      acc[1][0] = mfma32(a1, b0, acc[1][0]);
      acc[1][1] = mfma32(a1, b1, acc[1][1]);
    }
  }

  // epilogues. C lane layout (lanes along N): acc[a][b][i] -> row 64 rg + 32 a + (i & 3) + 8 (i >> 2) + 4 h of the
  // tile, column (4 cb + 2 cg + b) * 32 + r
  const bool active = cg == 0 || pair1;  // wave-uniform
  const int ent0 = seg0 + row0;
  if constexpr (GLU) {
    // (gate, up) = (tile 4 cb + 2 cg, + 1): output columns [(2 cb + cg) * 32, + 32). Through a per-wave LDS tile
    // [64 rows][32] bf16 (the ring is dead once every wave is past its last stage), then 16 B per lane, 4 lanes a row
    __syncthreads();
    if (!active) return;
    bf16* tp = reinterpret_cast<bf16*>(smem) + w * 64 * 32;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float g = acc[a][0][i], u = acc[a][1][i];
        tp[(32 * a + (i & 3) + 8 * (i >> 2) + 4 * h) * 32 + r] = (bf16)(g / (1.0f + __expf(-g)) * u);
      }
    // (one wave's LDS accesses complete in order: the reads below see its writes)
    const int n0 = (2 * cb + cg) * 32;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int qi = j * 64 + lane, row = qi >> 2, c8 = qi & 3;
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(tp + row * 32 + 8 * c8);
      const int m = 64 * rg + row;
      if (m < rows) store_bf16x8(Y + (int64_t)(ent0 + m) * ldy + n0 + 8 * c8, v);
    }
  } else {
    if (!active) return;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int m = 64 * rg + 32 * a + (i & 3) + 8 * (i >> 2) + 4 * h;
        if (m < rows) {
          const int ent = ent0 + m;
          float* o = out + (int64_t)perm_tok[ent] * ldo + (4 * cb + 2 * cg) * 32 + r;
          const float pw = perm_w[ent];
          atomicAdd(o, pw * acc[a][0][i]);
          atomicAdd(o + 32, pw * acc[a][1][i]);
        }
      }
  }
}

template <int WF>
static hipError_t grouped_tile_launch(const bf16* X, int64_t ldx, const void* Wt, typename gtg::Scale<WF>::type sc,
                                      int e_local, int N, int K, const int* perm_tok, const float* perm_w,
                                      const int* expert_off, int e_lo, int n_ent, int glu, bf16* Y, int64_t ldy,
                                      float* out, int64_t ldo, hipStream_t st) {
  using namespace gtg;
  const int rt_max = (n_ent + BM - 1) / BM + e_local;  // >= sum over the local experts of ceil(cnt_e / BM)
  const dim3 grid((unsigned)rt_max * ((N + BN - 1) / BN));
  const char* wt = static_cast<const char*>(Wt);
  if (glu)
    grouped_tile_gemm_kernel<WF, true><<<grid, NW * 64, 0, st>>>(X, ldx, wt, N, K, perm_tok, perm_w, expert_off, e_lo,
                                                                 e_local, rt_max, Y, ldy, out, ldo, sc);
  else
    grouped_tile_gemm_kernel<WF, false><<<grid, NW * 64, 0, st>>>(X, ldx, wt, N, K, perm_tok, perm_w, expert_off, e_lo,
                                                                  e_local, rt_max, Y, ldy, out, ldo, sc);
  return hipGetLastError();
}

// Expert MLP halves of prefill-sized steps on the expert tiles (see grouped_tile_gemm_kernel). n_ent: routed entries
// (the length of perm_tok / perm_w); glu: gate_up from X[perm_tok[entry]] with fused SwiGLU into Y [n_ent, N/2]; else
// down from X[entry] with the weighted combine into out f32 [T, N]. wfmt, Wt and scale as kafka_launch_wstream_grouped.
extern "C" hipError_t kafka_launch_grouped_tile_gemm(const bf16* X, int64_t ldx, int wfmt, const void* Wt,
                                                    const void* scale, int e_local, int N, int K, const int* perm_tok,
                                                    const float* perm_w, const int* expert_off, int e_lo, int n_ent,
                                                    int glu, bf16* Y, int64_t ldy, float* out, int64_t ldo,
                                                    hipStream_t st) {
  using namespace gtg;
  if (N <= 0 || K <= 0 || N % 64 != 0 || K % 256 != 0 || ldx % 8 != 0) return hipErrorInvalidValue;
  if (Wt == nullptr || e_local > 16 || (glu ? (Y == nullptr || ldy % 8 != 0) : out == nullptr))
    return hipErrorInvalidValue;
  if ((wfmt == WF_BF16) != (scale == nullptr)) return hipErrorInvalidValue;  // quantised tiles need their scales
  if (wfmt != WF_BF16 && wfmt != WF_FP8 && wfmt != WF_MXFP4) return hipErrorInvalidValue;
  if (n_ent < 1 || e_local < 1) return hipSuccess;
  switch (wfmt) {
    case WF_FP8:
      return grouped_tile_launch<WF_FP8>(X, ldx, Wt, static_cast<const float*>(scale), e_local, N, K, perm_tok, perm_w,
                                         expert_off, e_lo, n_ent, glu, Y, ldy, out, ldo, st);
    case WF_MXFP4:
      return grouped_tile_launch<WF_MXFP4>(X, ldx, Wt, static_cast<const char*>(scale), e_local, N, K, perm_tok,
                                           perm_w, expert_off, e_lo, n_ent, glu, Y, ldy, out, ldo, st);
    default:
      return grouped_tile_launch<WF_BF16>(X, ldx, Wt, NoScale{}, e_local, N, K, perm_tok, perm_w, expert_off, e_lo,
                                          n_ent, glu, Y, ldy, out, ldo, st);
  }
}

}  // namespace kafka
