// MXFP8 activations on the MXFP4 expert tiles (gfx950): the expert MLP halves of prefill-sized MoE steps on
// v_mfma_scale_f32_32x32x64_f8f6f4, A = e4m3 (cbsz 0), B = e2m1 (blgp 4), both block scales as the instruction's scale
// operands. Nothing is dequantised in VALU and no bf16 MFMA runs here.
//     per local expert el and its routing segment [expert_off[e_lo + el], expert_off[e_lo + el + 1]):
//     GLU:      Y[entry, :N/2]  = silu(gate) * up of Xq[perm_tok[entry]] . W_el^T            (bf16)
//     GLU_MX:   (Aq, Ae)[entry] = the MXFP8 quantisation of that bf16 row                      (e4m3 + e8m0)
//     COMBINE:  out[perm_tok[entry], n] += perm_w[entry] * (Xq[entry] . W_el^T)               (fp32 atomics)
// The contract is grouped_tile_gemm_kernel<WF_MXFP4, GLU>'s (grouped_tile_gemm.hip): local experts [e_lo, e_lo +
// e_local), e_local <= 16, segments read from expert_off on the device (no host sync), N % 64 == 0, K % 256 == 0, tiles
// and scales indexed by the LOCAL expert, out zeroed by the caller.
//
// Operands: Xq e4m3 [rows, K] in natural K order (ldxq % 16 == 0) and Xe e8m0 [rows, K/32], as act_quant_mxfp8_kernel or
// the GLU_MX epilogue below leave them; Wt4 / Se the stored expert image (e2m1 [E, N/32, K/64, 64, 16], e8m0
// [E, N/32, K/64, 32, 2]): the dense image per expert, no re-tiling. The operand and scale layout of the 32 x 32 x 64
// scaled MFMA is written up in the header of tile_gemm_mx.hip.
//
// Split of work: the dense scaled kernel's (tile_gemm_mx_kernel), not the 2 x 2 split of the bf16 grouped kernel.
//   * 8 waves own one (expert, 256-entry row tile, 256-column block); wave w = row half w & 1 x column group w >> 1, a
//     4 x 2 block of scaled MFMAs with 8 accumulators; a ring of three 128-deep stages of 52 KB (Xq 32 KB, Wt4 16 KB,
//     2 KB of Xe, 2 KB of Se), everything by LDS-DMA, 8 loads per wave and stage on every wave, one counted
//     `s_waitcnt vmcnt(8)` and one raw barrier per stage; B regrouped by two v_permlane32_swap, A two ds_read_b128 per
//     fragment, scales from small LDS reads selected by op_sel. Per accumulator the same instruction over ascending K
//     as the dense kernel and no split-K: the GLU output of one expert with an identity routing is bit-equal to
//     tile_gemm_mx_kernel<EPI_GLU>.
//   * the grouped prologue is what is new. The grid is (ceil(n_ent / 256) + e_local) row tiles x ceil(N / 256) column
//     blocks, the row tile the fastest index (the row tiles of an expert, neighbours in launch order, read one W column
//     block while it is in L2 / MALL); a workgroup finds (expert, row tile) by the prefix over ceil(cnt_e / 256) and
//     exits at once past the last tile. Both activation operands are GATHERED by the per-lane DMA source: lane row m
//     reads Xq row perm_tok[ent] (GLU halves) or row ent (COMBINE) with the source-side chunk swizzle c ^ (m & 7), and
//     the 4-B exponent fetch of wave w for rows 32 w + r gathers the same row of Xe. Rows past the segment re-read the
//     segment's last row and are never stored. N tail as in the dense kernel: nbt in {2, 4, 6, 8}, waves past N re-read
//     the first pair and store nothing.
//   * epilogues, each through the wave's own 8 KB LDS tile once the ring is dead. GLU: tile_epilogue<EPI_GLU>
//     unchanged, row0 = the tile's first entry. GLU_MX: a wave's (gate, up) pair is 32 output columns = exactly one MX
//     block along the K of the down GEMM, so after silu(g) * u is rounded to bf16 into the LDS tile each lane reads
//     its 16 B, the 4 lanes of a row run the quantiser's body (mx_quant.h) and store 8 B of e4m3 each and one e8m0
//     byte per row: the bf16 intermediate [n_ent, F] is never written or read back. The result equals
//     ops.reference.mxfp8_quant of the bf16 GLU output bit for bit. COMBINE: fp32 atomics from the accumulators (lanes
//     along N), exactly k contributions per token.
// Registers, LDS and occupancy: profiles/moe_act_mxfp8/resource_usage.txt.
#include <type_traits>

#include "common.h"
#include "mx_quant.h"
#include "tile_epilogue.h"

namespace kafka {

namespace gmx {
using namespace tlg;
enum { GMX_GLU = 0, GMX_GLU_MX = 1, GMX_COMBINE = 2 };
constexpr int BM = 256, BN = 256, BK = 128;
constexpr int NW = 8;          // waves
constexpr int NT_B = BN / 32;  // column tiles of a block
constexpr int NS = 3;          // ring stages
constexpr int XB = BM * BK;    // Xq bytes per stage (32 KB)
constexpr int WB = BN * BK / 2;  // Wt4 bytes per stage (16 KB)
constexpr int EB = NW * 256;   // one scale area: eight 256-B slots
constexpr int STAGE = XB + WB + 2 * EB;
constexpr int DX = XB / 1024 / NW, DW = WB / 1024 / NW;  // Xq / Wt4 DMA instructions per wave per stage
constexpr int DPS = DX + DW + 2;
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
}  // namespace gmx

// rt_max: row tiles of the grid (blockIdx.x = cb * rt_max + row tile)
template <int EPI>
__global__ __launch_bounds__(512, 1) void grouped_tile_gemm_mx_kernel(
    const uint8_t* __restrict__ Xq, int64_t ldxq, const uint8_t* __restrict__ Xe, const char* __restrict__ Wt,
    const char* __restrict__ Se, int N, int K, const int* __restrict__ perm_tok, const float* __restrict__ perm_w,
    const int* __restrict__ expert_off, int e_lo, int e_local, int rt_max, bf16* __restrict__ Y, int64_t ldy,
    uint8_t* __restrict__ Aq, uint8_t* __restrict__ Ae, float* __restrict__ out, int64_t ldo) {
  using namespace gmx;
  constexpr bool GATHER = EPI != GMX_COMBINE;
  constexpr int RB = BK, CPR = BK / 16, KB = BK / 64;  // Xq row bytes / 16-B chunks / k-steps per stage
  static_assert(DX == 4 && DW == 2 && CPR == 8 && KB == 2, "stage shape");
  static_assert(NS * STAGE <= 160 * 1024 && NS * STAGE >= NW * 8192, "LDS of one gfx950 workgroup; epilogue tiles");
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
  const int ent0 = seg0 + row0;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int rh = w & 1, cg = w >> 1;
  const int NT = N >> 5;                      // column tiles of an expert (even)
  const int nbt = min(NT_B, NT - cb * NT_B);  // column tiles of this block: 2, 4, 6 or 8
  // column tile t of the block, or where it is past N a tile of the block's first pair (its loads land in t's slots,
  // unused)
  auto tile_of = [&](int t) { return cb * NT_B + (t < nbt ? t : (t & 1)); };
  const int nst = K / BK;  // even, >= 2

  // per-lane DMA sources of this wave's share of a stage (stage s adds s * BK K columns)
  // Xq: instruction j = DX w + u covers LDS bytes [1024 j, +1024) = 8 rows; lane -> (row, slot), the row gathered
  const uint8_t* xsrc[DX];
#pragma unroll
  for (int u = 0; u < DX; ++u) {
    const int row = 8 * (DX * w + u) + lane / CPR, slot = lane % CPR;
    const int ent = ent0 + min(row, rows - 1);
    const int64_t src = GATHER ? (int64_t)perm_tok[ent] : (int64_t)ent;
    xsrc[u] = Xq + src * ldxq + 16 * (slot ^ (row % CPR));
  }
  // Xe: the stage's four exponents of row 32 w + r (both half-waves), the same gathered row
  const uint8_t* esrc;
  {
    const int ent = ent0 + min(32 * w + r, rows - 1);
    const int64_t src = GATHER ? (int64_t)perm_tok[ent] : (int64_t)ent;
    esrc = Xe + src * (K >> 5);
  }
  // Wt4 / Se of the LOCAL expert: wave w fetches column tile w of the block, the vectors kb4 = 2 s, 2 s + 1 of a stage
  const int64_t v0 = ((int64_t)el * NT + tile_of(w)) * (K >> 6);
  const char* wsrc = Wt + v0 * 1024 + lane * 16;
  const char* ssrc = Se + v0 * 64 + r * 4;
  auto issue = [&](int s) {
    char* base = smem + (s % NS) * STAGE;
#pragma unroll
    for (int u = 0; u < DX; ++u) dma16(xsrc[u] + s * BK, base + (DX * w + u) * 1024);
#pragma unroll
    for (int u = 0; u < DW; ++u) dma16(wsrc + (int64_t)(s * DW + u) * 1024, base + XB + (DW * w + u) * 1024);
    dma4(esrc + s * (BK / 32), base + XB + WB + w * 256);
    dma4(ssrc + (int64_t)s * (DW * 64), base + XB + WB + EB + w * 256);
  };

  f32x16 acc[4][2];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;

  for (int s = 0; s < NS - 1; ++s) issue(s);
  for (int s = 0; s < nst; ++s) {
    // this wave's DMAs of stage s have landed (stage s + 1 may be in flight), then every wave's have, and every wave
    // is done reading slot (s + NS - 1) % NS (stage s - 1)
    if (s + 1 < nst) wait_vmcnt<DPS>();
    else wait_vmcnt<0>();
    asm volatile("s_barrier" ::: "memory");
    if (s + NS - 1 < nst) issue(s + NS - 1);
    const char* xs = smem + (s % NS) * STAGE;
    const char* ws = xs + XB;
    const char* es = ws + WB;
    // scales of the stage: byte 0 = the lane's block of k-step 0, byte 2 = of k-step 1
    int sa[4], sb[2];
#pragma unroll
    for (int a = 0; a < 4; ++a)
      sa[a] = (int)(*reinterpret_cast<const uint32_t*>(es + (4 * rh + a) * 256 + 4 * r) >> (8 * h));
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const char* p = es + EB + (2 * cg + b) * 256 + 2 * r;
      const uint32_t lo = *reinterpret_cast<const uint16_t*>(p), hi = *reinterpret_cast<const uint16_t*>(p + 64);
      sb[b] = (int)((lo | (hi << 16)) >> (8 * h));
    }
    auto kstep = [&](auto kc) {  // (op_sel is an immediate: the k-step is a compile-time value)
      constexpr int kk = decltype(kc)::value;
      i32x8 bv[2];
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const u32x4 q = *reinterpret_cast<const u32x4*>(ws + ((2 * cg + b) * DW + kk) * 1024 + lane * 16);
        const auto p02 = __builtin_amdgcn_permlane32_swap(q[0], q[2], false, false);
        const auto p13 = __builtin_amdgcn_permlane32_swap(q[1], q[3], false, false);
        bv[b] = i32x8{(int)p02[0], (int)p02[1], (int)p13[0], (int)p13[1], 0, 0, 0, 0};
      }
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const int m = 128 * rh + 32 * a + r;
        const i32x4 lo = *reinterpret_cast<const i32x4*>(xs + m * RB + 16 * ((4 * kk + h) ^ (m % CPR)));
        const i32x4 hi = *reinterpret_cast<const i32x4*>(xs + m * RB + 16 * ((4 * kk + 2 + h) ^ (m % CPR)));
        const i32x8 av = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        acc[a][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv[0], acc[a][0], 0, 4, 2 * kk, sa[a], 2 * kk,
                                                                    sb[0]);
        acc[a][1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv[1], acc[a][1], 0, 4, 2 * kk, sa[a], 2 * kk,
                                                                    sb[1]);
      }
    };
    kstep(std::integral_constant<int, 0>{});
    kstep(std::integral_constant<int, 1>{});
  }

  // epilogues. C lane layout (lanes along N): acc[a][b][i] -> row 128 rh + 32 a + (i & 3) + 8 (i >> 2) + 4 h of the
  // tile, column cb * 256 + 64 cg + 32 b + r of W
  const int mw = 128 * rh, nw = cb * BN + 64 * cg;
  if constexpr (EPI == GMX_COMBINE) {
    if (2 * cg >= nbt) return;  // wave-uniform: the column group lies past N
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int m = mw + 32 * a + (i & 3) + 8 * (i >> 2) + 4 * h;
        if (m < rows) {
          const int ent = ent0 + m;
          float* o = out + (int64_t)perm_tok[ent] * ldo + nw + r;
          const float pw = perm_w[ent];
          atomicAdd(o, pw * acc[a][0][i]);
          atomicAdd(o + 32, pw * acc[a][1][i]);
        }
      }
  } else {
    // through the wave's own 8 KB LDS tile: the ring is dead once every wave is past its last stage
    __syncthreads();
    if (2 * cg >= nbt) return;
    char* tp = smem + w * 8192;
    if constexpr (EPI == GMX_GLU) {
      tile_epilogue<EPI_GLU>(acc, tp, lane, mw, nw, ent0, rows, 0, N, 0, Y, ldy, nullptr);
    } else {
      tile_epilogue_glu_mx(acc, tp, lane, mw, nw, ent0, rows, N >> 1, Aq, Ae);  // (tile_epilogue.h: EPI_GLU_MX)
    }
  }
}

// Expert MLP halves with MXFP8 activations on the MXFP4 expert tiles (see grouped_tile_gemm_mx_kernel). Xq e4m3
// [rows, K] with row stride ldxq % 16 == 0 and Xe e8m0 [rows, K/32] contiguous: token rows gathered through perm_tok
// with glu, one row per routed entry otherwise. glu: fused SwiGLU into Y bf16 [n_ent, N/2] (row stride ldy % 8 == 0), or
// where Aq is given into its MXFP8 form Aq [n_ent, N/2] / Ae [n_ent, N/64], both contiguous (exactly one of Y and the
// pair); else the weighted combine into out f32 [T, N] (zeroed by the caller). hipErrorInvalidValue for a misaligned
// ldxq, null pointers, e_local > 16, N % 64 != 0 and K % 256 != 0; a no-op for n_ent < 1.
extern "C" hipError_t kafka_launch_grouped_tile_gemm_mx(const uint8_t* Xq, int64_t ldxq, const uint8_t* Xe,
                                                       const void* Wt4, const void* Se, int e_local, int N, int K,
                                                       const int* perm_tok, const float* perm_w, const int* expert_off,
                                                       int e_lo, int n_ent, int glu, bf16* Y, int64_t ldy, uint8_t* Aq,
                                                       uint8_t* Ae, float* out, int64_t ldo, hipStream_t st) {
  using namespace gmx;
  if (N <= 0 || K <= 0 || N % 64 != 0 || K % 256 != 0 || ldxq % 16 != 0 || ldxq < K) return hipErrorInvalidValue;
  if (Xq == nullptr || Xe == nullptr || Wt4 == nullptr || Se == nullptr || perm_tok == nullptr || perm_w == nullptr ||
      expert_off == nullptr || e_local > 16 || e_lo < 0)
    return hipErrorInvalidValue;
  if (glu) {
    if ((Y != nullptr) == (Aq != nullptr) || (Aq != nullptr) != (Ae != nullptr)) return hipErrorInvalidValue;
    if (Y != nullptr && ldy % 8 != 0) return hipErrorInvalidValue;
  } else if (out == nullptr) {
    return hipErrorInvalidValue;
  }
  if (n_ent < 1 || e_local < 1) return hipSuccess;
  const int64_t rt_max = (int64_t)(n_ent + BM - 1) / BM + e_local;  // >= sum over the local experts of ceil(cnt_e / BM)
  if (rt_max * ((N + BN - 1) / BN) > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(rt_max * ((N + BN - 1) / BN)));
  const char* wt = static_cast<const char*>(Wt4);
  const char* se = static_cast<const char*>(Se);
  if (!glu)
    grouped_tile_gemm_mx_kernel<GMX_COMBINE><<<grid, NW * 64, 0, st>>>(
        Xq, ldxq, Xe, wt, se, N, K, perm_tok, perm_w, expert_off, e_lo, e_local, (int)rt_max, Y, ldy, Aq, Ae, out, ldo);
  else if (Aq != nullptr)
    grouped_tile_gemm_mx_kernel<GMX_GLU_MX><<<grid, NW * 64, 0, st>>>(
        Xq, ldxq, Xe, wt, se, N, K, perm_tok, perm_w, expert_off, e_lo, e_local, (int)rt_max, Y, ldy, Aq, Ae, out, ldo);
  else
    grouped_tile_gemm_mx_kernel<GMX_GLU><<<grid, NW * 64, 0, st>>>(
        Xq, ldxq, Xe, wt, se, N, K, perm_tok, perm_w, expert_off, e_lo, e_local, (int)rt_max, Y, ldy, Aq, Ae, out, ldo);
  return hipGetLastError();
}

}  // namespace kafka
