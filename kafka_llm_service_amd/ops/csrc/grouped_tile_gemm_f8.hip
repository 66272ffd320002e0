// fp8 activations on the fp8 expert tiles (gfx950): the expert MLP halves of prefill-sized MoE steps on the 32 x 32 x 64
// f8f6f4 MFMA with both operands e4m3 (cbsz 0, blgp 0, both scale operands the constant 0: the UNSCALED instruction).
// Nothing is dequantised in VALU and no bf16 MFMA runs here: one power-of-two exponent per activation row, one
// power-of-two scale per weight row, both applied to the fp32 accumulators in the epilogue.
//     per local expert el and its routing segment [expert_off[e_lo + el], expert_off[e_lo + el + 1]):
//     with P[row] = (Xq[row] . W_el^T) * 2^Ea[row] * St_el[n]:
//     GLU:      Y[entry, :N/2]  = silu(gate) * up of P[perm_tok[entry]]                        (bf16)
//     COMBINE:  out[perm_tok[entry], n] += perm_w[entry] * P[entry]                            (fp32 atomics)
// The contract is grouped_tile_gemm_kernel<WF_FP8, GLU>'s (grouped_tile_gemm.hip) and
// kafka_launch_grouped_tile_gemm_mx's: local experts [e_lo, e_lo + e_local), e_local <= 16, segments read from expert_off on the device (no host sync),
// N % 64 == 0, K % 256 == 0, tiles and row scales indexed by the LOCAL expert, out zeroed by the caller, n_ent < 1 a
// no-op, a refused call writes nothing.
//
// Operands: Wt8 / St the stored fp8 expert image (e4m3 [E, N/32, K/32, 64, 16] + fp32 row scales [E, N] in tile order)
// exactly as tile_experts_fp8 leaves it: the dense image per expert, no second copy and no re-tiling. Xq e4m3 bytes
// [rows, K] in FP8-TILE K ORDER (ldxq % 16 == 0) and Ea int32 [rows], as act_quant_fp8_kernel (tile_gemm_f8.hip) leaves
// them; the K order and the measured operand layout of the e4m3 x e4m3 form are written up in that unit's header.
//
// Split of work (what was built)
//   * the main loop is tile_gemm_f8_kernel's: 8 waves own one (expert, 256-entry row tile, 256-column block); wave w =
//     row half w & 1 x column group w >> 1, a 4 x 2 block of MFMAs with 8 accumulators; a ring of FIVE 64-deep stages of
//     32 KB (Xq 16 KB with the chunk swizzle c ^ ((m >> 2) & 3) on the DMA source side, Wt8 16 KB), everything by
//     LDS-DMA, 2 + 2 loads per wave and stage, one counted `s_waitcnt vmcnt` and one raw barrier per stage, no register
//     load in the K loop. Per accumulator the same MFMAs over ascending K as the dense kernel and no split-K: the GLU
//     output of one expert with an identity routing is bit-equal to tile_gemm_f8_kernel<EPI_GLU>.
//   * the grouped prologue is grouped_tile_gemm_mx_kernel's: the grid is (ceil(n_ent / 256) + e_local) row tiles x
//     ceil(N / 256) column blocks, the row tile the fastest index; a workgroup finds (expert, row tile) by the scalar
//     prefix over ceil(cnt_e / 256) and exits at once past the last tile. Activation rows are GATHERED by the per-lane
//     DMA source: lane row m reads Xq row perm_tok[ent] (GLU) or row ent (COMBINE). Rows past the segment re-read the
//     segment's last row and are never stored. N tail as in the dense kernel: nbt in {2, 4, 6, 8}, waves past N re-read
//     the first pair and store nothing.
//   * exponents: once the ring is dead the 256 row exponents of the tile (gathered through perm_tok in the GLU half,
//     read by entry in the COMBINE half) and the 256 column exponents of the LOCAL expert's row scales go into 2 KB of
//     LDS behind the epilogue tiles, as integers; the accumulators are scaled with v_ldexp_f32 (exact; 2^ea * sw is
//     never formed as a float: it could leave fp32's range where the product does not).
//   * epilogues. GLU: tile_epilogue<EPI_GLU> unchanged, row0 = the tile's first entry, bf16 [n_ent, N/2]. COMBINE: fp32
//     atomics from the scaled accumulators (lanes along N), exactly k contributions per token.
//   * LDS 160 KB, 1 workgroup per CU; VGPRs and the absence of scratch: profiles/moe_act_fp8/resource_usage.txt.
// Not built: a quantising GLU epilogue. A per-row format needs the amax over the whole of F and no 256-column tile can
// know it, so the intermediate between the halves stays a bf16 [n_ent, F] tensor and act_quant_fp8_kernel runs on it
// with M = n_ent, K = F (it reads each row once). Nor a 128-row tile for short segments.
#include "common.h"
#include "tile_epilogue.h"

namespace kafka {

namespace gf8 {
using namespace tlg;
constexpr int BM = 256, BN = 256, BK = 64;
constexpr int NW = 8;          // waves
constexpr int NT_B = BN / 32;  // column tiles of a block
constexpr int NS = 5;          // ring stages
constexpr int XB = BM * BK;    // Xq bytes per stage (16 KB)
constexpr int WB = BN * BK;    // Wt8 bytes per stage (16 KB)
constexpr int STAGE = XB + WB;
constexpr int DX = XB / 1024 / NW, DW = WB / 1024 / NW;  // Xq / Wt8 DMA instructions per wave per stage
constexpr int DPS = DX + DW;
constexpr int EPB = NW * 8192;  // the epilogue tiles; the exponents of the tile's rows and columns follow
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// s_waitcnt vmcnt(n * DPS) for a wave-uniform n in [0, NS - 2] (the count is an immediate)
__device__ __forceinline__ void wait_stages(int n) {
  static_assert(NS == 5, "one case per stage that may stay in flight");
  switch (n) {
    case 0: wait_vmcnt<0>(); break;
    case 1: wait_vmcnt<DPS>(); break;
    case 2: wait_vmcnt<2 * DPS>(); break;
    default: wait_vmcnt<3 * DPS>(); break;
  }
}
}  // namespace gf8

// rt_max: row tiles of the grid (blockIdx.x = cb * rt_max + row tile)
template <bool GLU>
__global__ __launch_bounds__(512, 1) void grouped_tile_gemm_f8_kernel(
    const uint8_t* __restrict__ Xq, int64_t ldxq, const int* __restrict__ Ea, const char* __restrict__ Wt,
    const float* __restrict__ St, int N, int K, const int* __restrict__ perm_tok, const float* __restrict__ perm_w,
    const int* __restrict__ expert_off, int e_lo, int e_local, int rt_max, bf16* __restrict__ Y, int64_t ldy,
    float* __restrict__ out, int64_t ldo) {
  using namespace gf8;
  constexpr int RB = BK, CPR = BK / 16;  // Xq row bytes / 16-B chunks of a stage
  static_assert(DX == 2 && DW == 2 && CPR == 4, "stage shape");
  static_assert(NS * STAGE <= 160 * 1024 && NS * STAGE >= EPB + 2048, "LDS of one gfx950 workgroup; epilogue area");
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
  const int nst = K / BK;  // a multiple of 4
  // the row of Xq / Ea behind row m of the tile (rows past the segment: the segment's last)
  auto src_row = [&](int m) {
    const int ent = ent0 + min(m, rows - 1);
    return GLU ? (int64_t)perm_tok[ent] : (int64_t)ent;
  };

  // per-lane DMA sources of this wave's share of a stage (stage s adds s * BK K columns)
  // Xq: instruction j = DX w + u covers LDS bytes [1024 j, +1024) = 16 rows; lane -> (row, slot), the row gathered
  const uint8_t* xsrc[DX];
#pragma unroll
  for (int u = 0; u < DX; ++u) {
    const int row = 16 * (DX * w + u) + lane / CPR, slot = lane % CPR;
    xsrc[u] = Xq + src_row(row) * ldxq + 16 * (slot ^ ((row >> 2) & 3));
  }
  // Wt8 of the LOCAL expert: wave w fetches column tile w of the block, the stored tiles kb2 = 2 s, 2 s + 1 of a stage
  const char* wsrc = Wt + ((int64_t)el * NT + tile_of(w)) * (K >> 5) * 1024 + lane * 16;
  auto issue = [&](int s) {
    char* base = smem + (s % NS) * STAGE;
#pragma unroll
    for (int u = 0; u < DX; ++u) dma16(xsrc[u] + s * BK, base + (DX * w + u) * 1024);
#pragma unroll
    for (int u = 0; u < DW; ++u) dma16(wsrc + (int64_t)(s * DW + u) * 1024, base + XB + (DW * w + u) * 1024);
  };

  f32x16 acc[4][2];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;

  for (int s = 0; s < NS - 1; ++s) issue(s);  // (nst >= 4)
  for (int s = 0; s < nst; ++s) {
    // this wave's DMAs of stage s have landed (up to NS - 2 later stages may be in flight), then every wave's have, and
    // every wave is done reading slot (s + NS - 1) % NS (stage s - 1)
    wait_stages(min(NS - 2, nst - 1 - s));
    asm volatile("s_barrier" ::: "memory");
    if (s + NS - 1 < nst) issue(s + NS - 1);
    const char* xs = smem + (s % NS) * STAGE;
    const char* ws = xs + XB;
    i32x8 bv[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const char* p = ws + (2 * cg + b) * DW * 1024 + lane * 16;
      const i32x4 lo = *reinterpret_cast<const i32x4*>(p), hi = *reinterpret_cast<const i32x4*>(p + 1024);
      bv[b] = i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int m = 128 * rh + 32 * a + r, sw = (m >> 2) & 3;
      const i32x4 lo = *reinterpret_cast<const i32x4*>(xs + m * RB + 16 * (h ^ sw));
      const i32x4 hi = *reinterpret_cast<const i32x4*>(xs + m * RB + 16 * ((2 + h) ^ sw));
      const i32x8 av = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      acc[a][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv[0], acc[a][0], 0, 0, 0, 0, 0, 0);
      acc[a][1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv[1], acc[a][1], 0, 0, 0, 0, 0, 0);
    }
  }

  // the ring is dead: the exponents of the tile's 256 rows (threads 0-255, the gathered row's) and of its 256 columns
  // (threads 256-511; St holds powers of two, normal fp32; the LOCAL expert's scales) go behind the epilogue tiles
  __syncthreads();
  int* ex = reinterpret_cast<int*>(smem + EPB);
  if (tid < BM) ex[tid] = Ea[src_row(tid)];
  else ex[tid] = (int)((__float_as_uint(St[(int64_t)el * N + 32 * tile_of((tid - BM) >> 5) + r]) >> 23) & 0xffu) - 127;
  __syncthreads();
  if (2 * cg >= nbt) return;  // wave-uniform: the column group lies past N
  // acc[a][b][i] is row 128 rh + 32 a + 8 (i >> 2) + 4 h + (i & 3), column 64 cg + 32 b + r of the tile
  const int ew[2] = {ex[BM + 64 * cg + r], ex[BM + 64 * cg + 32 + r]};
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const i32x4 er = *reinterpret_cast<const i32x4*>(ex + 128 * rh + 32 * a + 8 * j + 4 * h);
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[a][b][4 * j + i] = __builtin_ldexpf(acc[a][b][4 * j + i], er[i] + ew[b]);
    }
  const int mw = 128 * rh, nw = cb * BN + 64 * cg;
  if constexpr (GLU) {
    // through the wave's own 8 KB LDS tile (tile_epilogue.h)
    tile_epilogue<EPI_GLU>(acc, smem + w * 8192, lane, mw, nw, ent0, rows, 0, N, 0, Y, ldy, nullptr);
  } else {
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
  }
}

// Expert MLP halves with per-row fp8 activations on the fp8 expert tiles (see grouped_tile_gemm_f8_kernel). Xq e4m3
// [rows, K] in fp8-tile K order with row stride ldxq % 16 == 0 and Ea int32 [rows]: token rows gathered through
// perm_tok with glu, one row per routed entry otherwise. glu: fused SwiGLU into Y bf16 [n_ent, N/2] (row stride
// ldy % 8 == 0); else the weighted combine into out f32 [T, N] (zeroed by the caller). hipErrorInvalidValue for a
// misaligned or short ldxq, null pointers, e_local > 16, N % 64 != 0, K % 256 != 0, with glu a null Y or ldy % 8 != 0,
// without it a null out; a no-op for n_ent < 1.
extern "C" hipError_t kafka_launch_grouped_tile_gemm_f8(const uint8_t* Xq, int64_t ldxq, const int* Ea, const void* Wt8,
                                                       const float* St, int e_local, int N, int K, const int* perm_tok,
                                                       const float* perm_w, const int* expert_off, int e_lo, int n_ent,
                                                       int glu, bf16* Y, int64_t ldy, float* out, int64_t ldo,
                                                       hipStream_t st) {
  using namespace gf8;
  if (N <= 0 || K <= 0 || N % 64 != 0 || K % 256 != 0 || ldxq % 16 != 0 || ldxq < K) return hipErrorInvalidValue;
  if (Xq == nullptr || Ea == nullptr || Wt8 == nullptr || St == nullptr || perm_tok == nullptr || perm_w == nullptr ||
      expert_off == nullptr || e_local > 16 || e_lo < 0)
    return hipErrorInvalidValue;
  if (glu ? (Y == nullptr || ldy % 8 != 0) : out == nullptr) return hipErrorInvalidValue;
  if (n_ent < 1 || e_local < 1) return hipSuccess;
  const int64_t rt_max = (int64_t)(n_ent + BM - 1) / BM + e_local;  // >= sum over the local experts of ceil(cnt_e / BM)
  if (rt_max * ((N + BN - 1) / BN) > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(rt_max * ((N + BN - 1) / BN)));
  const char* wt = static_cast<const char*>(Wt8);
  if (glu)
    grouped_tile_gemm_f8_kernel<true><<<grid, NW * 64, 0, st>>>(Xq, ldxq, Ea, wt, St, N, K, perm_tok, perm_w,
                                                               expert_off, e_lo, e_local, (int)rt_max, Y, ldy, out, ldo);
  else
    grouped_tile_gemm_f8_kernel<false><<<grid, NW * 64, 0, st>>>(Xq, ldxq, Ea, wt, St, N, K, perm_tok, perm_w,
                                                                expert_off, e_lo, e_local, (int)rt_max, Y, ldy, out,
                                                                ldo);
  return hipGetLastError();
}

}  // namespace kafka
