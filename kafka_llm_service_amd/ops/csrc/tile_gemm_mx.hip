// MXFP8 activations on the MXFP4 weight tiles (gfx950): Y[M, N] = Xq[M, K] . W^T on v_mfma_scale_f32_32x32x64_f8f6f4,
// A = e4m3 (cbsz 0), B = e2m1 (blgp 4), both block scales as the instruction's scale operands: nothing is dequantised
// in VALU. The contract is tile_gemm_kernel<WF_MXFP4, EPI>'s (tile_gemm.hip): any M >= 1, N % 64 == 0, K % 256 == 0, the
// same split plan (kafka_tile_gemm_plan), grid order (row tile fastest), rows past M re-reading row M - 1, the N-tail
// rule, and the three epilogues (tile_epilogue.h: plain bf16 / fused silu(g) * u on GLU tiles / fp32 slabs [S, M, N]).
//
// Operands
//   Xq  e4m3 bytes, row-major in natural K order (ldxq % 16 == 0), Xe e8m0 [M, K/32]: act_quant_mxfp8_kernel below.
//   Wt4 / Se: the stored MXFP4 image of wstream_gemm.hip "WFMT", unchanged: no second copy, no re-tiling at load.
//
// Operand layout of the 32 x 32 x 64 form, as measured on the MI355X with one-hot rows and per-block scales. The two
// operand widths differ. The scale of (row i, 32-column block kb of the k-step) is read from lane i + 32 kb.
//   B (e2m1, 4 VGPRs): lane (r, h = lane / 32) holds the 32 K values of block h, ascending through its 32 nibbles. In
//      Wt4 lane (r, h) holds the columns 16 j + 8 h : +8 in dword j, so block 0 of row r is dwords 0, 1 of the lanes
//      (r, 0), (r, 1) and block 1 their dwords 2, 3. Two v_permlane32_swap per fragment put them together: swap(d0, d2)
//      leaves lane (r, 0) with {d0 of (r, 0), d0 of (r, 1)} = columns 0-7, 8-15 and lane (r, 1) with {d2 of (r, 0), d2
//      of (r, 1)} = columns 32-39, 40-47; swap(d1, d3) the columns 16 further. Interleaved, both halves hold their block
//      in natural K order. The LDS image of W stays the stored one (one ds_read_b128 per fragment); the two swaps are
//      the VALU work per 4 MFMAs of 16 passes each.
//   A (e4m3, 8 VGPRs): lane (m, h) holds in VGPRs 0-3 the K values 16 h : +16 of block 0 and in VGPRs 4-7 the K values
//      32 + 16 h : +16 of block 1 (NOT 32 consecutive values: a lane has half of each block). It reads the 16-B chunks
//      4 kk + h and 4 kk + 2 + h of its row of the stage (two ds_read_b128).
//   scales: lane (., h) supplies block h of the k-step, for A and for B.
//
// Split of work (what was built)
//   * workgroup = 8 waves, 256 x 256 tile, wave w = row half w & 1 (128 rows) x column group w >> 1 (64 columns): a
//     4 x 2 block of 32 x 32 x 64 scaled MFMAs, 8 accumulators. Per 64-deep k-step 8 A reads + 2 B reads feed 8 MFMAs
//     that each do the work of four bf16 ones.
//   * ring of three 128-deep stages of 52 KB (156 KB of the 160): Xq 32 KB (row m = 128 B, 16-B chunk c at slot
//     c ^ (m & 7), permuted on the source side), Wt4 16 KB (wave w fetches the two 1 KB vectors of column tile w), and
//     two 2 KB scale areas of eight 256-B slots: Xe (wave w: the 4 exponent bytes of rows 32 w : +32, one dword per
//     row and stage) and Se (wave w: tile w's 2 x 64 B). Everything goes by LDS-DMA: 4 + 2 + 1 + 1 = 8 loads per wave
//     and stage on every wave (the upper half-wave of a scale load re-reads into the slot's spare 128 B), so there is
//     one counted `s_waitcnt vmcnt(8)` and one raw barrier per 128 K columns: half the barriers of the bf16 kernel.
//   * scales: a row's stage dword is [block (kk 0, h 0), (0, 1), (1, 0), (1, 1)]; shifted right by 8 h it carries the
//     lane's kk = 0 scale in byte 0 and kk = 1 in byte 2, selected with op_sel 0 / 2. B likewise from two 2-B reads per
//     tile. 4 + 4 LDS reads per wave and stage serve its 16 MFMAs; no register load sits in the loop (tile_gemm.hip's
//     FP8 prologue has the reason).
// Not built: a dword-granular DMA that would regroup the B blocks on the way in (64 DMA instructions per stage instead
// of 16); a four-stage ring of 64-deep stages (twice the barriers); 256-deep stages (two would not leave the next
// stage's DMA a free slot under 160 KB); the quantiser in the attention epilogue (RMSNorm and the GLU epilogue have
// it: norm_act.hip rmsnorm_quant_kernel, tile_epilogue.h EPI_GLU_MX). fp8 weight tiles (their K order
// per lane differs) have their own unit, tile_gemm_f8.hip, which permutes the activations instead. Registers, LDS and occupancy: profiles/act_mxfp8/resource_usage.txt.
#include <type_traits>

#include "common.h"
#include "mx_quant.h"
#include "tile_epilogue.h"

namespace kafka {

namespace tmx {
using namespace tlg;
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
}  // namespace tmx

// rts: row tiles of the grid (blockIdx.x = cb * rts + row tile); kper: K columns of one split (a multiple of 256)
template <int EPI>
__global__ __launch_bounds__(512, 1) void tile_gemm_mx_kernel(const uint8_t* __restrict__ Xq, int64_t ldxq,
                                                               const uint8_t* __restrict__ Xe,
                                                               const char* __restrict__ Wt,
                                                               const char* __restrict__ Se, int M, int N, int K,
                                                               int kper, int rts, bf16* __restrict__ Y, int64_t ldy,
                                                               float* __restrict__ P, uint8_t* __restrict__ Aq,
                                                               uint8_t* __restrict__ Ae) {
  using namespace tmx;
  constexpr int RB = BK, CPR = BK / 16, KB = BK / 64;  // Xq row bytes / 16-B chunks / k-steps per stage
  static_assert(DX == 4 && DW == 2 && CPR == 8 && KB == 2, "stage shape");
  static_assert(NS * STAGE <= 160 * 1024 && NS * STAGE >= NW * 8192, "LDS of one gfx950 workgroup; epilogue tiles");
  __shared__ __attribute__((aligned(1024))) char smem[NS * STAGE];

  const int cb = blockIdx.x / rts, rt = blockIdx.x - cb * rts;
  const int row0 = rt * BM;
  const int rows = min(BM, M - row0);  // >= 1
  const int k0 = blockIdx.y * kper;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int rh = w & 1, cg = w >> 1;
  const int NT = N >> 5;                      // column tiles of W (even)
  const int nbt = min(NT_B, NT - cb * NT_B);  // column tiles of this block: 2, 4, 6 or 8
  // column tile t of the block, or where it is past N a tile of the block's first pair (its loads land in t's slots,
  // unused)
  auto tile_of = [&](int t) { return cb * NT_B + (t < nbt ? t : (t & 1)); };
  const int nst = kper / BK;  // even, >= 2

  // per-lane DMA sources of this wave's share of a stage (stage s adds s * BK K columns)
  // Xq: instruction j = DX w + u covers LDS bytes [1024 j, +1024) = 8 rows; lane -> (row, slot)
  const uint8_t* xsrc[DX];
#pragma unroll
  for (int u = 0; u < DX; ++u) {
    const int row = 8 * (DX * w + u) + lane / CPR, slot = lane % CPR;
    xsrc[u] = Xq + (int64_t)(row0 + min(row, rows - 1)) * ldxq + k0 + 16 * (slot ^ (row % CPR));
  }
  // Xe: the stage's four exponents of row 32 w + r (both half-waves)
  const uint8_t* esrc = Xe + (int64_t)(row0 + min(32 * w + r, rows - 1)) * (K >> 5) + (k0 >> 5);
  // Wt4 / Se: wave w fetches column tile w of the block, the vectors kb4 = 2 s, 2 s + 1 of a stage
  const int64_t v0 = (int64_t)tile_of(w) * (K >> 6) + (k0 >> 6);
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

  // epilogues (tile_epilogue.h): each wave through its own 8 KB LDS tile once the ring is dead
  __syncthreads();
  if (2 * cg >= nbt) return;  // wave-uniform: the column group lies past N
  if constexpr (EPI == EPI_GLU_MX)  // silu(g) * u as MXFP8 rows Aq [M, N/2] / Ae [M, N/64]: the down projection's input
    tile_epilogue_glu_mx(acc, smem + w * 8192, lane, 128 * rh, cb * BN + 64 * cg, row0, rows, N >> 1, Aq, Ae);
  else
    tile_epilogue<EPI>(acc, smem + w * 8192, lane, 128 * rh, cb * BN + 64 * cg, row0, rows, M, N, blockIdx.y, Y, ldy, P);
}

// MXFP8 quantiser: X bf16 [M, K] (K % 256 == 0) -> Xq e4m3 [M, K] in natural order, Xe e8m0 [M, K/32]. The rule is
// ops.reference.mxfp8_quant's: per 32-column block e = the frexp exponent of amax / 448 (so amax / 2^e lies in
// [224, 448): never clipped), stored biased by 127 and clamped to [7, 247], 127 for an all-zero block; elements
// x / 2^e rounded to nearest-even by v_cvt_scalef32_pk_fp8_f32. One 16-B load per lane, the block's amax over its 4
// lanes (on the bf16 bit patterns: e follows from the exponent field and whether the mantissa reaches 1.75 = 448 / 256,
// no division), one 8-B store of elements per lane and one 8-B store of exponents per half-wave (256 columns).
__global__ __launch_bounds__(256) void act_quant_mxfp8_kernel(const bf16* __restrict__ X, int64_t ldx, int M, int K,
                                                              uint8_t* __restrict__ Xq, uint8_t* __restrict__ Xe) {
  const int cpr = K >> 3;  // 16-B chunks of a row: a multiple of 32, so a half-wave stays in one row
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = t < (int64_t)M * cpr;  // uniform per half-wave
  const int64_t row = live ? t / cpr : 0;
  const int c = live ? (int)(t - row * cpr) : 0;
  const int lane = threadIdx.x & 63;
  u32x4 raw = {0, 0, 0, 0};
  if (live) raw = *reinterpret_cast<const u32x4*>(X + row * ldx + 8 * c);
  uint32_t o[2];
  const int eb = mxfp8_quant_lane(raw, o);  // (mx_quant.h: the block's amax over its 4 lanes, exponent rule, e4m3 bytes)
  const uint2 ev = mxfp8_exps_halfwave(eb, lane);  // the 8 exponents of the half-wave's 256 columns
  if (live) {
    *reinterpret_cast<uint2*>(Xq + row * K + 8 * c) = make_uint2(o[0], o[1]);
    if ((lane & 31) == 0) *reinterpret_cast<uint2*>(Xe + row * (K >> 5) + (c >> 2)) = ev;
  }
}

// X bf16 [M, K] with row stride ldx (ldx % 8 == 0) -> Xq uint8 [M, K] and Xe uint8 [M, K/32], both contiguous.
// hipErrorInvalidValue for M < 1, K % 256 != 0, a misaligned or short ldx and null pointers.
extern "C" hipError_t kafka_launch_act_quant_mxfp8(const bf16* X, int64_t ldx, int M, int K, uint8_t* Xq, uint8_t* Xe,
                                                  hipStream_t st) {
  if (M < 1 || K <= 0 || K % 256 != 0 || ldx % 8 != 0 || ldx < K) return hipErrorInvalidValue;
  if (X == nullptr || Xq == nullptr || Xe == nullptr) return hipErrorInvalidValue;
  const int64_t blocks = ((int64_t)M * (K >> 3) + 255) / 256;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  act_quant_mxfp8_kernel<<<(unsigned)blocks, 256, 0, st>>>(X, ldx, M, K, Xq, Xe);
  return hipGetLastError();
}

// Y = Xq . W^T with MXFP8 activations (Xq e4m3 [M, K], row stride ldxq % 16 == 0; Xe e8m0 [M, K/32] contiguous) on the
// MXFP4 tiles Wt4 / Se (see tile_gemm_mx_kernel). Outputs, splits and glu as for kafka_launch_tile_gemm. With glu, Aq /
// Ae given instead of Y: the GLU output in MXFP8 form (Aq e4m3 [M, N/2], Ae e8m0 [M, N/64], contiguous), the bytes the
// quantiser above makes of the bf16 Y; exactly one of Y and the pair.
extern "C" hipError_t kafka_launch_tile_gemm_mx(const uint8_t* Xq, int64_t ldxq, const uint8_t* Xe, const void* Wt4,
                                               const void* Se, int M, int N, int K, int splits, int glu, bf16* Y,
                                               int64_t ldy, float* P, uint8_t* Aq, uint8_t* Ae, hipStream_t st) {
  using namespace tmx;
  if (M < 1 || N <= 0 || K <= 0 || N % 64 != 0 || K % 256 != 0 || ldxq % 16 != 0 || ldxq < K)
    return hipErrorInvalidValue;
  if (splits < 1 || splits > 8 || K % (256 * splits) != 0 || (glu && splits > 1)) return hipErrorInvalidValue;
  if (Xq == nullptr || Xe == nullptr || Wt4 == nullptr || Se == nullptr) return hipErrorInvalidValue;
  if ((Aq != nullptr) != (Ae != nullptr) || (Aq != nullptr && (!glu || Y != nullptr))) return hipErrorInvalidValue;
  if (Aq == nullptr && (splits > 1 ? P == nullptr : (Y == nullptr || ldy % 8 != 0))) return hipErrorInvalidValue;
  const int rts = (M + BM - 1) / BM;
  if ((int64_t)rts * ((N + BN - 1) / BN) > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)rts * ((N + BN - 1) / BN), splits);
  const char* wt = static_cast<const char*>(Wt4);
  const char* se = static_cast<const char*>(Se);
  const int kper = K / splits;
#define KAFKA_TGMX(EPI) \
  tile_gemm_mx_kernel<EPI><<<grid, NW * 64, 0, st>>>(Xq, ldxq, Xe, wt, se, M, N, K, kper, rts, Y, ldy, P, Aq, Ae)
  if (Aq != nullptr) KAFKA_TGMX(EPI_GLU_MX);
  else if (glu) KAFKA_TGMX(EPI_GLU);
  else if (splits > 1) KAFKA_TGMX(EPI_SLAB);
  else KAFKA_TGMX(EPI_PLAIN);
#undef KAFKA_TGMX
  return hipGetLastError();
}

}  // namespace kafka
