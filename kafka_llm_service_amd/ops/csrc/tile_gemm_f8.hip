// fp8 activations on the fp8 weight tiles (gfx950): Y[M, N] = (Xq[M, K] . Wq^T) * 2^ea[m] * sw[n] on the 32 x 32 x 64
// f8f6f4 MFMA with both operands e4m3 (cbsz 0, blgp 0): the W8A8 mode. Nothing is dequantised in VALU and there are no
// block scales: one power-of-two exponent per activation row, one power-of-two scale per weight row, both applied to
// the fp32 accumulators in the epilogue. The contract is tile_gemm_kernel<WF_FP8, EPI>'s (tile_gemm.hip): any M >= 1,
// N % 64 == 0, K % 256 == 0, the same split plan (kafka_tile_gemm_plan), grid order (row tile fastest), rows past M
// re-reading row M - 1, the N-tail rule, and the three epilogues (tile_epilogue.h: plain bf16 / fused silu(g) * u on GLU
// tiles / fp32 slabs [S, M, N]).
//
// MFMA form: __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4 with both scale operands the constant 0, which hipcc
// selects as the UNSCALED v_mfma_f32_32x32x64_f8f6f4 (no scale VGPRs, no extra VALU; checked in the ISA).
//
// Operands
//   Wt8 / St: the stored fp8 image of wstream_gemm.hip "WFMT" ([N/32][K/32][64][16] + fp32 row scales [N] in tile
//      order), unchanged: no second copy, no re-tiling at load.
//   Xq  e4m3 bytes [M, K] in FP8-TILE K ORDER (below), Ea int32 [M]: act_quant_fp8_kernel below.
//
// K order. Operand layout of the e4m3 x e4m3 form at 8 VGPRs, measured on the MI355X with one-hot bytes (B one-hot at
// every (lane, byte), A rows one-hot by the A layout that tile_gemm_mx.hip measured): B MIRRORS A. Lane (i, h = lane /
// 32) holds in bytes 0-15 the K values 16 h : +16 and in bytes 16-31 the K values 32 + 16 h : +16 of the k-step, for
// row i of A and for column i of B; all 2048 (lane, byte) positions of B were found once, none elsewhere.
//   There are no scales along K, so any permutation of a k-step's 64 K values is correct if A and B use the same one.
//   B is fixed by the stored tiles: lane (r, h) of tile kb2 holds the columns 32 kb2 + 8 h : +8 (bytes 0-7) and 32 kb2
//   + 16 + 8 h : +8 (bytes 8-15); the tiles 2 j, 2 j + 1 are bytes 0-15 and 16-31 of its fragment of k-step j. So byte
//   p of lane (., h) is column   64 j + 32 (p >> 4) + 16 ((p >> 3) & 1) + 8 h + (p & 7)   for both operands.
//   A is permuted instead of W, by the quantiser: in every 32-byte group of a row of Xq the two middle 8-byte runs
//   trade places (columns 0-7, 16-23, 8-15, 24-31; an involution, ops.fp8_act_order). Then the 16-B chunk 2 g + h of a
//   row is exactly what lane (., h) needs of the 32-column group g, and a lane's A fragment is two ds_read_b128: the
//   chunks h and 2 + h of its row of the stage.
//
// Split of work (what was built)
//   * workgroup = 8 waves, 256 x 256 tile, wave w = row half w & 1 (128 rows) x column group w >> 1 (64 columns): a
//     4 x 2 block of 32 x 32 x 64 MFMAs, 8 accumulators. Per k-step 8 A reads + 4 B reads (ds_read_b128) feed 8 MFMAs
//     that each do the work of four bf16 ones.
//   * ring of FIVE 64-deep stages of 32 KB (all 160 KB): Xq 16 KB (row m = 64 B, 16-B chunk c at slot c ^ ((m >> 2) &
//     3), permuted on the source side: the 16 rows a quarter-wave reads spread over all 64 banks), Wt8 16 KB (wave w
//     fetches the two 1 KB stored tiles 2 s, 2 s + 1 of column tile w). Everything goes by LDS-DMA, 2 + 2 loads per
//     wave and stage, one counted `s_waitcnt vmcnt` and one raw barrier per stage. Four stages (128 KB) are in flight
//     under a stage's MFMAs. Three 64 KB stages do not fit; two 128-deep stages would leave one stage (16 MFMAs per
//     wave) to cover a DMA round trip; five 64-deep ones cover it with four at twice the barriers. Neither
//     alternative was built or measured.
//   * no register load sits in the K loop (tile_gemm.hip's FP8 prologue has the reason): the row exponents Ea and the
//     column scales St are fetched once the ring is dead, by all 512 threads into 2 KB of LDS behind the epilogue
//     tiles, as integer exponents; the accumulators are scaled with v_ldexp_f32 (exact, and 2^ea * sw is never formed:
//     it could leave fp32's range where the product does not).
//   * LDS 160 KB, 1 workgroup per CU; VGPRs and the absence of scratch: profiles/act_fp8/resource_usage.txt.
// (The quantiser fused into RMSNorm: norm_act.hip rmsnorm_quant_kernel.) Not built: the quantiser in the attention epilogue; fp8 activations on the streaming or skinny
// GEMMs; the lm_head. (The grouped expert kernel for fp8 Mixtral is grouped_tile_gemm_f8.hip.)
#include "common.h"
#include "mx_quant.h"
#include "tile_epilogue.h"

namespace kafka {

namespace tf8 {
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
constexpr int EPB = NW * 8192;  // the epilogue tiles; the exponents of the block's rows and columns follow
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
}  // namespace tf8

// rts: row tiles of the grid (blockIdx.x = cb * rts + row tile); kper: K columns of one split (a multiple of 256)
template <int EPI>
__global__ __launch_bounds__(512, 1) void tile_gemm_f8_kernel(const uint8_t* __restrict__ Xq, int64_t ldxq,
                                                               const int* __restrict__ Ea,
                                                               const char* __restrict__ Wt,
                                                               const float* __restrict__ St, int M, int N, int K,
                                                               int kper, int rts, bf16* __restrict__ Y, int64_t ldy,
                                                               float* __restrict__ P) {
  using namespace tf8;
  constexpr int RB = BK, CPR = BK / 16;  // Xq row bytes / 16-B chunks of a stage
  static_assert(DX == 2 && DW == 2 && CPR == 4, "stage shape");
  static_assert(NS * STAGE <= 160 * 1024 && NS * STAGE >= EPB + 2048, "LDS of one gfx950 workgroup; epilogue area");
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
  const int nst = kper / BK;  // a multiple of 4

  // per-lane DMA sources of this wave's share of a stage (stage s adds s * BK K columns)
  // Xq: instruction j = DX w + u covers LDS bytes [1024 j, +1024) = 16 rows; lane -> (row, slot)
  const uint8_t* xsrc[DX];
#pragma unroll
  for (int u = 0; u < DX; ++u) {
    const int row = 16 * (DX * w + u) + lane / CPR, slot = lane % CPR;
    xsrc[u] = Xq + (int64_t)(row0 + min(row, rows - 1)) * ldxq + k0 + 16 * (slot ^ ((row >> 2) & 3));
  }
  // Wt8: wave w fetches column tile w of the block, the stored tiles kb2 = 2 s, 2 s + 1 of a stage
  const char* wsrc = Wt + ((int64_t)tile_of(w) * (K >> 5) + (k0 >> 5)) * 1024 + lane * 16;
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

  // the ring is dead: the exponents of the block's 256 rows (threads 0-255) and of its 256 columns (threads 256-511;
  // St holds powers of two, normal fp32) go behind the epilogue tiles
  __syncthreads();
  int* ex = reinterpret_cast<int*>(smem + EPB);
  if (tid < BM) ex[tid] = Ea[row0 + min(tid, rows - 1)];
  else ex[tid] = (int)((__float_as_uint(St[32 * tile_of((tid - BM) >> 5) + r]) >> 23) & 0xffu) - 127;
  __syncthreads();
  if (2 * cg >= nbt) return;  // wave-uniform: the column group lies past N
  // acc[a][b][i] is row 128 rh + 32 a + 8 (i >> 2) + 4 h + (i & 3), column 64 cg + 32 b + r of the block
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
  // epilogues (tile_epilogue.h): each wave through its own 8 KB LDS tile
  tile_epilogue<EPI>(acc, smem + w * 8192, lane, 128 * rh, cb * BN + 64 * cg, row0, rows, M, N, blockIdx.y, Y, ldy, P);
}

// Per-row fp8 quantiser: X bf16 [M, K] (K % 256 == 0) -> Xq e4m3 [M, K] in fp8-tile K order (file header), Ea int32
// [M]. The rule is ops.reference.fp8_quant's over a whole row: e = the frexp exponent of amax / 448 (amax / 2^e lies in
// [224, 448)), clamped to [-100, 100], 0 for an all-zero row; elements x * 2^-e saturated to +-448 and rounded to
// nearest-even by v_cvt_pk_fp8_f32 (rope_kv.hip's conversion).
// A row needs its whole-K amax before a byte is written, so a row is read ONCE and held in registers: TPR threads per
// row (one wave for K <= 1024, four rows per workgroup; else the workgroup's 256), thread t owning the units t, t + TPR,
// ... of the row, a unit being the 16-B output chunk 2 g + h = the input chunks 4 g + h and 4 g + 2 + h (two 16-B loads,
// one 16-B store: the permutation costs nothing). U units per thread cover K <= 4096 U; the amax is taken on the bf16
// bit patterns (e follows from the exponent field and whether the mantissa reaches 1.75 = 448 / 256, no division),
// over the wave with DPP shuffles and over the four waves through 16 B of LDS. HOLD = false (K > 32768) re-reads the
// row for the second pass instead of holding it.
template <int TPR, int U, bool HOLD>
__global__ __launch_bounds__(256) void act_quant_fp8_kernel(const bf16* __restrict__ X, int64_t ldx, int M, int K,
                                                            uint8_t* __restrict__ Xq, int* __restrict__ Ea) {
  constexpr int RPB = 256 / TPR;  // rows of a workgroup
  __shared__ uint32_t wam[4];
  const int t = threadIdx.x % TPR;
  const int64_t row = (int64_t)blockIdx.x * RPB + threadIdx.x / TPR;
  const bool live = row < M;  // wave-uniform
  const int units = K >> 4;
  const bf16* x = X + (live ? row : 0) * ldx;
  // the two 16-B input chunks of unit u: columns 32 g + 8 h : +8 and 32 g + 16 + 8 h : +8 (g = u / 2, h = u % 2)
  auto load = [&](int u, u32x4 (&v)[2]) {
    const bf16* p = x + 32 * (u >> 1) + 8 * (u & 1);
    v[0] = *reinterpret_cast<const u32x4*>(p);
    v[1] = *reinterpret_cast<const u32x4*>(p + 16);
  };
  u32x4 raw[U][2];
  uint32_t am = 0;  // the largest |x| as a bf16 bit pattern
  for (int base = 0; base < (HOLD ? 1 : units); base += TPR * U) {
#pragma unroll
    for (int i = 0; i < U; ++i) {
      const int u = base + t + i * TPR;
      raw[i][0] = raw[i][1] = u32x4{0, 0, 0, 0};
      if (live && u < units) load(u, raw[i]);
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) am = max(am, max(raw[i][c][j] & 0x7fffu, (raw[i][c][j] >> 16) & 0x7fffu));
    }
  }
#pragma unroll
  for (int d = 1; d < 64; d *= 2) am = max(am, (uint32_t)__shfl_xor((int)am, d, 64));
  if constexpr (TPR == 256) {
    if ((threadIdx.x & 63) == 0) wam[threadIdx.x >> 6] = am;
    __syncthreads();
    am = max(max(wam[0], wam[1]), max(wam[2], wam[3]));
  }
  const int e = fp8_row_exp(am);  // (mx_quant.h: the exponent rule and the element conversion, shared with RMSNorm)
  if (!live) return;
  const float inv = exp2i(-e);
  if (t == 0) Ea[row] = e;
  for (int base = 0; base < (HOLD ? 1 : units); base += TPR * U) {
#pragma unroll
    for (int i = 0; i < U; ++i) {
      const int u = base + t + i * TPR;
      if (u >= units) continue;
      if constexpr (!HOLD) load(u, raw[i]);
      uint32_t lo[2], hi[2];
      fp8_quant8(raw[i][0], inv, lo);
      fp8_quant8(raw[i][1], inv, hi);
      *reinterpret_cast<u32x4*>(Xq + row * K + 16 * u) = u32x4{lo[0], lo[1], hi[0], hi[1]};
    }
  }
}

// X bf16 [M, K] with row stride ldx (ldx % 8 == 0) -> Xq uint8 [M, K] (fp8-tile K order) and Ea int32 [M], both
// contiguous. hipErrorInvalidValue for M < 1, K % 256 != 0, a misaligned or short ldx and null pointers.
extern "C" hipError_t kafka_launch_act_quant_fp8(const bf16* X, int64_t ldx, int M, int K, uint8_t* Xq, int* Ea,
                                                hipStream_t st) {
  if (M < 1 || K <= 0 || K % 256 != 0 || ldx % 8 != 0 || ldx < K) return hipErrorInvalidValue;
  if (X == nullptr || Xq == nullptr || Ea == nullptr) return hipErrorInvalidValue;
  if (K <= 1024)
    act_quant_fp8_kernel<64, 1, true><<<(M + 3) / 4, 256, 0, st>>>(X, ldx, M, K, Xq, Ea);
  else if (K <= 4096)
    act_quant_fp8_kernel<256, 1, true><<<M, 256, 0, st>>>(X, ldx, M, K, Xq, Ea);
  else if (K <= 8192)
    act_quant_fp8_kernel<256, 2, true><<<M, 256, 0, st>>>(X, ldx, M, K, Xq, Ea);
  else if (K <= 16384)
    act_quant_fp8_kernel<256, 4, true><<<M, 256, 0, st>>>(X, ldx, M, K, Xq, Ea);
  else if (K <= 32768)
    act_quant_fp8_kernel<256, 8, true><<<M, 256, 0, st>>>(X, ldx, M, K, Xq, Ea);
  else
    act_quant_fp8_kernel<256, 8, false><<<M, 256, 0, st>>>(X, ldx, M, K, Xq, Ea);
  return hipGetLastError();
}

// Y = (Xq . Wq^T) * 2^Ea[m] * St[n] with fp8 activations (Xq e4m3 [M, K] in fp8-tile K order, row stride ldxq % 16 ==
// 0; Ea int32 [M]) on the fp8 tiles Wt8 / St (see tile_gemm_f8_kernel). Outputs, splits and glu as for
// kafka_launch_tile_gemm.
extern "C" hipError_t kafka_launch_tile_gemm_f8(const uint8_t* Xq, int64_t ldxq, const int* Ea, const void* Wt8,
                                               const float* St, int M, int N, int K, int splits, int glu, bf16* Y,
                                               int64_t ldy, float* P, hipStream_t st) {
  using namespace tf8;
  if (M < 1 || N <= 0 || K <= 0 || N % 64 != 0 || K % 256 != 0 || ldxq % 16 != 0 || ldxq < K)
    return hipErrorInvalidValue;
  if (splits < 1 || splits > 8 || K % (256 * splits) != 0 || (glu && splits > 1)) return hipErrorInvalidValue;
  if (Xq == nullptr || Ea == nullptr || Wt8 == nullptr || St == nullptr) return hipErrorInvalidValue;
  if (splits > 1 ? P == nullptr : (Y == nullptr || ldy % 8 != 0)) return hipErrorInvalidValue;
  const int rts = (M + BM - 1) / BM;
  if ((int64_t)rts * ((N + BN - 1) / BN) > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)rts * ((N + BN - 1) / BN), splits);
  const char* wt = static_cast<const char*>(Wt8);
  const int kper = K / splits;
  if (glu)
    tile_gemm_f8_kernel<EPI_GLU><<<grid, NW * 64, 0, st>>>(Xq, ldxq, Ea, wt, St, M, N, K, kper, rts, Y, ldy, P);
  else if (splits > 1)
    tile_gemm_f8_kernel<EPI_SLAB><<<grid, NW * 64, 0, st>>>(Xq, ldxq, Ea, wt, St, M, N, K, kper, rts, Y, ldy, P);
  else
    tile_gemm_f8_kernel<EPI_PLAIN><<<grid, NW * 64, 0, st>>>(Xq, ldxq, Ea, wt, St, M, N, K, kper, rts, Y, ldy, P);
  return hipGetLastError();
}

}  // namespace kafka
