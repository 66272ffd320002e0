// Dense prefill GEMM over the wave-tiled weights (gfx950): Y[M, N] = X[M, K] . W^T for any M >= 1 (built for M > 256).
//     plain:  Y bf16 [M, N]                                          (one split)
//     GLU:    Y bf16 [M, N/2] = silu(gate) * up                      (one split, GLU-interleaved tiles)
//     slabs:  P fp32 [S, M, N], split s = the K range [s K/S, (s + 1) K/S)  (the slab contract of fused_add_rmsnorm /
//             rope_kv_write / silu_mul; ops.slab_reduce)
// X bf16 row-major (ldx % 8 == 0); W in any tile format of kafka_abi.h (WF_BF16 / WF_FP8 / WF_MXFP4; layouts in
// wstream_gemm.hip "WFMT") with the fp8 row scales St [N] or the MXFP4 e8m0 image Se [N/32][K/64][32][2].
// N % 64 == 0, K % 256 == 0 (ops.tile_gemm_supported): every projection of the Llama-3 configs at TP 1..8.
//
// Why not the grouped tile kernel with one expert: that kernel gathers rows, combines with atomics and has neither a
// plain store nor a split-K, and its 2 x 2 wave block has the two limiters recorded for this repository's 2 x 2
// kernels: one LDS fragment read per MFMA, and every row-group wave dequantising the same B fragments for itself (four
// times per fragment). Here:
//
//   * workgroup = 8 waves owns a 256-row x 256-column tile. Wave w has the row half w & 1 (128 rows) and the column
//     group w >> 1 (64 columns = the column tiles 2 cg, 2 cg + 1 of the block's eight): a 4 x 2 block of 32 x 32 x 16
//     bf16 MFMAs, 8 accumulators (128 registers). Per k-step 4 A reads + 2 B reads feed 8 MFMAs (0.75 LDS reads per
//     MFMA instead of 1), and each B fragment is dequantised by two waves instead of four;
//   * grid: blockIdx.x = column block * row tiles + ROW TILE (fastest), so the workgroups resident together are the row
//     tiles of a few column blocks and W, the large operand, is read from HBM once (grouped_tile_gemm.hip's header has
//     the reasoning); blockIdx.y = K split;
//   * both operands go by LDS-DMA (global_load_lds) into a ring of 64-deep K stages, one counted `s_waitcnt vmcnt` and
//     one raw `s_barrier` per stage. X stage 32 KB: the 16-B chunk c of row m sits at slot c ^ (m & 7), permuted on the
//     source side (the DMA writes lane-linear); no gather; rows past M re-read row M - 1 and are never stored.
//     W stage: wave w fetches column tile w of the block: bf16 32 KB (4 DMA instructions per wave), fp8 16 KB (2),
//     mxfp4 8 KB + eight 256-B exponent slots (one 16-B DMA for the tile's 1 KB block and one 4-B DMA for its 64 B of
//     exponents), so every wave issues DX + DW loads per stage on every path and the counted wait is one constant;
//   * ring depth within 160 KB: fp8 3 x 48 KB, mxfp4 3 x 42 KB, bf16 2 x 64 KB (the next stage's DMA runs under this
//     stage's MFMAs; four 32-deep stages were not built);
//   * N tail (N % 256 in {64, 128, 192}): waves whose column group lies past N re-read the block's first pair into
//     their slots (same load count) and store nothing;
//   * W travels as raw bytes; a wave dequantises its two B fragments per k-step between the ds_read and the MFMAs
//     (dq8 / dq4 of common.h: the exact bf16 values). Activations are not quantised, the MFMA stays bf16, K ascends
//     within a split: the fp8 / mxfp4 outputs are bit-equal to the bf16 instantiation on the dequantised tiles;
//   * epilogues go through an 8 KB LDS tile per wave (the ring is dead by then), 32 rows at a time, and leave as 16-B
//     ordinary vector stores: plain bf16 a whole 128-B line per row and wave, GLU 64 B, slabs 256 B.
// Registers and occupancy per instantiation: profiles/tile_prefill/resource_usage.txt.
#include "common.h"
#include "tile_epilogue.h"  // EPI_*, tile_epilogue, dma16 / dma4 (shared with tile_gemm_mx.hip)

namespace kafka {

namespace tlg {
constexpr int BM = 256, BN = 256, BK = 64;
constexpr int NW = 8;                // waves
constexpr int NT_B = BN / 32;        // column tiles of a block
template <int WF>
struct Cfg {
  static constexpr bool WQ = WF != WF_BF16;
  static constexpr int NS = WF == WF_BF16 ? 2 : 3;   // ring stages
  static constexpr int XB = BM * BK * 2;             // X bytes per stage (32 KB)
  static constexpr int WB = BN * BK * 2 / (WF == WF_MXFP4 ? 4 : (WF == WF_FP8 ? 2 : 1));  // 32 / 16 / 8 KB
  static constexpr int SB = WF == WF_MXFP4 ? NT_B * 256 : 0;  // mxfp4: eight 256-B block-exponent slots per stage
  static constexpr int STAGE = XB + WB + SB;
  static constexpr int DX = XB / 1024 / NW;                   // X DMA instructions per wave per stage
  static constexpr int DW = WF == WF_MXFP4 ? 2 : WB / 1024 / NW;  // W (mxfp4: block + exponents) instructions
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
  typedef const float* type;  // St [N], tile order
};
template <>
struct Scale<WF_MXFP4> {
  typedef const char* type;   // Se [N/32][K/64][32][2] e8m0 bytes
};

}  // namespace tlg

// rts: row tiles of the grid (blockIdx.x = cb * rts + row tile); kper: K columns of one split (a multiple of 256)
template <int WF, int EPI>
__global__ __launch_bounds__(512, 1) void tile_gemm_kernel(const bf16* __restrict__ X, int64_t ldx,
                                                            const char* __restrict__ Wt, int M, int N, int K, int kper,
                                                            int rts, bf16* __restrict__ Y, int64_t ldy,
                                                            float* __restrict__ P,
                                                            typename tlg::Scale<WF>::type St) {
  using namespace tlg;
  using C = Cfg<WF>;
  constexpr int NS = C::NS, XB = C::XB, WB = C::WB, STAGE = C::STAGE, DX = C::DX, DW = C::DW, DPS = C::DPS;
  constexpr bool W8 = WF == WF_FP8, W4 = WF == WF_MXFP4, WQ = C::WQ;
  constexpr int RB = BK * 2, CPR = BK / 8, KB = BK / 16;  // X row bytes / 16-B chunks / k-steps per stage
  static_assert(DX == 4 && DW >= 2 && CPR == 8 && NS >= 2 && NS <= 3, "stage shape");
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
  const int nst = kper / BK;

  // per-lane DMA sources of this wave's share of a stage (stage s adds s * BK K columns)
  // X: instruction j = DX w + u covers LDS bytes [1024 j, +1024) = 8 rows; lane -> (row, slot), chunk c of row m at
  // slot c ^ (m % 8)
  const bf16* xsrc[DX];
#pragma unroll
  for (int u = 0; u < DX; ++u) {
    const int row = 8 * (DX * w + u) + lane / CPR, slot = lane % CPR;
    xsrc[u] = X + (int64_t)(row0 + min(row, rows - 1)) * ldx + k0 + 8 * (slot ^ (row % CPR));
  }
  // W: wave w fetches column tile w of the block. bf16: instruction u = k-step u, one 1 KB B fragment; fp8: u = the
  // block of k-steps 2u, 2u + 1; mxfp4: the tile's one block (four k-steps), then its 64 B of exponents (lanes >= 16
  // re-read them into the slot's unused 192 B)
  const char* wsrc[DW];
  {
    const int64_t tw = tile_of(w);
    if constexpr (W4) {
      const int64_t v = tw * (K >> 6) + (k0 >> 6);
      wsrc[0] = Wt + v * 1024 + lane * 16;
      wsrc[1] = St + v * 64 + (lane & 15) * 4;
    } else {
#pragma unroll
      for (int u = 0; u < DW; ++u) wsrc[u] = Wt + tw * K * C::TKB + ((int64_t)k0 * C::TKB + u * 1024) + lane * 16;
    }
  }
  auto issue = [&](int s) {
    char* base = smem + (s % NS) * STAGE;
#pragma unroll
    for (int u = 0; u < DX; ++u) dma16(xsrc[u] + s * BK, base + (DX * w + u) * 1024);
    if constexpr (W4) {
      dma16(wsrc[0] + (int64_t)s * 1024, base + XB + w * 1024);
      dma4(wsrc[1] + (int64_t)s * 64, base + XB + WB + w * 256);
    } else {
#pragma unroll
      for (int u = 0; u < DW; ++u) dma16(wsrc[u] + (int64_t)s * DW * 1024, base + XB + (DW * w + u) * 1024);
    }
  };

  float wsc[2] = {1.f, 1.f};  // fp8: 2^e of this lane's row in the wave's two column tiles
  f32x16 acc[4][2];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;

  // s_waitcnt vmcnt(n * DPS) for a wave-uniform n in [0, NS - 2] (the count is an immediate)
  auto wait_stage = [&](int n) {
    if (NS > 2 && n >= 1) wait_vmcnt<(NS > 2 ? 1 : 0) * DPS>();
    else wait_vmcnt<0>();
  };
  if constexpr (W8) {
    // the row scales are consumed here, between stage 0's issue and the rest of the prologue: hipcc waits for a register
    // load next to LDS-DMA loads with vmcnt(0), which left to the first dq8 would sit in the loop and drain the ring
    wsc[0] = St[32 * tile_of(2 * cg) + r];
    wsc[1] = St[32 * tile_of(2 * cg + 1) + r];
    issue(0);
    asm volatile("" : "+v"(wsc[0]), "+v"(wsc[1]));
    for (int s = 1; s < NS - 1; ++s) issue(s);  // (nst >= 4: kper % 256 == 0)
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
      const bf16x8 b0 = wfrag(0, kk);
      const bf16x8 b1 = wfrag(1, kk);
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const int m = 128 * rh + 32 * a + r;
        const bf16x8 av = *reinterpret_cast<const bf16x8*>(xs + m * RB + 16 * (c ^ (m % CPR)));
        acc[a][0] = mfma32(av, b0, acc[a][0]);
        acc[a][1] = mfma32(av, b1, acc[a][1]);
      }
    }
  }

  // epilogues (tile_epilogue.h): each wave through its own 8 KB LDS tile once the ring is dead
  __syncthreads();
  if (2 * cg >= nbt) return;  // wave-uniform: the column group lies past N
  // the wave's first row of the tile / its first column of W
  tile_epilogue<EPI>(acc, smem + w * 8192, lane, 128 * rh, cb * BN + 64 * cg, row0, rows, M, N, blockIdx.y, Y, ldy, P);
}

// Split plan (mirrored by ops.tile_gemm_plan): S doubles (S <= 8 and <= max_splits, K / S a multiple of 256) while the
// doubled grid still fits one workgroup per CU (256). The weight format plays no part; a GLU call passes max_splits 1.
extern "C" int kafka_tile_gemm_plan(int M, int N, int K, int max_splits, int* splits) {
  using namespace tlg;
  if (M < 1 || N <= 0 || K <= 0 || N % 64 != 0 || K % 256 != 0) return 1;
  const int64_t wgs = (int64_t)((M + BM - 1) / BM) * ((N + BN - 1) / BN);
  int s = 1;
  while (s * 2 <= max_splits && s * 2 <= 8 && K % (256 * s * 2) == 0 && wgs * s * 2 <= 256) s *= 2;
  *splits = s;
  return 0;
}

template <int WF>
static hipError_t tile_gemm_launch(const bf16* X, int64_t ldx, const void* Wt, typename tlg::Scale<WF>::type sc, int M,
                                   int N, int K, int splits, int glu, bf16* Y, int64_t ldy, float* P, hipStream_t st) {
  using namespace tlg;
  const int rts = (M + BM - 1) / BM;
  const dim3 grid((unsigned)rts * ((N + BN - 1) / BN), splits);
  const char* wt = static_cast<const char*>(Wt);
  const int kper = K / splits;
  if (glu)
    tile_gemm_kernel<WF, EPI_GLU><<<grid, NW * 64, 0, st>>>(X, ldx, wt, M, N, K, kper, rts, Y, ldy, P, sc);
  else if (splits > 1)
    tile_gemm_kernel<WF, EPI_SLAB><<<grid, NW * 64, 0, st>>>(X, ldx, wt, M, N, K, kper, rts, Y, ldy, P, sc);
  else
    tile_gemm_kernel<WF, EPI_PLAIN><<<grid, NW * 64, 0, st>>>(X, ldx, wt, M, N, K, kper, rts, Y, ldy, P, sc);
  return hipGetLastError();
}

// Y = X . W^T on the dense wave tiles (see tile_gemm_kernel). splits == 1: Y bf16 [M, N] (glu: the activated [M, N/2]),
// row stride ldy % 8 == 0; splits > 1 (2, 4 or 8; not with glu): P fp32 [splits, M, N]. wfmt, Wt and scale as for
// kafka_launch_wstream_gemm.
extern "C" hipError_t kafka_launch_tile_gemm(const bf16* X, int64_t ldx, int wfmt, const void* Wt, const void* scale,
                                            int M, int N, int K, int splits, int glu, bf16* Y, int64_t ldy, float* P,
                                            hipStream_t st) {
  using namespace tlg;
  if (M < 1 || N <= 0 || K <= 0 || N % 64 != 0 || K % 256 != 0 || ldx % 8 != 0 || ldx < K) return hipErrorInvalidValue;
  if (splits < 1 || splits > 8 || K % (256 * splits) != 0 || (glu && splits > 1)) return hipErrorInvalidValue;
  if (X == nullptr || Wt == nullptr || (splits > 1 ? P == nullptr : (Y == nullptr || ldy % 8 != 0)))
    return hipErrorInvalidValue;
  if ((wfmt == WF_BF16) != (scale == nullptr)) return hipErrorInvalidValue;  // quantised tiles need their scales
  if ((int64_t)((M + BM - 1) / BM) * ((N + BN - 1) / BN) > 0x7fffffffLL) return hipErrorInvalidValue;
  switch (wfmt) {
    case WF_BF16: return tile_gemm_launch<WF_BF16>(X, ldx, Wt, NoScale{}, M, N, K, splits, glu, Y, ldy, P, st);
    case WF_FP8:
      return tile_gemm_launch<WF_FP8>(X, ldx, Wt, static_cast<const float*>(scale), M, N, K, splits, glu, Y, ldy, P,
                                      st);
    case WF_MXFP4:
      return tile_gemm_launch<WF_MXFP4>(X, ldx, Wt, static_cast<const char*>(scale), M, N, K, splits, glu, Y, ldy, P,
                                        st);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace kafka
