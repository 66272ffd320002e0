// Skinny MFMA GEMM for mixed decode + prefill steps (129..256 rows) on the wave-tiled weights (gfx950).
//     Y[M, N] = X[M, K] . W[N, K]^T,   128 < M <= 256,  W in the wave-tiled layout of wstream_gemm.hip
//
// Between the weight-streaming decode GEMM (M <= 128: one MFMA B-fragment per 1 KB weight load, X from LDS) and
// hipBLASLt (large M) sit the steps that carry 64 decodes plus a new turn's prompt: 130-300 rows, where hipBLASLt
// runs at 1.3-2 TB/s (profiles/r02/gemm_sweep_M129_320.log) although the shape is still weight-bound: at 256 rows a
// workgroup that keeps every operand fragment busy on two MFMAs streams its weights at HBM rate.
//
//   * workgroup = 8 waves, tile 256 rows x 128 columns; wave w owns rows 64 (w & 3) .. + 64 and the column-tile
//     pair (cb * 4 + 2 (w >> 2), + 1): a 2 x 2 block of 32 x 32 MFMA tiles, so each A fragment (X) and each B
//     fragment (W) read from LDS feeds TWO v_mfma_f32_32x32x16_bf16 — the operand traffic per MFMA of the decode
//     kernel halved;
//   * both operands arrive by LDS-DMA (global_load_lds_dwordx4: no register round trip) into a 3-stage ring of
//     64-deep K stages (X 32 KB + W 16 KB per stage, 144 KB): per wave and stage 4 X + 2 W instructions, a counted
//     `s_waitcnt vmcnt` and one raw `s_barrier` per stage. W instructions are whole 1 KB B fragments (the tiled
//     layout is lane-linear already); X rows are 128 B with 16-B chunk c of row m at chunk c ^ (m & 7) — the DMA
//     writes lane-linear, so each lane LOADS the chunk that belongs at its LDS slot (source-side permutation) and the
//     A-fragment reads of 32 rows spread over the banks;
//   * split-K over gridDim.y for small N (fp32 slabs [S, M, N], summed by the consumer kernels like the decode
//     GEMM's); one split writes bf16, or with GLU-interleaved weights (tile 2j = gate, 2j + 1 = up: a wave's pair)
//     the activated silu(gate) * up [M, N / 2] straight from the accumulators.
// Rows >= M load row M - 1 (finite garbage, never stored).
//
// Quantised tiles (WF = WF_FP8 / WF_MXFP4, kafka_abi.h; layouts in wstream_gemm.hip "WFMT"): the same workgroup tile,
// 2 x 2 MFMA block, X path, 64-deep stages, ascending-K accumulation and epilogues; only the W half of a stage and
// the B-fragment reads differ. The RAW bytes go through the LDS-DMA ring and each wave dequantises its two tiles'
// fragments between the ds_read and the MFMAs (dq8 / dq4 of common.h: the exact bf16 values q * 2^e), so every
// accumulator sees the bf16 kernel's MFMA sequence on the dequantised weight and the outputs are bit-equal to it.
//   * fp8: a 64-deep stage of the 128 columns is 8 KB = 8 blocks of 1 KB, block (tile t, kb2) = the B fragments of
//     k-steps 2 kb2 and 2 kb2 + 1 of column tile t: ONE 16-B DMA instruction per wave (wave w: t = w / 2, kb2 = w % 2)
//     and one ds_read_b128 per tile and two k-steps. The fp32 row scale St[32 nb + r] of the lane's row is the
//     conversion's scale operand, loaded once per wave and tile next to stage 0 and waited for before the rest
//     of the prologue, so no compiler-placed vmcnt(0) for it lands inside the loop and drains the ring.
//   * mxfp4: a stage is 4 KB of W, one 1 KB block per column tile (dword kk of a lane's vector = k-step kk), and
//     64 B of e8m0 block exponents per tile (Se[nb][kb4][32][2 B]). Waves 0..3 own the W block of tile w (a 16-B DMA
//     instruction), waves 4..7 the exponents of tile w - 4 (a 4-B DMA instruction into a 256-B slot whose first 64 B
//     are the image: lane l reads dword l % 16) — the role is a wave-uniform branch (readfirstlane) that picks WHAT
//     the one extra instruction fetches, not whether there is one. So every wave issues exactly DX + 1 = 5 loads per
//     stage on every path, the counted `s_waitcnt vmcnt` immediate is the same constant for all eight waves, and
//     "stage s has landed" covers the scales of stage s (they are part of it). Chosen over sixteen 4-B weight
//     instructions per stage: those fetch 4 of every 16 bytes per instruction (four passes over each 1 KB run) to
//     save a ds_read_b128 that is conflict-free already. A lane's scale operand is uint32(e) << 23.
// A stage is 40 KB (fp8) / 37 KB (mxfp4); the ring is NS of them, and never less than the 128 KB of the slab
// epilogue's per-wave transposes. A split's first tile index is k0 / 32 (fp8) or k0 / 64 (mxfp4, scale image too).
// Measured (profiles/wq_skinny/): 4-19 % faster than the bf16 kernel on the dequantised tiles, 1.3-2.0x F.linear on
// the dequantised row-major copy for qkv / o / down, a tie on gate_up; 1.0-1.75 TB/s (fp8) and 0.54-1.0 TB/s (mxfp4) of
// quantised bytes, far from the streaming kernels' rates. Suspected, not isolated: at these shapes the kernel is not
// bound by the weight stream but by X, which every column block re-reads from L2 into LDS (N / 128 blocks x 256 rows
// x K = twice the bf16 weight's bytes), plus one barrier per 64-deep stage; halving or quartering W removes 1/6 and
// 1/4 of the LDS-DMA bytes only.
#include "common.h"

namespace kafka {

namespace skg {
constexpr int BM = 256, BN = 128;
constexpr int NW = 8;  // waves
// ring depth of the quantised instantiations. Both formats were built and timed at three and at four stages (these two
// constants were the only change; profiles/wq_skinny/ring_depth_{fp8,mxfp4}.jsonl, two rounds): fp8 at four stages (the
// whole 160 KB) -0.1 .. -0.5 us on qkv / down but +0.2 .. +0.5 us on o, inside the round-to-round spread: three stay;
// mxfp4 at four stages (148 KB) faster in 36 of 40 (projection, rows, round) cells, 1-2 %: four
constexpr int STAGES_FP8 = 3, STAGES_MXFP4 = 4;
template <int BK, int WF = WF_BF16>
struct Cfg {
  static constexpr bool WQ = WF != WF_BF16;
  static constexpr int XB = BM * BK * 2;     // X bytes per stage (32 KB at BK = 64)
  // W bytes per stage (at BK = 64: bf16 16 KB, fp8 8 KB, mxfp4 4 KB)
  static constexpr int WB = BN * BK * 2 / (WF == WF_MXFP4 ? 4 : (WF == WF_FP8 ? 2 : 1));
  static constexpr int SB = WF == WF_MXFP4 ? 1024 : 0;  // mxfp4: four 256-B block-exponent slots per stage
  static constexpr int STAGE = XB + WB + SB;
  static constexpr int DX = XB / 1024 / NW;  // X DMA instructions per wave per stage
  // W (mxfp4: W or scale) DMA instructions per wave per stage
  static constexpr int DW = WQ ? 1 : WB / 1024 / NW;
  static constexpr int DPS = DX + DW;
  static constexpr int RB = BK * 2;          // LDS bytes of one X row per stage
  static constexpr int CPR = BK / 8;         // 16-B chunks per X row per stage
};
// the scales travel as a trailing argument whose type depends on WF (an empty struct for bf16, whose argument block
// and register counts stay what they were: profiles/wq_skinny/resource_usage.txt); picked by specialisation, as
// wstream_gemm.hip's WfScales
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
}  // namespace skg

typedef __attribute__((address_space(3))) void skg_lds_t;

__device__ __forceinline__ void skg_dma16(const void* g, char* lds) {
  __builtin_amdgcn_global_load_lds(g, (skg_lds_t*)lds, 16, 0, 0);
}
__device__ __forceinline__ void skg_dma4(const void* g, char* lds) {
  __builtin_amdgcn_global_load_lds(g, (skg_lds_t*)lds, 4, 0, 0);
}

template <int N>
__device__ __forceinline__ void skg_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

template <int BK, int NS, int OCC, int WF = WF_BF16>
__global__ __launch_bounds__(512, OCC) void skinny_gemm_kernel(const bf16* __restrict__ X, int64_t ldx,
                                                               const bf16x8* __restrict__ Wt, int M, int N, int K,
                                                               int ks, bf16* __restrict__ Y, int64_t ldy,
                                                               float* __restrict__ P, int glu,
                                                               typename skg::Scale<WF>::type St) {
  using namespace skg;
  using C = Cfg<BK, WF>;
  constexpr int XB = C::XB, STAGE = C::STAGE, DX = C::DX, DW = C::DW, DPS = C::DPS, RB = C::RB, CPR = C::CPR;
  constexpr bool W8 = WF == WF_FP8, W4 = WF == WF_MXFP4, WQ = C::WQ;
  static_assert(DX >= 1 && DW >= 1 && (CPR == 8 || CPR == 4), "stage shape");
  static_assert(!WQ || BK == 64, "a quantised stage is eight (fp8) / four (mxfp4) 1 KB blocks: 64 K columns");
  // (quantised: the ring may be smaller than the slab epilogue's eight 16 KB transposes)
  constexpr int SMEM = WQ && NS * STAGE < NW * 64 * 64 * 4 ? NW * 64 * 64 * 4 : NS * STAGE;
  static_assert(SMEM <= 160 * 1024, "LDS of one gfx950 workgroup");
  __shared__ __attribute__((aligned(1024))) char smem[SMEM];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int rg = w & 3, cg = w >> 2;
  const int cb = blockIdx.x;
  const int k0 = blockIdx.y * ks;
  const int nst = ks / BK;
  const int K16 = K >> 4;

  // per-lane DMA sources of this wave's share of a stage (stage s adds s * BK to the K offset)
  // X: instruction j = DX w + u covers LDS bytes [1024 j, +1024) = 1024 / RB rows; lane -> row, slot (chunk c of row
  // m stored at slot c ^ (m % CPR))
  const bf16* xsrc[DX];
#pragma unroll
  for (int u = 0; u < DX; ++u) {
    const int j = DX * w + u, row = (1024 / RB) * j + lane / CPR, slot = lane % CPR;
    const int m = row < M ? row : M - 1;
    xsrc[u] = X + (int64_t)m * ldx + k0 + 8 * (slot ^ (row % CPR));
  }
  // W: instruction j = DW w + u = (tile t = j / KB, k-block kk = j % KB): one B fragment of column tile cb * 4 + t
  constexpr int KB = BK / 16;
  const bf16x8* wsrc[DW];
  // quantised: this wave's one extra instruction per stage. fp8: block (t = w / 2, kb2 = w % 2), 2 KB of a tile's run
  // per stage; mxfp4: waves 0..3 block t = w (1 KB per stage), waves 4..7 the 64 B of exponents of tile w - 4
  // (lanes >= 16 re-read them into the slot's unused 192 B). wq is w as a scalar: the role branch is wave-uniform
  const char* qsrc = nullptr;
  int wq = 0;
  if constexpr (W8) {
    qsrc = reinterpret_cast<const char*>(Wt) + ((int64_t)(cb * 4 + (w >> 1)) * (K >> 5) + (k0 >> 5) + (w & 1)) * 1024 +
           lane * 16;
  } else if constexpr (W4) {
    wq = __builtin_amdgcn_readfirstlane(w);
    const int64_t v = (int64_t)(cb * 4 + (wq & 3)) * (K >> 6) + (k0 >> 6);  // (tile, kb4) of stage 0
    qsrc = wq < 4 ? reinterpret_cast<const char*>(Wt) + v * 1024 + lane * 16 : St + v * 64 + (lane & 15) * 4;
  } else {
#pragma unroll
    for (int u = 0; u < DW; ++u) {
      const int j = DW * w + u, t = j / KB, kk = j % KB;
      wsrc[u] = Wt + ((int64_t)(cb * 4 + t) * K16 + (k0 >> 4) + kk) * 64 + lane;
    }
  }
  auto issue = [&](int s) {
    char* base = smem + (s % NS) * STAGE;
#pragma unroll
    for (int u = 0; u < DX; ++u) skg_dma16(xsrc[u] + s * BK, base + (DX * w + u) * 1024);
    if constexpr (W8) {
      skg_dma16(qsrc + (int64_t)s * 2048, base + XB + w * 1024);
    } else if constexpr (W4) {
      if (wq < 4)
        skg_dma16(qsrc + (int64_t)s * 1024, base + XB + wq * 1024);
      else
        skg_dma4(qsrc + (int64_t)s * 64, base + XB + C::WB + (wq - 4) * 256);
    } else {
#pragma unroll
      for (int u = 0; u < DW; ++u) skg_dma16(wsrc[u] + (int64_t)s * (BK / 16) * 64, base + XB + (DW * w + u) * 1024);
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
    if (NS > 5 && n >= 4) skg_vmcnt<(NS > 5 ? 4 : 0) * DPS>();
    else if (NS > 4 && n >= 3) skg_vmcnt<(NS > 4 ? 3 : 0) * DPS>();
    else if (NS > 3 && n >= 2) skg_vmcnt<(NS > 3 ? 2 : 0) * DPS>();
    else if (n >= 1) skg_vmcnt<DPS>();
    else skg_vmcnt<0>();
  };
  if constexpr (W8) {
    // the two tiles' row scales, consumed here, between stage 0's issue (nst >= 1) and the rest of the prologue: hipcc
    // waits for a register load next to LDS-DMA loads with vmcnt(0), and left to the first dq8 that wait would sit
    // inside the loop and drain the ring at every stage. Here it costs the later prologue stages one load latency, once
    wsc[0] = St[32 * (cb * 4 + 2 * cg) + r];
    wsc[1] = St[32 * (cb * 4 + 2 * cg + 1) + r];
    issue(0);
    asm volatile("" : "+v"(wsc[0]), "+v"(wsc[1]));
    for (int s = 1; s < NS - 1 && s < nst; ++s) issue(s);
  } else {
    for (int s = 0; s < NS - 1 && s < nst; ++s) issue(s);
  }
  for (int s = 0; s < nst; ++s) {
    // this wave's DMAs of stage s have landed (the NS - 2 later stages may still be in flight), then every wave's
    // have, and every wave is done reading slot (s + NS - 1) % NS (stage s - 1)
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
        if constexpr (W4) e2[b] = *reinterpret_cast<const uint16_t*>(ws + C::WB + (2 * cg + b) * 256 + 2 * r);
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

  // epilogue: C lane layout (lanes along N): acc[a][b][i] -> row 64 rg + 32 a + (i & 3) + 8 (i >> 2) + 4 h,
  // column (cb * 4 + 2 cg + b) * 32 + r
  const int nb0 = cb * 4 + 2 * cg;
  if (glu && P == nullptr) {  // (gate, up) = (tile nb0, tile nb0 + 1): output column block nb0 / 2
    const int n = (nb0 >> 1) * 32 + r;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int m = 64 * rg + 32 * a + (i & 3) + 8 * (i >> 2) + 4 * h;
        if (m < M) {
          const float g = acc[a][0][i], u = acc[a][1][i];
          Y[(int64_t)m * ldy + n] = (bf16)(g / (1.0f + __expf(-g)) * u);
        }
      }
    return;
  }
  if (P) {
    // split-K slab through a per-wave LDS transpose (the ring is dead once every wave is past its last stage): each
    // lane then writes 4 consecutive columns of a row with one 16-B sc1 store, 16 lanes per 256-B row (as the decode
    // GEMM's slabs)
    __syncthreads();  // (workgroup-uniform: P is a kernel argument)
    float* tp = reinterpret_cast<float*>(smem) + w * 64 * 64;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int i = 0; i < 16; ++i) tp[(32 * a + (i & 3) + 8 * (i >> 2) + 4 * h) * 64 + 32 * b + r] = acc[a][b][i];
    // (one wave's LDS accesses complete in order: the reads below see its writes)
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int q = j * 64 + lane, row = q >> 4, c4 = q & 15;
      const f32x4 v = *reinterpret_cast<const f32x4*>(tp + row * 64 + 4 * c4);
      const int m = 64 * rg + row;
      // GLU-interleaved pair: tile nb0 -> gate columns, nb0 + 1 -> up columns N/2 + ...
      const int n = glu ? ((c4 >> 3) ? (N >> 1) : 0) + (nb0 >> 1) * 32 + 4 * (c4 & 7) : nb0 * 32 + 4 * c4;
      if (m < M) store16_slab(P + ((int64_t)blockIdx.y * M + m) * N + n, v);
    }
    return;
  }
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int nb = nb0 + b;
    // GLU-interleaved tiles written un-split or as slabs: tile 2j -> gate columns [32 j, +32), 2j + 1 -> up N/2 + 32 j
    const int n = glu ? ((nb & 1) ? (N >> 1) : 0) + (nb >> 1) * 32 + r : nb * 32 + r;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int m = 64 * rg + 32 * a + (i & 3) + 8 * (i >> 2) + 4 * h;
        if (m < M) {
          if (P)
            P[((int64_t)blockIdx.y * M + m) * N + n] = acc[a][b][i];
          else
            Y[(int64_t)m * ldy + n] = (bf16)acc[a][b][i];
        }
      }
  }
}

// Split plan for a shape (mirrored by ops.skinny_plan): the fewest power-of-two splits that give >= 192 workgroups
// while every split keeps >= 4 K stages of 64.
extern "C" int kafka_skinny_plan(int M, int N, int K, int max_splits, int* splits) {
  using namespace skg;
  if (M <= 128 || M > BM || N % BN != 0 || K % 64 != 0) return 1;
  const int nx = N / BN;
  int s = 1;
  while (s * 2 <= max_splits && nx * s < 192 && K % (64 * s * 2) == 0 && K / (s * 2) >= 256) s *= 2;
  *splits = s;
  return 0;
}

// BK 64 x 3 stages (144 KB of LDS, one workgroup per CU; BK 32 x 6 stages and BK 32 x 3 stages at two workgroups
// per CU measured slower, profiles/r03/skinny_gemm/). Quantised tiles: skg::STAGES_FP8 / STAGES_MXFP4 stages.
template <int NS, int WF>
static hipError_t skinny_launch(const bf16* X, int64_t ldx, const void* Wt, typename skg::Scale<WF>::type sc, int M,
                                int N, int K, int splits, int glu, bf16* Y, int64_t ldy, float* P, hipStream_t st) {
  using namespace skg;
  skinny_gemm_kernel<64, NS, 1, WF><<<dim3(N / BN, splits), NW * 64, 0, st>>>(
      X, ldx, static_cast<const bf16x8*>(Wt), M, N, K, K / splits, Y, ldy, P, glu, sc);
  return hipGetLastError();
}

extern "C" hipError_t kafka_launch_skinny_gemm(const bf16* X, int64_t ldx, int wfmt, const void* Wt, const void* scale,
                                              int M, int N, int K, int splits, int glu, bf16* Y, int64_t ldy, float* P,
                                              hipStream_t st) {
  using namespace skg;
  if (M <= 0 || M > BM || N % BN != 0 || splits < 1 || K % (64 * splits) != 0 || ldx % 8 != 0) return hipErrorInvalidValue;
  if ((splits > 1) != (P != nullptr) || (splits == 1 && Y == nullptr) || (glu && N % 64 != 0))
    return hipErrorInvalidValue;
  if (Wt == nullptr || (wfmt == WF_BF16) != (scale == nullptr)) return hipErrorInvalidValue;
  switch (wfmt) {
    case WF_BF16: return skinny_launch<3, WF_BF16>(X, ldx, Wt, NoScale{}, M, N, K, splits, glu, Y, ldy, P, st);
    case WF_FP8:
      return skinny_launch<STAGES_FP8, WF_FP8>(X, ldx, Wt, static_cast<const float*>(scale), M, N, K, splits, glu, Y,
                                               ldy, P, st);
    case WF_MXFP4:
      return skinny_launch<STAGES_MXFP4, WF_MXFP4>(X, ldx, Wt, static_cast<const char*>(scale), M, N, K, splits, glu,
                                                   Y, ldy, P, st);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace kafka
