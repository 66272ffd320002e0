// Weight-streaming decode GEMM on pre-tiled weights (gfx950):   Y[M, N] = X[M, K] . W[N, K]^T,  M <= 128.
//
// At decode the weights are read exactly once per step and M (running sequences) is small, so this GEMM is an HBM
// stream of W with just enough MFMA work riding on it. Two layout decisions make the stream full-rate:
//
//   * W is stored "wave-tiled" (done once at load time, ops.tile_weight):  Wt[N/32][K/16][64 lanes][8] bf16 with
//     lane l = (r = l & 31, h = l >> 5) holding W[32 nb + r][16 kb + 8 h + j]. That is exactly the B fragment of
//     v_mfma_f32_32x32x16_bf16 for a 32-column tile, so every wave-instruction of the stream is ONE contiguous 1 KB
//     read (16 B per lane, non-temporal: each byte is used once), and one wave's whole K slice is a single
//     contiguous run. (A row-major [N, K] weight read as MFMA fragments touches 32 rows x 32 B per instruction.)
//   * X (the activations, <= 128 x K bf16, L2-resident) is staged per 128/256-deep K chunk into LDS with full-line
//     coalesced loads and read back as A fragments with ds_read_b128 from an XOR-swizzled image (chunk c of row m
//     at c ^ (m & 15): the 16 lanes of one LDS cycle hit 16 different bank groups). The 4 waves of a workgroup own 4
//     different 32-column tiles and share each X chunk, so X costs 1/4 of the W traffic on-chip and nothing in HBM.
//
// Work decomposition: workgroup = 4 waves = 128 output columns x one K split; grid (ceil(N / 128), S). S (1..8)
// is chosen on the host so the grid has >= 256 workgroups when N is small. S == 1 writes bf16 Y directly; S > 1
// writes fp32 partial slabs P[S][M][N] that the NEXT kernel sums while reading its input (rope_kv, fused
// add+RMSNorm, SwiGLU all accept slabs), so split-K costs no extra launch and no extra bf16 round trip.
// Pipelining: X chunk c+1 and the W fragments of chunk c+1 are issued before the MFMAs of chunk c; the LDS image of
// chunk c+1 is written after them (issue-early / write-late, one barrier per chunk).
// C = X . W^T comes out with lanes along N (col = lane & 31), so every epilogue store instruction writes two
// 128-B row segments.
#include "common.h"

#include <cstdlib>
#include <type_traits>

namespace kafka {

// ---- Fused decode-layer epilogues (FIN template argument) -------------------------------------------------------
// A pure decode layer used to be 9 launches: add+RMSNorm -> qkv -> RoPE/KV write -> cascade -> decode -> o ->
// add+RMSNorm -> gate_up -> down. With FIN the GEMMs absorb the three small kernels (VERDICT r05 "Next" #1):
//
//   * deferred RMSNorm: rmsnorm(h) . W^T = r (.) ((h (.) w) . W^T) with r[m] = rsqrt(mean_k h[m,k]^2 + eps). The
//     producer of h (the residual stream) writes X' = bf16(h (.) w) and, per 128-column block, the partial sums of
//     h^2 (ss [N/128][M]); the consumer GEMM streams X' as its A operand and applies r in its epilogue.
//   * split-K finisher: every split writes its fp32 tile as 16-B sc1 (write-through, agent-coherent) stores, waits
//     for them (vmcnt 0), takes a per-column-block ticket (relaxed agent-scope atomic), and the LAST split of the
//     column block sums the other S - 1 slabs with sc1 loads (compiler-tracked buffer loads, policy bit sc1) plus its
//     own tile from LDS, then runs the fused epilogue and re-arms the ticket. No fence: a release fence at agent scope
//     would write back this XCD's whole L2 from every workgroup (see attention.hip's ticket merge).
//       FIN_RES  (o, down):  h = resid + sum; resid <- bf16(h); xn <- bf16(h (.) nw); ss_out[cb][m] = sum_cols h^2
//       FIN_ROPE (qkv):      y = r (.) sum; rotate-half RoPE on q / k heads; q -> q_out, k / v -> the paged caches
//   * FIN_GLU (gate_up, one split): silu(r g) * (r u) in the SwiGLU epilogue; r from ss_in, whose loads are issued
//     at kernel start (their latency hides under the weight stream).
// One 128-column workgroup tile is exactly one head (D = 128), so the RoPE partner d +- 64 is in the same
// workgroup. Memory-model notes: common.h "Store / load scopes".
enum { FIN_NONE = 0, FIN_RES = 1, FIN_ROPE = 2, FIN_GLU = 3 };

// (FinArgs, the launchers' argument block for these epilogues: kafka_abi.h)

// split s's 16 B: from this XCD's L2 (the split stored it there: same XCD) or, flagged, agent-coherent (sc1)
template <bool MIXED>
__device__ __forceinline__ f32x4 load16_split(__amdgpu_buffer_rsrc_t rs, int byte_off, unsigned flags, int s) {
  if constexpr (MIXED) {
    if ((flags >> s) & 1u) return load16_sc1(rs, byte_off);
  }
  return load16_plain(rs, byte_off);
}

__device__ __forceinline__ int vt_pos16(int o) { return (o & ~15) | (o & 3) | ((o & 4) << 1) | ((o & 8) >> 1); }

// tp: this split's tile [4 column tiles][ROWS][32] fp32 in LDS; own column c of row m at tp[((c >> 5) * ROWS + m) * 32
// + (c & 31)]. P: slabs [S][Mtot][N]; the finisher is split `by`.
template <int S, int ROWS, int NTH, bool MIXED>
__device__ __forceinline__ void fin_res(const float* tp, const float* P, int by, int M, int Mtot, int N, int cb,
                                        const FinArgs& fa, int tid, unsigned flags) {
  constexpr int O = S - 1;                                  // the other splits' slabs
  constexpr int UB = O == 0 ? 8 : (28 / O >= 8 ? 8 : (28 / O < 1 ? 1 : 28 / O));  // <= 28 loads in flight
  const auto rs = buf_rsrc(P);
  const int c0 = cb * 128, nunits = M * 32;                 // unit = (row, 4 columns); a row = 32 consecutive lanes
  for (int q0 = tid; q0 < nunits; q0 += NTH * UB) {
    f32x4 pv[UB][O > 0 ? O : 1];
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const int q = min(q0 + u * NTH, nunits - 1);
      const int row = q >> 5, g = q & 31;
#pragma unroll
      for (int j = 0; j < O; ++j) {
        const int s = j < by ? j : j + 1;
        pv[u][j] = load16_split<MIXED>(rs, (int)((((int64_t)s * Mtot + row) * N + c0 + 4 * g) * 4), flags, s);
      }
    }
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const int q = q0 + u * NTH;
      const bool valid = q < nunits;  // whole 32-lane rows are valid or not (nunits = 32 M)
      const int row = min(q, nunits - 1) >> 5, g = q & 31;
      f32x4 v = *reinterpret_cast<const f32x4*>(tp + ((g >> 3) * ROWS + row) * 32 + 4 * (g & 7));
#pragma unroll
      for (int j = 0; j < O; ++j) v += pv[u][j];
      const int64_t col = c0 + 4 * g;
      const bf16x4 rb = *reinterpret_cast<const bf16x4*>(fa.resid + row * fa.ldr + col);
      const bf16x4 wb = *reinterpret_cast<const bf16x4*>(fa.nw + col);
      bf16x4 hs, xo;
      float ss = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        hs[j] = (bf16)(v[j] + (float)rb[j]);  // the residual stream is bf16 (as fused_add_rmsnorm)
        const float hf = (float)hs[j];
        ss += hf * hf;
        xo[j] = (bf16)(hf * (float)wb[j]);
      }
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
      if (valid) {
        *reinterpret_cast<bf16x4*>(fa.resid + row * fa.ldr + col) = hs;
        *reinterpret_cast<bf16x4*>(fa.xn + row * fa.ldxn + col) = xo;
        if (g == 0) fa.ss_out[(int64_t)cb * fa.ss_out_ld + row] = ss;
      }
    }
  }
}

template <int S, int ROWS, int NTH, bool MIXED>
__device__ __forceinline__ void fin_rope(const float* tp, const float* P, int by, int M, int Mtot, int N, int cb,
                                         const FinArgs& fa, int tid, const float* s_r, const int* s_pos,
                                         const int64_t* s_slot, unsigned flags) {
  constexpr int O = S - 1;
  const auto rs = buf_rsrc(P);
  const int head = cb, c0 = cb * 128;
  const bool is_q = head < fa.Hq, is_k = !is_q && head < fa.Hq + fa.Hkv;  // workgroup-uniform
  if (is_q || is_k) {
    // unit = (row, g < 16): columns 4g..4g+3 and their rotate-half partners 64 + 4g..
    constexpr int UB = O == 0 ? 4 : (14 / O >= 4 ? 4 : (14 / O < 1 ? 1 : 14 / O));
    const int nunits = M * 16;
    for (int q0 = tid; q0 < nunits; q0 += NTH * UB) {
      f32x4 pa[UB][O > 0 ? O : 1], pb[UB][O > 0 ? O : 1];
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const int q = min(q0 + u * NTH, nunits - 1);
        const int row = q >> 4, g = q & 15;
#pragma unroll
        for (int j = 0; j < O; ++j) {
          const int s = j < by ? j : j + 1;
          const int64_t base = ((int64_t)s * Mtot + row) * N + c0 + 4 * g;
          pa[u][j] = load16_split<MIXED>(rs, (int)(base * 4), flags, s);
          pb[u][j] = load16_split<MIXED>(rs, (int)((base + 64) * 4), flags, s);
        }
      }
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const int q = q0 + u * NTH;
        if (q >= nunits) continue;
        const int row = q >> 4, g = q & 15;
        f32x4 x1 = *reinterpret_cast<const f32x4*>(tp + ((g >> 3) * ROWS + row) * 32 + 4 * (g & 7));
        f32x4 x2 = *reinterpret_cast<const f32x4*>(tp + ((2 + (g >> 3)) * ROWS + row) * 32 + 4 * (g & 7));
#pragma unroll
        for (int j = 0; j < O; ++j) {
          x1 += pa[u][j];
          x2 += pb[u][j];
        }
        const float rr = s_r[row];
        const float* cs = fa.cos_sin + (int64_t)s_pos[row] * 128;
        const f32x4 cv = *reinterpret_cast<const f32x4*>(cs + 4 * g);
        const f32x4 sv = *reinterpret_cast<const f32x4*>(cs + 64 + 4 * g);
        bf16x4 o1, o2;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float a = x1[j] * rr, b = x2[j] * rr;
          o1[j] = (bf16)(a * cv[j] - b * sv[j]);
          o2[j] = (bf16)(b * cv[j] + a * sv[j]);
        }
        if (is_q) {
          bf16* dst = fa.q_out + row * fa.q_stride + head * 128 + 4 * g;
          *reinterpret_cast<bf16x4*>(dst) = o1;
          *reinterpret_cast<bf16x4*>(dst + 64) = o2;
        } else {
          const int64_t slot = s_slot[row];
          if (slot >= 0) {
            // element (key o, d) of a page at ((d >> 3) * 16 + o) * 8 + (d & 7): d = 4g..4g+3 is one 8-B run
            bf16* dst = fa.k_cache + ((slot >> 4) * fa.Hkv + (head - fa.Hq)) * 2048 + (slot & 15) * 8 +
                        (g >> 1) * 128 + 4 * (g & 1);
            *reinterpret_cast<bf16x4*>(dst) = o1;
            *reinterpret_cast<bf16x4*>(dst + 8 * 128) = o2;  // d + 64: 8 chunk planes further
          }
        }
      }
    }
  } else {
    // V head: unit = (row, g < 32), columns 4g..4g+3, scaled and transposed into the V^T page
    constexpr int UB = O == 0 ? 8 : (28 / O >= 8 ? 8 : (28 / O < 1 ? 1 : 28 / O));
    const int nunits = M * 32, vh = head - fa.Hq - fa.Hkv;
    for (int q0 = tid; q0 < nunits; q0 += NTH * UB) {
      f32x4 pv[UB][O > 0 ? O : 1];
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const int q = min(q0 + u * NTH, nunits - 1);
        const int row = q >> 5, g = q & 31;
#pragma unroll
        for (int j = 0; j < O; ++j) {
          const int s = j < by ? j : j + 1;
          pv[u][j] = load16_split<MIXED>(rs, (int)((((int64_t)s * Mtot + row) * N + c0 + 4 * g) * 4), flags, s);
        }
      }
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const int q = q0 + u * NTH;
        if (q >= nunits) continue;
        const int row = q >> 5, g = q & 31;
        const int64_t slot = s_slot[row];
        if (slot < 0) continue;
        f32x4 v = *reinterpret_cast<const f32x4*>(tp + ((g >> 3) * ROWS + row) * 32 + 4 * (g & 7));
#pragma unroll
        for (int j = 0; j < O; ++j) v += pv[u][j];
        const float rr = s_r[row];
        bf16* dst = fa.v_cache + ((slot >> 4) * fa.Hkv + vh) * 2048 + vt_pos16((int)(slot & 15)) + (4 * g) * 16;
#pragma unroll
        for (int j = 0; j < 4; ++j) dst[j * 16] = (bf16)(v[j] * rr);
      }
    }
  }
}

// wide (per call): which outputs may leave as 16-B sc1 stores — WIDE_P: the split-K slabs P (both launchers' slabs
// are contiguous fp32, so kafka_launch_wstream_gemm always sets it; the FIN_RES / FIN_ROPE finishers store their
// slabs themselves and never consult it), WIDE_Y: the un-split bf16 outputs (Y's rows 16-B aligned). Without the
// bit an output is written one element per accumulator. (No launcher reaches the per-element P stores today; the arm
// stays because dropping it changes register allocation — MT = 3 FIN_GLU gains 4 VGPR spills — which wants its own
// measurement.)
enum { WIDE_P = 1, WIDE_Y = 2 };
// WFMT (kafka_abi.h WF_*): the format of the weight tiles. Every format is a stream of 16-B vectors per lane, a
// wave-instruction one contiguous 1 KB run; a vector carries the B fragments of wf_ksteps(WFMT) k-steps, and the
// quantised formats are dequantised to the exact bf16 values right before their MFMAs, so MFMA, accumulators and
// epilogues are the bf16 kernel's. The quantised formats are FIN_NONE and NT only.
//
// WF_FP8 (ops.tile_weight_fp8): Wt is the e4m3 image Wt8[N/32][K/32][64 lanes][16 B] — bytes 0..7 of lane
// (r, h) of tile (nb, kb2) = W[32 nb + r][32 kb2 + 8 h : +8] (k-step 2 kb2), bytes 8..15 the same 8 columns 16 further
// (k-step 2 kb2 + 1) — so one 16-B load per lane carries the B fragments of TWO k-steps: half the loads, half the
// prefetch registers, half the bytes. St[32 nb + r] is the power-of-two scale of the lane's row; it is the scale
// operand of v_cvt_scalef32_pk_bf16_fp8 (dq8), so the B fragments are the exact bf16 values e4m3 * 2^e.
//
// WF_MXFP4 (ops.tile_weight_mxfp4): Wt is the e2m1 image Wt4[N/32][K/64][64 lanes][16 B] — bytes 4j..4j+3
// (dword j = 0..3) of lane (r, h) of tile (nb, kb4) = the eight nibbles W[32 nb + r][64 kb4 + 16 j + 8 h : +8], low
// nibble first (k-step 4 kb4 + j) — so one 16-B load per lane carries the B fragments of FOUR k-steps: a quarter of
// the loads, prefetch registers and bytes. The block scales are the e8m0 image Se[N/32][K/64][32 rows][2 B]: the two
// bytes of (nb, kb4, r) are the exponents of columns 64 kb4 : +32 (dwords 0, 1) and 64 kb4 + 32 : +32 (dwords 2, 3) of
// that row. The image does not depend on the plan (MT, KC, KW only decide how many (nb, kb4) groups a wave walks per
// chunk); a lane fetches one 2-B load per weight vector, and a wave's load is one contiguous 64-B run (both h halves
// read the same bytes). The scale loads are issued with the weights, ahead of them and under the same PIN fence, stay
// raw until their vector is dequantised, and become fp32 with a shift (uint32(e) << 23: e is clamped to [7, 247] by
// the quantiser). dq4 (v_cvt_scalef32_pk_bf16_fp4) makes the exact bf16 values e2m1 * 2^e.
//
// The argument list does not depend on WFMT: the scales (St / Se) travel in fa.wscale, the union partner of fa.ss_in
// (the quantised formats are FIN_NONE, where no epilogue reads ss_in), so the kernel's argument block — and with it
// every bf16 instantiation's register counts and occupancy — is byte for byte what it was before the quantised formats
// (profiles/wfmt/resource_usage.txt).
constexpr int wf_ksteps(int wfmt) { return wfmt == WF_MXFP4 ? 4 : (wfmt == WF_FP8 ? 2 : 1); }  // k-steps per 16-B vector
constexpr int wf_vshift(int wfmt) { return wfmt == WF_MXFP4 ? 6 : (wfmt == WF_FP8 ? 5 : 4); }  // log2 of its K columns
template <int WFMT>
using wf_vec = typename std::conditional<WFMT == WF_BF16, bf16x8, u32x4>::type;

template <int MT, int KC, bool NT, int KW, bool PIN, int FIN = FIN_NONE, int WFMT = WF_BF16>
__global__ __launch_bounds__(256 * KW) void wstream_gemm_kernel(const bf16* __restrict__ X, int64_t ldx,
                                                                 const bf16x8* __restrict__ Wt, int M, int N, int K,
                                                                 int ks, bf16* __restrict__ Y, int64_t ldy,
                                                                 float* __restrict__ P, int glu, int row_tiles,
                                                                 int wide, FinArgs fa) {
  constexpr int NTH = 256 * KW;
  constexpr int ROWS = 32 * MT;
  constexpr int CPR = KC / 8;             // 16-B chunks per X row of one K chunk
  constexpr int XL = ROWS * CPR / NTH;    // X chunks staged per thread
  constexpr int KSTEP = KC / 16;          // MFMA k-steps per K chunk
  constexpr int KSW = KSTEP / KW;         // k-steps of one wave (KW waves split each chunk along K)
  constexpr bool W8 = WFMT == WF_FP8, W4 = WFMT == WF_MXFP4;
  constexpr int KSV = KSW / wf_ksteps(WFMT);  // 16-B weight vectors of one wave per chunk
  constexpr int VSH = wf_vshift(WFMT);
  constexpr int NSC = W4 ? KSV : 1;           // mxfp4: raw block-scale pairs prefetched per chunk (one per vector)
  typedef wf_vec<WFMT> wvec;
  static_assert(CPR >= 16 && XL >= 1 && KSW >= 1, "chunk too small");
  static_assert(WFMT == WF_BF16 || (KSW % wf_ksteps(WFMT) == 0 && FIN == FIN_NONE && NT),
                "quantised tiles hold whole vectors of k-steps; plain epilogues and non-temporal loads only");
  static_assert(2 * ROWS * KC * 2 >= 4 * (KW - 1) * MT * 16 * 64 * 4, "LDS too small for the K-half reduction");
  __shared__ __attribute__((aligned(16))) bf16 xs[2][ROWS * KC];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ct = w & 3, kh = w >> 2;  // column tile of the workgroup, K part of the chunk
  const int r = lane & 31, h = lane >> 5;
  // row tiles (M > 32 MT): the row_tiles workgroups of one weight slice are placed on ONE XCD — workgroups b, b + 8,
  // ... under round-robin placement (blockIdx.x % 8 picks the XCD) — so the slice streams from HBM once and the other
  // row tiles read it from that XCD's L2 (the launch pads the column blocks to a multiple of 8; padding workgroups
  // exit); P stays [S][M_total][N]
  int cb = blockIdx.x, rti = 0;
  if (row_tiles > 1) {
    const int grp = blockIdx.x / (8 * row_tiles), rem = blockIdx.x % (8 * row_tiles);
    cb = grp * 8 + rem % 8;
    rti = rem / 8;
    if (cb >= (N + 127) / 128) return;  // padding workgroup (workgroup-uniform)
  }
  const int row0 = rti * ROWS;
  const int Mtot = M;
  M = min(ROWS, Mtot - row0);
  X += (int64_t)row0 * ldx;
  if (Y != nullptr) Y += (int64_t)row0 * ldy;
  if (P != nullptr) P += (int64_t)row0 * N;
  const int nb = cb * 4 + ct;
  // wave-uniform: a tail wave past the last column tile streams a valid tile and skips only its stores — every
  // load and MFMA stays unconditional, so hipcc's waitcnt pass sees straight-line code and keeps counted vmcnt
  // waits (a divergent `if` around the loads collapses them to vmcnt(0..1) at the join)
  const bool active = nb < (N >> 5);
  const int k0 = blockIdx.y * ks;
  const int nchunks = ks / KC;
  const int nbl = active ? nb : (N >> 5) - 1;
  // (every layout: K / 16 bf16, K / 32 fp8 or K / 64 mxfp4 vectors of 64 lanes x 16 B per tile row, KSV per wave and
  // chunk)
  const int64_t v0 = (int64_t)nbl * (K >> VSH) + (k0 >> VSH) + kh * KSV;  // this wave's first vector
  const wvec* wp = reinterpret_cast<const wvec*>(Wt) + v0 * 64 + lane;
  float wsc = 1.f;  // fp8: 2^e of this lane's weight row
  if constexpr (W8) wsc = static_cast<const float*>(fa.wscale)[32 * nbl + r];
  // mxfp4: the lane's row in the block-scale image, 32 rows x 2 B per vector (same tile and vector index as wp: in range
  // wherever the weight load is)
  const uint16_t* sp = nullptr;
  if constexpr (W4) sp = static_cast<const uint16_t*>(fa.wscale) + v0 * 32 + r;

  // phase stamps (FinArgs::stamps, benchmarks only): 0 start, 1 main loop done, 2 slab stores drained, 3 ticket
  // taken (finisher), 4 finisher done
  auto stamp = [&](int k) {
    if constexpr (FIN != FIN_NONE)
      if (fa.stamps != nullptr && tid == 0)
        fa.stamps[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 8 + k] = __builtin_amdgcn_s_memrealtime();
  };
  stamp(0);
  // FIN_GLU: this thread's share of the row-scale partials ss_in[j][row], issued before the stream (host-checked:
  // tpr = a power of two >= nss / SSL threads per row, M * tpr <= NTH)
  constexpr int SSL = FIN == FIN_GLU ? 4096 / NTH : 1;
  float ssv[SSL];
  int tpr = 1;
  if constexpr (FIN == FIN_GLU) {
    while (tpr * SSL < fa.nss) tpr <<= 1;
    const int row = tid / tpr, j0 = (tid % tpr) * SSL;
#pragma unroll
    for (int i = 0; i < SSL; ++i)
      ssv[i] = (fa.ss_in != nullptr && row < M && j0 + i < fa.nss) ? fa.ss_in[(int64_t)(j0 + i) * fa.ss_ld + row] : 0.f;
  }

  bf16x8 xr[XL];
  auto load_x = [&](int ch) {
#pragma unroll
    for (int i = 0; i < XL; ++i) {
      const int idx = tid + NTH * i;
      const int row = idx / CPR, c = idx % CPR;
      const int m = row < M ? row : M - 1;  // rows >= M compute garbage that is never stored
      xr[i] = load_bf16x8(X + (int64_t)m * ldx + k0 + ch * KC + c * 8);
    }
  };
  auto store_x = [&](int buf) {
#pragma unroll
    for (int i = 0; i < XL; ++i) {
      const int idx = tid + NTH * i;
      const int row = idx / CPR, c = idx % CPR;
      *reinterpret_cast<bf16x8*>(&xs[buf][row * KC + 8 * (c ^ (row & 15))]) = xr[i];
    }
  };
  auto load_w = [&](wvec(&wv)[KSV], uint16_t(&sv)[NSC], int ch) {
    if constexpr (W4) {
      // the block scales first: loads return in order, so the first dequantisation waits for them and vector 0 only
#pragma unroll
      for (int t = 0; t < KSV; ++t)
        sv[t] = __builtin_nontemporal_load(sp + (int64_t)(ch * (KSV * KW) + t) * 32);
    }
#pragma unroll
    for (int t = 0; t < KSV; ++t) {
      const wvec* p = wp + (int64_t)(ch * (KSV * KW) + t) * 64;
      wv[t] = NT ? __builtin_nontemporal_load(p) : *p;
    }
    // PIN keeps the prefetch where it is issued: left alone, the machine scheduler sinks these loads (and the X
    // loads before them) below the MFMAs of the current chunk (shorter register live ranges), which leaves the next
    // chunk a prefetch distance of ~0, so every chunk waits out the full HBM latency
    if constexpr (PIN) __builtin_amdgcn_sched_barrier(0);
  };
  f32x16 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[mt][i] = 0.f;
  auto compute = [&](int buf, const wvec(&wv)[KSV], const uint16_t(&sv)[NSC]) {
#pragma unroll
    for (int t = 0; t < KSW; ++t) {
      bf16x8 wf;
      if constexpr (W4) {
        // dequantised right before its MFMAs: the prefetch registers keep the raw nibbles and exponent bytes; dword
        // t & 3 of vector t >> 2 is this k-step, its block exponent byte (t & 3) >> 1 of the vector's pair
        const u32x4 v = wv[t >> 2];
        const uint32_t e2 = sv[t >> 2];
        const uint32_t eb = (t & 2) ? e2 >> 8 : e2 & 0xffu;
        wf = dq4(v[t & 3], __builtin_bit_cast(float, eb << 23));
      } else if constexpr (W8) {
        // dequantised right before its MFMAs: the prefetch registers keep the raw fp8
        const u32x4 v = wv[t >> 1];
        wf = (t & 1) ? dq8(v[2], v[3], wsc) : dq8(v[0], v[1], wsc);
      } else {
        wf = wv[t];
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int m = mt * 32 + r, c = 2 * (kh * KSW + t) + h;
        const bf16x8 xf = *reinterpret_cast<const bf16x8*>(&xs[buf][m * KC + 8 * (c ^ (m & 15))]);
        acc[mt] = mfma32(xf, wf, acc[mt]);
      }
    }
  };

  wvec wa[KSV], wb[KSV];
  uint16_t sa[NSC], sb[NSC];  // (mxfp4 only: dead otherwise)
  // X first: its LDS image is written while the first weight chunk is still in flight (loads return in order)
  load_x(0);
  load_w(wa, sa, 0);
  store_x(0);
  __syncthreads();
  int ch = 0;
  // steady state: two chunks per trip, both prefetches in range (no conditional loads inside the trip); chunk ch is
  // in buffer 0 / wa
  for (; ch + 2 < nchunks; ch += 2) {
    load_x(ch + 1);
    load_w(wb, sb, ch + 1);
    compute(0, wa, sa);
    store_x(1);
    __syncthreads();
    load_x(ch + 2);
    load_w(wa, sa, ch + 2);
    compute(1, wb, sb);
    store_x(0);
    __syncthreads();
  }
  // tail: one or two chunks left (chunk ch is in buffer 0 / wa)
  if (ch + 1 < nchunks) {
    load_x(ch + 1);
    load_w(wb, sb, ch + 1);
    compute(0, wa, sa);
    store_x(1);
    __syncthreads();
    compute(1, wb, sb);
  } else {
    compute(0, wa, sa);
  }

  if constexpr (KW > 1) {
    // the KW waves of a column tile hold partial sums over different k-steps: fold them through LDS (the X stage
    // is dead now), every wave reaches both barriers
    float* red = reinterpret_cast<float*>(&xs[0][0]);
    __syncthreads();
    if (kh > 0) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) red[((((kh - 1) * 4 + ct) * MT + mt) * 16 + i) * 64 + lane] = acc[mt][i];
    }
    __syncthreads();
    if (kh == 0) {
#pragma unroll
      for (int j = 1; j < KW; ++j)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int i = 0; i < 16; ++i) acc[mt][i] += red[((((j - 1) * 4 + ct) * MT + mt) * 16 + i) * 64 + lane];
    }
  }
  if constexpr (FIN == FIN_RES || FIN == FIN_ROPE) {
    __shared__ int s_last;
    __shared__ float s_r[FIN == FIN_ROPE ? ROWS : 1];
    __shared__ int s_pos[FIN == FIN_ROPE ? ROWS : 1];
    __shared__ int64_t s_slot[FIN == FIN_ROPE ? ROWS : 1];
    const int S = gridDim.y, by = blockIdx.y;
    float* tp = reinterpret_cast<float*>(&xs[0][0]);  // [4][ROWS][32] fp32: this split's tile (the X stage is dead)
    // Home XCD: workgroups are dealt to the 8 XCDs round-robin (linear id % 8), so with N / 128 a multiple of 8 every
    // split of column block cb runs on XCD cb % 8 and the finisher is one of them: the slabs can go through that XCD's
    // L2 (plain stores, L2-hit loads) instead of the agent-coherent level. Each split CHECKS it (hardware XCC_ID);
    // one that is not home stores sc1 and flags its bit in the ticket (bits 8 + s), so the finisher loads that slab
    // sc1. A finisher that is itself not home cannot reach the home L2 of the others: it sets fa.err.
    const int lin = blockIdx.y * gridDim.x + blockIdx.x;
    const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 0xfu;  // hwreg(HW_REG_XCC_ID, 0, 4)
    const bool home = (gridDim.x & 7) == 0 && (int)xcc == (lin & 7);
    __shared__ unsigned s_flags;
    stamp(1);
    // FIN_ROPE: every split loads the per-row partials / position / slot (the finisher is not known yet) into
    // registers before its slab stores and parks them in LDS after issuing them, so the load round trip overlaps the
    // store drain. Thread (row = tid % ROWS, part = tid / ROWS) sums partials part, part + PARTS, ... (nss <= 32,
    // host-checked); the PARTS sums of a row are added in a fixed order (deterministic).
    constexpr int PARTS = NTH / ROWS >= 8 ? 8 : (NTH / ROWS >= 4 ? 4 : (NTH / ROWS >= 2 ? 2 : 1));
    constexpr int JL = FIN == FIN_ROPE ? 32 / PARTS : 1;
    __shared__ float s_ssp[FIN == FIN_ROPE ? PARTS : 1][FIN == FIN_ROPE ? ROWS : 1];
    const int prow = tid % ROWS, ppart = tid / ROWS;
    const bool pact = FIN == FIN_ROPE && ppart < PARTS && prow < M;
    float ssv2[JL];
    int posv = 0;
    int64_t slotv = -1;
    if constexpr (FIN == FIN_ROPE) {
      if (pact) {
#pragma unroll
        for (int u = 0; u < JL; ++u) {
          const int j = ppart + PARTS * u;
          ssv2[u] = (fa.ss_in != nullptr && j < fa.nss) ? fa.ss_in[(int64_t)j * fa.ss_ld + prow] : 0.f;
        }
        if (ppart == 0) {
          posv = (int)fa.positions[prow];
          slotv = fa.slots != nullptr ? fa.slots[prow] : -1;
        }
      }
    }
    __syncthreads();  // (the K-part fold's LDS reads are done)
    if (kh == 0) {
      float* tw = tp + ct * (ROWS * 32);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) tw[(mt * 32 + (i & 3) + 8 * (i >> 2) + 4 * h) * 32 + r] = acc[mt][i];
      if (S > 1) {
        // (one wave's LDS accesses complete in order: the reads below see its writes)
#pragma unroll
        for (int j = 0; j < ROWS / 8; ++j) {
          const int q = j * 64 + lane, row = q >> 3, c4 = q & 7;
          const f32x4 v = *reinterpret_cast<const f32x4*>(tw + row * 32 + 4 * c4);
          if (row < M) {
            float* dst = P + ((int64_t)by * Mtot + row) * N + cb * 128 + ct * 32 + 4 * c4;
            if (home)
              *reinterpret_cast<f32x4*>(dst) = v;  // into this XCD's L2, where the finisher will read it
            else
              store16_slab(dst, v);
          }
        }
      }
    }
    if constexpr (FIN == FIN_ROPE) {
      if (pact) {
        float sacc = 0.f;
#pragma unroll
        for (int u = 0; u < JL; ++u) sacc += ssv2[u];
        s_ssp[ppart][prow] = sacc;
        if (ppart == 0) {
          s_pos[prow] = posv;
          s_slot[prow] = slotv;
        }
      }
      __syncthreads();
      if (tid < M) {
        float sacc = 0.f;
#pragma unroll
        for (int p = 0; p < PARTS; ++p) sacc += s_ssp[p][tid];
        s_r[tid] = fa.ss_in != nullptr ? rsqrtf(sacc * fa.inv_d + fa.eps) : 1.f;
      }
    }
    if (S > 1) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this split's slab has reached the coherent level
      stamp(2);
      __syncthreads();
      if (tid == 0) {
        int* tk = fa.tickets + cb;
        const int add = 1 + (home ? 0 : (256 << by));
        const int t = __hip_atomic_fetch_add(tk, add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int tot = t + add;
        s_last = (tot & 255) == S;
        s_flags = (unsigned)(tot >> 8) & 255u;
        if ((tot & 255) == S) {
          __hip_atomic_store(tk, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm
          const unsigned others = ((1u << S) - 1u) & ~(1u << by);
          if (!home && (s_flags & others) != others && fa.err != nullptr) atomicOr(fa.err, 1);
        }
      }
      __syncthreads();
      if (!s_last) return;  // workgroup-uniform
      stamp(3);
    } else {
      if (tid == 0) s_flags = 0;
      __syncthreads();
    }
    const unsigned flags = s_flags;
#define KAFKA_FIN_S(S_)                                                                                     \
  case S_:                                                                                                  \
    if constexpr (FIN == FIN_RES) {                                                                         \
      if (flags == 0)                                                                                       \
        fin_res<S_, ROWS, NTH, false>(tp, P, by, M, Mtot, N, cb, fa, tid, 0u);                              \
      else                                                                                                  \
        fin_res<S_, ROWS, NTH, true>(tp, P, by, M, Mtot, N, cb, fa, tid, flags);                            \
    } else {                                                                                                \
      if (flags == 0)                                                                                       \
        fin_rope<S_, ROWS, NTH, false>(tp, P, by, M, Mtot, N, cb, fa, tid, s_r, s_pos, s_slot, 0u);         \
      else                                                                                                  \
        fin_rope<S_, ROWS, NTH, true>(tp, P, by, M, Mtot, N, cb, fa, tid, s_r, s_pos, s_slot, flags);       \
    }                                                                                                       \
    break;
    switch (S) {
      KAFKA_FIN_S(1)
      KAFKA_FIN_S(2)
      KAFKA_FIN_S(4)
      KAFKA_FIN_S(8)
      default: break;  // (host-checked: S in {1, 2, 4, 8})
    }
#undef KAFKA_FIN_S
    if (fa.stamps != nullptr) {
      __syncthreads();
      stamp(4);
    }
    return;
  }
  if (glu && P == nullptr) {
    // fused SwiGLU epilogue (weight tiles GLU-interleaved: tile 2j = gate rows [32j, 32j+32), tile 2j+1 = the
    // matching up rows): odd waves hand their up tile to the even wave of the pair through LDS, which writes
    // silu(gate) * up straight from the fp32 accumulators into Y [M, N/2]
    float* red = reinterpret_cast<float*>(&xs[0][0]);
    // FIN_GLU: deferred RMSNorm of X, r[row] from the partials loaded at kernel start (1 without ss_in)
    __shared__ float s_rg[FIN == FIN_GLU ? ROWS : 1];
    if constexpr (FIN == FIN_GLU) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < SSL; ++i) s += ssv[i];
      for (int o = tpr >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      const int row = tid / tpr;
      if (tid % tpr == 0 && row < ROWS) s_rg[row] = fa.ss_in != nullptr ? rsqrtf(s * fa.inv_d + fa.eps) : 1.f;
    }
    auto rrow = [&](int m) { return FIN == FIN_GLU ? s_rg[m < ROWS ? m : ROWS - 1] : 1.f; };
    __syncthreads();
    if (kh == 0 && (ct & 1)) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) red[(((ct >> 1) * MT + mt) * 16 + i) * 64 + lane] = acc[mt][i];
    }
    __syncthreads();
    if (wide & WIDE_Y) {
      // the workgroup's 64 output columns (128 B per row) through an LDS tile, then 16-B sc1 stores: 8 lanes per row
      bf16* ty = reinterpret_cast<bf16*>(red + 2 * MT * 16 * 64);  // [ROWS][64], after the up-tile exchange
      if (active && kh == 0 && !(ct & 1)) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int m = mt * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
            const float rr = rrow(m);
            const float g = acc[mt][i] * rr, u = red[(((ct >> 1) * MT + mt) * 16 + i) * 64 + lane] * rr;
            ty[m * 64 + (ct >> 1) * 32 + r] = (bf16)(g / (1.0f + __expf(-g)) * u);
          }
      }
      __syncthreads();
      const int c0 = cb * 64, W2 = N >> 1;
      for (int q = tid; q < ROWS * 8; q += NTH) {
        const int row = q >> 3, c = q & 7;
        if (row < M && c0 + 8 * c < W2)
          store16_slab(reinterpret_cast<float*>(Y + (int64_t)row * ldy + c0 + 8 * c),
                       *reinterpret_cast<const f32x4*>(ty + row * 64 + 8 * c));
      }
    } else if (active && kh == 0 && !(ct & 1)) {
      const int n = (nb >> 1) * 32 + r;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int m = mt * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
          if (m < M) {
            const float rr = rrow(m);
            const float g = acc[mt][i] * rr, u = red[(((ct >> 1) * MT + mt) * 16 + i) * 64 + lane] * rr;
            Y[(int64_t)m * ldy + n] = (bf16)(g / (1.0f + __expf(-g)) * u);
          }
        }
    }
  } else if (P == nullptr && !glu && (wide & WIDE_Y)) {
    // un-split bf16 output (the lm_head): the workgroup's 128 columns (256 B per row) through an LDS tile, then
    // 16-B sc1 stores, 8 lanes per 128-B line
    bf16* ty = reinterpret_cast<bf16*>(&xs[0][0]);  // [ROWS][128]
    __syncthreads();  // (workgroup-uniform: P, glu and wide are kernel arguments)
    if (active && kh == 0) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) ty[(mt * 32 + (i & 3) + 8 * (i >> 2) + 4 * h) * 128 + ct * 32 + r] = (bf16)acc[mt][i];
    }
    __syncthreads();
    const int c0 = cb * 128;
    for (int q = tid; q < ROWS * 16; q += NTH) {
      const int row = q >> 4, c = q & 15;
      if (row < M && c0 + 8 * c < N)
        store16_slab(reinterpret_cast<float*>(Y + (int64_t)row * ldy + c0 + 8 * c),
                     *reinterpret_cast<const f32x4*>(ty + row * 128 + 8 * c));
    }
  } else if (P != nullptr && (wide & WIDE_P)) {
    // split-K slab through a per-wave LDS transpose (the X stage is dead): each lane then holds 4 consecutive columns
    // of a row and writes them with one 16-B sc1 store (the line leaves this XCD's L2 — the consumer kernel runs on
    // every XCD — and the launch ends with fewer dirty lines to write back)
    float* tp = reinterpret_cast<float*>(&xs[0][0]) + ct * (ROWS * 32);
    __syncthreads();  // (workgroup-uniform: P and wide are kernel arguments)
    if (active && kh == 0) {
      const int cbase = glu ? ((nb & 1) ? (N >> 1) : 0) + (nb >> 1) * 32 : nb * 32;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) tp[(mt * 32 + (i & 3) + 8 * (i >> 2) + 4 * h) * 32 + r] = acc[mt][i];
      // (one wave's LDS accesses complete in order: the reads below see its writes)
#pragma unroll
      for (int j = 0; j < ROWS / 8; ++j) {
        const int q = j * 64 + lane, row = q >> 3, c4 = q & 7;
        const f32x4 v = *reinterpret_cast<const f32x4*>(tp + row * 32 + 4 * c4);
        if (row < M) {
          store16_slab(P + ((int64_t)blockIdx.y * Mtot + row) * N + cbase + 4 * c4, v);
        }
      }
    }
  } else if (active && kh == 0) {
    // GLU-interleaved tiles written un-split: tile 2j -> gate columns [32j, +32), tile 2j+1 -> up columns N/2 + 32j
    const int n = glu ? ((nb & 1) ? (N >> 1) : 0) + (nb >> 1) * 32 + r : nb * 32 + r;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int m = mt * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
        if (m < M) {
          if (P)
            P[((int64_t)blockIdx.y * Mtot + m) * N + n] = acc[mt][i];
          else
            Y[(int64_t)m * ldy + n] = (bf16)acc[mt][i];
        }
      }
  }
}

// Grouped (MoE) variant: one weight stream per expert over wave-tiled expert weights Wt[E_local][N/32][K/16][64][8].
// Grid (ceil(N / 128), E_local, row tiles of 32 * MT); expert e's rows are the routing segment
// [expert_off[e], expert_off[e + 1]) read on the device (no host sync after the router); workgroups past the end
// of their expert's segment exit at once, and row tiles past it skip their MFMAs (wave-uniform).
//   GATHER: A row = X[perm_tok[entry]] (token activations), else X[entry] (expert-sorted intermediate).
//   Epilogue GLU (GLU-interleaved tiles): Y[entry, :N/2] = silu(gate) * up, bf16 — the SwiGLU of the expert MLP.
//   Epilogue COMBINE: out_f32[perm_tok[entry], n] += perm_w[entry] * y (a token gets exactly k contributions).
// (MT = 4: at most 256 registers so two workgroups share a CU — left free the compiler took 316, one wave per SIMD:
// the 128-row expert tiles streamed 8 % slower, Mixtral 128 threads 5,155 vs 5,234 tok/s, profiles/r06/mixtral/;
// MT = 2 spills 32+ registers under the same bound and keeps its 324)
//
// WFMT = WF_FP8 (fp8 expert weights, ops.tile_experts_fp8): Wt is the e4m3 image Wt8[E_local][N/32][K/32][64][16 B] of
// the dense kernel's WF_FP8 per expert and St[E_local][N] the power-of-two row scales in tile order, both indexed by
// the LOCAL expert (expert_off by e_lo + el). A wave loads KSTEP / 2 vectors per chunk, keeps raw fp8 in wa / wb and
// dequantises each vector right before its two k-steps' MFMAs (dq8, the row scale being the conversion's scale
// operand), so the accumulators hold true values and the X stage, the MT = 4 rule and both epilogues are the bf16
// kernel's. St is a trailing argument whose type depends on WFMT — an empty struct for bf16, which never reads it: the
// 24 bf16 instantiations compile to the register counts they had before fp8 (profiles/wfp8_moe/resource_usage.txt,
// profiles/wfmt/resource_usage.txt).
//
// WFMT = WF_MXFP4 (MXFP4 expert weights, ops.tile_experts_mxfp4): Wt is the e2m1 image Wt4[E_local][N/32][K/64][64][16 B]
// of the dense kernel's WF_MXFP4 per expert (GLU-interleaved for w13) and Se[E_local][N/32][K/64][32 rows][2 B] the dense
// e8m0 block-scale image per expert, both indexed by the LOCAL expert like the fp8 pair. A wave loads KSTEP / 4 vectors
// per chunk (4 at KC = 256, 2 at KC = 128) and with each one its raw 2-B scale pair (byte 0: dwords 0, 1; byte 1: dwords
// 2, 3), issued ahead of the weight vectors under the same PIN fence; nibbles and exponent bytes stay raw in wa / wb and
// sa / sb and each k-step's dword is dequantised right before its MFMAs (dq4 with uint32(e) << 23 as its scale
// operand), exactly as the dense W4 path. The B fragments are the exact bf16 values e2m1 * 2^e, so every accumulator
// sees the MFMA sequence of the bf16 kernel on the dequantised experts (the GLU half is bit-equal to it). The scale
// address is in range wherever the weight address is (same tile and vector index), inactive tail waves included, so
// every load stays unconditional. MT = 4 fits its 256-register bound without scratch (the raw prefetch is 2 x 2
// vectors, a quarter of bf16's), so it keeps the shared occupancy bound (profiles/wfp4_moe/resource_usage.txt).
// (The type is picked by a specialisation, not by std::conditional<WFMT == WF_FP8, ...>: that expression would be part
// of the kernel's mangled name, with the unnamed enum's compiler-made name in it, which the host and the device pass
// number differently — the host stub then registers a symbol the code object does not have.)
struct NoScales {};
template <int WFMT>
struct WfScales {
  typedef NoScales type;
};
template <>
struct WfScales<WF_FP8> {
  typedef const float* type;
};
template <>
struct WfScales<WF_MXFP4> {
  typedef const uint16_t* type;  // raw e8m0 pairs
};
template <int MT, int KC, bool GATHER, bool COMBINE, bool PIN, int WFMT = WF_BF16>
__global__ __launch_bounds__(256, MT == 4 ? 2 : 1) void wstream_grouped_kernel(const bf16* __restrict__ X, int64_t ldx,
                                                               const bf16x8* __restrict__ Wt, int N, int K,
                                                               const int* __restrict__ perm_tok,
                                                               const float* __restrict__ perm_w,
                                                               const int* __restrict__ expert_off, int e_lo,
                                                               bf16* __restrict__ Y, int64_t ldy,
                                                               float* __restrict__ out, int64_t ldo,
                                                               typename WfScales<WFMT>::type St) {
  constexpr int ROWS = 32 * MT;
  constexpr int CPR = KC / 8;
  constexpr int XL = ROWS * CPR / 256;
  constexpr int KSTEP = KC / 16;
  constexpr bool W8 = WFMT == WF_FP8, W4 = WFMT == WF_MXFP4;
  constexpr int KSV = KSTEP / wf_ksteps(WFMT);  // 16-B weight vectors per chunk
  constexpr int NSC = W4 ? KSV : 1;             // mxfp4: raw block-scale pairs prefetched per chunk (one per vector)
  typedef wf_vec<WFMT> wvec;
  static_assert(CPR >= 16 && XL >= 1, "chunk too small");
  static_assert(KSTEP % wf_ksteps(WFMT) == 0, "quantised tiles hold whole vectors of k-steps");
  __shared__ __attribute__((aligned(16))) bf16 xs[2][ROWS * KC];
  const int el = blockIdx.y, e = e_lo + el;
  const int seg0 = expert_off[e];
  const int cnt = expert_off[e + 1] - seg0;
  const int row0 = blockIdx.z * ROWS;
  if (row0 >= cnt) return;  // workgroup-uniform
  const int rows = min(ROWS, cnt - row0);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int nb = blockIdx.x * 4 + w;
  const bool active = nb < (N >> 5);
  // (an inactive tail wave streams the last tile, and reads its scales; every layout: K / 16 bf16, K / 32 fp8 or
  // K / 64 mxfp4 vectors of 64 lanes x 16 B per tile row)
  const int nbl = active ? nb : (N >> 5) - 1;
  const int64_t v0 = ((int64_t)el * (N >> 5) + nbl) * (K >> wf_vshift(WFMT));  // this wave's first vector
  const wvec* wp = reinterpret_cast<const wvec*>(Wt) + v0 * 64 + lane;
  float wsc = 1.f;  // fp8: 2^e of this lane's weight row
  if constexpr (W8) wsc = St[(int64_t)el * N + 32 * nbl + r];
  // mxfp4: the lane's row in the block-scale image, 32 rows x 2 B per vector (same expert, tile and vector index as wp:
  // in range wherever the weight load is)
  const uint16_t* sp = nullptr;
  if constexpr (W4) sp = St + v0 * 32 + r;
  const int nchunks = K / KC;

  // A-row sources of this thread's staged chunks (fixed over K)
  const bf16* xsrc[XL];
#pragma unroll
  for (int i = 0; i < XL; ++i) {
    const int idx = tid + 256 * i;
    const int row = idx / CPR, c = idx % CPR;
    const int ent = seg0 + row0 + min(row, rows - 1);  // rows past the segment reload a valid row, never stored
    const int64_t src = GATHER ? (int64_t)perm_tok[ent] : (int64_t)ent;
    xsrc[i] = X + src * ldx + c * 8;
  }
  bf16x8 xr[XL];
  auto load_x = [&](int ch) {
#pragma unroll
    for (int i = 0; i < XL; ++i) xr[i] = load_bf16x8(xsrc[i] + ch * KC);
  };
  auto store_x = [&](int buf) {
#pragma unroll
    for (int i = 0; i < XL; ++i) {
      const int idx = tid + 256 * i;
      const int row = idx / CPR, c = idx % CPR;
      *reinterpret_cast<bf16x8*>(&xs[buf][row * KC + 8 * (c ^ (row & 15))]) = xr[i];
    }
  };
  auto load_w = [&](wvec(&wv)[KSV], uint16_t(&sv)[NSC], int ch) {
    if constexpr (W4) {
      // the block scales first: loads return in order, so the first dequantisation waits for them and vector 0 only
#pragma unroll
      for (int t = 0; t < KSV; ++t) sv[t] = __builtin_nontemporal_load(sp + (int64_t)(ch * KSV + t) * 32);
    }
#pragma unroll
    for (int t = 0; t < KSV; ++t) wv[t] = __builtin_nontemporal_load(wp + (int64_t)(ch * KSV + t) * 64);
    if constexpr (PIN) __builtin_amdgcn_sched_barrier(0);  // (prefetch kept ahead of the MFMAs, as wstream_gemm)
  };
  const int mt_used = (rows + 31) >> 5;  // row tiles with live rows (uniform)
  f32x16 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[mt][i] = 0.f;
  auto compute = [&](int buf, const wvec(&wv)[KSV], const uint16_t(&sv)[NSC]) {
#pragma unroll
    for (int t = 0; t < KSTEP; ++t) {
      bf16x8 wf;
      if constexpr (W4) {
        // dequantised right before its MFMAs: the prefetch registers keep the raw nibbles and exponent bytes; dword
        // t & 3 of vector t >> 2 is this k-step, its block exponent byte (t & 3) >> 1 of the vector's pair
        const u32x4 v = wv[t >> 2];
        const uint32_t e2 = sv[t >> 2];
        const uint32_t eb = (t & 2) ? e2 >> 8 : e2 & 0xffu;
        wf = dq4(v[t & 3], __builtin_bit_cast(float, eb << 23));
      } else if constexpr (W8) {
        // dequantised right before its MFMAs: the prefetch registers keep the raw fp8
        const u32x4 v = wv[t >> 1];
        wf = (t & 1) ? dq8(v[2], v[3], wsc) : dq8(v[0], v[1], wsc);
      } else {
        wf = wv[t];
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        // MT = 4 computes every row tile (rows past the segment hold a valid row, never stored): with the MFMAs of
        // unused tiles skipped behind a branch, the last accumulator register of tile 0 was read before its final
        // MFMA had written it (row 27 / 31 of a 28..32-row expert wrong at K = 512; the 128-row tile's MFMAs are
        // cheap next to its weight stream)
        if (MT == 4 || mt < mt_used) {
          const int m = mt * 32 + r, c = 2 * t + h;
          const bf16x8 xf = *reinterpret_cast<const bf16x8*>(&xs[buf][m * KC + 8 * (c ^ (m & 15))]);
          acc[mt] = mfma32(xf, wf, acc[mt]);
        }
      }
    }
  };
  wvec wa[KSV], wb[KSV];
  uint16_t sa[NSC], sb[NSC];  // (mxfp4 only: dead otherwise)
  load_x(0);
  load_w(wa, sa, 0);
  store_x(0);
  __syncthreads();
  int ch = 0;
  for (; ch + 2 < nchunks; ch += 2) {
    load_x(ch + 1);
    load_w(wb, sb, ch + 1);
    compute(0, wa, sa);
    store_x(1);
    __syncthreads();
    load_x(ch + 2);
    load_w(wa, sa, ch + 2);
    compute(1, wb, sb);
    store_x(0);
    __syncthreads();
  }
  if (ch + 1 < nchunks) {
    load_x(ch + 1);
    load_w(wb, sb, ch + 1);
    compute(0, wa, sa);
    store_x(1);
    __syncthreads();
    compute(1, wb, sb);
  } else {
    compute(0, wa, sa);
  }

  if constexpr (!COMBINE) {
    // SwiGLU epilogue: odd waves hand their up tile to the even wave of the pair through LDS
    float* red = reinterpret_cast<float*>(&xs[0][0]);
    __syncthreads();
    if (w & 1) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) red[(((w >> 1) * MT + mt) * 16 + i) * 64 + lane] = acc[mt][i];
    }
    __syncthreads();
    if (!active || (w & 1)) return;
    const int n = (nb >> 1) * 32 + r;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int m = mt * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
        if (m < rows) {
          const float g = acc[mt][i], u = red[(((w >> 1) * MT + mt) * 16 + i) * 64 + lane];
          Y[(int64_t)(seg0 + row0 + m) * ldy + n] = (bf16)(g / (1.0f + __expf(-g)) * u);
        }
      }
  } else {
    if (!active) return;
    const int n = nb * 32 + r;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int m = mt * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
        if (m < rows) {
          const int ent = seg0 + row0 + m;
          atomicAdd(out + (int64_t)perm_tok[ent] * ldo + n, perm_w[ent] * acc[mt][i]);
        }
      }
  }
}

// Y[m, n] = sum_s P[s, m, n] (bf16), 8 columns per thread: the standalone combine for callers without a
// slab-aware consumer (TP all-reduce inputs, tests).
__global__ __launch_bounds__(256) void slab_reduce_kernel(const float* __restrict__ P, int S, int M, int N,
                                                          bf16* __restrict__ Y, int64_t ldy) {
  const int64_t idx = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
  if (idx >= (int64_t)M * N) return;
  const int m = (int)(idx / N), n = (int)(idx % N);
  const int64_t ps = (int64_t)M * N;
  float v[8];
  load_in8(v, nullptr, P, S, ps, idx);
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (bf16)v[j];
  store_bf16x8(Y + (int64_t)m * ldy + n, o);
}

// Host plan: row tiles MT, K chunk KC and split count S for a shape; returns 0 if supported (mirrored by
// ops.stream_plan). max_splits caps S (1 forces a direct bf16 output).
//   MT: 1 tile up to 32 rows, 2 up to 64, 3 up to 96 (a decode batch plus a short new-turn chunk: three 32-row tiles
//   on 256-deep chunks, 96 KB X stage; +0.24 % over four on 128-deep ones, profiles/r04/bench_ab_wstream_mt3.jsonl),
//   4 up to 128 (128-deep chunks: 256-deep ones lose 1.9 %, profiles/r04/bench_ab_wstream_mt4_kc256.jsonl), 6 up to
//   192 (a decode batch plus a ~100-token new turn: one 192-row tile on 128-deep chunks, 96 KB X stage, ~210
//   registers at one wave per SIMD; two 128-row tiles sharing the weight slice lost to hipBLASLt, r02/r05). Beyond
//   192 rows (tiled-only models) the rows are split over row tiles of 128.
//   Measured and rejected (profiles/r04/): 64-row tiles sharing a weight slice in one XCD's L2 beyond 64 rows (-0.6 %)
//   and 33..64 rows as two 32-row tiles (-4.8 %).
extern "C" int kafka_wstream_plan(int M, int N, int K, int max_splits, int* mt, int* kc, int* splits) {
  if (M < 1 || M > 256 || N % 32 != 0 || N <= 0) return 1;
  const int MT = M <= 32 ? 1 : (M <= 64 ? 2 : (M <= 96 ? 3 : (M <= 128 || M > 192 ? 4 : 6)));
  const int KC = MT >= 4 ? 128 : 256;
  if (K % KC != 0 || K <= 0) return 2;
  const int nx = (N + 127) / 128 * ((M + 32 * MT - 1) / (32 * MT));  // workgroups per split (x row tiles)
  const int chunks = K / KC;
  // split until the grid reaches ~192 workgroups: measured on MI355X (benchmarks/wstream_sweep.py,
  // profiles/wstream_sweep_r01.log; split targets 96..384 re-checked in profiles/r04/bench_ab_split_target_*.jsonl)
  // — every extra split adds 2 x M x N x 4 B of slab traffic, so e.g. gate_up (N = 28672) at M = 64 runs fastest
  // unsplit and qkv (N = 6144) with S = 4. With the pinned prefetch, gate_up at 97..128 rows also runs fastest
  // unsplit (53.3 us at 114 rows with its fused SwiGLU vs 60.4 + a SwiGLU pass split in two;
  // profiles/r05/wstream_sweep_pin.jsonl), so MT = 4 shares the target (it was 256).
  const int target = 192;
  int s = 1;
  while (s * 2 <= max_splits && s * 2 <= 8 && chunks % (s * 2) == 0 && nx * s < target) s *= 2;
  *mt = MT;
  *kc = KC;
  *splits = s;
  return 0;
}

// One launch of wstream_gemm_kernel: the kernel's arguments, the grid and the stream.
struct WsLaunch {
  const bf16* X;
  int64_t ldx;
  const bf16x8* wt;
  int M, N, K, ks;
  bf16* Y;
  int64_t ldy;
  float* p;
  int glu, rt, wide;
  FinArgs fa;
  dim3 grid;
  hipStream_t st;
};

// The instantiations of one (MT, KC, KW, PIN) configuration: the plain epilogue on every tile format (bf16 with
// non-temporal or plain loads, the quantised formats non-temporal only) and, up to 128 rows, the three fused
// epilogues on bf16 tiles.
template <int MT, int KC, int KW, bool PIN>
static hipError_t launch_ws_cfg(const WsLaunch& a, int fin, int wfmt, int nt) {
  void (*k)(const bf16*, int64_t, const bf16x8*, int, int, int, int, bf16*, int64_t, float*, int, int, int, FinArgs) =
      nullptr;
  if (fin == FIN_NONE) {
    if (wfmt == WF_FP8) k = wstream_gemm_kernel<MT, KC, true, KW, PIN, FIN_NONE, WF_FP8>;
    else if (wfmt == WF_MXFP4) k = wstream_gemm_kernel<MT, KC, true, KW, PIN, FIN_NONE, WF_MXFP4>;
    else if (nt) k = wstream_gemm_kernel<MT, KC, true, KW, PIN>;
    else k = wstream_gemm_kernel<MT, KC, false, KW, PIN>;
  } else if constexpr (MT != 6) {  // (the 192-row tile has no finishers)
    if (fin == FIN_RES) k = wstream_gemm_kernel<MT, KC, true, KW, PIN, FIN_RES>;
    else if (fin == FIN_ROPE) k = wstream_gemm_kernel<MT, KC, true, KW, PIN, FIN_ROPE>;
    else k = wstream_gemm_kernel<MT, KC, true, KW, PIN, FIN_GLU>;
  }
  if (k == nullptr) return hipErrorInvalidValue;
  k<<<a.grid, 256 * KW, 0, a.st>>>(a.X, a.ldx, a.wt, a.M, a.N, a.K, a.ks, a.Y, a.ldy, a.p, a.glu, a.rt, a.wide, a.fa);
  return hipGetLastError();
}

// The (MT, KC, KW) configurations of wstream_gemm_kernel, for both launchers below.
static hipError_t launch_ws(const WsLaunch& a, int mt, int kc, int kw, int pin, int fin, int wfmt, int nt) {
#define KAFKA_WS_CFG(MT_, KC_, KW_)                                          \
  if (mt == MT_ && kc == KC_ && kw == KW_)                                   \
    return pin ? launch_ws_cfg<MT_, KC_, KW_, true>(a, fin, wfmt, nt)        \
               : launch_ws_cfg<MT_, KC_, KW_, false>(a, fin, wfmt, nt);
  KAFKA_WS_CFG(1, 256, 1)
  KAFKA_WS_CFG(1, 256, 2)
  KAFKA_WS_CFG(2, 256, 1)
  KAFKA_WS_CFG(2, 256, 2)
  KAFKA_WS_CFG(3, 256, 1)
  KAFKA_WS_CFG(4, 128, 1)
  KAFKA_WS_CFG(4, 128, 2)
  KAFKA_WS_CFG(6, 128, 1)
#undef KAFKA_WS_CFG
  return hipErrorInvalidValue;
}

// wfmt (WF_*) names the layout of Wt and of its scales: bf16 tiles [N/32][K/16][64][8] without scales; fp8 tiles
// [N/32][K/32][64][16] e4m3 bytes with St [N] fp32 row scales in tile order; MXFP4 tiles [N/32][K/64][64][16] e2m1
// bytes with Se [N/32][K/64][32][2] e8m0 block exponents. Every format runs the same plans, grid, outputs and
// (mt, kc, kw, pin) configurations; the quantised ones stream with non-temporal loads only.
extern "C" hipError_t kafka_launch_wstream_gemm(const bf16* X, int64_t ldx, int wfmt, const void* Wt, const void* scale,
                                               int M, int N, int K, int mt, int kc, int splits, int nt, int kw, int pin,
                                               int glu, bf16* Y, int64_t ldy, float* P, hipStream_t st) {
  if (M < 1) return hipSuccess;
  if (glu && (N % 64 != 0 || kw > 2)) return hipErrorInvalidValue;  // (the SwiGLU epilogue runs after the KW fold)
  switch (wfmt) {
    case WF_BF16:
      if (scale != nullptr) return hipErrorInvalidValue;
      break;
    case WF_FP8:
    case WF_MXFP4:  // whole weight vectors along K (32 / 64 columns), with their scales
      if (K % (1 << wf_vshift(wfmt)) != 0 || N % 32 != 0 || Wt == nullptr || scale == nullptr || !nt)
        return hipErrorInvalidValue;
      break;
    default: return hipErrorInvalidValue;
  }
  if (K % (kc * splits) != 0 || (splits > 1 && P == nullptr) || (splits == 1 && P == nullptr && Y == nullptr))
    return hipErrorInvalidValue;
  WsLaunch a{};
  a.X = X, a.ldx = ldx, a.wt = static_cast<const bf16x8*>(Wt), a.M = M, a.N = N, a.K = K, a.Y = Y, a.ldy = ldy;
  a.glu = glu, a.st = st;
  a.rt = (M + 32 * mt - 1) / (32 * mt);  // row tiles of 32 * mt rows
  const int nblk = (N + 127) / 128;
  a.grid = dim3((a.rt > 1 ? (nblk + 7) / 8 * 8 : nblk) * a.rt, splits);  // (row tiles: column blocks padded to 8)
  a.ks = K / splits;
  a.p = splits > 1 ? P : nullptr;
  // split-K slabs leave as 16-B sc1 stores through an LDS transpose (was one 4-B store per accumulator, the lines
  // kept dirty in the XCD's L2): +2.0 % on the headline, in-step GPU time 7.50 vs 7.65 ms
  // (profiles/r05/bench_ab_wstream_slab16_sc1.jsonl).
  // The un-split bf16 outputs (fused SwiGLU, lm_head) the same way through a workgroup LDS tile, whole 128-B lines
  // per store instruction (was one 2-B store per accumulator, half lines): +1.1..2.1 %, in-step GPU time 7.37 vs
  // 7.45-7.49 ms (profiles/r05/bench_ab_wstream_wide_y.jsonl) — 16-B stores of Y need 16-B aligned rows
  const bool y_unaligned = Y != nullptr && (ldy % 8 != 0 || reinterpret_cast<uintptr_t>(Y) % 16 != 0);
  a.wide = y_unaligned ? WIDE_P : (WIDE_P | WIDE_Y);
  a.fa.wscale = scale;  // (see the kernel's header comment)
  return launch_ws(a, mt, kc, kw, pin, FIN_NONE, wfmt, nt);
}

// Fused decode-layer GEMMs (FIN_RES / FIN_ROPE / FIN_GLU above): one row tile (M <= 128), N % 128 == 0, S in
// {1, 2, 4, 8}; P = [S][M][N] fp32 scratch (unused for S == 1); FIN_GLU needs S == 1.
extern "C" hipError_t kafka_launch_wstream_fin(int fin, const bf16* X, int64_t ldx, const bf16* Wt, int M, int N, int K,
                                              int mt, int kc, int splits, int kw, int pin, bf16* Y, int64_t ldy,
                                              float* P, const FinArgs* fa_in, hipStream_t st) {
  if (M < 1) return hipSuccess;
  const FinArgs fa = *fa_in;
  if (M > 32 * mt || M > 128 || N % 128 != 0 || K % (kc * splits) != 0) return hipErrorInvalidValue;
  if (!(splits == 1 || splits == 2 || splits == 4 || splits == 8)) return hipErrorInvalidValue;
  if (fin == FIN_GLU) {
    const int ssl = 4096 / (256 * kw);
    int tpr = 1;
    while (tpr * ssl < fa.nss) tpr <<= 1;
    if (splits != 1 || Y == nullptr || tpr > 64 || M * tpr > 256 * kw) return hipErrorInvalidValue;
  } else if (fin == FIN_RES) {
    if (fa.resid == nullptr || fa.nw == nullptr || fa.xn == nullptr || fa.ss_out == nullptr) return hipErrorInvalidValue;
  } else if (fin == FIN_ROPE) {
    if (fa.nss > 32 || fa.positions == nullptr || fa.cos_sin == nullptr || fa.q_out == nullptr || N != (fa.Hq + 2 * fa.Hkv) * 128 ||
        (fa.slots != nullptr && (fa.k_cache == nullptr || fa.v_cache == nullptr)))
      return hipErrorInvalidValue;
  } else {
    return hipErrorInvalidValue;
  }
  if (fin != FIN_GLU && ((splits > 1 && (P == nullptr || fa.tickets == nullptr))))
    return hipErrorInvalidValue;
  WsLaunch a{};
  a.X = X, a.ldx = ldx, a.wt = reinterpret_cast<const bf16x8*>(Wt), a.M = M, a.N = N, a.K = K, a.Y = Y, a.ldy = ldy;
  a.fa = fa, a.st = st, a.rt = 1;
  a.grid = dim3(N / 128, splits);
  a.ks = K / splits;
  a.p = splits > 1 ? P : nullptr;
  // (only FIN_GLU's Y consults it: wide stores when its rows are 16-B aligned)
  a.wide = (Y != nullptr && (ldy % 8 != 0 || reinterpret_cast<uintptr_t>(Y) % 16 != 0)) ? 0 : WIDE_Y;
  a.glu = fin == FIN_GLU ? 1 : 0;
  return launch_ws(a, mt, kc, kw, pin, fin, WF_BF16, 1);
}

extern "C" hipError_t kafka_launch_slab_reduce(const float* P, int S, int M, int N, bf16* Y, int64_t ldy,
                                              hipStream_t st) {
  if (M < 1) return hipSuccess;
  if (N % 8 != 0) return hipErrorInvalidValue;
  const int64_t total = (int64_t)M * N / 8;
  slab_reduce_kernel<<<(int)((total + 255) / 256), 256, 0, st>>>(P, S, M, N, Y, ldy);
  return hipGetLastError();
}

}  // namespace kafka

namespace kafka {
// One launch of wstream_grouped_kernel: the kernel's arguments (scale: St for fp8 tiles, Se for mxfp4 ones), the grid
// and the stream.
struct WgLaunch {
  const bf16* X;
  int64_t ldx;
  const bf16x8* wt;
  int N, K;
  const int* perm_tok;
  const float* perm_w;
  const int* expert_off;
  int e_lo;
  bf16* Y;
  int64_t ldy;
  float* out;
  int64_t ldo;
  const void* scale;
  dim3 grid;
  hipStream_t st;
};

template <int MT, bool G, bool C>
static void launch_wg_cfg(const WgLaunch& a, int wfmt, int pin) {
  constexpr int KC = MT == 4 ? 128 : 256;
  auto go = [&](auto kern, auto sc) {
    kern<<<a.grid, 256, 0, a.st>>>(a.X, a.ldx, a.wt, a.N, a.K, a.perm_tok, a.perm_w, a.expert_off, a.e_lo, a.Y, a.ldy,
                                   a.out, a.ldo, sc);
  };
  if (wfmt == WF_FP8) {
    const auto* st = static_cast<const float*>(a.scale);
    pin ? go(wstream_grouped_kernel<MT, KC, G, C, true, WF_FP8>, st)
        : go(wstream_grouped_kernel<MT, KC, G, C, false, WF_FP8>, st);
  } else if (wfmt == WF_MXFP4) {
    const auto* se = static_cast<const uint16_t*>(a.scale);
    pin ? go(wstream_grouped_kernel<MT, KC, G, C, true, WF_MXFP4>, se)
        : go(wstream_grouped_kernel<MT, KC, G, C, false, WF_MXFP4>, se);
  } else {
    pin ? go(wstream_grouped_kernel<MT, KC, G, C, true>, NoScales{})
        : go(wstream_grouped_kernel<MT, KC, G, C, false>, NoScales{});
  }
}

// Grouped streaming GEMM for the expert MLP (see wstream_grouped_kernel). max_rows bounds any expert's segment
// (the token count T: a token picks an expert at most once); glu: gate_up with fused SwiGLU into Y [n_ent, N/2];
// else combine into out_f32 [T, N].
// wfmt: bf16 expert tiles Wt [E_local][N/32][K/16][64][8] without scales, fp8 ones [E_local][N/32][K/32][64][16]
// e4m3 bytes with St [E_local][N] fp32 row scales in tile order (ops.tile_experts_fp8), or MXFP4 ones
// [E_local][N/32][K/64][64][16] e2m1 bytes with Se [E_local][N/32][K/64][32][2] e8m0 block exponents
// (ops.tile_experts_mxfp4); same grid, MT choice and outputs.
extern "C" hipError_t kafka_launch_wstream_grouped(const bf16* X, int64_t ldx, int wfmt, const void* Wt,
                                                  const void* scale, int e_local, int N, int K, const int* perm_tok,
                                                  const float* perm_w, const int* expert_off, int e_lo, int max_rows,
                                                  int gather, bf16* Y, int64_t ldy, float* out, int64_t ldo, int pin,
                                                  hipStream_t st) {
  if (max_rows < 1 || e_local < 1) return hipSuccess;
  if (N % 64 != 0 || K % 256 != 0 || (out == nullptr) == (Y == nullptr)) return hipErrorInvalidValue;
  switch (wfmt) {
    case WF_BF16:
      if (scale != nullptr) return hipErrorInvalidValue;
      break;
    case WF_FP8:
    case WF_MXFP4:  // (K % 256 == 0 above: whole 32- / 64-column weight vectors)
      if (Wt == nullptr || scale == nullptr) return hipErrorInvalidValue;
      break;
    default: return hipErrorInvalidValue;
  }
  // MT = 4 (128-row tiles on 128-deep K chunks) for large steps: with 64-row tiles every
  // row tile of an expert re-streams its weights, and those tiles run far apart in dispatch order (blockIdx.z is the
  // slowest dimension), so no cache keeps the slice between them — an expert with 65..128 rows read its 352 MB twice.
  // (64-row tiles stay below 193 rows: an expert then rarely fills a second tile, and they stream faster there —
  // benchmarks/moe_bench.py T = 128 / 192: 493 / 522 vs 517 / 551 us per layer; T = 256 / 384 / 512: 761 / 1002 /
  // 1303 vs 601 / 691 / 1004, profiles/r06/mixtral/)
  const int MT = max_rows <= 32 ? 1 : (max_rows <= 192 ? 2 : 4);
  const WgLaunch a{X, ldx, static_cast<const bf16x8*>(Wt), N, K, perm_tok, perm_w, expert_off, e_lo, Y, ldy, out, ldo,
                   scale, dim3((N + 127) / 128, e_local, (max_rows + 32 * MT - 1) / (32 * MT)), st};
  const bool comb = out != nullptr;
#define KAFKA_WG(MT_)                                                                                        \
  (gather ? (comb ? launch_wg_cfg<MT_, true, true>(a, wfmt, pin) : launch_wg_cfg<MT_, true, false>(a, wfmt, pin))   \
          : (comb ? launch_wg_cfg<MT_, false, true>(a, wfmt, pin) : launch_wg_cfg<MT_, false, false>(a, wfmt, pin)))
  if (MT == 1) KAFKA_WG(1);
  else if (MT == 2) KAFKA_WG(2);
  else KAFKA_WG(4);
#undef KAFKA_WG
  return hipGetLastError();
}
}  // namespace kafka
