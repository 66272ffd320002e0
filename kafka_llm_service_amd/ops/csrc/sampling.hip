// Token sampler for gfx950: greedy / temperature / top-k / top-p in one kernel, one 1024-thread workgroup per row.
//
//   temperature == 0       -> argmax (first maximal index)
//   otherwise              -> Gumbel-max over x = logits / T with counter-based uniforms (seed, step, index):
//                             an exact sample of softmax(x) in one pass, no sort, no normalisation pass.
//   top_k > 0 or top_p < 1 -> rejection on a pivot: draw c from the tokens strictly above the pivot, accept iff
//                             (#tokens with x > x_c) < k and (mass of tokens with x > x_c) < p; otherwise raise the
//                             pivot to x_c and redraw. Accepted draws are exactly distributed as the renormalised
//                             top-k/top-p distribution; rounds are bounded (fallback: argmax).
//                             Every comparison is strict, which fixes the tie rule: tokens tied with the candidate
//                             count neither toward k nor toward the mass, and tokens tied with the pivot are not
//                             redrawn (top_k = 1 over a maximum that occurs twice returns either of the two).
//                             ops/reference.py sample_replay replays these decisions with the same random stream.
//   min_p (RowProc [7])    -> keep x_i >= max + ln(min_p): one more test on a top-k / top-p row's candidates; alone
//                             it stays on the plain stream and split (sample_min_p_split), two passes per slice.
// All reads are 16-byte vectors; every pass is one streaming read of the row (bf16 or fp32 logits).
// Greedy and plain-temperature rows (no top-k / top-p) are split over `nsplit` workgroups (grid (B, nsplit)): each
// takes a slice of the vocabulary, publishes its (value, index) winner, and the last of a row's workgroups to take
// its ticket reduces them — the noise of index i is the same in every split, so the token is the one-workgroup
// result. A 64-row decode batch then runs 512 workgroups instead of 64 (128k-entry rows: 62 -> ~10 us).
#include "row_scan.h"

namespace kafka {

constexpr int SNT = 1024;
constexpr int SAMPLE_MAX_ROWS = 65536;  // ws: tickets [SAMPLE_MAX_ROWS] | partials [B][nsplit][2]

__device__ __forceinline__ float gumbel(uint64_t seed, uint64_t stream, uint64_t idx) {
  const float u = uniform01(seed, stream, idx);  // (0, 1]
  return -__logf(-__logf(fminf(u, 0.99999994f)));
}

// Plain-temperature rows: the per-element noise from a per-row 64-bit key (two splitmix64 rounds, once per thread)
// and a 32-bit integer hash of the index (two lowbias32 rounds: 4 v_mul_lo_u32 instead of the ~16 32-bit multiplies
// two 64-bit splitmix rounds cost per element) — the noise stream is still a pure function of (seed, step, index),
// so every split of a row draws the same noise for an index and the token is the one-workgroup result.
__device__ __forceinline__ uint32_t lowbias32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
__device__ __forceinline__ float gumbel_fast(uint64_t key, uint32_t idx) {
  const uint32_t h = lowbias32(lowbias32(idx + (uint32_t)key) ^ (uint32_t)(key >> 32));
  const float u = ((float)(h >> 8) + 1.0f) * (1.0f / 16777216.0f);  // (0, 1]
  return -__logf(-__logf(fminf(u, 0.99999994f)));
}

// Per-row logits processing on the device (PROC instantiation; VERDICT r03 "Next round" #3): proc[row] = int32 x 8
//   [0] mode: 0 = none, 1 = vocab bitmask (row [1] of mask_tab), 2 = forced token ([1] is the id: no draw at all)
//   [2] penalty slot: row of counts[slot][V] (the row's generated-token counts, -1 = none) and of rep_tab
//   [3] presence penalty, [4] frequency penalty (fp32 bits)
//   [5] logit-bias row of bias_tab, [6] its entry count (0 = no bias; clamped to LOGIT_BIAS_MAX)
//   [7] min_p: the fp32 bits of lmp = float32(ln(min_p)), the host's logarithm (0 = off; min_p = 1 is -0.0). Under
//       temperature token i is kept iff x_i / T >= max(x / T) + lmp — one fp32 add, so every token is tested on its own
//       once the maximum is known — intersected with top-k / top-p; greedy and forced rows ignore it.
// The logit of token i becomes  (y_i - freq * c_i - (c_i > 0 ? pres : 0)) + b_i  (OpenAI presence / frequency
// penalties, then the request's logit_bias, before temperature), or -inf where the grammar mask has a zero bit; the
// sampler then runs unchanged over it, and the thread that writes the row's token also bumps counts[slot][token] —
// the next step (stream-ordered) sees it, so penalties need no landed tokens on the host and no per-row torch ops
// over the [B, V] logits.
// Repetition penalty (rep_tab fp32 [slots, 2] = (r, 1 / r), both rounded on the host; a null table or r == 1: none):
// y_i = x_i unless token i is SEEN by the row's sequence, then x_i * (1 / r) for x_i > 0 and x_i * r otherwise — one
// fp32 multiply rounded on its own (__fmul_rn: no fma with the subtraction that follows), never a division. Seen is
// counts[slot][i] != 0: the word holds the generated count in its low 30 bits (c_i above, what presence and frequency
// use) and COUNT_SEEN_PROMPT where the host seeded a prompt token of the slot's sequence, so the multiply rides on the
// load the penalties already make. emit_token's += 1 leaves the flag alone. The host sets flags and a factor r != 1
// together and clears both when a slot is recycled, so a row without a factor holds plain counts and runs the code it
// ran before the flag existed.
// The bias is sparse: a row of bias_tab holds n <= LOGIT_BIAS_MAX ascending ids and their biases (kafka_abi.h). A
// workgroup stages its row's pairs in LDS once; every 16-byte logit load then finds the first id >= its index by
// binary search there (<= 9 LDS reads) and adds the few biases that fall into its 8 indices: no dense [slots, V]
// table, no HBM traffic per pass.
struct RowProc {
  int mode, arg, slot;
  float pres, freq;
  const uint32_t* mask;
  int* cnt;
  int nb;           // staged logit-bias pairs (bias_lds)
  const int* bias;  // the row of bias_tab they come from
  bool minp;        // proc[7] != 0
  float lmp;        // ln(min_p) <= 0 (0 when off)
  bool rep;         // the slot's rep_tab row holds r != 1
  float r, inv_r;   // repetition penalty and its host-rounded reciprocal
};

template <bool PROC>
__device__ __forceinline__ RowProc row_proc(const int* proc, const uint32_t* mask_tab, int64_t mask_ld, int* counts,
                                            int64_t cnt_ld, const int* bias_tab, int64_t bias_ld,
                                            const float* rep_tab, int row) {
  RowProc r{0, -1, -1, 0.f, 0.f, nullptr, nullptr, 0, nullptr, false, 0.f, false, 1.f, 1.f};
  if constexpr (PROC) {
    const int* p = proc + (int64_t)row * 8;
    r.minp = p[7] != 0;
    r.lmp = fminf(__int_as_float(p[7]), 0.f);  // (a positive or NaN word from a broken host keeps the maximum itself)
    r.mode = p[0];
    r.arg = p[1];
    r.slot = p[2];
    r.pres = __int_as_float(p[3]);
    r.freq = __int_as_float(p[4]);
    if (r.mode == 1) r.mask = mask_tab + (int64_t)r.arg * mask_ld;
    if (r.slot >= 0) r.cnt = counts + (int64_t)r.slot * cnt_ld;
    if (rep_tab != nullptr && r.cnt != nullptr) {
      r.r = rep_tab[2 * r.slot];
      r.inv_r = rep_tab[2 * r.slot + 1];
      r.rep = r.r != 1.f;
    }
    if (bias_tab != nullptr && p[6] > 0) {
      r.nb = min(p[6], LOGIT_BIAS_MAX);
      r.bias = bias_tab + (int64_t)p[5] * bias_ld;
    }
  }
  return r;
}

// The workgroup's staged bias pairs: ids at [0, nb), biases (fp32 bits) at [LOGIT_BIAS_MAX, LOGIT_BIAS_MAX + nb).
// Only the PROC instantiations name it, so the others carry no LDS for it.
template <bool PROC>
__device__ __forceinline__ int* bias_lds() {
  static_assert(PROC, "the plain sampler has no bias table");
  __shared__ int sb[2 * LOGIT_BIAS_MAX];
  return sb;
}

// index of the first staged id >= i (nb if none)
__device__ __forceinline__ int bias_lower_bound(const int* sb, int nb, int i) {
  int lo = 0, hi = nb;
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (sb[m] < i) lo = m + 1; else hi = m;
  }
  return lo;
}

// 8 logits starting at index i0 (a multiple of 8), processed
template <typename T, bool PROC, bool REP = false>
__device__ __forceinline__ void load8p(const T* x, int i0, const RowProc& rp, float (&v)[8]) {
  Vec8<T>::load(x + i0, v);
  if constexpr (PROC) {
    if (rp.cnt != nullptr) {
      const int4 c0 = *reinterpret_cast<const int4*>(rp.cnt + i0);
      const int4 c1 = *reinterpret_cast<const int4*>(rp.cnt + i0 + 4);
      const int c[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
      if constexpr (REP) {  // (only such a slot holds flags: the other rows keep the code they had)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int g = c[j] & (COUNT_SEEN_PROMPT - 1);
          if (c[j] != 0) v[j] = __fmul_rn(v[j], v[j] > 0.f ? rp.inv_r : rp.r);
          v[j] -= rp.freq * (float)g + (g > 0 ? rp.pres : 0.f);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] -= rp.freq * (float)c[j] + (c[j] > 0 ? rp.pres : 0.f);
      }
    }
    if (rp.nb > 0) {
      const int* sb = bias_lds<PROC>();
      for (int k = bias_lower_bound(sb, rp.nb, i0); k < rp.nb; ++k) {
        const int d = sb[k] - i0;
        if (d >= 8) break;
        const float b = __int_as_float(sb[LOGIT_BIAS_MAX + k]);
#pragma unroll
        for (int j = 0; j < 8; ++j)  // (v stays in registers: no indexing by d)
          if (j == d) v[j] += b;
      }
    }
    if (rp.mask != nullptr) {
      const uint32_t bits = (rp.mask[i0 >> 5] >> (i0 & 31)) & 0xffu;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (!((bits >> j) & 1u)) v[j] = -INFINITY;
    }
  }
}

template <typename T, bool PROC, bool REP = false>
__device__ __forceinline__ float load1p(const T* x, int i, const RowProc& rp) {
  float v = (float)x[i];
  if constexpr (PROC) {
    if (rp.cnt != nullptr) {
      const int c = rp.cnt[i];
      if constexpr (REP) {
        const int g = c & (COUNT_SEEN_PROMPT - 1);
        if (c != 0) v = __fmul_rn(v, v > 0.f ? rp.inv_r : rp.r);
        v -= rp.freq * (float)g + (g > 0 ? rp.pres : 0.f);
      } else {
        v -= rp.freq * (float)c + (c > 0 ? rp.pres : 0.f);
      }
    }
    if (rp.nb > 0) {
      const int* sb = bias_lds<PROC>();
      const int k = bias_lower_bound(sb, rp.nb, i);
      if (k < rp.nb && sb[k] == i) v += __int_as_float(sb[LOGIT_BIAS_MAX + k]);
    }
    if (rp.mask != nullptr && !((rp.mask[i >> 5] >> (i & 31)) & 1u)) v = -INFINITY;
  }
  return v;
}

template <bool PROC>
__device__ __forceinline__ void emit_token(int64_t* out_tokens, int row, int tok, int V, const RowProc& rp) {
  tok = tok >= 0 && tok < V ? tok : 0;  // an all-NaN row (a broken upstream kernel) must not yield an id >= V
  out_tokens[row] = tok;
  if constexpr (PROC) {
    if (rp.cnt != nullptr) rp.cnt[tok] += 1;  // the row's only writer this step (one row per sequence)
  }
}

// One pass over slice s of the row as the sampler sees it: f(x_i * inv_t, i) over the processed logits.
template <typename T, bool PROC, bool REP, typename F>
__device__ __forceinline__ void scan_row(const T* x, const RowProc& rp, const RowSlice& s, float inv_t, F&& f) {
  scan_slice<SNT>(
      s, [&](int i0, float (&v)[8]) { load8p<T, PROC, REP>(x, i0, rp, v); },
      [&](int i) { return load1p<T, PROC, REP>(x, i, rp); }, [&](float v, int i) { f(v * inv_t, i); });
}

// Thread 0 of split sp publishes the split's two-int partial and takes the row's ticket (the ticket protocol of
// common.h); the last of the row's nsplit arrivals reads every pair, g(k, a_k, b_k), and gets true.
// ws: tickets (zero, re-armed by the last arrival) | [B][nsplit][2]
template <typename G>
__device__ __forceinline__ bool publish_pair(int* ws, int row, int sp, int nsplit, int a, int b, G&& g) {
  int* p0 = ws + SAMPLE_MAX_ROWS + (int64_t)row * nsplit * 2;
  publish(p0 + 2 * sp, a);
  publish(p0 + 2 * sp + 1, b);
  if (!take_ticket(ws + row, nsplit)) return false;
  for (int k = 0; k < nsplit; ++k) {
    const int ak = peek(p0 + 2 * k), bk = peek(p0 + 2 * k + 1);
    g(k, ak, bk);
  }
  return true;
}

// the split's LDS, outside the template so that a kernel with two row bodies holds it once
struct MinPLds {
  float* pm;
  int *pw, *pflag, *last;
};
__device__ __forceinline__ MinPLds min_p_lds() {
  __shared__ float pm[64];
  __shared__ int pw[64];
  __shared__ int pflag[64];
  __shared__ int s_last;
  return MinPLds{pm, pw, pflag, &s_last};
}

// min_p alone (T > 0, no effective top-k / top-p; PROC rows only): the kept set {xv >= max + lmp} needs the row maximum
// and nothing else, so the row stays on the plain stream (gumbel_fast, the plain rows' key: the token does not depend
// on nsplit) and stays split. A split reads its slice twice: the slice maximum m_s, then the argmax of xv + noise over
// {xv >= m_s + lmp} (the second read comes from L2). It publishes (m_s, winner index) in the two-int partial. The last
// workgroup forms thr = max m_s + lmp. fp32 add is monotonic, so m_s + lmp <= thr: a slice's own candidate set held the
// row's, and a winner that passes thr is exactly the slice's argmax over the row's set (its score is a pure function of
// (key, index, logit), recomputed here). A slice below thr gives nothing; a slice at or above thr whose winner fell
// below it is rescanned with thr by the whole workgroup (one slice of V / nsplit; rare on a peaked row, common on flat
// random logits, where most of a slice's mass lies between the two thresholds).
template <typename T, bool REP>
__device__ __forceinline__ void sample_min_p_split(const T* x, int V, const RowProc& rp, float inv_t, uint64_t key,
                                                   int row, int sp, int nsplit, int* ws, int64_t* out_tokens,
                                                   float* sv, int* si, float* red) {
  const MinPLds lds = min_p_lds();  // per slice (nsplit <= 64): maximum, winner, "rescan"
  float* pm = lds.pm;
  int *pw = lds.pw, *pflag = lds.pflag;
  int& s_last = *lds.last;
  // best of xv + noise over slice k's tokens with xv >= thr
  auto scan = [&](int k, float thr, Cand a) -> Cand {
    scan_row<T, true, REP>(x, rp, row_slice(V, k, nsplit), inv_t, [&](float xv, int i) {
      if (xv >= thr) a = better(a, Cand{xv + gumbel_fast(key, i), i});
    });
    return a;
  };
  float m = -INFINITY;
  scan_row<T, true, REP>(x, rp, row_slice(V, sp, nsplit), inv_t, [&](float xv, int) { m = fmaxf(m, xv); });
  m = block_max<SNT>(m, red);
  Cand a = block_argmax<SNT>(scan(sp, m + rp.lmp, Cand{-INFINITY, CAND_NONE}), sv, si);
  if (nsplit == 1) {  // one slice: its threshold is the row's
    if (threadIdx.x == 0) emit_token<true>(out_tokens, row, a.i, V, rp);
    return;
  }
  if (threadIdx.x == 0)
    s_last = publish_pair(ws, row, sp, nsplit, __float_as_int(m), a.i, [&](int k, int mk, int wk) {
      pm[k] = __int_as_float(mk);
      pw[k] = wk;
    });
  __syncthreads();
  if (!s_last) return;  // (uniform) the whole last workgroup stays: a rescan is a job for all of it
  float M = -INFINITY;
  for (int k = 0; k < nsplit; ++k) M = fmaxf(M, pm[k]);
  const float thr = M + rp.lmp;
  Cand r{-INFINITY, CAND_NONE};
  if ((int)threadIdx.x < nsplit) {  // thread k judges slice k
    const int w = pw[threadIdx.x];
    int flag = 0;
    if (pm[threadIdx.x] >= thr && w >= 0 && w < V) {
      const float xv = load1p<T, true, REP>(x, w, rp) * inv_t;
      if (xv >= thr) r = Cand{xv + gumbel_fast(key, w), w}; else flag = 1;
    }
    pflag[threadIdx.x] = flag;
  }
  __syncthreads();
  for (int k = 0; k < nsplit; ++k)
    if (pflag[k]) r = scan(k, thr, r);
  r = block_argmax<SNT>(r, sv, si);
  if (threadIdx.x == 0) emit_token<true>(out_tokens, row, r.i, V, rp);
}

// One row's draw (the kernel below has read its RowProc, written a forced row and staged the bias pairs). REP: the
// row's slot has a repetition penalty; a uniform branch in the kernel picks the instantiation once per workgroup, so
// the loops of rows without it are the loops they were.
template <typename T, bool PROC, bool REP>
__device__ __forceinline__ void sample_row(const T* x, int V, const float* temperature, const float* top_p,
                                           const int* top_k, const int64_t* seeds, const int64_t* step_ptr,
                                           int64_t* out_tokens, int max_rounds, int* ws, const RowProc& rp, int row,
                                           int sp, int nsplit, float* sv, int* si, float* red) {
  const float temp = temperature ? temperature[row] : 0.f;
  const float tp = top_p ? top_p[row] : 1.f;
  const int tk = top_k ? top_k[row] : 0;
  const bool filtered = temp > 0.f && ((tp < 1.f) || (tk > 0 && tk < V));

  if (!filtered) {
    // argmax of x (greedy) or of x / T + Gumbel noise over this workgroup's slice of the row
    const bool greedy = !(temp > 0.f);
    const float inv_t = greedy ? 1.f : 1.f / temp;
    const uint64_t seed = seeds ? (uint64_t)seeds[row] : 0x1234ull;
    const uint64_t stream = (uint64_t)(step_ptr ? step_ptr[0] : 0) << 8;  // round 0 of the filtered path
    const uint64_t key = mix64(seed ^ mix64(stream * 0x632BE59BD9B4E019ull));
    if constexpr (PROC) {
      if (rp.minp && !greedy) {  // the row's proc[7]: uniform over its workgroups; every other row runs what it ran
        sample_min_p_split<T, REP>(x, V, rp, inv_t, key, row, sp, nsplit, ws, out_tokens, sv, si, red);
        return;
      }
    }
    Cand a{-INFINITY, CAND_NONE};
    scan_row<T, PROC, REP>(x, rp, row_slice(V, sp, nsplit), inv_t, [&](float xv, int i) {
      a = better(a, Cand{greedy ? xv : xv + gumbel_fast(key, i), i});
    });
    a = block_argmax<SNT>(a, sv, si);
    if (threadIdx.x != 0) return;
    if (nsplit > 1) {  // the row's token is the best of its splits' winners: the last split to arrive finds it
      const Cand mine = a;
      a = Cand{-INFINITY, CAND_NONE};
      if (!publish_pair(ws, row, sp, nsplit, __float_as_int(mine.v), mine.i,
                        [&](int, int vk, int ik) { a = better(a, Cand{__int_as_float(vk), ik}); }))
        return;
    }
    emit_token<PROC>(out_tokens, row, a.i, V, rp);
    return;
  }
  if (sp != 0) return;  // top-k / top-p rows: one workgroup runs the whole-row rejection sampler
  const RowSlice all = row_slice(V, 0, 1);
  const float inv_t = 1.f / temp;
  const int64_t step = step_ptr ? step_ptr[0] : 0;
  const uint64_t seed = seeds ? (uint64_t)seeds[row] : 0x1234ull;

  // max of x (needed for the mass test only), then z = sum of exp(x - max)
  float mx = -INFINITY;
  scan_row<T, PROC, REP>(x, rp, all, inv_t, [&](float xv, int) { mx = fmaxf(mx, xv); });
  mx = block_max<SNT>(mx, red);
  float z = 0.f;
  scan_row<T, PROC, REP>(x, rp, all, inv_t, [&](float xv, int) { z += __expf(xv - mx); });
  z = block_sum<SNT>(z, red);
  // min_p: a candidate also passes the row's threshold (z and the mass stay the whole row's: the ratio to the maximum
  // does not change under renormalisation). The maximum passes its own threshold, so round 0 has a candidate.
  const float thr = PROC && rp.minp ? mx + rp.lmp : -INFINITY;

  float pivot = -INFINITY;
  int result = -1;
  for (int round = 0; round < max_rounds; ++round) {
    const uint64_t stream = ((uint64_t)step << 8) ^ (uint64_t)round;
    Cand a{-INFINITY, CAND_NONE};
    // scan_slice's loop pair over `all`, in its order, written out: as a scan_row call this pass spills SGPRs in the
    // REP instantiation (profiles/sampler_rowscan/resource_usage.txt)
    auto draw = [&](float xv, int i) {
      if (PROC ? (xv > pivot && xv >= thr) : xv > pivot) a = better(a, Cand{xv + gumbel(seed, stream, i), i});
    };
    for (int vi = all.v0 + threadIdx.x; vi < all.v1; vi += SNT) {
      float v[8];
      load8p<T, PROC, REP>(x, vi * 8, rp, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) draw(v[j] * inv_t, vi * 8 + j);
    }
    for (int i = all.t0 + threadIdx.x; i < all.t1; i += SNT) draw(load1p<T, PROC, REP>(x, i, rp) * inv_t, i);
    a = block_argmax<SNT>(a, sv, si);
    if (a.i == CAND_NONE) break;
    const float xc = load1p<T, PROC, REP>(x, a.i, rp) * inv_t;
    float mass = 0.f, cnt = 0.f;
    scan_row<T, PROC, REP>(x, rp, all, inv_t, [&](float xv, int) {
      if (xv > xc) {
        mass += __expf(xv - mx);
        cnt += 1.f;
      }
    });
    mass = block_sum<SNT>(mass, red) / z;
    cnt = block_sum<SNT>(cnt, red);
    const bool ok_p = mass < tp;
    const bool ok_k = (tk <= 0) || (cnt < (float)tk);
    if (ok_p && ok_k) {
      result = a.i;
      break;
    }
    pivot = xc;
  }
  if (result < 0) {  // fallback: argmax of the processed row itself (x * 1)
    Cand a{-INFINITY, CAND_NONE};
    scan_row<T, PROC, REP>(x, rp, all, 1.f, [&](float v, int i) { a = better(a, Cand{v, i}); });
    result = block_argmax<SNT>(a, sv, si).i;
  }
  if (threadIdx.x == 0) emit_token<PROC>(out_tokens, row, result, V, rp);
}

// REP: the launch has a rep_tab (some live slot has a repetition penalty). Without one the PROC kernel neither reads the
// table nor carries the penalised row body: it is the kernel it was before the penalty existed.
template <typename T, bool PROC, bool REP>
__global__ __launch_bounds__(SNT) void sample_kernel(const T* __restrict__ logits, int64_t stride, int V,
                                                      const float* __restrict__ temperature,
                                                      const float* __restrict__ top_p, const int* __restrict__ top_k,
                                                      const int64_t* __restrict__ seeds, const int64_t* __restrict__ step_ptr,
                                                      int64_t* __restrict__ out_tokens, int max_rounds,
                                                      int* __restrict__ ws, const int* __restrict__ proc,
                                                      const uint32_t* __restrict__ mask_tab, int64_t mask_ld,
                                                      int* __restrict__ counts, int64_t cnt_ld,
                                                      const int* __restrict__ bias_tab, int64_t bias_ld,
                                                      const float* __restrict__ rep_tab) {
  __shared__ float sv[SNT / 64];
  __shared__ int si[SNT / 64];
  __shared__ float red[SNT / 64];
  const int row = blockIdx.x, sp = blockIdx.y, nsplit = gridDim.y;
  const T* x = logits + (int64_t)row * stride;
  const RowProc rp = row_proc<PROC>(proc, mask_tab, mask_ld, counts, cnt_ld, bias_tab, bias_ld,
                                    REP ? rep_tab : nullptr, row);
  if (PROC && rp.mode == 2) {  // forced token (a fixed piece of a tool-call grammar): every split returns, no ticket
    if (sp == 0 && threadIdx.x == 0) emit_token<PROC>(out_tokens, row, rp.arg, V, rp);
    return;
  }
  if constexpr (PROC) {
    if (rp.nb > 0) {  // rp is the row's, so the branch and its barrier are uniform; every split stages the same pairs
      int* sb = bias_lds<PROC>();
      if ((int)threadIdx.x < rp.nb) {
        sb[threadIdx.x] = rp.bias[threadIdx.x];
        sb[LOGIT_BIAS_MAX + threadIdx.x] = rp.bias[LOGIT_BIAS_MAX + threadIdx.x];
      }
      __syncthreads();
    }
  }
  if constexpr (PROC && REP) {
    if (rp.rep) {  // (uniform: the row's)
      sample_row<T, true, true>(x, V, temperature, top_p, top_k, seeds, step_ptr, out_tokens, max_rounds, ws, rp, row,
                                sp, nsplit, sv, si, red);
      return;
    }
  }
  sample_row<T, PROC, false>(x, V, temperature, top_p, top_k, seeds, step_ptr, out_tokens, max_rounds, ws, rp, row, sp,
                             nsplit, sv, si, red);
}

// ws (optional): int32 workspace of >= SAMPLE_MAX_ROWS + 2 * B * nsplit entries whose first SAMPLE_MAX_ROWS are zero
// (tickets, re-armed by the kernel); without it every row is one workgroup. proc (optional, int32 [B, 8], see
// RowProc) selects the logits-processing instantiation; mask_tab uint32 [rows, mask_ld] and counts int32
// [slots, cnt_ld] (cnt_ld >= V rounded up to 8) are only read for rows that name them; bias_tab int32 [rows, bias_ld]
// (kafka_abi.h) likewise — without it the kernel biases no row, whatever proc[6] says. rep_tab (optional, fp32
// [slots, 2], as many rows as counts): the slots' repetition penalties (r, 1 / r); without it no row is multiplied.
extern "C" hipError_t kafka_launch_sample(const void* logits, bool is_bf16, int64_t stride, int B, int V, const float* temperature,
                         const float* top_p, const int* top_k, const int64_t* seeds, const int64_t* step,
                         int64_t* out_tokens, int* ws, int nsplit, const int* proc, const uint32_t* mask_tab,
                         int64_t mask_ld, int* counts, int64_t cnt_ld, const int* bias_tab, int64_t bias_ld,
                         const float* rep_tab, hipStream_t st) {
  if (B == 0) return hipSuccess;
  if (ws == nullptr || nsplit < 1) nsplit = 1;
  if (B > SAMPLE_MAX_ROWS || nsplit > 64) return hipErrorInvalidValue;
  if (proc != nullptr && (mask_ld * 32 < V || (counts != nullptr && cnt_ld < ((V + 7) & ~7))))
    return hipErrorInvalidValue;
  if (proc != nullptr && bias_tab != nullptr && bias_ld < 2 * LOGIT_BIAS_MAX) return hipErrorInvalidValue;
  const dim3 grid(B, nsplit);
#define KAFKA_SAMPLE(T_, P_, R_)                                                                                     \
  sample_kernel<T_, P_, R_><<<grid, SNT, 0, st>>>(reinterpret_cast<const T_*>(logits), stride, V, temperature, top_p, \
                                                  top_k, seeds, step, out_tokens, 32, ws, proc, mask_tab, mask_ld,   \
                                                  counts, cnt_ld, bias_tab, bias_ld, rep_tab)
  const bool rep = proc != nullptr && counts != nullptr && rep_tab != nullptr;
  if (is_bf16) {
    if (rep) KAFKA_SAMPLE(bf16, true, true);
    else if (proc) KAFKA_SAMPLE(bf16, true, false);
    else KAFKA_SAMPLE(bf16, false, false);
  } else {
    if (rep) KAFKA_SAMPLE(float, true, true);
    else if (proc) KAFKA_SAMPLE(float, true, false);
    else KAFKA_SAMPLE(float, false, false);
  }
#undef KAFKA_SAMPLE
  return hipGetLastError();
}

}  // namespace kafka
