// Per-token log-probabilities for gfx950: for every scored row of the logits, log softmax of the sampled token and the
// K (<= 20) most likely tokens, in ONE streaming read of the row (bf16 or fp32 logits, 16-byte loads).
//
// The scores are those of the RAW logits: no temperature, no penalties, no grammar mask — what the model assigned,
// not what the sampler drew from. Per row:
//   lse       = log sum_i exp(x_i)          fp32: max of the slice, then sum of exp(x - max), rescaled at the merge
//   tok_lp    = x[token] - lse
//   top_id[j] = the j-th entry in the order (value descending, index ascending) — `better()` of row_scan.h; bf16
//               logits over 128k entries tie all the time, so the rule is exact, not "some index of the j-th value"
//   top_lp[j] = x[top_id[j]] - lse;  slots past the row's length (V < K) hold id -1 and -inf
// A NaN entry counts as -inf everywhere (it never wins a comparison and adds nothing to the sum), so an id is
// always -1 or in [0, V) whatever the input.
//
// Launch: grid (R, nsplit), 1024 threads, like sample_kernel. A workgroup takes a slice of the row's 8-entry vectors
// (128,256 entries over 8 splits: two vectors = 16 entries per thread, held in registers; a slice that does not fit
// — one workgroup on a long row — re-reads its own entries, cached by then, instead). Selection never goes back to
// HBM: every thread keeps the best of its entries below a bound, each wave draws K winners from its 64 lanes (the
// winner's lane alone rescans its registers), and wave 0 merges the 16 sorted wave lists by their heads. With
// nsplit > 1 the workgroup publishes (max, sum, its K winners) and the last of a row's workgroups to take its ticket
// merges the nsplit sorted lists the same way (the ticket protocol of common.h).
#include "row_scan.h"

namespace kafka {

constexpr int LNT = 1024;
constexpr int LNW = LNT / 64;
constexpr int LP_KMAX = 20;
constexpr int LP_NV = 2;               // 8-entry vectors a thread holds in registers
constexpr int LP_MAX_ROWS = 8192;      // ws: tickets [LP_MAX_ROWS] | partials [R][nsplit][LP_PART]
constexpr int LP_MAX_SPLIT = 64;       // one lane per split in the merge
constexpr int LP_PART = 2 + 2 * LP_KMAX;  // (max bits, sum bits, K x (value bits, index))

__device__ __forceinline__ float no_nan(float v) { return v == v ? v : -INFINITY; }

// The entries this thread owns: vectors v0 + tid, v0 + tid + 1024, ... below v1 (in `reg` when REG, else re-read) and
// the tail entry `ti` (>= 0 for the first V % 8 threads of the row's last split).
template <typename T, bool REG, bool AL, typename F>
__device__ __forceinline__ void own_entries(const T* __restrict__ x, const float (&reg)[LP_NV][8], int v0, int v1,
                                            int ti, float tv, F&& f) {
  if constexpr (REG) {
#pragma unroll
    for (int k = 0; k < LP_NV; ++k) {
      const int vi = v0 + (int)threadIdx.x + k * LNT;
      if (vi < v1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) f(reg[k][j], vi * 8 + j);
      }
    }
  } else {
    scan_slice<LNT>(
        RowSlice{v0, v1, 0, 0},  // (the tail entry is in tv)
        [&](int i0, float (&v)[8]) {
          Vec8<T, AL>::load(x + i0, v);
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = no_nan(v[j]);
        },
        [&](int) { return 0.f; }, f);
  }
  if (ti >= 0) f(tv, ti);
}

template <typename T, bool REG, bool AL>
__device__ __forceinline__ Cand own_best(const T* __restrict__ x, const float (&reg)[LP_NV][8], int v0, int v1, int ti,
                                         float tv, Cand bound) {
  Cand best{-INFINITY, CAND_NONE};
  own_entries<T, REG, AL>(x, reg, v0, v1, ti, tv, [&](float v, int i) {
    const Cand c{v, i};
    if (cand_after(c, bound)) best = better(best, c);
  });
  return best;
}

// One wave: K winners of `n` sorted lists (list l = entries [l * K, l * K + K) of lv / li, n <= 64) by their heads;
// lane j returns winner j.
__device__ __forceinline__ Cand merge_heads(const float* lv, const int* li, int n, int K, int lane) {
  int pos = 0;
  Cand head{-INFINITY, CAND_NONE};
  if (lane < n) head = Cand{lv[lane * K], li[lane * K]};
  Cand mine{-INFINITY, CAND_NONE};
  for (int r = 0; r < K; ++r) {
    const Cand w = wave_best(head);
    if (lane == r) mine = w;
    if (lane < n && head.i == w.i && w.i != CAND_NONE) {
      ++pos;
      head = pos < K ? Cand{lv[lane * K + pos], li[lane * K + pos]} : Cand{-INFINITY, CAND_NONE};
    }
  }
  return mine;
}

template <typename T, bool REG, bool AL>
__global__ __launch_bounds__(LNT) void token_logprobs_kernel(const T* __restrict__ logits, int64_t stride, int V,
                                                              const int* __restrict__ rows,
                                                              const int64_t* __restrict__ tokens, int K,
                                                              float* __restrict__ tok_lp, float* __restrict__ top_lp,
                                                              int* __restrict__ top_id, int64_t ld,
                                                              int* __restrict__ ws) {
  __shared__ float red[LNW];
  __shared__ float lv[LP_MAX_SPLIT * LP_KMAX];
  __shared__ int li[LP_MAX_SPLIT * LP_KMAX];
  const int r = blockIdx.x, sp = blockIdx.y, nsplit = gridDim.y;
  const int row = rows ? rows[r] : r;
  const T* x = logits + (int64_t)row * stride;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const RowSlice sl = row_slice(V, sp, nsplit);
  const int v0 = sl.v0, v1 = sl.v1;
  const int ti = sl.t0 + tid < sl.t1 ? sl.t0 + tid : -1;
  const float tv = ti >= 0 ? no_nan((float)x[ti]) : -INFINITY;
  float reg[LP_NV][8];
  if constexpr (REG) {
#pragma unroll
    for (int k = 0; k < LP_NV; ++k) {
      const int vi = v0 + tid + k * LNT;
      if (vi < v1) {
        Vec8<T, AL>::load(x + (int64_t)vi * 8, reg[k]);
#pragma unroll
        for (int j = 0; j < 8; ++j) reg[k][j] = no_nan(reg[k][j]);
      }
    }
  }

  // (max, sum of exp(x - max)) of the slice
  float m = -INFINITY;
  own_entries<T, REG, AL>(x, reg, v0, v1, ti, tv, [&](float v, int) { m = fmaxf(m, v); });
  m = block_max<LNT>(m, red);
  const float ms = m == -INFINITY ? 0.f : m;  // an empty or all -inf slice sums to 0
  float s = 0.f;
  own_entries<T, REG, AL>(x, reg, v0, v1, ti, tv, [&](float v, int) { s += __expf(v - ms); });
  s = block_sum<LNT>(s, red);

  // K winners of the slice: per wave from its lanes' bests, then wave 0 over the 16 wave lists
  Cand mine{-INFINITY, CAND_NONE};
  if (K > 0) {
    Cand cur = own_best<T, REG, AL>(x, reg, v0, v1, ti, tv, Cand{INFINITY, -1});
    for (int j = 0; j < K; ++j) {
      const Cand w = wave_best(cur);
      if (lane == 0) {
        lv[wave * K + j] = w.v;
        li[wave * K + j] = w.i;
      }
      if (cur.i == w.i && w.i != CAND_NONE) cur = own_best<T, REG, AL>(x, reg, v0, v1, ti, tv, w);
    }
    __syncthreads();
    if (wave != 0) return;
    mine = merge_heads(lv, li, LNW, K, lane);
  } else if (wave != 0) {
    return;
  }

  float lse = ms + __logf(s);
  if (nsplit > 1) {
    // ws: tickets (zero, re-armed by the last arrival) | [R][nsplit][LP_PART]; the ticket protocol of common.h
    int* p0 = ws + LP_MAX_ROWS + (int64_t)r * nsplit * LP_PART;
    int* part = p0 + sp * LP_PART;
    if (lane == 0) {
      publish(part, __float_as_int(m));
      publish(part + 1, __float_as_int(s));
    }
    if (lane < K) {
      publish(part + 2 + 2 * lane, __float_as_int(mine.v));
      publish(part + 3 + 2 * lane, mine.i);
    }
    int last = 0;
    if (lane == 0) last = take_ticket(ws + r, nsplit);  // (its wait is the wave's: every lane's stores above)
    if (!__shfl(last, 0, 64)) return;
    float pm = -INFINITY, ps = 0.f;
    if (lane < nsplit) {
      pm = __int_as_float(peek(p0 + lane * LP_PART));
      ps = __int_as_float(peek(p0 + lane * LP_PART + 1));
    }
    const float gm = wave_max(pm);
    const float gms = gm == -INFINITY ? 0.f : gm;
    const float gs = wave_sum(lane < nsplit ? ps * __expf(pm - gms) : 0.f);
    lse = gms + __logf(gs);
    if (K > 0) {
      // the nsplit sorted lists into LDS (only this wave is left in the workgroup), then merged by their heads
      for (int e = lane; e < nsplit * K; e += 64) {
        const int* q = p0 + (e / K) * LP_PART + 2 + 2 * (e % K);
        lv[e] = __int_as_float(peek(q));
        li[e] = peek(q + 1);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      mine = merge_heads(lv, li, nsplit, K, lane);
    }
  }

  if (lane < K) {
    const bool ok = mine.i != CAND_NONE;
    top_id[(int64_t)r * ld + lane] = ok ? mine.i : -1;
    top_lp[(int64_t)r * ld + lane] = ok ? mine.v - lse : -INFINITY;
  }
  if (lane == 0) {
    const int64_t t = tokens[row];
    const float xv = (t >= 0 && t < V) ? no_nan((float)x[t]) : -INFINITY;
    tok_lp[(int64_t)r * ld] = xv - lse;
  }
}

// rows (optional): int32 [R] rows of `logits` to score (nullptr: rows 0..R-1); tokens: int64, indexed by logits row.
// Record r is written at tok_lp[r * ld], top_lp[r * ld + j], top_id[r * ld + j] (j < K): three views of one packed
// buffer, or three tensors of a common row stride. ws (optional): int32 workspace of >= LP_MAX_ROWS + R * nsplit *
// LP_PART entries whose first LP_MAX_ROWS are zero (tickets, re-armed by the kernel); without it, or for V < 16384,
// every row is one workgroup.
extern "C" hipError_t kafka_launch_token_logprobs(const void* logits, bool is_bf16, int64_t stride, int V,
                                                  const int* rows, int R, const int64_t* tokens, int K, float* tok_lp,
                                                  float* top_lp, int* top_id, int64_t ld, int* ws, int nsplit,
                                                  hipStream_t st) {
  if (R == 0) return hipSuccess;
  if (ws == nullptr || nsplit < 1 || V < 16384) nsplit = 1;
  if (V < 1 || K < 0 || K > LP_KMAX || R > LP_MAX_ROWS || nsplit > LP_MAX_SPLIT) return hipErrorInvalidValue;
  const int nvec = V >> 3;
  const bool reg = (nvec + nsplit - 1) / nsplit <= LP_NV * LNT;
  const dim3 grid(R, nsplit);
  const int64_t esz = is_bf16 ? 2 : 4;
  const bool al = reinterpret_cast<uintptr_t>(logits) % 16 == 0 && (stride * esz) % 16 == 0;
#define KAFKA_LOGPROBS(T_, R_, A_)                                                                                  \
  token_logprobs_kernel<T_, R_, A_><<<grid, LNT, 0, st>>>(reinterpret_cast<const T_*>(logits), stride, V, rows,    \
                                                          tokens, K, tok_lp, top_lp, top_id, ld, ws)
#define KAFKA_LOGPROBS_T(T_)                                          \
  do {                                                                \
    if (reg && al) KAFKA_LOGPROBS(T_, true, true);                    \
    else if (reg) KAFKA_LOGPROBS(T_, true, false);                    \
    else if (al) KAFKA_LOGPROBS(T_, false, true);                     \
    else KAFKA_LOGPROBS(T_, false, false);                            \
  } while (0)
  if (is_bf16) KAFKA_LOGPROBS_T(bf16); else KAFKA_LOGPROBS_T(float);
#undef KAFKA_LOGPROBS_T
#undef KAFKA_LOGPROBS
  return hipGetLastError();
}

}  // namespace kafka
