"""Paged attention against inputs whose right answer is known key by key (ops/csrc/attention.hip, attn_tile.hip).

randn Q/K/V and an absolute 0.02 cannot see one wrong key in a long row (the output of L keys shrinks like 1/sqrt(L)).
Two constructions can:

* census (fp32 partials + lse): Q = 0, so every unmasked score is 0, every P is 1 and every rescale factor is 1. V is a
  small-integer signature of where the key lives (logical position bits, their complements, physical page bits, slot
  one-hot, pseudo-random integers in [-2, 2] keyed by position and head: exact in bf16 and in e4m3 with its power-of-two
  exponent), K stays randn and must not matter. Over n attended keys O * n is the integer sum of their signatures
  (int64 prefix sums, no CPU attention) and lse2 = log2 n:
    |O n - sum| <= 0.25  (sums < 2^24 are exact in the fp32 accumulators, the one normalisation costs a few ulp of at
                          most 3.3e4 < 0.01, and any missing / extra / substituted key moves some dimension by >= 1)
    |lse2 - log2 n| <= log2((n + 1) / n) / 3   (a third of the one-key step; 1.5e-5 at n = 32.8k, fp32 ulp there 1e-6)
    an empty range gives lse2 = -inf.
  Everything outside the attended keys (stale slots, the poison page behind every row's table) holds V = 1024.
* needle (bf16 ``out`` paths): K randn, the query of a probe is alpha K[p] (alpha = 3: ~34 nats over a N(0, 3)
  background), so the output is V[p]: |out - V[p]| <= 2^-8 |V[p]| (one bf16 ulp) + the leak |ref - V[p]| the fp32
  reference shows on that probe (asserted <= 1e-3 on the CPU). Next to every bound sits a poison key just outside it:
  key vector 1.5 x the needle's (it outscores the needle), V = 1024 where the key belongs to nobody. In the causal
  prefill a token's poison is the next token's needle: positions of one parity (per KV head) hold 1.5 x the key below
  them and are probed with alpha = 3 / 1.5^2, so both roles score as above; two worlds of opposite parity give every
  token but a sequence's last its poison in every KV head.

The CPU tests (unmarked) run every construction through the reference path of ``ops`` and show that the checks catch
hi -+ 1, lo -+ 1, q_limit -+ 1, a duplicated block-table entry and a masked 32-key block.
"""
import functools
import math
from types import SimpleNamespace

import pytest
import torch

from kafka_llm_service_amd import ops
from kafka_llm_service_amd.ops import reference as ref

D, PAGE = 128, 16
SCALE = 1 / math.sqrt(D)
POISON_V = 1024.0                      # exact in bf16 and e4m3
CPU = torch.device("cpu")
BIG = 1 << 30
VT = torch.tensor([ref.vt_pos(o) for o in range(PAGE)])
HEADS = [(32, 8), (8, 1)]
DEC_MAXPG = MAX_STAGED_PAGES = 2048    # csrc/attention.hip, csrc/attn_tile.hip (MAXPG)
LDS_PAGE_VARIANTS = (0, 1, 3)          # prefill variants that stage page ids in LDS (launch_prefill, attn_tile.hip)


# ---------------------------------------------------------------------------------------------------- paged worlds
def _tables(lens, seed, width=None):
    """Shuffled pages for rows of ``lens`` keys; every table entry past a row's pages names the poison page."""
    g = torch.Generator().manual_seed(seed)
    npg = [-(-l // PAGE) for l in lens]
    total = sum(npg) + 3
    perm = torch.randperm(total, generator=g)
    poison = int(perm[0])
    bt = torch.full((len(lens), (max(npg) + 3) if width is None else width), poison, dtype=torch.int32)
    c = 1
    for b, n in enumerate(npg):
        bt[b, :n] = perm[c:c + n].int()
        c += n
    return bt, poison, total, g


def _pack(kn, vn, fp8):
    """Natural-order K, V [n, Hkv, 16, D] -> the caches in the kernels' page layout."""
    if fp8:
        return ref.fp8_pack_pages(kn, vn)
    n, hkv = kn.shape[:2]
    k = kn.reshape(n, hkv, PAGE, D // 8, 8).permute(0, 1, 3, 2, 4).reshape(n, hkv, PAGE, D).contiguous()
    v = torch.empty(n, hkv, D, PAGE)
    v[..., VT] = vn.transpose(2, 3)
    return k.to(torch.bfloat16), v.to(torch.bfloat16)


def _signature(pos, page, Hkv):
    """int64 [n, Hkv, D]: where key ``pos`` (in physical page ``page``) lives, as small integers."""
    n, bit = pos.numel(), torch.arange(16)
    s = torch.zeros(n, Hkv, D, dtype=torch.int64)
    pb = (pos[:, None] >> bit) & 1
    s[:, :, 0:16] = pb[:, None]
    s[:, :, 16:32] = 1 - pb[:, None]
    s[:, :, 32:48] = ((page[:, None] >> bit) & 1)[:, None]
    s[:, :, 48:64] = torch.nn.functional.one_hot(pos % PAGE, PAGE)[:, None]
    x = pos[:, None, None] * 2654435761 + torch.arange(Hkv)[None, :, None] * 40503 + torch.arange(64)[None, None] * 97
    x = ((x & 0xFFFFFFFF) ^ (x >> 15)) * 2246822519 & 0xFFFFFFFF
    x = (x ^ (x >> 13)) * 3266489917 & 0xFFFFFFFF
    s[:, :, 64:] = (x ^ (x >> 16)) % 5 - 2
    return s


@functools.lru_cache(maxsize=None)
def _census_world(lens, Hkv, fp8, seed=0):
    bt, poison, nb, g = _tables(lens, seed)
    kn = torch.randn(nb, Hkv, PAGE, D, generator=g)
    vn = torch.full((nb, Hkv, PAGE, D), POISON_V)
    cs = []
    for b, L in enumerate(lens):
        pos = torch.arange(L)
        page = bt[b, pos // PAGE].long()
        sig = _signature(pos, page, Hkv)
        vn[page, :, pos % PAGE] = sig.float()
        c = torch.zeros(L + 1, Hkv, D, dtype=torch.int64)
        c[1:] = sig.cumsum(0)
        cs.append(c)
    k, v = _pack(kn, vn, fp8)
    return SimpleNamespace(k=k, v=v, bt=bt, lens=lens, Hkv=Hkv, cs=cs, poison=poison)


def _explain(d):
    """The signature difference (got - want) of one census sum, decoded."""
    cnt = (d[0:16] + d[16:32]).tolist()
    msg = f"keys extra(+)/missing(-) per position bit {cnt}; position-bit sums {d[0:16].tolist()}; page-bit sums " \
          f"{d[32:48].tolist()}; slot histogram {d[48:64].tolist()}"
    if len(set(cnt)) == 1 and abs(cnt[0]) == 1:
        p = sum(1 << i for i in range(16) if d[i] == cnt[0])
        pg = sum(1 << i for i in range(16) if d[32 + i] == cnt[0])
        msg = f"one key {'extra' if cnt[0] > 0 else 'missing'}: position {p}, page id {pg}, slot {p % PAGE}; " + msg
    return msg


def census_check(w, part, lse, entries, what=""):
    """``entries``: (row, slot, table row, lo, hi) -> part[row, :, slot] must be the census of keys [lo, hi) of that
    table row, for every head."""
    part = part.detach().to(CPU).double()
    lse = lse.detach().to(CPU).double().reshape(part.shape[:3])
    G = part.shape[1] // w.Hkv
    e = torch.tensor(entries, dtype=torch.long)
    rows, slots, tb = e[:, 0], e[:, 1], e[:, 2]
    empty = e[:, 4] <= e[:, 3]  # (an empty range may lie past the row's keys, e.g. kv_start > seq_len)
    lo, hi = e[:, 3].masked_fill(empty, 0), e[:, 4].masked_fill(empty, 0)
    want = torch.zeros(len(entries), w.Hkv, D, dtype=torch.int64)
    for b in tb.unique().tolist():
        m = tb == b
        want[m] = w.cs[b][hi[m]] - w.cs[b][lo[m]]
    want = want.repeat_interleave(G, dim=1).double()
    n = (hi - lo).double()[:, None]
    got, gl = part[rows, :, slots], lse[rows, :, slots]
    ok_o = ((got * n[..., None] - want).abs() <= 0.25).all(-1)
    n1 = n.clamp(min=1)
    ok_l = (gl - torch.log2(n1)).abs() <= torch.log2((n1 + 1) / n1) / 3
    ok = torch.where(n > 0, ok_o & ok_l, gl == float("-inf"))
    if not bool(ok.all()):
        i, hq = (~ok).nonzero()[0].tolist()
        # decoded with the key count the kernel itself reports (2^lse2), so one lost key reads as exactly that key
        n_got = torch.exp2(gl[i, hq]).nan_to_num(nan=0.0, posinf=0.0).round()
        d = (got[i, hq] * n_got - want[i, hq]).nan_to_num(nan=-9e6, posinf=9e6, neginf=-9e6).round().long()
        raise AssertionError(
            f"{what}: {int((~ok).sum())} of {ok.numel()} (entry, head) censuses wrong; first: row {int(rows[i])} slot "
            f"{int(slots[i])} head {hq} keys [{int(lo[i])}, {int(hi[i])}) of table row {int(tb[i])}: lse2 "
            f"{gl[i, hq].item():.7f} want {math.log2(n[i, 0].item()) if n[i, 0] > 0 else float('-inf'):.7f}, "
            f"max |O n - sum| {(got[i, hq] * n[i, 0] - want[i, hq]).abs().max().item():.3f}; {_explain(d)}")


def needle_check(out, ref_out, vp, what=""):
    """|out - V[p]| <= 2^-8 |V[p]| + the reference's own leak on that probe; out / ref_out / vp [..., D]."""
    out, ref_out, vp = out.detach().to(CPU).double(), ref_out.double(), vp.double()
    leak = (ref_out - vp).abs().amax(-1, keepdim=True)
    ok = ((out - vp).abs() <= 2.0 ** -8 * vp.abs() + leak).all(-1)
    if not bool(ok.all()):
        idx = (~ok).nonzero()[0].tolist()
        err = (out - vp)[tuple(idx)]
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.numel()} probes off their needle; first (row/token, "
                             f"head) {idx}: max |out - V[p]| {err.abs().max().item():.4f} (out max "
                             f"{out[tuple(idx)].abs().max().item():.1f}; ~{POISON_V:.0f} = a poison key was attended), "
                             f"reference leak {leak[tuple(idx)].item():.2e}")


# ---------------------------------------------------------------------------------------------------- census: decode
PAIRS = [(0, 1), (0, 16), (15, 17), (31, 33), (32, 64), (33, 63), (5, 5), (0, 47), (100, 257), (37, 1000),
         (1024, 2049)]
UNI_LENS = (1, 15, 16, 17, 32, 33, 63, 65, 257, 1000, 2049)
UNI_STARTS = [0, 5, 16, 31, 32, 33, 0, 64, 100, 999, 2048]


def _decode_partials(w, Hq, items, S_total, dev):
    B = len(w.lens)
    q = torch.zeros(B, Hq, D, dtype=torch.bfloat16, device=dev)
    part = torch.full((B, Hq, S_total, D), float("nan"), device=dev)
    lse = torch.full((B, Hq, S_total), float("nan"), device=dev)
    ops.attn_decode_items(q, w.k.to(dev), w.v.to(dev), w.bt.to(dev), items.to(dev), part, lse, SCALE)
    return part, lse


def _pair_items(pairs, row=1):
    """One item per (lo, hi) on table row ``row``, each with a slot of its own, and one whole-row item on row 0."""
    it = [[row, lo, hi, s, len(pairs), 0, 0, 0] for s, (lo, hi) in enumerate(pairs)] + [[0, 0, 100, 0, 1, 0, 0, 0]]
    return torch.tensor(it, dtype=torch.int32), [(r[0], r[3] + r[5], r[0], r[1], r[2]) for r in it]


def _census_decode_items(dev, Hq, Hkv, fp8, pairs=PAIRS):
    w = _census_world((100, 2060), Hkv, fp8)
    items, entries = _pair_items(pairs)
    part, lse = _decode_partials(w, Hq, items, len(pairs), dev)
    census_check(w, part, lse, entries, f"decode items fp8={fp8}")


def _census_decode_uniform(dev, Hq, Hkv, fp8, S, starts):
    w = _census_world(UNI_LENS, Hkv, fp8, seed=1)
    B = len(UNI_LENS)
    sl = torch.tensor(UNI_LENS, dtype=torch.int32)
    ks = torch.tensor(starts, dtype=torch.int32) if starts is not None else None
    items = ops.uniform_decode_items(sl, ks, S, 0).tolist()
    for b in range(B):  # the planner's pieces tile [kv_start, len) in order, without gaps
        at = min(starts[b] if starts is not None else 0, UNI_LENS[b])
        for r in (r for r in items if r[0] == b and r[2] > r[1]):
            assert r[1] == at, (b, items)
            at = r[2]
        assert at == UNI_LENS[b], (b, items)
    q = torch.zeros(B, Hq, D, dtype=torch.bfloat16, device=dev)
    part = torch.full((B, Hq, S, D), float("nan"), device=dev)
    lse = torch.full((B, Hq, S), float("nan"), device=dev)
    ops.attn_decode(q, w.k.to(dev), w.v.to(dev), w.bt.to(dev), sl.to(dev), ks.to(dev) if ks is not None else None,
                    part, lse, S, 0, SCALE)
    census_check(w, part, lse, [(r[0], r[3], r[0], r[1], r[2]) for r in items],
                 f"uniform decode S={S} kv_start={'set' if starts else None} fp8={fp8}")


@pytest.mark.gpu
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_census_decode_items(cuda, Hq, Hkv, fp8):
    _census_decode_items(cuda, Hq, Hkv, fp8)


@pytest.mark.gpu
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_census_decode_uniform_splits(cuda, Hq, Hkv, fp8):
    for S in (1, 3, 8):
        for starts in (None, UNI_STARTS):
            _census_decode_uniform(cuda, Hq, Hkv, fp8, S, starts)


# One row of 2049 * 16 + 5 keys, Hq = 2, Hkv = 1 (~2,053 pages, 16 MB in bf16). A piece stages the page ids of
# [lo & ~31, hi) in LDS when they are at most DEC_MAXPG, else it reads the block table from global memory.
LIMIT_LEN = (DEC_MAXPG + 1) * PAGE + 5
LIMIT_PAIRS = [(0, DEC_MAXPG * PAGE),      # pages 0 .. 2047: exactly DEC_MAXPG, the last LDS-staged size
               (37, LIMIT_LEN),            # pages 2 .. 2049: DEC_MAXPG again, from an unaligned start, to a ragged end
               (5, LIMIT_LEN),             # pages 0 .. 2049: DEC_MAXPG + 2 -> the global-table path
               (32, LIMIT_LEN + 0),        # pages 2 .. 2049 (staged) next to ...
               (31, LIMIT_LEN)]            # ... pages 0 .. 2049 (global): one key moves the piece across the limit


def _staged(lo, hi):
    return ((hi - 1) >> 4) - ((lo & ~31) >> 4) + 1 <= DEC_MAXPG


@pytest.mark.gpu
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_census_decode_page_staging_limit(cuda, fp8):
    assert [_staged(*p) for p in LIMIT_PAIRS] == [True, True, False, True, False]
    w = _census_world((100, LIMIT_LEN), 1, fp8, seed=2)
    items, entries = _pair_items(LIMIT_PAIRS)
    part, lse = _decode_partials(w, 2, items, len(LIMIT_PAIRS), cuda)
    census_check(w, part, lse, entries, f"decode staging limit fp8={fp8}")


# --------------------------------------------------------------------------------------------------- census: prefill
CTX, NEW = (0, 37, 512, 700), (70, 1, 33, 40)   # the causal test's sequences + 700 keys of context under 40 tokens
CHUNKS = [(0, BIG), (0, 45), (45, 300), (300, BIG)]  # slot 0: the whole range; slots 1..3: unaligned key chunks


def _prefill_items(G, variant, ranges, ctx=CTX, new=NEW, shift=0):
    """Items, per-token q_limit (+ ``shift``) and census entries: every token of every sequence over every range
    (slot = index in ``ranges``), tiles of the variant's size."""
    tile = ops.tile_rows(variant) // G
    items, entries, lim, t0 = [], [], [], 0
    for b, (c, n) in enumerate(zip(ctx, new)):
        lim += [c + i + shift for i in range(n)]
        for s, (lo, hi) in enumerate(ranges):
            hi = min(hi, c + n)
            if lo >= hi:
                continue
            items += [[t0 + st, min(tile, n - st), b, lo, hi, s, 0, 0] for st in range(0, n, tile)]
            entries += [(t0 + i, s, b, lo, min(hi, c + i + 1)) for i in range(n)]
        t0 += n
    return torch.tensor(items, dtype=torch.int32), torch.tensor(lim, dtype=torch.int32), entries


def _census_prefill(dev, Hq, Hkv, fp8, variant, shift=0):
    w = _census_world(tuple(c + n for c, n in zip(CTX, NEW)), Hkv, fp8, seed=3)
    items, lim, entries = _prefill_items(Hq // Hkv, variant, CHUNKS, shift=shift)
    T = sum(NEW)
    q = torch.zeros(T, Hq, D, dtype=torch.bfloat16, device=dev)
    part = torch.full((T, Hq, len(CHUNKS), D), float("nan"), device=dev)
    lse = torch.full((T, Hq, len(CHUNKS)), float("nan"), device=dev)
    ops.attn_prefill(items.to(dev), q, w.k.to(dev), w.v.to(dev), w.bt.to(dev), lim.to(dev), SCALE, out_part=part,
                     lse_part=lse, variant=variant)
    census_check(w, part, lse, entries, f"prefill variant {variant} fp8={fp8}")


VARIANTS = [(0, False), (1, False), (2, False), (3, False), (0, True), (1, True), (2, True)]
VARIANT_IDS = [f"v{v}-{'fp8' if f else 'bf16'}" for v, f in VARIANTS]


@pytest.mark.gpu
@pytest.mark.parametrize("variant,fp8", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_census_prefill(cuda, Hq, Hkv, variant, fp8):
    _census_prefill(cuda, Hq, Hkv, fp8, variant)


@pytest.mark.gpu
@pytest.mark.parametrize("variant,fp8", VARIANTS, ids=VARIANT_IDS)
def test_census_prefill_staged_pages_limit(cuda, variant, fp8):
    """A 1-token item over exactly MAX_STAGED_PAGES pages passes the census; one page more gives NaN (lse and rows) on
    the variants that stage page ids in LDS, as their comments promise, and is an ordinary item on variant 2. Every
    table entry is a valid page, so nothing is read out of bounds either way."""
    w = _census_world((100, LIMIT_LEN), 1, fp8, seed=2)
    n0, n1 = MAX_STAGED_PAGES * PAGE, (MAX_STAGED_PAGES + 1) * PAGE
    items = torch.tensor([[0, 1, 1, 0, n0, 0, 0, 0], [0, 1, 1, 0, n1, 1, 0, 0]], dtype=torch.int32, device=cuda)
    q = torch.zeros(1, 2, D, dtype=torch.bfloat16, device=cuda)
    part = torch.zeros(1, 2, 2, D, device=cuda)
    lse = torch.zeros(1, 2, 2, device=cuda)
    lim = torch.full((1,), BIG, dtype=torch.int32, device=cuda)
    ops.attn_prefill(items, q, w.k.to(cuda), w.v.to(cuda), w.bt.to(cuda), lim, SCALE, out_part=part, lse_part=lse,
                     variant=variant)
    census_check(w, part, lse, [(0, 0, 1, 0, n0)], f"variant {variant}: {MAX_STAGED_PAGES} pages")
    if variant in LDS_PAGE_VARIANTS:
        assert torch.isnan(lse[0, :, 1]).all() and torch.isnan(part[0, :, 1]).all(), \
            f"variant {variant}: an item past MAX_STAGED_PAGES must give NaN, got lse {lse[0, :, 1].tolist()}"
    else:
        census_check(w, part, lse, [(0, 1, 1, 0, n1)], f"variant {variant}: {MAX_STAGED_PAGES + 1} pages")


# ---------------------------------------------------------------------------------------------------- needle worlds
def _fill_rows(lens, Hkv, fp8, seed, build):
    """Caches of rows built by ``build(b, L, alloc, r) -> (K, V) [alloc, Hkv, D]`` in natural order (r: randn directions
    of that shape; alloc = the row's pages x 16, so the stale slots of the last page are the builder's too). The poison page
    holds, slot by slot, 1.5 x the last key of row slot % B and V = 1024. -> world with the caches as stored (``kf`` /
    ``vf`` [alloc, Hkv, D] per row, dequantised)."""
    bt, poison, nb, g = _tables(lens, seed)
    kn = torch.randn(nb, Hkv, PAGE, D, generator=g)
    vn = torch.full((nb, Hkv, PAGE, D), POISON_V)
    for b, L in enumerate(lens):
        alloc = -(-L // PAGE) * PAGE
        r = torch.randn(alloc, Hkv, D, generator=g)
        # |r|^2 = D for every key: a needle scores 3 sqrt(D) = 33.9 nats and its poison half as much again, whatever
        # the draw (chi^2 tails of |r|^2 would let the odd probe leak more than the condition allows)
        K, V = build(b, L, alloc, r * (math.sqrt(D) / r.norm(dim=-1, keepdim=True)))
        x = torch.arange(alloc)
        kn[bt[b, x // PAGE].long(), :, x % PAGE] = K
        vn[bt[b, x // PAGE].long(), :, x % PAGE] = V
        kn[poison, :, b::len(lens)] = 1.5 * K[L - 1][:, None]
    k, v = _pack(kn, vn, fp8)
    kf, vf = zip(*(ref.gather_kv(k, v, bt[b], -(-L // PAGE) * PAGE) for b, L in enumerate(lens)))
    return SimpleNamespace(k=k, v=v, bt=bt, lens=lens, Hkv=Hkv, kf=kf, vf=vf, poison=poison)


# decode rows: (keys, prefix chunks, suffix pieces). A key between two ranges belongs to nobody: it holds 1.5 x the
# keys either side of it and V = 1024, as do the keys below the first range's lo and the stale slots past the row.
DEC_ROWS = [(45, [], [(0, 45)]),
            (300, [], [(21, 300)]),
            (517, [], [(5, 130), (131, 517)]),
            (2049, [], [(0, 33), (34, 64), (65, 1000), (1001, 1024), (1025, 2049)]),
            (420, [(0, 200)], [(201, 420)]),
            (900, [(0, 45), (46, 300), (301, 512)], [(512, 700), (701, 900)])]


@functools.lru_cache(maxsize=None)
def _decode_needle_world(Hkv, fp8, rows=tuple((r[0], tuple(r[1]), tuple(r[2])) for r in DEC_ROWS)):
    def build(b, L, alloc, r):
        att = torch.zeros(alloc + 1, dtype=torch.bool)
        for lo, hi in rows[b][1] + rows[b][2]:
            att[lo:hi] = True
        K, V = r.clone(), torch.randn(r.shape, generator=torch.Generator().manual_seed(100 + b))
        for x in range(alloc):
            if att[x]:
                continue
            V[x] = POISON_V
            if x >= L:
                K[x] = 1.5 * r[L - 1]
            elif (x and att[x - 1]) or att[x + 1]:
                K[x] = 1.5 * ((r[x - 1] if x and att[x - 1] else 0) + (r[x + 1] if att[x + 1] else 0))
        return K, V

    w = _fill_rows(tuple(r[0] for r in rows), Hkv, fp8, 5, build)
    w.rows = rows
    # needles: the first and last key of every piece and prefix chunk (the keys either side of kv_start and the last
    # key of the row among them)
    w.needles = [sorted({p for lo, hi in pre + suf for p in (lo, hi - 1)}) for _, pre, suf in rows]
    w.pre_items = torch.tensor([[b, 1, b, lo, hi, c, 0, 0] for b, (_, pre, _) in enumerate(rows)
                                for c, (lo, hi) in enumerate(pre)], dtype=torch.int32)
    w.dec_items = torch.tensor([[b, lo, hi, s, len(suf), len(pre), 0, 0] for b, (_, pre, suf) in enumerate(rows)
                                for s, (lo, hi) in enumerate(suf)], dtype=torch.int32)
    w.S_total = max(len(pre) + len(suf) for _, pre, suf in rows)
    return w


def _decode_probes(w, Hq, launch):
    """q [B, Hq, D] and V[p] [B, Hq, D]: head hq of row b probes needle (hq + b + launch * Hq) of the row's list."""
    B, G = len(w.lens), Hq // w.Hkv
    q, vp = torch.empty(B, Hq, D), torch.empty(B, Hq, D)
    for b in range(B):
        for hq in range(Hq):
            p = w.needles[b][(hq + b + launch * Hq) % len(w.needles[b])]
            q[b, hq] = 3 * w.kf[b][p, hq // G]
            vp[b, hq] = w.vf[b][p, hq // G]
    return q.to(torch.bfloat16), vp


def _decode_needle_run(w, q, dev, pre_bf16, variant, out_dtype, pre_items=None, dec_items=None, bt=None):
    B, Hq = q.shape[:2]
    part = torch.zeros(B, Hq, w.S_total, D, device=dev)
    lse = torch.full((B, Hq, w.S_total), float("-inf"), device=dev)
    pre = torch.zeros(B, Hq, w.S_total, D, dtype=torch.bfloat16, device=dev) if pre_bf16 else None
    k, v, q = w.k.to(dev), w.v.to(dev), q.to(dev)
    bt = (w.bt if bt is None else bt).to(dev)
    lim = torch.full((B,), BIG, dtype=torch.int32, device=dev)
    ops.attn_prefill((w.pre_items if pre_items is None else pre_items).to(dev), q, k, v, bt, lim, SCALE,
                     out_part=pre if pre_bf16 else part, lse_part=lse, variant=variant)
    out = torch.full((B, Hq, D), float("nan"), dtype=out_dtype, device=dev)
    ops.attn_decode_items(q, k, v, bt, (w.dec_items if dec_items is None else dec_items).to(dev), part, lse, SCALE,
                          out=out, pre_part=pre)
    return out


DEC_NEEDLE_CASES = [("f32", 0, False), ("bf16", 3, False), ("f32", 0, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("pre,variant,fp8", DEC_NEEDLE_CASES, ids=["pre-f32", "pre-bf16-v3", "pre-f32-fp8"])
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_needle_decode_fused_merge(cuda, Hq, Hkv, pre, variant, fp8):
    """One-piece rows, rows of 2 and 5 pieces (ticket merge) and rows with 1 and 3 prefix partials, in one launch;
    three launches (the counters re-arm), each probing the next needles of every row."""
    w = _decode_needle_world(Hkv, fp8)
    for launch in range(3):
        q, vp = _decode_probes(w, Hq, launch)
        o_ref = _decode_needle_run(w, q, CPU, pre == "bf16", variant, torch.float32)
        out = _decode_needle_run(w, q, cuda, pre == "bf16", variant, torch.bfloat16)
        needle_check(out, o_ref, vp, f"decode needle launch {launch}")


@functools.lru_cache(maxsize=None)
def _prefill_needle_world(Hkv, fp8, flip):
    lens = tuple(c + n for c, n in zip(CTX, NEW))
    coef = []

    def build(b, L, alloc, r):
        K, V = r.clone(), torch.randn(r.shape, generator=torch.Generator().manual_seed(200 + b))
        x, h = torch.arange(alloc)[:, None], torch.arange(Hkv)[None]
        up = (x > CTX[b]) & (x < L) & ((x + h + flip) % 2 == 0)    # [alloc, Hkv]: holds 1.5 x the (plain) key below
        K[1:][up[1:]] = 1.5 * r[:-1][up[1:]]
        K[L:] = 1.5 * K[L - 1]
        V[L:] = POISON_V
        coef.append(torch.where(up, 1.5, 1.0))
        return K, V

    w = _fill_rows(lens, Hkv, fp8, 7, build)
    w.coef = coef
    return w


def _prefill_probes(w, Hq):
    """q [T, Hq, D] and V[p]: token i of sequence b probes its own position ctx + i (its q_limit) in every head."""
    G = Hq // w.Hkv
    qs, vs = [], []
    for b, (c, n) in enumerate(zip(CTX, NEW)):
        p = torch.arange(c, c + n)
        qs.append((3 / w.coef[b][p] ** 2)[..., None] * w.kf[b][p])
        vs.append(w.vf[b][p])
    f = lambda t: torch.cat(t).repeat_interleave(G, dim=1)
    return f(qs).to(torch.bfloat16), f(vs)


def _prefill_needle_run(w, q, dev, variant, out_dtype, shift=0):
    items, lim, _ = _prefill_items(q.shape[1] // w.Hkv, variant, [(0, BIG)], shift=shift)
    items[:, 5] = -1
    out = torch.full(q.shape, float("nan"), dtype=out_dtype, device=dev)
    ops.attn_prefill(items.to(dev), q.to(dev), w.k.to(dev), w.v.to(dev), w.bt.to(dev), lim.to(dev), SCALE, out=out,
                     variant=variant)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("variant,fp8", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_needle_prefill_causal(cuda, Hq, Hkv, variant, fp8):
    for flip in (0, 1):
        w = _prefill_needle_world(Hkv, fp8, flip)
        q, vp = _prefill_probes(w, Hq)
        o_ref = _prefill_needle_run(w, q, CPU, variant, torch.float32)
        out = _prefill_needle_run(w, q, cuda, variant, torch.bfloat16)
        needle_check(out, o_ref, vp, f"prefill needle variant {variant} fp8={fp8} parity {flip}")


# ---------------------------------------------------------------------------------------------------------- CPU tests
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_census_constructions_pass_on_the_reference(fp8):
    """The closed-form sums are what reference.py computes (the CPU path of ``ops``), on a reduced matrix."""
    _census_decode_items(CPU, 8, 1, fp8)
    _census_decode_uniform(CPU, 8, 1, fp8, 3, UNI_STARTS)
    _census_decode_uniform(CPU, 4, 2, fp8, 8, None)
    _census_prefill(CPU, 8, 1, fp8, 0)
    _census_prefill(CPU, 4, 2, fp8, 3)


def test_signature_values_are_exact_in_both_page_formats():
    w8, w16 = _census_world((100, 2060), 2, True), _census_world((100, 2060), 2, False)
    for w in (w8, w16):
        _, v = ref.gather_kv(w.k, w.v, w.bt[1], 2060)
        assert torch.equal(v.long().cumsum(0), w.cs[1][1:])
        _, v = ref.gather_kv(w.k, w.v, w.bt[0], 112)
        assert (v[100:] == POISON_V).all()  # the stale slots of the last page


def _raises(fn, *a, **kw):
    with pytest.raises(AssertionError):
        fn(*a, **kw)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_census_detects_mutants(fp8):
    Hq, Hkv = 8, 2
    w = _census_world((100, 2060), Hkv, fp8)
    pairs = [(37, 1000), (15, 17), (1024, 2049)]
    items, entries = _pair_items(pairs)
    census_check(w, *_decode_partials(w, Hq, items, 3, CPU), entries, "unmutated")
    for s in range(3):      # hi -+ 1 and lo -+ 1 of every item
        for col, d in ((1, -1), (1, 1), (2, -1), (2, 1)):
            m = items.clone()
            m[s, col] += d
            _raises(census_check, w, *_decode_partials(w, Hq, m, 3, CPU), entries)
    # one block-table entry duplicated over its neighbour (a page read twice, the next one never)
    for pg in (3, 40, 127):
        m = SimpleNamespace(**vars(w))
        m.bt = w.bt.clone()
        m.bt[1, pg + 1] = m.bt[1, pg]
        _raises(census_check, w, *_decode_partials(m, Hq, items, 3, CPU), entries)
    # one 32-key block masked out of (37, 1000): the merge of the pieces either side of it
    two, _ = _pair_items([(37, 512), (544, 1000)])
    part, lse = _decode_partials(w, Hq, two, 2, CPU)
    o, l = torch.empty(2, Hq, D), torch.empty(2, Hq)
    ref.attn_merge(part, lse, o, l)
    _raises(census_check, w, o[:, :, None], l[:, :, None], [(1, 0, 1, 37, 1000)])
    # q_limit -+ 1 on the prefill kernels' reference
    _census_prefill(CPU, Hq, Hkv, fp8, 0)
    for shift in (-1, 1):
        _raises(_census_prefill, CPU, Hq, Hkv, fp8, 0, shift=shift)


def _all_needle_inputs():
    """(what, V[p], fp32 reference output) of every probe input the GPU tests use."""
    for Hq, Hkv in HEADS:
        for pre, variant, fp8 in DEC_NEEDLE_CASES:
            w = _decode_needle_world(Hkv, fp8)
            for launch in range(3):
                q, vp = _decode_probes(w, Hq, launch)
                yield f"decode {Hq}/{Hkv} {pre} fp8={fp8} launch {launch}", vp, \
                    _decode_needle_run(w, q, CPU, pre == "bf16", variant, torch.float32)
        for fp8 in (False, True):
            for flip in (0, 1):
                w = _prefill_needle_world(Hkv, fp8, flip)
                q, vp = _prefill_probes(w, Hq)
                yield f"prefill {Hq}/{Hkv} fp8={fp8} parity {flip}", vp, \
                    _prefill_needle_run(w, q, CPU, 0, torch.float32)


def test_needle_leak_condition():
    """Every probe's reference output is its V[p] within 1e-3 (the condition the needle tolerance rests on), so every
    construction also passes its own check on the reference."""
    for what, vp, o_ref in _all_needle_inputs():
        leak = (o_ref - vp).abs().amax().item()
        assert leak <= 1e-3, f"{what}: reference leak {leak:.2e}"
        needle_check(o_ref, o_ref, vp, what)


def test_needle_detects_mutants():
    Hq, Hkv = 32, 8
    w = _decode_needle_world(Hkv, False)
    q, vp = _decode_probes(w, Hq, 0)
    good = _decode_needle_run(w, q, CPU, False, 0, torch.float32)
    needle_check(good, good, vp, "unmutated")
    row2 = [i for i, r in enumerate(w.dec_items.tolist()) if r[0] == 2]       # pieces (5, 130) and (131, 517)
    muts = [(row2[0], 1, -1), (row2[0], 1, 1), (row2[0], 2, -1), (row2[0], 2, 1),  # lo -+ 1, hi -+ 1 of a piece
            (row2[1], 1, -1), (row2[1], 2, 1),       # the gap key from above; a stale slot past the row's last key
            (row2[1], 1, 29)]                        # the rest of the needle's 32-key block masked out: (160, 517)
    for i, col, d in muts:
        m = w.dec_items.clone()
        m[i, col] += d
        _raises(needle_check, _decode_needle_run(w, q, CPU, False, 0, torch.float32, dec_items=m), good, vp)
    # prefix chunks of row 5: kv_hi + 1 attends the gap key, kv_hi - 1 drops the chunk's last needle
    pre5 = [i for i, r in enumerate(w.pre_items.tolist()) if r[0] == 5]
    for d in (-1, 1):
        m = w.pre_items.clone()
        m[pre5[0], 4] += d
        _raises(needle_check, _decode_needle_run(w, q, CPU, False, 0, torch.float32, pre_items=m), good, vp)
    # a needle's page replaced by its neighbour's
    bt = w.bt.clone()
    bt[2, 129 // PAGE] = bt[2, 129 // PAGE - 1]
    _raises(needle_check, _decode_needle_run(w, q, CPU, False, 0, torch.float32, bt=bt), good, vp)
    # q_limit -+ 1 in the causal prefill, both parities
    for flip in (0, 1):
        wp = _prefill_needle_world(Hkv, False, flip)
        qp, vpp = _prefill_probes(wp, Hq)
        goodp = _prefill_needle_run(wp, qp, CPU, 0, torch.float32)
        for shift in (-1, 1):
            _raises(needle_check, _prefill_needle_run(wp, qp, CPU, 0, torch.float32, shift=shift), goodp, vpp)
