"""The host step planner (engine/step_plan.py) at production scale, on the CPU: a seeded corpus of steps — 18k-token
shared prefixes, 128 rows, 8k-token prompts, bursts of joined new turns, every planner setting both ways — driven
through ``ModelRunner.build_host`` on a stub runner (fake sequences, a fake KV manager), then

* a census of every plan: each query token's keys [0, limit] are covered exactly once by the items that name it,
  partial slots are distinct and in range, rows with partials are merged exactly once;
* the packed buffers' layout: the named sections tile them, ``views`` hands out exactly those sections and the TP
  wire format reproduces them.
"""
import ast
import copy
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from kafka_llm_service_amd.engine import model_runner as mr
from kafka_llm_service_amd.engine import step_plan as sp

PAGE = 16
MAX_BLOCKS = 4096


# ---- the corpus ---------------------------------------------------------------------------------------------------
class FakeSeq:
    def __init__(self, seq_id: int, total_len: int, pages: np.ndarray, pending: bool = False):
        self.seq_id, self.total_len, self.pages, self.pending = seq_id, total_len, pages, pending

    def token_at(self, p: int) -> int:
        return -1 if self.pending and p == self.total_len - 1 else (self.seq_id * 7919 + p * 31) % 50000

    def tokens_range(self, a: int, b: int) -> np.ndarray:
        return (self.seq_id * 7919 + np.arange(a, b) * 31) % 50000


class FakeKVM:
    """Block tables and slots straight from the sequences' page lists."""

    def __init__(self, seqs):
        self.pages = {s.seq_id: s.pages for s in seqs}

    def fill_block_tables(self, seq_ids, bt: np.ndarray) -> None:
        for r, i in enumerate(seq_ids):
            n = min(len(self.pages[i]), bt.shape[1])
            bt[r, :n] = self.pages[i][:n]

    def fill_slots(self, seq_id: int, a: int, b: int, slots: np.ndarray, r: int) -> None:
        pos = np.arange(a, b)
        slots[r:r + b - a] = self.pages[seq_id][pos // PAGE].astype(np.int64) * PAGE + pos % PAGE


class _Builder:
    def __init__(self, rng):
        self.rng, self.next_page, self.next_id, self.seqs = rng, 1, 1, []

    def fresh(self, n: int) -> np.ndarray:
        p = np.arange(self.next_page, self.next_page + n, dtype=np.int32)
        self.next_page += n
        return p

    def seq(self, total_len: int, head: np.ndarray = None, pending: bool = False) -> FakeSeq:
        """A sequence of ``total_len`` tokens whose block table starts with the pages ``head``."""
        head = np.zeros(0, np.int32) if head is None else head
        need = -(-total_len // PAGE)
        pages = np.concatenate([head[:need], self.fresh(max(0, need - len(head)))])
        s = FakeSeq(self.next_id, total_len, pages, pending)
        self.next_id += 1
        self.seqs.append(s)
        return s


def _pick(rng, fixed, lo, hi):
    return int(rng.choice(fixed)) if rng.random() < 0.6 else int(rng.integers(lo, hi + 1))


def make_case(seed: int) -> SimpleNamespace:
    """One step: planner settings + a batch (decode rows in 0..3 prefix groups and loose, prefill chunks)."""
    rng = np.random.default_rng(seed)
    flag = lambda p=0.5: bool(rng.random() < p)  # noqa: E731
    st = SimpleNamespace(hkv=8, tile=int(rng.choice([64, 32])), joins=flag(), join_suffix=flag(), fixed=flag(),
                         graphs=flag(), cascade=flag(0.8), pad=flag(), min_prefix=int(rng.choice([512, 512, 256, 1024])),
                         target_wgs=256, prefill_kv_chunk=int(rng.choice([1024, 256, 64])))
    b = _Builder(rng)
    kind = rng.choice(["decode", "mixed", "prefill"], p=[0.4, 0.45, 0.15])
    decode, prefixes = [], []
    if kind != "prefill":
        B = _pick(rng, [1, 2, 3, 8, 17, 64, 128], 1, 128)
        for g in range(int(rng.integers(0, 4)) if B >= 2 else 0):
            # prefixes from 512 tokens to past MAX_PREFIX_CHUNKS x the chunk and near MAX_ITEM_KEYS
            pp = _pick(rng, [512, 1024, 4096, 8208, 18000, 18432, 31008, 31984, 32992], 512, 33000) // PAGE
            if g and flag(0.4):  # shares only its first pages (fewer than any min_prefix) with the group before
                k = int(rng.integers(1, 256 // PAGE))
                prefixes.append(np.concatenate([prefixes[-1][:k], b.fresh(pp - k)]))
            else:
                prefixes.append(b.fresh(pp))
        for _ in range(B):
            g = int(rng.integers(-1, len(prefixes))) if prefixes else -1
            pending = flag(0.2)
            if g < 0:
                n = int(np.exp(rng.uniform(0, np.log(40000))))
                decode.append(b.seq(max(1, min(40000, n)), pending=pending))
            elif flag(0.1):  # starts with the group's pages but is too short to share the prefix
                decode.append(b.seq(int(rng.integers(1, st.min_prefix)), prefixes[g], pending))
            else:
                P = len(prefixes[g]) * PAGE
                sfx = _pick(rng, [1, 2, 16, 17, 40, 300, 2000, 7000], 1, 7000)
                decode.append(b.seq(min(40000, P + sfx), prefixes[g], pending))
    prefill = []
    if kind != "decode":
        for _ in range(int(rng.integers(1, 4))):
            what = rng.choice(["cold", "chunk", "joined", "turn", "burst"])
            head = prefixes[int(rng.integers(0, len(prefixes)))] if prefixes and what in ("joined", "burst") else None
            P = 0 if head is None else len(head) * PAGE
            if what == "cold":
                n = _pick(rng, [1, 7, 64, 65, 300, 2048, 8192], 1, 8192)
                prefill.append((b.seq(n), 0, n))
            elif what == "chunk":  # a piece of a long prompt: not its first tokens and / or not its last
                a = int(rng.choice([0, 512, 2048, 4100]))
                n = _pick(rng, [512, 2048], 1, 4096)
                prefill.append((b.seq(a + n + int(rng.choice([0, 1, 700]))), a, a + n))
            else:
                for _ in range(8 if what == "burst" else 1):
                    hist = int(rng.choice([0, 16, 48, 500, 2000])) if head is not None else int(rng.integers(100, 20000))
                    n = int(rng.integers(5, 61)) if what == "burst" else _pick(rng, [1, 30, 64, 100, 300], 1, 300)
                    prefill.append((b.seq(P + hist + n, head), P + hist, P + hist + n))
    return SimpleNamespace(seed=seed, settings=st, seqs=b.seqs,
                           batch=SimpleNamespace(decode=decode, prefill=prefill))


def stub_runner(module, case):
    """A ``module.ModelRunner`` with only what ``build_host`` and ``views`` read (no model, no device)."""
    st = case.settings
    r = object.__new__(module.ModelRunner)
    r.model = SimpleNamespace(hkv=st.hkv, hq=1, D=1, scale=1.0)
    r.kvm = FakeKVM(case.seqs)
    r.device = torch.device("cpu")
    r.max_blocks, r.pad_rows, r.graphs = MAX_BLOCKS, st.pad, (object() if st.graphs else None)
    r.use_cascade, r.cascade_min_prefix, r.tile = st.cascade, st.min_prefix, st.tile
    r.variant, r.join_suffix, r.fixed_decode_items = (3 if st.joins else 0), st.join_suffix, st.fixed
    r.cascade_bf16 = st.joins
    r.target_wgs, r.prefill_kv_chunk = st.target_wgs, st.prefill_kv_chunk
    r.tok_buf = torch.arange(1000, 1000 + 512, dtype=torch.int64)
    return r


def _cut(buf, sections: dict) -> dict:
    """{section: view of ``buf``}, every section."""
    return {name: sp.section(buf, sections, name) for name in sections}


@pytest.fixture(scope="module")
def steps():
    """(case, runner, HostStep, sampled sequences) of the corpus, built once."""
    out = []
    for seed in range(160):
        case = make_case(seed)
        r = stub_runner(mr, case)
        h, seqs = r.build_host(case.batch)
        out.append((case, r, h, seqs))
    return out


def test_corpus_reaches_the_bounds(steps):
    """The corpus is what the small engine never is: every setting both ways, prefix passes capped at
    MAX_PREFIX_CHUNKS, joined and suffix-joined tiles, split prefill tiles, padded rows, 128-row steps."""
    for f in ("joins", "join_suffix", "fixed", "graphs", "cascade", "pad"):
        assert {getattr(c.settings, f) for c, *_ in steps} == {False, True}, f
    assert {c.settings.tile for c, *_ in steps} == {32, 64}
    hs = [h for _, _, h, _ in steps]
    assert max(h.B for h in hs) == 128 and max(h.cascade_prefix for h in hs) > 32000
    assert max(h.stats["cascade_groups"] for h in hs) == 3
    assert any(h.prefix_joined and h.n_items == 0 for h in hs) and any(h.prefix_joined and h.n_items for h in hs)
    assert any(h.n_merge and not h.prefix_joined for h in hs) and any(h.T > h.B + 8000 for h in hs)
    npre = [int(_cut(h.i32, h.i32_sections())["decode_items"][:, sp.DEC.npre].max()) for h in hs if h.B]
    assert max(npre) == sp.MAX_PREFIX_CHUNKS
    assert any(c.settings.pad and h.T > h.B + sum(b - a for _, a, b in c.batch.prefill) for c, _, h, _ in steps)


# ---- plan census --------------------------------------------------------------------------------------------------
def _census(h, fixed_decode: bool) -> None:
    s32 = _cut(h.i32, h.i32_sections())
    s64 = _cut(h.i64, h.i64_sections())
    limit = s32["q_limit"].astype(np.int64)
    B = h.B
    T_real = B + int((s64["slots"][B:] >= 0).sum())  # (padding rows have no KV slot)
    dec = s32["decode_items"].astype(np.int64)
    dec = dec[dec[:, sp.DEC.split] >= 0]
    pre = s32["prefix_items"].astype(np.int64)    # q rows of the whole step
    fill = s32["prefill_items"].astype(np.int64)  # q rows of the prefill part: row B + q_start
    IT = sp.ITEM
    fill[:, IT.q_start] += B
    tiles = np.concatenate([pre, fill])
    q_start, q_count = tiles[:, IT.q_start], tiles[:, IT.q_count]
    # every (row, kv_lo, kv_hi, slot) a token is named with
    rows = np.concatenate([dec[:, sp.DEC.b], np.repeat(q_start, q_count) + _ramp(q_count)])
    rep = lambda col: np.repeat(tiles[:, col], q_count)  # noqa: E731
    lo = np.concatenate([dec[:, sp.DEC.lo], rep(IT.kv_lo)])
    hi = np.concatenate([dec[:, sp.DEC.hi], rep(IT.kv_hi)])
    slot = np.concatenate([dec[:, sp.DEC.npre] + dec[:, sp.DEC.split], rep(IT.split)])
    assert rows.min(initial=0) >= 0 and rows.max(initial=0) < T_real, "an item names a padding row or none"
    # -- coverage: the (causally clipped) ranges of a token tile [0, limit + 1)
    hi_c = np.minimum(hi, limit[rows] + 1)
    keep = hi_c > lo
    order = np.lexsort((lo[keep], rows[keep]))
    r, a, b = rows[keep][order], lo[keep][order], hi_c[keep][order]
    first = np.r_[True, r[1:] != r[:-1]]
    last = np.r_[first[1:], True]
    assert np.array_equal(r[first], np.arange(T_real)), "a token without items"
    assert (a[first] == 0).all() and (b[last] == limit[r[last]] + 1).all(), "keys missing at an end"
    assert (a[1:][~first[1:]] == b[:-1][~first[1:]]).all(), "a gap or a key attended twice"
    # -- no item spans more than MAX_ITEM_KEYS keys. A tile item's kv_hi is the key bound of its chunk, which the
    # kernel clips causally: the keys it reads (and stages page ids for) end at the limit of the tile's last token
    # Excluded by name: the items of ``decode_items_fixed``. It deals a fixed number of pieces, so a step of many
    # long rows gets pieces past the bound (corpus seed 62: 128 rows, one piece of 32,284 keys), on the parent commit
    # too; the decode kernel stages the page ids of a piece's first 32k keys and reads the table for the rest
    if not fixed_decode:
        assert (dec[:, sp.DEC.hi] - dec[:, sp.DEC.lo]).max(initial=0) <= sp.MAX_ITEM_KEYS, "a decode item too long"
    span = np.minimum(tiles[:, IT.kv_hi], limit[q_start + q_count - 1] + 1) - tiles[:, IT.kv_lo]
    assert span.max(initial=0) <= sp.MAX_ITEM_KEYS, span.max(initial=0)
    # -- partial slots: distinct per row, below the row's buffer size, at most MAX_PARTIALS
    part = slot >= 0
    cap = np.where(rows < B, h.s_total, h.prefill_splits)
    assert (slot[part] < cap[part]).all(), "a partial slot past its buffer"
    pairs = rows[part] * 4096 + slot[part]
    assert len(np.unique(pairs)) == len(pairs), "two items write one partial slot"
    per_row = np.bincount(rows[part], minlength=h.T)
    assert per_row.max(initial=0) <= sp.MAX_PARTIALS
    # -- decode rows are merged by the decode kernel: nsplit pieces each, behind npre prefix partials
    own, alt = pre[pre[:, IT.alt] == 0], pre[pre[:, IT.alt] != 0]  # prefix items of decode rows / joined prefill rows
    for col, want in ((sp.DEC.nsplit, np.bincount(dec[:, sp.DEC.b], minlength=B)),
                      (sp.DEC.npre, np.bincount(np.repeat(own[:, IT.q_start], own[:, IT.q_count]) +
                                                _ramp(own[:, IT.q_count]), minlength=B)[:B])):
        assert (dec[:, col] == want[dec[:, sp.DEC.b]]).all()
    assert (own[:, IT.q_start] + own[:, IT.q_count] <= B).all() and (alt[:, IT.q_start] >= B).all()
    # -- prefill rows: a row either gets one whole item, or partials and exactly one merge range
    whole = np.bincount(rows[~part], minlength=h.T)
    assert (whole[B:T_real] + (per_row[B:T_real] > 0) == 1).all(), "a prefill row both whole and partial, or neither"
    merged = np.zeros(h.T, dtype=np.int64)
    for m_lo, m_hi in s32["merge_ranges"]:
        merged[B + m_lo:B + m_hi] += 1
    assert np.array_equal(merged[B:], (per_row[B:] > 0).astype(np.int64)), "merge ranges != rows with partials"


def _ramp(counts: np.ndarray) -> np.ndarray:
    """0 .. c - 1 for every c of ``counts``, concatenated."""
    return np.arange(counts.sum()) - np.repeat(np.cumsum(counts) - counts, counts)


def test_plan_census(steps):
    """Over the corpus: every key of every token exactly once, slots distinct and in range, rows with partials merged
    exactly once, no item over MAX_ITEM_KEYS (but ``decode_items_fixed`` pieces: see ``_census``), no row over
    MAX_PARTIALS."""
    for case, _, h, _ in steps:
        try:
            _census(h, fixed_decode=case.settings.fixed or case.settings.graphs)
        except AssertionError as e:
            raise AssertionError(f"corpus seed {case.seed} ({case.settings}): {e}") from e


# ---- layout -------------------------------------------------------------------------------------------------------
def _tiles_exactly(sections: dict, size: int) -> None:
    end = 0
    for name, (off, shape) in sections.items():
        assert off == end, f"{name}: gap or overlap at {off} (previous section ends at {end})"
        end = off + int(np.prod(shape))
    assert end == size


def _launch_late_rows(h) -> None:
    """What ``ModelRunner.launch`` does with rows whose token is still in flight: destinations, then sources."""
    dst = [row for row, _, _ in h.patch]
    h.late_off, h.n_late = h.i64.size, len(dst)
    h.i64 = np.concatenate([h.i64, np.asarray(dst + [2 * d + 1 for d in dst], dtype=np.int64)])


def test_sections_tile_the_buffers_and_views_hands_them_out(steps):
    for case, r, h, seqs in steps:
        if h.patch:
            h = copy.copy(h)
            _launch_late_rows(h)
        _tiles_exactly(h.i32_sections(), h.i32.size)
        _tiles_exactly(h.i64_sections(), h.i64.size)
        s32, s64 = _cut(h.i32, h.i32_sections()), _cut(h.i64, h.i64_sections())
        # the sections hold what the step is made of
        B = h.B
        for j, (s, _, _) in enumerate(case.batch.prefill):
            n = min(len(s.pages), h.bt_w)
            assert np.array_equal(s32["block_tables"][B + j, :n], s.pages[:n])
        assert sorted(s.total_len - 1 for s in case.batch.decode) == sorted(s64["positions"][:B].tolist())
        real = s64["slots"] >= 0
        assert np.array_equal(s32["q_limit"][real], s64["positions"][real])
        assert [s.total_len - 1 for s in seqs] == s64["positions"][s64["logit_rows"]].tolist()
        # views: the same sections as tensors
        inp = r.views(torch.from_numpy(h.i64.copy()), torch.from_numpy(h.i32), h)
        m = inp.attn
        eq = lambda t, a: t is not None and np.array_equal(t.numpy(), a)  # noqa: E731
        assert eq(m.block_tables, s32["block_tables"]) and eq(m.q_limit, s32["q_limit"])
        assert eq(inp.positions, s64["positions"]) and eq(inp.slot_mapping, s64["slots"])
        assert eq(inp.logit_rows, s64["logit_rows"])
        if B:
            assert eq(m.decode_items, s32["decode_items"]) and m.s_total == h.s_total
        assert (m.prefix_items is None) == (h.n_prefix_items == 0) and (m.prefill_items is None) == (h.n_items == 0)
        assert h.n_prefix_items == 0 or eq(m.prefix_items, s32["prefix_items"])
        assert h.n_items == 0 or eq(m.prefill_items, s32["prefill_items"])
        if h.prefill_splits:
            assert m.prefill_merge == [tuple(x) for x in s32["merge_ranges"].tolist()] and h.n_merge
        else:
            assert h.n_merge == 0
        want = s64["tokens"].copy()
        if h.n_late:  # late rows: gathered from the previous step's sampler output
            want[s64["late_dst"]] = r.tok_buf.numpy()[s64["late_src"]]
        assert eq(inp.tokens, want)


def test_wire_format_reproduces_every_section(steps):
    """unpack_plan(pack_plan(h)) gives back every section, block tables shipped trimmed (bt_need < bt_w) or whole."""
    sample = sp.SampleParams(np.zeros(1, np.float32), np.ones(1, np.float32), np.zeros(1, np.int32),
                             np.ones(1, np.int64), None, True)
    trimmed = whole = 0
    for _, _, h, _ in steps:
        hdr, payload = sp.pack_plan(h, sample)
        h2, _ = sp.unpack_plan(hdr, payload)
        assert h2.i32_sections() == h.i32_sections() and h2.i64_sections() == h.i64_sections()
        a, b = _cut(h.i32, h.i32_sections()), _cut(h2.i32, h2.i32_sections())
        # (block-table columns past bt_need hold no page a kernel of the step reads: they come back as zeros)
        a["block_tables"] = np.where(np.arange(h.bt_w) < h.bt_need, a["block_tables"], 0)
        assert all(np.array_equal(a[k], b[k]) for k in a) and np.array_equal(h.i64, h2.i64)
        shipped = int(hdr[1 + len(sp._PLAN_SCALARS) + 1])
        assert shipped == h.i32.size - h.nbt * (h.bt_w - h.bt_need)
        trimmed += h.bt_need < h.bt_w
        whole += h.bt_need == h.bt_w
    assert trimmed and whole


# ---- the module ---------------------------------------------------------------------------------------------------
def test_step_plan_is_pure():
    """engine/step_plan.py imports numpy and the standard library only (no torch, runner, sequences or KV manager),
    at module level and inside its functions."""
    tree = ast.parse(Path(sp.__file__).read_text())
    mods = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            mods |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            mods.add((node.module or "").split(".")[0])
    assert mods <= {"__future__", "math", "dataclasses", "typing", "numpy"}, mods


def test_records_stay_tuples():
    items, _, _ = sp.plan_prefill_items([(0, 64, 0, 64, 300), (64, 64, 0, 20000, 20000, 18000, 28)], 8, 256, 256)
    assert [it for it in items if it[sp.ITEM.split] < 0] == [(0, 64, 0, 0, 300, -1, 0, 0)]
    assert (sp.ITEM.kv_lo, sp.ITEM.kv_hi, sp.TILE.extent, sp.DEC.npre) == (3, 4, 3, 5)
    assert np.asarray(items, dtype=np.int32).shape == (len(items), sp.ITEM_INTS)
    assert sp.Group(3, 4) == (3, 4) and sp.Tile(0, 64, 0, 64, 300) == (0, 64, 0, 64, 300, 0, 0)
    assert sp.DecodeItem._fields == ("b", "lo", "hi", "split", "nsplit", "npre", "pad0", "pad1")
    assert sp.TileItem._fields == ("q_start", "q_count", "bt_row", "kv_lo", "kv_hi", "split", "alt", "pad")
