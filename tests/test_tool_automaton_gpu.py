"""The automaton tool grammar on the GPU: the mask and advance kernels (ops/csrc/table_grammar.hip) against the CPU
definition word for word and record for record — all five phases, an LDS-sized and a global-sized table in one launch,
mask rows 8-byte aligned and not — the sampler over device-written rows in a mixed batch, and the engine eager and
under hipGraphs against the CPU reference on the engine's own logits. Integers throughout: every comparison is an
equality."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from kafka_llm_service_amd import ops
from kafka_llm_service_amd.engine import json_mode as jm
from kafka_llm_service_amd.engine import json_schema as js
from kafka_llm_service_amd.engine import tool_automaton as ta
from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
from kafka_llm_service_amd.engine.logits_proc import LogitsProcessor
from kafka_llm_service_amd.engine.sequence import SamplingParams, Sequence
from kafka_llm_service_amd.ops import reference as ref
from test_json_mode import synthetic_table, tokenize
from test_sampler_replay import _capped, _same
from test_tool_automaton import CALLS, FINITE, TOOL_SETS, body, check_call, fn, longest_body

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A5A5A
BIG = [fn("pick", {"type": "object", "required": ["s", "e"], "properties": {
    "s": {"type": "string"}, "e": {"enum": ["m%03d" % i for i in range(400)]}}})]
BIG_DOC = b'{"name":"pick","parameters":{"s":"x\\u00e9\xc3\xa9","e":"m317"}}'


@pytest.fixture(scope="module")
def two_tables():
    """(buffer, dfa, a call of its language): a body staged in LDS and one walked in global memory."""
    names = [t["function"]["name"] for t in TOOL_SETS["weather"]]
    small = ta.compile_tool_body(TOOL_SETS["weather"], names, "llama3")
    big = ta.compile_tool_body(BIG, ["pick"], "llama3")
    assert small.nbytes <= js.SCHEMA_LDS_BYTES < big.nbytes <= js.SCHEMA_TAB_BYTES
    assert ref.schema_walk(js.START, BIG_DOC, big) == js.DONE
    return [(3, small, body(*CALLS["weather"][1], "llama3")), (1, big, BIG_DOC)]


def _pool(cuda, tables, n=5):
    pool = ops.SchemaTables(n, cuda)
    for b, d, _ in tables:
        pool.load(b, d.cls, d.trans)
    return pool


def _records(tables):
    """(buffer, dfa, record) over every phase, the states of a call, DONE, DEAD and states at and past S."""
    out = []
    for b, d, doc in tables:
        states = sorted({ref.schema_walk(js.START, doc[:i], d) for i in range(len(doc) + 1)})
        assert js.DONE in states and js.DEAD not in states
        recs = [(s, ta.TOOL_BODY) for s in states] + [(js.DEAD, ta.TOOL_BODY), (d.S, ta.TOOL_BODY),
                                                       (js.SCHEMA_MAX_STATES - 1, ta.TOOL_BODY)]
        for ph in (ta.TOOL_FREE, ta.TOOL_OPEN, ta.TOOL_TEXT, ta.TOOL_CLOSED):
            recs += [(js.START, ph), (states[len(states) // 2], ph), (js.DONE, ph), (js.DEAD, ph)]
        out += [(b, d, np.array([s, ph, 0, b + 1], np.int32)) for s, ph in recs]
    return out


def _envelopes(V):
    ids = sorted({min(i, V - 1) for i in (0, 31, 32, 63, 64, V - 1)})
    return [(a, c) for a in ids for c in ids]


def _mask_tab(cuda, rows, W, shift):
    """A mask table of ``rows`` rows whose first word sits ``shift`` words behind an aligned address: with an even W
    every row is 8-byte aligned for shift 0 and none for shift 1; with an odd W they alternate."""
    flat = torch.full((rows * W + 2,), SENTINEL, dtype=torch.int32, device=cuda)
    assert flat.data_ptr() % 8 == 0
    return flat, flat[shift:shift + rows * W].view(rows, W)


@pytest.mark.parametrize("V", [1, 63, 64, 65, 1000, 1057])
def test_mask_kernel_equals_reference_in_every_phase(cuda, V, two_tables):
    table = synthetic_table(V)
    tabs = ops.JsonTables(table, cuda)
    pool = _pool(cuda, two_tables)
    assert pool.kinds()[0] == 3  # both instantiations run
    recs = _records(two_tables)
    env = _envelopes(V)
    k, row0, spare = len(recs), 3, 2
    assert k > 150 and {int(r[1]) for _, _, r in recs} == set(range(ta.TOOL_PHASES))
    slots = np.random.default_rng(k).permutation(k + spare)[:k]
    state = np.zeros((k + spare, 4), np.int32)
    rows = np.zeros((k, 5), np.int32)
    for i, (sl, (b, _, rec)) in enumerate(zip(slots, recs)):
        state[sl] = rec
        rows[i] = [k - 1 - i, sl, b, *env[i % len(env)]]
    want = [ref.tool_mask_words(rec, int(r[3]), int(r[4]), d, table) for (b, d, rec), r in zip(recs, rows)]
    results = []
    for shift, kw in ((0, {}), (1, {}), (1, dict(tokens=256, dword=False)), (0, dict(tokens=4096))):
        flat, mask_tab = _mask_tab(cuda, row0 + k + spare + 1, table.W, shift)
        aligned = {(mask_tab.data_ptr() + 4 * r * table.W) % 8 == 0 for r in range(mask_tab.shape[0])}
        assert aligned == ({True, False} if table.W % 2 and mask_tab.shape[0] > 1 else {shift == 0})
        ops.tool_mask(tabs, pool, torch.from_numpy(rows).to(cuda), k, torch.from_numpy(state).to(cuda), mask_tab,
                      row0, **kw)
        mt, fl = mask_tab.cpu().numpy(), flat.cpu().numpy()
        for i, sl in enumerate(slots):
            assert np.array_equal(mt[row0 + sl].view(np.uint32), want[i]), (V, shift, kw, recs[i][2], rows[i])
        written = {int(row0 + sl) for sl in slots}
        for r in range(mt.shape[0]):
            if r not in written:
                assert (mt[r] == SENTINEL).all(), f"V {V}: row {r} is no slot's row and was written"
        assert (fl[:shift] == SENTINEL).all() and (fl[shift + mt.size:] == SENTINEL).all()
        results.append(mt)
    # a launch with one instantiation alone writes the fill rows too (and leaves the other one's walk rows)
    for only, (b_other) in ((1, two_tables[1][0]), (2, two_tables[0][0])):
        flat, mask_tab = _mask_tab(cuda, row0 + k + spare + 1, table.W, 0)
        ops.ext().tool_mask(pool.strans, pool.scls, pool.sdim, tabs.tok_off, tabs.tok_bytes,
                            torch.from_numpy(rows).to(cuda), k, torch.from_numpy(state).to(cuda), mask_tab, row0,
                            only, pool.kinds()[1], 1024, True)
        mt = mask_tab.cpu().numpy()
        for i, sl in enumerate(slots):
            b, d, rec = recs[i]
            walk = rec[1] == ta.TOOL_BODY and rec[0] != js.DONE and rec[0] < d.S
            if walk and b == b_other:
                assert (mt[row0 + sl] == SENTINEL).all()
            else:
                assert np.array_equal(mt[row0 + sl].view(np.uint32), want[i])


def test_mask_kernel_on_the_llama3_table(cuda, two_tables):
    from kafka_llm_service_amd.engine.tokenizer import get_tokenizer

    tok = get_tokenizer()
    table = jm.table_for(tok, tok.eos_ids)
    assert table.V == 128256
    plan = ta.plan_for(tok, TOOL_SETS["weather"], "auto")
    b, d, doc = two_tables[0]
    assert d is plan.dfa
    at = lambda n: ref.schema_walk(js.START, doc[:n], d)
    named = {"free": (js.START, ta.TOOL_FREE), "open": (js.START, ta.TOOL_OPEN), "start": (js.START, ta.TOOL_BODY),
             "in the name": (at(12), ta.TOOL_BODY), "in a string": (at(52), ta.TOOL_BODY),
             "before the last }": (at(len(doc) - 1), ta.TOOL_BODY), "done": (js.DONE, ta.TOOL_BODY),
             "text": (js.START, ta.TOOL_TEXT), "closed": (js.DONE, ta.TOOL_CLOSED), "dead": (js.DEAD, ta.TOOL_BODY)}
    assert named["in a string"][0] not in (js.DEAD, js.DONE)
    tabs, pool = ops.JsonTables(table, cuda), _pool(cuda, two_tables[:1])
    k = len(named)
    slots = np.random.default_rng(k).permutation(k + 2)[:k]
    state = np.zeros((k + 2, 4), np.int32)
    for sl, (s, ph) in zip(slots, named.values()):
        state[sl] = [s, ph, 0, b + 1]
    rows = np.stack([np.arange(k), slots, np.full(k, b), np.full(k, plan.open), np.full(k, plan.close)],
                    axis=1).astype(np.int32)
    mask_tab = torch.full((1 + k + 2, table.W), SENTINEL, dtype=torch.int32, device=cuda)
    ops.tool_mask(tabs, pool, torch.from_numpy(rows).to(cuda), k, torch.from_numpy(state).to(cuda), mask_tab, 1)
    mt = mask_tab.cpu().numpy()
    for (name, (s, ph)), sl in zip(named.items(), slots):
        w = ref.tool_mask_words(state[sl], plan.open, plan.close, d, table)
        g = mt[1 + sl].view(np.uint32)
        assert np.array_equal(g, w), f"{name}: {int((g != w).sum())} of {w.size} words differ"
        print(name, "allows", int(np.unpackbits(w.view(np.uint8)).sum()), "tokens")
    bits = lambda n: np.flatnonzero(np.unpackbits(mt[1 + slots[list(named).index(n)]].view(np.uint8),
                                                  bitorder="little")).tolist()
    assert bits("open") == [plan.open] and bits("done") == bits("closed") == [plan.close] and bits("dead") == []
    assert bits("free") == bits("text") == list(range(table.V))


def test_skipped_rows_leave_the_canary(cuda, two_tables):
    table = synthetic_table(330)
    tabs = ops.JsonTables(table, cuda)
    b, d, _ = two_tables[0]
    pool = _pool(cuda, two_tables[:1])  # (buffer 0 holds no table: S = 0)
    op, cl = 5, 329
    good = [js.START, ta.TOOL_OPEN, 0, b + 1]
    st0 = [good, [js.START, ta.TOOL_OPEN, 0, 2], [js.START, 5, 0, b + 1], [js.START, -1, 0, b + 1],
           [js.START, 0, 0, 0], good]
    state = torch.tensor(st0, dtype=torch.int32, device=cuda)
    n_slots = len(st0)
    cases = {"slot past the table": [0, n_slots, b, op, cl], "slot below 0": [0, -1, b, op, cl],
             "sampled row past": [4, 0, b, op, cl], "sampled row below 0": [-1, 0, b, op, cl],
             "table past the pool": [0, 0, 5, op, cl], "table below 0": [0, 0, -1, op, cl],
             "table without dimensions": [0, 0, 0, op, cl], "record of another table": [0, 1, b, op, cl],
             "phase past 4": [0, 2, b, op, cl], "phase below 0": [0, 3, b, op, cl],
             "a JSON-mode record": [0, 4, b, op, cl], "open past V": [0, 0, b, 330, cl],
             "open below 0": [0, 0, b, -1, cl], "close past V": [0, 0, b, op, 330], "close below 0": [0, 0, b, op, -7]}
    # (S, C) outside the limits: a pool whose dimensions say so
    sampled = torch.full((4,), op, device=cuda)
    for name, row in cases.items():
        rows = torch.tensor([row], dtype=torch.int32, device=cuda)
        mask_tab = torch.full((2 + n_slots, table.W), SENTINEL, dtype=torch.int32, device=cuda)
        ops.tool_mask(tabs, pool, rows, 4, state, mask_tab, 2, used=[b])
        ops.tool_advance(tabs, pool, rows, sampled, state)
        assert (mask_tab.cpu().numpy() == SENTINEL).all(), name
        assert state.cpu().tolist() == st0, name
    for S, C in ((1, 4), (js.SCHEMA_MAX_STATES + 1, 4), (8, 0), (8, 257), (8192, 32)):
        bad = _pool(cuda, two_tables[:1])
        bad.sdim[b] = torch.tensor([S, C], dtype=torch.int32)
        rows = torch.tensor([[0, 0, b, op, cl]], dtype=torch.int32, device=cuda)
        mask_tab = torch.full((2 + n_slots, table.W), SENTINEL, dtype=torch.int32, device=cuda)
        ops.tool_mask(tabs, bad, rows, 4, state, mask_tab, 2, used=[b])
        ops.tool_advance(tabs, bad, rows, sampled, state)
        assert (mask_tab.cpu().numpy() == SENTINEL).all() and state.cpu().tolist() == st0, (S, C)
    # the good row beside skipped ones is written, and only it
    rows = torch.tensor([cases["phase past 4"], [1, 5, b, op, cl], cases["open past V"]], dtype=torch.int32,
                        device=cuda)
    mask_tab = torch.full((2 + n_slots, table.W), SENTINEL, dtype=torch.int32, device=cuda)
    ops.tool_mask(tabs, pool, rows, 4, state, mask_tab, 2)
    mt = mask_tab.cpu().numpy()
    assert np.array_equal(mt[2 + 5].view(np.uint32), ref.tool_mask_words(np.array(good), op, cl, d, table))
    assert (np.delete(mt, 7, axis=0) == SENTINEL).all()
    ops.tool_advance(tabs, pool, rows, sampled, state)
    assert state.cpu().tolist() == st0[:5] + [[js.START, ta.TOOL_BODY, 0, b + 1]]


def test_advance_kernel_record_for_record(cuda, two_tables):
    table = synthetic_table(1000)
    tabs = ops.JsonTables(table, cuda)
    pool = _pool(cuda, two_tables)
    op, cl = 3, 999  # (ids without bytes, as the real envelope's)
    assert table.lens[op] == 0 and table.lens[cl] == 0
    # whole calls, one per table and starting phase, walked on the device
    items = [(b, d, [op] + tokenize(table, doc) + [cl, cl], ph) for b, d, doc in two_tables
             for ph in (ta.TOOL_OPEN, ta.TOOL_FREE)]
    items.append((two_tables[0][0], two_tables[0][1], tokenize(table, b"plain text") + [op, cl], ta.TOOL_FREE))
    k, steps = len(items), max(len(t) for _, _, t, _ in items)
    slots = np.random.default_rng(2).permutation(k + 3)[:k]
    rows = torch.from_numpy(np.stack([np.arange(k), slots, [b for b, _, _, _ in items], np.full(k, op), np.full(k, cl)],
                                     axis=1).astype(np.int32)).to(cuda)
    st0 = np.zeros((k + 3, 4), np.int32)
    for sl, (b, _, _, ph) in zip(slots, items):
        st0[sl] = ta.tool_record(js.START, ph, b)
    others = np.setdiff1d(np.arange(k + 3), slots)
    st0[others] = [7, 8, 9, 0]  # (other slots: anything, and it must stay)
    state = torch.from_numpy(st0).to(cuda)
    want = [st0[sl].copy() for sl in slots]
    for j in range(steps):
        ids = [t[j] if j < len(t) else cl for _, _, t, _ in items]
        ops.tool_advance(tabs, pool, rows, torch.tensor(ids, device=cuda), state)
        want = [ref.tool_advance_ref(r, t, op, cl, d, table) for r, t, (_, d, _, _) in zip(want, ids, items)]
        got = state.cpu().numpy()
        for i, sl in enumerate(slots):
            assert got[sl].tolist() == want[i].tolist(), (j, i)
        assert (got[others] == [7, 8, 9, 0]).all()
    assert [w.tolist()[:2] for w in want] == [[js.DONE, ta.TOOL_CLOSED]] * 4 + [[js.START, ta.TOOL_TEXT]]
    # every DEAD case, the moves that are no walk, and the records that stay
    b, d, doc = two_tables[1]
    mid = ref.schema_walk(js.START, doc[:20], d)
    colon, x = tokenize(table, b":")[0], tokenize(table, b"x")[0]
    cases = [([js.START, ta.TOOL_OPEN], x), ([js.START, ta.TOOL_OPEN], cl), ([js.START, ta.TOOL_OPEN], op),
             ([js.DONE, ta.TOOL_BODY], x), ([js.DONE, ta.TOOL_BODY], op), ([js.DONE, ta.TOOL_BODY], cl),
             ([mid, ta.TOOL_BODY], colon), ([mid, ta.TOOL_BODY], op), ([mid, ta.TOOL_BODY], cl),
             ([mid, ta.TOOL_BODY], table.V + 5), ([mid, ta.TOOL_BODY], -1), ([js.DEAD, ta.TOOL_BODY], x),
             ([d.S, ta.TOOL_BODY], x), ([mid, ta.TOOL_FREE], x), ([mid, ta.TOOL_FREE], op), ([mid, ta.TOOL_TEXT], op),
             ([js.DONE, ta.TOOL_CLOSED], x), ([js.DEAD, ta.TOOL_OPEN], op)]
    state = torch.tensor([r + [0, b + 1] for r, _ in cases], dtype=torch.int32, device=cuda)
    rows = torch.tensor([[i, i, b, op, cl] for i in range(len(cases))], dtype=torch.int32, device=cuda)
    ops.tool_advance(tabs, pool, rows, torch.tensor([t for _, t in cases], device=cuda), state)
    got, n_dead = state.cpu().tolist(), 0
    for i, (r, t) in enumerate(cases):
        w = ref.tool_advance_ref(np.array(r + [0, b + 1]), t, op, cl, d, table).tolist()
        assert got[i] == w, (i, r, t)
        n_dead += w[0] == js.DEAD
    assert n_dead == 11 and got[5][:2] == [js.DONE, ta.TOOL_CLOSED] and got[2][:2] == [js.START, ta.TOOL_BODY]


def _body_states(tables):
    """(buffer, dfa, state) over what the schema corpus visits: the states of a document from START to DONE, DEAD, and
    states at and past S."""
    out = []
    for b, d, doc in tables:
        states = sorted({ref.schema_walk(js.START, doc[:i], d) for i in range(len(doc) + 1)})
        assert js.START in states and js.DONE in states and js.DEAD not in states
        out += [(b, d, s) for s in states + [js.DEAD, d.S, js.SCHEMA_MAX_STATES - 1]]
    return out


def _one_eos_table(V):
    """``synthetic_table(V)`` with the last id as its only EOS: the `close` of the tool rows below."""
    t = synthetic_table(V)
    return jm.JsonTable.from_byte_strings([t.bytes_of(i) for i in range(V)], [V - 1])


@pytest.mark.parametrize("V", [1, 63, 64, 65, 1057])
def test_a_schema_row_is_a_body_row_without_an_envelope(cuda, V, two_tables):
    """What one kernel pair for both row widths rests on: the state ``s`` as the schema record (s, 0, 0, tab + 1) and
    as the tool record (s, TOOL_BODY, 0, tab + 1) gives the same mask word for word — ``schema_mask_ref``'s, and in
    DONE, where `close` is the table's one EOS id, ``tool_mask_words``' too — and, advanced over the same id, the same
    word 0. Tables in LDS and in global memory, rows 8-byte aligned and not; rows of no slot keep the sentinel."""
    table = _one_eos_table(V)
    tabs, pool = ops.JsonTables(table, cuda), _pool(cuda, two_tables)
    assert pool.kinds()[0] == 3 and table.eos_ids.tolist() == [V - 1]
    op, cl = min(3, V - 1), V - 1
    corpus = _body_states(two_tables)
    k, row0, spare = len(corpus), 3, 2
    assert k > 60 and {js.START, js.DONE, js.DEAD} <= {s for _, _, s in corpus}
    # the schema record of corpus[i] in slot perm[2 i], its tool twin in slot perm[2 i + 1]
    perm = np.random.default_rng(V).permutation(2 * k + spare)
    state = np.zeros((2 * k + spare, 4), np.int32)
    srows, trows = np.zeros((k, 3), np.int32), np.zeros((k, 5), np.int32)
    for i, (b, _, s) in enumerate(corpus):
        state[perm[2 * i]], state[perm[2 * i + 1]] = js.state_record(s, b), ta.tool_record(s, ta.TOOL_BODY, b)
        srows[i], trows[i] = [i, perm[2 * i], b], [k - 1 - i, perm[2 * i + 1], b, op, cl]
    want = [ref.schema_mask_ref(s, d, table) for _, d, s in corpus]
    for shift in (0, 1):
        flat, mask_tab = _mask_tab(cuda, row0 + 2 * k + spare + 1, table.W, shift)
        st = torch.from_numpy(state.copy()).to(cuda)
        ops.schema_mask(tabs, pool, torch.from_numpy(srows).to(cuda), k, st, mask_tab, row0)
        ops.tool_mask(tabs, pool, torch.from_numpy(trows).to(cuda), k, st, mask_tab, row0)
        mt, fl = mask_tab.cpu().numpy(), flat.cpu().numpy()
        for i, (b, d, s) in enumerate(corpus):
            g_s, g_t = mt[row0 + perm[2 * i]].view(np.uint32), mt[row0 + perm[2 * i + 1]].view(np.uint32)
            assert np.array_equal(g_s, g_t), (V, shift, b, s)
            assert np.array_equal(g_s, want[i]), (V, shift, b, s)
            if s == js.DONE:
                assert np.array_equal(g_t, ref.tool_mask_words(state[perm[2 * i + 1]], op, cl, d, table))
                assert np.flatnonzero(np.unpackbits(g_t.view(np.uint8), bitorder="little")).tolist() == [cl]
        written = {int(row0 + sl) for sl in perm[:2 * k]}
        for r in range(mt.shape[0]):
            if r not in written:
                assert (mt[r] == SENTINEL).all(), f"V {V}: row {r} is no slot's row and was written"
        assert (fl[:shift] == SENTINEL).all() and (fl[shift + mt.size:] == SENTINEL).all()
        assert st.cpu().numpy().tolist() == state.tolist()  # (a mask launch writes no record)


def test_a_schema_row_advances_as_a_body_row(cuda, two_tables):
    """The advance half of the test above: both records over the same sampled id — a valid continuation, a dead byte,
    an id without bytes, an id past V; in DONE the `close` id, where the schema row stays DONE and the tool row
    closes — leave the same word 0, ``schema_advance_ref``'s, and every other word as its own reference says."""
    V = 1057
    table = _one_eos_table(V)
    tabs, pool = ops.JsonTables(table, cuda), _pool(cuda, two_tables)
    op, cl, empty = 5, V - 1, 3
    assert table.lens[empty] == 0 and table.lens[op] > 0
    single = [t for t in range(V - 1) if table.lens[t] == 1]
    cases, kinds = [], set()  # (buffer, dfa, state, sampled id)
    for b, d, s in _body_states(two_tables):
        if s == js.DONE:
            cases.append((b, d, s, cl))
            continue
        nxt = {t: ref.schema_advance_ref(s, t, d, table) for t in single}
        live = next((t for t, n in nxt.items() if n != js.DEAD), None)
        dead = next(t for t, n in nxt.items() if n == js.DEAD)
        kinds.add(live is not None)
        cases += [(b, d, s, t) for t in (live, dead, empty, V + 5) if t is not None]
    assert kinds == {True, False}  # (DEAD and the states past S have no continuation)
    k, spare = len(cases), 3
    perm = np.random.default_rng(k).permutation(2 * k + spare)
    st0 = np.zeros((2 * k + spare, 4), np.int32)
    st0[perm[2 * k:]] = [7, 8, 9, 0]  # (other slots: anything, and it must stay)
    srows, trows = np.zeros((k, 3), np.int32), np.zeros((k, 5), np.int32)
    for i, (b, _, s, _) in enumerate(cases):
        st0[perm[2 * i]], st0[perm[2 * i + 1]] = js.state_record(s, b), ta.tool_record(s, ta.TOOL_BODY, b)
        srows[i], trows[i] = [i, perm[2 * i], b], [i, perm[2 * i + 1], b, op, cl]
    state = torch.from_numpy(st0.copy()).to(cuda)
    sampled = torch.tensor([t for _, _, _, t in cases], device=cuda)
    ops.tool_advance(tabs, pool, torch.from_numpy(trows).to(cuda), sampled, state)
    ops.schema_advance(tabs, pool, torch.from_numpy(srows).to(cuda), sampled, state)
    got = state.cpu().numpy()
    for i, (b, d, s, t) in enumerate(cases):
        g_s, g_t = got[perm[2 * i]].tolist(), got[perm[2 * i + 1]].tolist()
        assert g_s[0] == g_t[0] == ref.schema_advance_ref(s, t, d, table), (i, b, s, t)
        assert g_s[1:] == [0, 0, b + 1], (i, b, s, t)
        assert g_t == ref.tool_advance_ref(st0[perm[2 * i + 1]], t, op, cl, d, table).tolist(), (i, b, s, t)
        if s == js.DONE:
            assert g_s[0] == js.DONE and g_t[1] == ta.TOOL_CLOSED
    assert (got[perm[2 * k:]] == [7, 8, 9, 0]).all()


def test_sampler_reads_device_written_rows_in_a_mixed_batch(cuda):
    """Tool rows in every phase beside a JSON-mode row, a schema row, host-masked rows and plain rows at T = 0.9 over
    the Llama-3 vocabulary: the GPU's mask table equals the CPU's (which the reference wrote), the draws equal
    ``sample_replay``'s under those masks, the records advance as ``tool_advance_ref`` says, and every other row draws
    what it draws without the tool rows."""
    from kafka_llm_service_amd.engine.tokenizer import get_tokenizer

    tok = get_tokenizer()
    table = jm.table_for(tok, tok.eos_ids)
    B, V = 16, table.V
    x = (torch.randn(B, V, generator=torch.Generator().manual_seed(5)) * 3).clamp(-15.5, 15.5).to(torch.bfloat16)
    plan_w, plan_f = ta.plan_for(tok, TOOL_SETS["weather"], "required"), ta.plan_for(tok, FINITE, "auto")
    doc = body(*CALLS["weather"][1], "llama3")
    at = lambda n: ref.schema_walk(js.START, doc[:n], plan_w.dfa)
    tool = {1: (plan_w, js.START, ta.TOOL_OPEN), 2: (plan_f, js.START, ta.TOOL_FREE),
            5: (plan_w, at(0), ta.TOOL_BODY), 6: (plan_w, at(52), ta.TOOL_BODY), 9: (plan_w, js.DONE, ta.TOOL_BODY),
            11: (plan_f, js.START, ta.TOOL_TEXT), 13: (plan_f, js.DONE, ta.TOOL_CLOSED)}
    schema = js.canonical_text(ta.strictify(TOOL_SETS["shell"][0]["function"]["parameters"]))
    seqs, rows, g = [], [], torch.Generator().manual_seed(9)
    for i in range(B):
        p = dict(temperature=0.9)
        if i in tool:
            p["tool_plan"] = tool[i][0]
        elif i == 3:
            p["json_mode"] = True
        elif i == 7:
            p["json_schema"] = schema
        s = Sequence(f"r{i}", [1], SamplingParams(**p))
        if i in tool or i in (3, 7):
            rows.append((i, s, None))
        elif i % 4 == 0:  # host-masked rows: an id list
            rows.append((i, s, torch.randint(0, V, (int(torch.randint(2, 3000, (1,), generator=g)),),
                                             generator=g).tolist()))
        seqs.append(s)

    def run(dev, with_tools):
        lp = LogitsProcessor(dev, V, max_slots=32, mask_rows=16, json_slots=12)
        lp.set_json_table(table)
        use = [r for r in rows if with_tools or r[1].params.tool_plan is None]
        proc, upd = lp.build(use, B, n_decode=0)
        up = torch.from_numpy if str(dev) == "cpu" else (lambda a: torch.from_numpy(a).to(dev))
        lp.apply(upd, up)
        tr, sr, jr = lp.tool_rows(proc), lp.schema_rows(proc), lp.json_rows(proc)
        if tr is not None:  # the records the rows stand in
            st = np.stack([ta.tool_record(tool[i][1], tool[i][2], b) for i, _, b, _, _ in tr.tolist()])
            lp.jstate.index_copy_(0, up(tr[:, 1].astype(np.int64)), up(st))
        tabs, mt = lp.json_tables(), lp.tables()[0]
        ops.json_mask(tabs, up(jr), lp.jstate, mt, lp.n_mask_rows)
        ops.schema_mask(tabs, lp.schema_pool(), up(sr), B, lp.jstate, mt, lp.n_mask_rows)
        if tr is not None:
            ops.tool_mask(tabs, lp.schema_pool(), up(tr), B, lp.jstate, mt, lp.n_mask_rows)
        return lp, proc, tr

    lp_c, proc, tr = run("cpu", True)
    assert tr[:, 0].tolist() == sorted(tool) and len(set(tr[:, 2].tolist())) == 2
    temp, seeds, step = torch.full((B,), 0.9), torch.arange(B, dtype=torch.long) * 13 + 1, torch.tensor([4])
    pd_c = torch.from_numpy(proc)
    rep = ref.sample_replay(x, temp, None, None, seeds, step, proc=pd_c, mask_tab=lp_c.tables()[0],
                            counts=lp_c.tables()[1], nsplit=8)
    msg = _capped(rep, "mixed tool batch")
    for i, (plan, s, ph) in tool.items():  # the replay's own draws respect the reference masks
        assert ref.tool_mask_ref([s, ph, 0, 1], plan.open, plan.close, plan.dfa, table)[int(rep.tokens[i])]
    assert int(rep.tokens[1]) == plan_w.open and int(rep.tokens[9]) == plan_w.close == int(rep.tokens[13])
    lp_g, proc_g, tr_g = run(cuda, True)
    assert np.array_equal(proc_g, proc) and np.array_equal(tr_g, tr)
    assert torch.equal(lp_g.tables()[0].cpu(), lp_c.tables()[0])  # every mask row, device-written or uploaded
    xg = x.to(cuda)
    tok_g = ops.sample(xg, temp.to(cuda), None, None, seeds.to(cuda), step.to(cuda), proc=pd_c.to(cuda),
                       mask_tab=lp_g.tables()[0], counts=lp_g.tables()[1], bias_tab=lp_g.bias_table())
    _same(tok_g, rep, msg)
    ops.tool_advance(lp_g.json_tables(), lp_g.schema_pool(), torch.from_numpy(tr_g).to(cuda), tok_g, lp_g.jstate)
    for i, slot, b, op, cl in tr_g.tolist():
        plan, s, ph = tool[i]
        want = ref.tool_advance_ref([s, ph, 0, b + 1], int(tok_g[i]), op, cl, plan.dfa, table)
        assert lp_g.jstate[slot].cpu().tolist() == want.tolist() and want[0] != js.DEAD
    lp_n, proc_n, tr_n = run(cuda, False)
    assert tr_n is None
    tok_n = ops.sample(xg, temp.to(cuda), None, None, seeds.to(cuda), step.to(cuda),
                       proc=torch.from_numpy(proc_n).to(cuda), mask_tab=lp_n.tables()[0], counts=lp_n.tables()[1],
                       bias_tab=lp_n.bias_table())
    others = [i for i in range(B) if i not in tool]
    assert torch.equal(tok_n[others], tok_g[others]) and not torch.equal(tok_n[sorted(tool)], tok_g[sorted(tool)])


def test_engine_eager_and_graphs_follow_the_reference(cuda):
    """tiny-llama with two steps in flight, eager and with hipGraphs: automaton tool requests (required over a finite
    language, required over the shell tools, auto) beside a JSON-mode, a schema and a plain request. The engine's own
    logits are recorded at every sampler launch; every tool row's token must be allowed by ``tool_mask_ref`` of the
    reference record — seeded where the plan seeds it, over the table the plan shipped, advanced by
    ``tool_advance_ref`` — and every greedy row's token the first argmax under that mask. The finite-language request
    ends in a parsed, valid call. The graphed engine emits the same tokens, and the plain request replays."""
    from kafka_llm_service_amd.engine.tokenizer import tokenizer_for_model

    g = torch.Generator().manual_seed(3)
    prompts = [[128000] + torch.randint(0, 5000, (m,), generator=g).tolist() for m in (17, 23, 9, 30, 12, 15, 11)]
    n = 14
    cfg = dict(model="tiny-llama", device="cuda:0", num_kv_blocks=256, max_model_len=2048)
    eager = LLMEngine(EngineConfig(**cfg))
    eager.runner.fixed_decode_items = True  # the graph engine's decode split, so both sum in the same order
    table = eager._json_table()
    tok = tokenizer_for_model(eager.model_cfg)
    plan = ta.plan_for(tok, FINITE, "required")
    auto = {"tools": FINITE, "tool_choice": "auto", "mode": "automaton"}
    schema = js.canonical_text(ta.strictify(TOOL_SETS["shell"][0]["function"]["parameters"]))
    sps = [SamplingParams(temperature=0.0, max_tokens=2 + longest_body(plan.dfa),
                          tool_grammar={"tools": FINITE, "tool_choice": "required", "mode": "automaton"}),
           SamplingParams(temperature=0.0, max_tokens=n, ignore_eos=True),
           SamplingParams(temperature=0.0, max_tokens=n, ignore_eos=True,
                          tool_grammar={"tools": TOOL_SETS["shell"], "tool_choice": "required", "mode": "automaton"}),
           SamplingParams(temperature=0.0, max_tokens=n, json_mode=True, ignore_eos=True),
           SamplingParams(temperature=1.0, seed=7, max_tokens=n, ignore_eos=True,
                          tool_grammar={"tools": TOOL_SETS["weather"], "tool_choice": "required",
                                        "mode": "automaton"}),
           SamplingParams(temperature=0.0, max_tokens=n, ignore_eos=True, tool_grammar=auto),
           SamplingParams(temperature=0.0, max_tokens=n, json_schema=schema, ignore_eos=True)]
    records, orig = [], eager.runner.sample_device

    def sample_device(logits, sp):
        toks = orig(logits, sp)
        records.append((logits.clone(), sp, toks.clone()))  # (read after the run: nothing waits for the GPU here)
        return toks

    eager.runner.sample_device = sample_device
    seqs = [eager.add_request(f"r{i}", p, sp) for i, (p, sp) in enumerate(zip(prompts, sps))]
    while not all(s.finished for s in seqs):
        eager.step()
    eager.runner.sample_device = orig
    got = [list(s.output_ids) for s in seqs]
    assert seqs[0].finish_reason == "stop"
    check_call(tok, got[0], FINITE, plan)
    st = eager.runner.lp.stats
    assert st["tool_seeds"] == 4 and st["schema_table_uploads"] == 4 and st["forced_rows"] == 0
    state, tabs, checked, drawn = {}, {}, 0, 0
    for logits, sp, toks in records:
        if sp.upd is not None:
            for buf, cls, trans in sp.upd.tool_tabs:
                tabs[buf] = js.SchemaDfa(cls.copy(), trans.copy(), "")
            for slot, rec in zip(sp.upd.tool_slots.tolist(), sp.upd.tool_states.tolist()):
                state[slot] = np.array(rec, np.int32)
        if sp.tool_rows is None:
            continue
        x, toks = logits.float().cpu(), toks.cpu()
        for i, slot, buf, op, cl in sp.tool_rows.tolist():
            keep = torch.from_numpy(ref.tool_mask_ref(state[slot], op, cl, tabs[buf], table))
            t = int(toks[i])
            assert keep[t], (i, slot, t, state[slot])
            drawn += 1
            if sp.temp[i] == 0:
                row = x[i].masked_fill(~keep, float("-inf"))
                assert t == int(torch.nonzero(row == row.max())[0]), (i, slot, t)
                checked += 1
            state[slot] = ref.tool_advance_ref(state[slot], t, op, cl, tabs[buf], table)
    # requests 0, 2 and 4: every token (and at most one launch planned ahead of request 0's end); the auto request: its
    # first token, and one more launch at the most before the host has seen it land as text
    assert got[5][0] != plan.open and len(tabs) == 3
    base = len(got[0]) + len(got[2])
    assert base + 1 <= checked <= base + 4 and drawn >= checked + len(got[4])
    graphed = LLMEngine(EngineConfig(**cfg, use_graphs=True), model=eager.model)
    got_g = graphed.generate(prompts, sps)
    assert not graphed.runner.graphs.disabled and got_g == got
    # the auto request once it is text, and the plain request: graphable again
    more = graphed.generate(prompts[1:2], [sps[1]])
    assert graphed.runner.graphs.stats["replays"] > 0 and more[0] == got[1]
    r0 = graphed.runner.graphs.stats["replays"]
    text = graphed.generate(prompts[5:6], [sps[5]])[0]
    assert text[0] != plan.open and graphed.runner.graphs.stats["replays"] >= r0 + n - 4


def test_engine_preemption_resumes_with_the_same_tokens(cuda):
    g = torch.Generator().manual_seed(5)
    prompts = [[128000] + torch.randint(0, 5000, (50,), generator=g).tolist() for _ in range(4)]
    sp = SamplingParams(temperature=0.0, max_tokens=20, ignore_eos=True,
                        tool_grammar={"tools": TOOL_SETS["shell"], "tool_choice": "required", "mode": "automaton"})
    big = LLMEngine(EngineConfig(model="tiny-llama", device="cuda:0", num_kv_blocks=256, max_model_len=2048))
    want = big.generate(prompts, sp)
    eng = LLMEngine(EngineConfig(model="tiny-llama", device="cuda:0", num_kv_blocks=12, max_model_len=2048),
                    model=big.model)
    got = eng.generate(prompts, sp)
    st = eng.runner.lp.stats
    assert eng.sched.num_preemptions > 0 and st["tool_seeds"] > 4 and st["schema_table_uploads"] == 1
    assert got == want and all(len(o) == 20 for o in got)
    table = big._json_table()
    from kafka_llm_service_amd.engine.tokenizer import tokenizer_for_model

    plan = ta.plan_for(tokenizer_for_model(big.model_cfg), TOOL_SETS["shell"], "required")
    for o in got:
        rec = ta.tool_record(js.START, ta.TOOL_OPEN, 0)
        for t in o:
            assert ref.tool_mask_ref(rec, plan.open, plan.close, plan.dfa, table)[t]
            rec = ref.tool_advance_ref(rec, t, plan.open, plan.close, plan.dfa, table)
