"""Structured outputs on the GPU: the mask and advance kernels (ops/csrc/json_schema.hip) against the CPU definition word
for word and record for record — tables in LDS and in global memory in one launch — the sampler over device-written
rows in a mixed batch, and the engine eager and under hipGraphs against the CPU reference sampler and automaton on the
engine's own logits. Integers throughout: every comparison is an equality."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from kafka_llm_service_amd import ops
from kafka_llm_service_amd.engine import json_mode as jm
from kafka_llm_service_amd.engine import json_schema as js
from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
from kafka_llm_service_amd.engine.logits_proc import LogitsProcessor
from kafka_llm_service_amd.engine.sequence import SamplingParams, Sequence
from kafka_llm_service_amd.ops import reference as ref
from test_json_mode import synthetic_table, tokenize
from test_json_schema import BOOL, INT, NUM, SCHEMAS, STR, arr, conforms, doc_states, obj
from test_sampler_replay import _capped, _same

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A5A5A


def _padded(k: int) -> dict:
    """The ``scalars`` shape beside an enum of k members: the enum sizes the table."""
    return obj({"s": STR, "i": INT, "n": NUM, "b": BOOL, "e": {"enum": ["m%03d" % i for i in range(k)]}})


_PAD_DOCS = [b'{"s":"x\\u00e9\xc3\xa9","i":-12,"n":1.5e3,"b":true,"e":"m007"}',
             b'{ "s" : "" , "i" : 0 , "n" : 0.25 , "b" : false , "e" : "m120" }']


@pytest.fixture(scope="module")
def three_tables():
    """(dfa, documents) x 3: the smallest table there is, one just under SCHEMA_LDS_BYTES and one just over it."""
    tiny = js.compile_schema(SCHEMAS["empty"][0])
    k = 121
    while js.compile_schema(_padded(k + 1)).nbytes <= js.SCHEMA_LDS_BYTES:
        k += 1
    under, over = js.compile_schema(_padded(k)), js.compile_schema(_padded(k + 1))
    assert tiny.S == 3 and tiny.nbytes == 3 * tiny.C * 2 < 64
    assert js.SCHEMA_LDS_BYTES - 3 * under.C * 2 < under.nbytes <= js.SCHEMA_LDS_BYTES < over.nbytes \
        <= js.SCHEMA_LDS_BYTES + 3 * over.C * 2
    return [(tiny, SCHEMAS["empty"][1]), (under, _PAD_DOCS), (over, _PAD_DOCS)]


def _pool(cuda, dfas, n=5, bufs=(3, 0, 4)):
    pool = ops.SchemaTables(n, cuda)
    for b, d in zip(bufs, dfas):
        pool.load(b, d.cls, d.trans)
    return pool


def _corpus(three_tables):
    """(buffer, dfa, state) of every state the documents reach, the three tables interleaved, plus DEAD and a state
    past S (both walk as DEAD)."""
    bufs = (3, 0, 4)
    per = [[(b, d, s) for s in doc_states(d, docs)] for b, (d, docs) in zip(bufs, three_tables)]
    out = [x for i in range(max(map(len, per))) for p in per for x in p[i:i + 1]]
    d = three_tables[1][0]
    return out + [(0, d, js.DEAD), (0, d, d.S), (0, d, js.SCHEMA_MAX_STATES - 1)]


@pytest.mark.parametrize("V", [1, 31, 64, 65, 1000])
def test_mask_kernel_equals_reference_with_tables_in_lds_and_global_memory(cuda, V, three_tables):
    table = synthetic_table(V)
    tabs = ops.JsonTables(table, cuda)
    pool = _pool(cuda, [d for d, _ in three_tables])
    assert pool.kinds()[0] == 3  # both instantiations run
    corpus = _corpus(three_tables)
    k, row0, spare = len(corpus), 3, 2
    assert k > 100 and {b for b, _, _ in corpus} == {0, 3, 4}
    slots = np.random.default_rng(k).permutation(k + spare)[:k]
    state = np.zeros((k + spare, 4), np.int32)
    for sl, (b, _, s) in zip(slots, corpus):
        state[sl] = [s, 0, 0, b + 1]
    rows = np.stack([np.arange(k)[::-1], slots, [b for b, _, _ in corpus]], axis=1).astype(np.int32)
    mask_tab = torch.full((row0 + k + spare + 1, table.W), SENTINEL, dtype=torch.int32, device=cuda)
    ops.schema_mask(tabs, pool, torch.from_numpy(rows).to(cuda), k, torch.from_numpy(state).to(cuda), mask_tab, row0)
    mt = mask_tab.cpu().numpy()
    want = {}
    nbits = 0
    for sl, (b, d, s) in zip(slots, corpus):
        if (b, s) not in want:
            want[b, s] = ref.schema_mask_ref(s, d, table)
        assert np.array_equal(mt[row0 + sl].view(np.uint32), want[b, s]), (V, b, s)
        nbits += int(np.unpackbits(want[b, s].view(np.uint8)).sum())
    written = {int(row0 + sl) for sl in slots}
    for r in range(mt.shape[0]):
        if r not in written:
            assert (mt[r] == SENTINEL).all(), f"V {V}: row {r} is no slot's row and was written"
    assert V < 31 or nbits > k
    # the other tile size and the byte-wise token loads agree
    for kw in (dict(tokens=256), dict(dword=False), dict(tokens=4096, dword=False)):
        mask_tab.fill_(SENTINEL)
        ops.schema_mask(tabs, pool, torch.from_numpy(rows).to(cuda), k, torch.from_numpy(state).to(cuda), mask_tab,
                        row0, **kw)
        assert np.array_equal(mask_tab.cpu().numpy(), mt), kw


def test_mask_kernel_skips_rows_out_of_range(cuda, three_tables):
    table = synthetic_table(330)
    tabs = ops.JsonTables(table, cuda)
    d = three_tables[1][0]
    pool = _pool(cuda, [d], n=2, bufs=(1,))  # (buffer 0 holds no table: S = 0)
    state = torch.tensor([[js.START, 0, 0, 2]] * 3, dtype=torch.int32, device=cuda)
    state[0, 3] = 0  # (slot 0: a JSON-mode record; a schema row naming it is not its row)
    rows = torch.tensor([[0, 1, 1], [0, 3, 1], [0, -1, 1], [5, 0, 1], [-1, 0, 1], [0, 0, 2], [0, 0, -1], [0, 2, 0],
                         [1, 0, 1]], dtype=torch.int32, device=cuda)
    mask_tab = torch.full((2 + 3, table.W), SENTINEL, dtype=torch.int32, device=cuda)
    ops.schema_mask(tabs, pool, rows, 4, state, mask_tab, 2)
    mt = mask_tab.cpu().numpy()
    assert np.array_equal(mt[3].view(np.uint32), ref.schema_mask_ref(js.START, d, table))
    assert (mt[[0, 1, 2, 4]] == SENTINEL).all()
    ops.schema_advance(tabs, pool, rows, torch.full((4,), tokenize(table, b"{")[0], device=cuda), state)
    assert state.cpu().tolist() == [[js.START, 0, 0, 0], [ref.schema_walk(js.START, b"{", d), 0, 0, 2], [js.START, 0, 0, 2]]


def test_mask_kernel_on_the_llama3_table(cuda):
    from kafka_llm_service_amd.engine.tokenizer import get_tokenizer

    tok = get_tokenizer()
    table = jm.table_for(tok, tok.eos_ids)
    assert table.V == 128256
    schema = obj({"name": STR, "n": NUM, "color": {"enum": ["red", "green", "blue"]}, "tags": arr(INT), "ok": BOOL})
    dfa = js.compile_schema(schema)
    at = lambda text: ref.schema_walk(js.START, text, dfa)
    named = {"start": js.START, "in a forced key": at(b'{"na'), "in a free string": at(b'{"name":"va'),
             "mid escape": at(b'{"name":"a\\'), "mid UTF-8": at(b'{"name":"\xe2\x82'), "mid number": at(b'{"name":"","n":-12.5e'),
             "inside an enum": at(b'{"name":"","n":1,"color":"gr'),
             "after a value in an array": at(b'{"name":"","n":1,"color":"red","tags":[1 '),
             "before the last }": at(b'{"name":"","n":1,"color":"red","tags":[],"ok":true '),
             "done": at(b'{"name":"","n":1,"color":"red","tags":[],"ok":true}')}
    assert named["done"] == js.DONE and js.DEAD not in named.values()
    tabs, pool = ops.JsonTables(table, cuda), _pool(cuda, [dfa], n=2, bufs=(1,))
    k = len(named)
    slots = np.random.default_rng(k).permutation(k + 2)[:k]
    state = np.zeros((k + 2, 4), np.int32)
    state[slots, 0], state[slots, 3] = list(named.values()), 2
    rows = np.stack([np.arange(k), slots, np.ones(k)], axis=1).astype(np.int32)
    mask_tab = torch.full((1 + k + 2, table.W), SENTINEL, dtype=torch.int32, device=cuda)
    ops.schema_mask(tabs, pool, torch.from_numpy(rows).to(cuda), k, torch.from_numpy(state).to(cuda), mask_tab, 1)
    mt = mask_tab.cpu().numpy()
    for (name, s), sl in zip(named.items(), slots):
        w = ref.schema_mask_ref(s, dfa, table)
        g = mt[1 + sl].view(np.uint32)
        assert np.array_equal(g, w), f"{name}: {int((g != w).sum())} of {w.size} words differ"
        print(name, "allows", int(np.unpackbits(w.view(np.uint8)).sum()), "tokens")
    last = mt[1 + slots[-1]].view(np.uint32)
    assert np.flatnonzero(np.unpackbits(last.view(np.uint8), bitorder="little")).tolist() == sorted(tok.eos_ids)


def test_advance_kernel_walks_the_documents_on_the_device(cuda, three_tables):
    table = synthetic_table(1000)
    tabs = ops.JsonTables(table, cuda)
    pool = _pool(cuda, [d for d, _ in three_tables])
    items = [(b, d, tokenize(table, doc)) for b, (d, docs) in zip((3, 0, 4), three_tables) for doc in docs]
    eos = int(table.eos_ids[0])
    k, steps = len(items), max(len(t) for _, _, t in items) + 1
    slots = np.random.default_rng(2).permutation(k + 3)[:k]
    rows = torch.from_numpy(np.stack([np.arange(k), slots, [b for b, _, _ in items]], axis=1).astype(np.int32)).to(cuda)
    st0 = np.zeros((k + 3, 4), np.int32)
    st0[slots, 3] = [b + 1 for b, _, _ in items]
    st0[np.setdiff1d(np.arange(k + 3), slots)] = [7, 8, 9, 0]  # (other slots: anything, and it must stay)
    state = torch.from_numpy(st0).to(cuda)
    want = [js.START] * k
    for j in range(steps):
        ids = [t[j] if j < len(t) else eos for _, _, t in items]  # (a finished document draws the EOS and stays DONE)
        ops.schema_advance(tabs, pool, rows, torch.tensor(ids, device=cuda), state)
        want = [ref.schema_advance_ref(s, t, d, table) for s, t, (_, d, _) in zip(want, ids, items)]
        got = state.cpu().numpy()
        for i, sl in enumerate(slots):
            assert got[sl].tolist() == [want[i], 0, 0, items[i][0] + 1], (j, i)
        assert (got[np.setdiff1d(np.arange(k + 3), slots)] == [7, 8, 9, 0]).all()
    assert all(s == js.DONE for s in want)
    # a token the state rejects, an id without bytes, ids outside the vocabulary: DEAD, as the reference; DEAD stays
    d = three_tables[2][0]
    s0 = ref.schema_walk(js.START, b'{"s":"x","i":1', d)
    bad = [tokenize(table, b":")[0], 3, table.V + 5, -1, tokenize(table, b",")[0]]
    state = torch.tensor([[s0, 0, 0, 5]] * 4 + [[js.DEAD, 0, 0, 5]], dtype=torch.int32, device=cuda)
    rows = torch.tensor([[i, i, 4] for i in range(5)], dtype=torch.int32, device=cuda)
    ops.schema_advance(tabs, pool, rows, torch.tensor(bad, device=cuda), state)
    for i, t in enumerate(bad):
        assert state[i].cpu().tolist() == [js.DEAD, 0, 0, 5]
        assert ref.schema_advance_ref(s0 if i < 4 else js.DEAD, t, d, table) == js.DEAD


def test_sampler_reads_device_written_masks_in_a_mixed_batch(cuda):
    """Schema rows, JSON-mode rows, tool-mask rows, forced rows and plain rows at T = 0.9 over the Llama-3 vocabulary:
    the schema rows draw what ``sample_replay`` draws under the reference mask, every other row what it draws without
    the schema rows."""
    from kafka_llm_service_amd.engine.tokenizer import get_tokenizer

    tok = get_tokenizer()
    table = jm.table_for(tok, tok.eos_ids)
    B, V = 16, table.V
    x = (torch.randn(B, V, generator=torch.Generator().manual_seed(5)) * 3).clamp(-15.5, 15.5).to(torch.bfloat16)
    sA, sB = SCHEMAS["scalars"][0], SCHEMAS["pydantic_like"][0]
    tA, tB = js.canonical_text(sA), js.canonical_text(sB)
    texts = {1: (sA, b""), 5: (sB, b'{"items":[{"name":"a'), 9: (sA, b'{"s":"x","i":-'), 13: (sB, b'{"items":[],"ok":false}'),
             6: (sA, b'{"s":"\xc3')}
    jtexts = {3: b'{"a":[1', 12: b'{"a'}
    seqs, rows, g = [], [], torch.Generator().manual_seed(9)
    for i in range(B):
        p = dict(temperature=0.9)
        if i in texts:
            p["json_schema"] = tA if texts[i][0] is sA else tB
        elif i in jtexts:
            p["json_mode"] = True
        s = Sequence(f"r{i}", [1], SamplingParams(**p))
        if i in texts or i in jtexts:
            rows.append((i, s, None))
        elif i % 4 == 0:
            rows.append((i, s, torch.randint(0, V, (int(torch.randint(2, 3000, (1,), generator=g)),),
                                             generator=g).tolist()))
        elif i % 4 == 2:
            rows.append((i, s, [int(torch.randint(0, V, (1,), generator=g))]))
        seqs.append(s)

    def run(dev, with_schema):
        lp = LogitsProcessor(dev, V, max_slots=32, mask_rows=16, json_slots=8)
        lp.set_json_table(table)
        use = [r for r in rows if with_schema or r[1].params.json_schema is None]
        proc, upd = lp.build(use, B, n_decode=0)
        up = torch.from_numpy if str(dev) == "cpu" else (lambda a: torch.from_numpy(a).to(dev))
        lp.apply(upd, up)
        sr, jr = lp.schema_rows(proc), lp.json_rows(proc)
        if sr is not None:  # the states the rows stand in, seeded like a re-prefill would
            st = np.stack([js.state_record(ref.schema_walk(js.START, texts[i][1], js.compile_schema(texts[i][0])), b)
                           for i, _, b in sr.tolist()])
            lp.jstate.index_copy_(0, up(sr[:, 1].astype(np.int64)), up(st))
        st = np.stack([jm.state_record(ref.json_walk(jm.START_STATE, jtexts[i])) for i, _ in jr.tolist()])
        lp.jstate.index_copy_(0, up(jr[:, 1].astype(np.int64)), up(st))
        tabs, mt = lp.json_tables(), lp.tables()[0]
        ops.json_mask(tabs, up(jr), lp.jstate, mt, lp.n_mask_rows)
        if sr is not None:
            ops.schema_mask(tabs, lp.schema_pool(), up(sr), B, lp.jstate, mt, lp.n_mask_rows)
        return lp, proc, sr

    lp_c, proc, sr = run("cpu", True)
    assert sr[:, 0].tolist() == sorted(texts) and len(set(sr[:, 2].tolist())) == 2
    temp, seeds, step = torch.full((B,), 0.9), torch.arange(B, dtype=torch.long) * 13 + 1, torch.tensor([4])
    pd_c = torch.from_numpy(proc)
    rep = ref.sample_replay(x, temp, None, None, seeds, step, proc=pd_c, mask_tab=lp_c.tables()[0],
                            counts=lp_c.tables()[1], nsplit=8)
    msg = _capped(rep, "mixed schema batch")
    for i, (schema, text) in texts.items():  # the replay's own draws respect the reference masks
        dfa = js.compile_schema(schema)
        keep = np.unpackbits(ref.schema_mask_ref(ref.schema_walk(js.START, text, dfa), dfa, table).view(np.uint8),
                             bitorder="little")
        assert keep[int(rep.tokens[i])]
    assert int(rep.tokens[13]) in tok.eos_ids  # (the closed document)
    lp_g, proc_g, sr_g = run(cuda, True)
    assert np.array_equal(proc_g, proc) and np.array_equal(sr_g, sr)
    assert torch.equal(lp_g.tables()[0].cpu(), lp_c.tables()[0])  # every mask row, device-written or uploaded
    xg = x.to(cuda)
    kw = dict(mask_tab=lp_g.tables()[0], counts=lp_g.tables()[1], bias_tab=lp_g.bias_table())
    tok_g = ops.sample(xg, temp.to(cuda), None, None, seeds.to(cuda), step.to(cuda), proc=pd_c.to(cuda), **kw)
    _same(tok_g, rep, msg)
    ops.schema_advance(lp_g.json_tables(), lp_g.schema_pool(), torch.from_numpy(sr_g).to(cuda), tok_g, lp_g.jstate)
    for i, slot, b in sr_g.tolist():
        dfa = js.compile_schema(texts[i][0])
        want = ref.schema_advance_ref(ref.schema_walk(js.START, texts[i][1], dfa), int(tok_g[i]), dfa, table)
        assert lp_g.jstate[slot].cpu().tolist() == [want, 0, 0, b + 1] and want != js.DEAD
    # the same batch without the schema rows: every other row draws the same token
    lp_n, proc_n, sr_n = run(cuda, False)
    assert sr_n is None and lp_n.spool is None
    tok_n = ops.sample(xg, temp.to(cuda), None, None, seeds.to(cuda), step.to(cuda),
                       proc=torch.from_numpy(proc_n).to(cuda), mask_tab=lp_n.tables()[0], counts=lp_n.tables()[1],
                       bias_tab=lp_n.bias_table())
    others = [i for i in range(B) if i not in texts]
    assert torch.equal(tok_n[others], tok_g[others]) and not torch.equal(tok_n[sorted(texts)], tok_g[sorted(texts)])


OK_SCHEMA = obj({"ok": BOOL})
DEEP_SCHEMA = SCHEMAS["pydantic_like"][0]


def _alive(dfa, table, out, eos) -> int:
    s = js.START
    for i, t in enumerate(out):
        if s == js.DONE:
            assert t in eos, (i, t)
            continue
        s = ref.schema_advance_ref(s, t, dfa, table)
        assert s != js.DEAD, (i, t, table.bytes_of(t))
    return s


def test_engine_eager_and_graphs_emit_documents_of_the_schema(cuda):
    """tiny-llama with two steps in flight, eager and with hipGraphs: json_schema requests beside a JSON-mode and a
    plain one. The engine's own logits are recorded at every sampler launch, and every greedy schema row's token must
    be the CPU reference's choice on those logits: the first argmax under ``schema_mask_ref`` of the reference state,
    seeded where the plan seeds it, over the table the plan shipped, advanced by ``schema_advance_ref`` (the T = 1 row's
    draws are held to the mask here; the draw itself is replayed in the mixed-batch test above). The
    ``{"ok": boolean}`` request (whitespace-only tokens biased away, counted on the CPU: at most 300) finishes with
    "stop" and its text parses and validates. The graphed engine emits the same tokens; the plain request equals
    its run without the structured ones."""
    from kafka_llm_service_amd.engine.tokenizer import tokenizer_for_model

    g = torch.Generator().manual_seed(3)
    prompts = [[128000] + torch.randint(0, 5000, (m,), generator=g).tolist() for m in (17, 23, 9, 30, 12)]
    n = 14
    cfg = dict(model="tiny-llama", device="cuda:0", num_kv_blocks=256, max_model_len=2048)
    eager = LLMEngine(EngineConfig(**cfg))
    eager.runner.fixed_decode_items = True  # the graph engine's decode split, so both sum in the same order
    table = eager._json_table()
    tok = tokenizer_for_model(eager.model_cfg)
    ws = [i for i in range(table.V) if table.lens[i] and not table.bytes_of(i).strip(b" \t\n\r")]
    assert 0 < len(ws) <= 300
    t_ok, t_deep = js.canonical_text(OK_SCHEMA), js.canonical_text(DEEP_SCHEMA)
    sps = [SamplingParams(temperature=0.0, max_tokens=40, json_schema=t_ok, logit_bias={i: -100.0 for i in ws}),
           SamplingParams(temperature=0.0, max_tokens=n, ignore_eos=True),
           SamplingParams(temperature=0.0, max_tokens=n, json_schema=t_deep, ignore_eos=True),
           SamplingParams(temperature=0.0, max_tokens=n, json_mode=True, ignore_eos=True),
           SamplingParams(temperature=1.0, seed=7, max_tokens=n, json_schema=t_deep, ignore_eos=True)]
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
    assert seqs[0].finish_reason == "stop" and got[0][-1] in eager.eos
    text = tok.decode(got[0])
    assert conforms(OK_SCHEMA, text.encode()), text
    d_ok, d_deep = js.compile_schema(OK_SCHEMA), js.compile_schema(DEEP_SCHEMA)
    assert _alive(d_ok, table, got[0], eager.eos) == js.DONE
    for j in (2, 4):
        assert len(got[j]) == n
        _alive(d_deep, table, got[j], eager.eos)
    st = eager.runner.lp.stats
    assert st["schema_seeds"] == 3 and st["schema_table_uploads"] == 2 and st["json_seeds"] == 1
    state, tabs, checked = {}, {}, 0
    for logits, sp, toks in records:
        if sp.upd is not None:
            for buf, cls, trans in sp.upd.schema_tabs:
                tabs[buf] = js.SchemaDfa(cls.copy(), trans.copy(), "")
            for slot, rec in zip(sp.upd.json_slots.tolist(), sp.upd.json_states.tolist()):
                if rec[3]:
                    state[slot] = rec[0]
        if sp.schema_rows is None:
            continue
        x, toks = logits.float().cpu(), toks.cpu()
        for i, slot, buf in sp.schema_rows.tolist():
            keep = torch.from_numpy(np.unpackbits(ref.schema_mask_ref(state[slot], tabs[buf], table).view(np.uint8),
                                                  bitorder="little")[:table.V].astype(bool))
            t = int(toks[i])
            assert keep[t], (i, slot, t)
            if sp.temp[i] == 0:  # every greedy schema row: the first argmax of (logits + bias) under the mask
                row = x[i].clone()
                if sp.proc[i, 6]:  # (the request's logit_bias: its count rides in the row, the entries are known here)
                    assert sp.proc[i, 6] == len(ws)
                    row[ws] += -100.0
                row = row.masked_fill(~keep, float("-inf"))
                assert t == int(torch.nonzero(row == row.max())[0]), (i, slot, t)
                checked += 1
            state[slot] = ref.schema_advance_ref(state[slot], t, tabs[buf], table)
    # requests 0 and 2, every token — and the one launch planned ahead of request 0's EOS landing (two steps are in
    # flight), whose draw in DONE is an EOS again and is dropped
    assert len(got[0]) + n <= checked <= len(got[0]) + n + 1 and len(tabs) == 2
    assert tabs[min(tabs)].tobytes() in (d_ok.tobytes(), d_deep.tobytes())
    graphed = LLMEngine(EngineConfig(**cfg, use_graphs=True), model=eager.model)
    got_g = graphed.generate(prompts, sps)
    assert not graphed.runner.graphs.disabled and got_g == got
    # the plain request alone: the same tokens, and its decode steps replay
    more = graphed.generate(prompts[1:2], [sps[1]])
    assert graphed.runner.graphs.stats["replays"] > 0 and more[0] == got[1]


def test_engine_preemption_reseeds_schema_rows(cuda):
    eng = LLMEngine(EngineConfig(model="tiny-llama", device="cuda:0", num_kv_blocks=12, max_model_len=2048))
    table = eng._json_table()
    g = torch.Generator().manual_seed(5)
    prompts = [[128000] + torch.randint(0, 5000, (50,), generator=g).tolist() for _ in range(4)]
    sp = SamplingParams(temperature=0.0, max_tokens=20, json_schema=js.canonical_text(DEEP_SCHEMA), ignore_eos=True)
    got = eng.generate(prompts, sp)
    st = eng.runner.lp.stats
    assert eng.sched.num_preemptions > 0 and st["schema_seeds"] > 4 and st["schema_table_uploads"] == 1
    dfa = js.compile_schema(DEEP_SCHEMA)
    for o in got:
        assert len(o) == 20
        _alive(dfa, table, o, eng.eos)
