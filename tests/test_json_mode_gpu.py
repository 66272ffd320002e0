"""JSON mode on the GPU: the mask and advance kernels (ops/csrc/json_mask.hip) against the CPU definition word for word
and record for record, the sampler over device-written mask rows, and the engine eager and under hipGraphs against
the CPU reference sampler and automaton on the engine's own logits. Integers throughout: every comparison is an
equality."""
from __future__ import annotations

import json

import numpy as np
import pytest
import torch

from kafka_llm_service_amd import ops
from kafka_llm_service_amd.engine import json_mode as jm
from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
from kafka_llm_service_amd.engine.logits_proc import LogitsProcessor
from kafka_llm_service_amd.engine.sequence import SamplingParams, Sequence
from kafka_llm_service_amd.ops import reference as ref
from test_json_mode import VALID, _nest, alive_prefixes, corpus_states, synthetic_table, tokenize
from test_sampler_replay import _capped, _same

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A5A5A


def _device_masks(cuda, table, states, row0=3, spare=2):
    """One launch over ``states`` (row i -> slot: a permutation, so no slot is its row's index); returns (mask rows by
    state, the whole mask table) — rows outside [row0, row0 + slots) must keep the sentinel."""
    tabs = ops.JsonTables(table, cuda)
    k = len(states)
    slots = np.random.default_rng(k).permutation(k + spare)[:k]
    state = np.zeros((k + spare, 4), np.int32)
    for s, st in zip(slots, states):
        state[s] = jm.state_record(st)
    rows = np.stack([np.arange(k)[::-1], slots], axis=1).astype(np.int32)
    mask_tab = torch.full((row0 + k + spare + 1, table.W), SENTINEL, dtype=torch.int32, device=cuda)
    ops.json_mask(tabs, torch.from_numpy(rows).to(cuda), torch.from_numpy(state).to(cuda), mask_tab, row0)
    mt = mask_tab.cpu().numpy()
    return [mt[row0 + s].view(np.uint32) for s in slots], mt, set(int(row0 + s) for s in slots)


@pytest.fixture(scope="module")
def states():
    return corpus_states()


@pytest.mark.parametrize("V", [1, 31, 64, 65, 1000])
def test_mask_kernel_equals_reference_on_synthetic_vocabularies(cuda, V, states):
    table = synthetic_table(V)
    assert table.lens.max() == (64 if V >= 3 else 0) and (V < 31 or table.lens[3] == 0)
    got, mt, written = _device_masks(cuda, table, states)
    for st, g in zip(states, got):
        assert np.array_equal(g, ref.json_mask_ref(st, table)), (V, st, jm.STATE_NAMES[st[0]])
    for r in range(mt.shape[0]):
        if r not in written:
            assert (mt[r] == SENTINEL).all(), f"V {V}: row {r} is no slot's row and was written"
    nbits = sum(int(np.unpackbits(g.view(np.uint8)).sum()) for g in got)
    assert V < 31 or nbits > len(states)  # (the masks are not all empty)


def test_mask_kernel_on_the_llama3_table(cuda):
    from kafka_llm_service_amd.engine.tokenizer import get_tokenizer

    tok = get_tokenizer()
    table = jm.table_for(tok, tok.eos_ids)
    assert table.V == 128256
    at = lambda text: ref.json_walk(jm.START_STATE, text)
    named = {"start": jm.START_STATE, "in key": at(b'{"ke'), "in string": at(b'{"k":"va'), "mid escape": at(b'{"k":"a\\'),
             "mid \\u": at(b'{"k":"\\u00'), "mid UTF-8": at(b'{"k":"\xe2\x82'), "after value in object": at(b'{"k":1 '),
             "after value in array": at(b'{"k":[1 '), "mid number": at(b'{"k":[-12.5e'), "depth 32": at(_nest(32)[:-32]),
             "done": at(b'{"k":[]}')}
    assert named["depth 32"][1] == 32 and named["done"] == (jm.DONE, 0, 0)
    assert all(st[0] != jm.DEAD for st in named.values())
    got, _, _ = _device_masks(cuda, table, list(named.values()))
    for (name, st), g in zip(named.items(), got):
        w = ref.json_mask_ref(st, table)
        assert np.array_equal(g, w), f"{name}: {int((g != w).sum())} of {w.size} words differ"
        print(name, "allows", int(np.unpackbits(w.view(np.uint8)).sum()), "tokens")
    assert np.flatnonzero(np.unpackbits(got[-1].view(np.uint8), bitorder="little")).tolist() == sorted(tok.eos_ids)


def test_advance_kernel_walks_the_corpus_on_the_device(cuda):
    table = synthetic_table(1000)
    tabs = ops.JsonTables(table, cuda)
    docs = [tokenize(table, d) for d in VALID]
    eos = int(table.eos_ids[0])
    k, steps = len(docs), max(len(d) for d in docs) + 1
    slots = np.random.default_rng(1).permutation(k + 3)[:k]
    rows = torch.from_numpy(np.stack([np.arange(k), slots], axis=1).astype(np.int32)).to(cuda)
    state = torch.zeros(k + 3, 4, dtype=torch.int32, device=cuda)  # (all zero: START at depth 0)
    want = [jm.START_STATE] * k
    for j in range(steps):
        ids = [d[j] if j < len(d) else eos for d in docs]  # (a finished document draws the EOS and stays DONE)
        ops.json_advance(tabs, rows, torch.tensor(ids, device=cuda), state)
        want = [ref.json_advance_ref(st, t, table) for st, t in zip(want, ids)]
        got = state.cpu().numpy()
        for i, s in enumerate(slots):
            assert jm.record_state(got[s]) == want[i] and got[s, 3] == 0, (j, VALID[i], ids[i])
        assert not got[np.setdiff1d(np.arange(k + 3), slots)].any()  # the other slots are untouched
    assert all(st == (jm.DONE, 0, 0) for st in want)
    # a token that the state rejects, an id without bytes and an id outside the vocabulary: DEAD, as the reference
    st0 = ref.json_walk(jm.START_STATE, b'{"a":1')
    bad = [tokenize(table, b":")[0], 3, table.V + 5, -1]
    state = torch.from_numpy(np.stack([jm.state_record(st0)] * 4)).to(cuda)
    rows = torch.tensor([[i, i] for i in range(4)], dtype=torch.int32, device=cuda)
    ops.json_advance(tabs, rows, torch.tensor(bad, device=cuda), state)
    for i, t in enumerate(bad):
        assert jm.record_state(state[i].cpu().numpy()) == ref.json_advance_ref(st0, t, table) == (jm.DEAD,) + st0[1:]


def test_sampler_reads_device_written_masks_in_a_mixed_batch(cuda):
    """JSON rows, tool-mask rows, forced rows and plain rows at T = 0.9 over the Llama-3 vocabulary: the JSON rows draw
    what ``sample_replay`` draws under the reference mask, and the other rows what they draw without the JSON rows."""
    from kafka_llm_service_amd.engine.tokenizer import get_tokenizer

    tok = get_tokenizer()
    table = jm.table_for(tok, tok.eos_ids)
    B, V = 16, table.V
    x = (torch.randn(B, V, generator=torch.Generator().manual_seed(5)) * 3).clamp(-15.5, 15.5).to(torch.bfloat16)
    texts = [b"", b'{"a', b'{"a":', b'{"a":[1', b'{"a":{"b":"\xc3', b'{}']
    seqs, rows, g = [], [], torch.Generator().manual_seed(9)
    for i in range(B):
        json_row = i % 4 == 1 or i in (6, 12)
        s = Sequence(f"r{i}", [1], SamplingParams(temperature=0.9, json_mode=json_row))
        if json_row:
            rows.append((i, s, None))
        elif i % 4 == 0:
            rows.append((i, s, torch.randint(0, V, (int(torch.randint(2, 3000, (1,), generator=g)),),
                                             generator=g).tolist()))
        elif i % 4 == 2:
            rows.append((i, s, [int(torch.randint(0, V, (1,), generator=g))]))
        seqs.append(s)
    jrow_ids = [i for i, s, _ in rows if s.params.json_mode]
    assert len(jrow_ids) == 6

    def run(dev, with_json):
        lp = LogitsProcessor(dev, V, max_slots=32, mask_rows=16, json_slots=8)
        lp.set_json_table(table)
        use = [r for r in rows if with_json or not r[1].params.json_mode]
        proc, upd = lp.build(use, B, n_decode=0)
        up = torch.from_numpy if str(dev) == "cpu" else (lambda a: torch.from_numpy(a).to(dev))
        lp.apply(upd, up)
        jr = lp.json_rows(proc)
        if jr is not None:  # the states the rows stand in: one text each, seeded like a re-prefill would
            st = np.stack([jm.state_record(ref.json_walk(jm.START_STATE, texts[j])) for j in range(len(jr))])
            lp.jstate.index_copy_(0, up(jr[:, 1].astype(np.int64)), up(st))
        return lp, proc, jr

    lp_c, proc, jr = run("cpu", True)
    assert jr[:, 0].tolist() == jrow_ids and jr[0, 1] != jr[0, 0]
    ops.json_mask(lp_c.json_tables(), torch.from_numpy(jr), lp_c.jstate, lp_c.tables()[0], lp_c.n_mask_rows)
    temp, seeds, step = torch.full((B,), 0.9), torch.arange(B, dtype=torch.long) * 13 + 1, torch.tensor([4])
    pd_c = torch.from_numpy(proc)
    rep = ref.sample_replay(x, temp, None, None, seeds, step, proc=pd_c, mask_tab=lp_c.tables()[0],
                            counts=lp_c.tables()[1], nsplit=8)
    msg = _capped(rep, "mixed JSON batch")
    for j, i in enumerate(jrow_ids):  # the replay's own draws respect the reference masks
        keep = np.unpackbits(ref.json_mask_ref(ref.json_walk(jm.START_STATE, texts[j]), table).view(np.uint8),
                             bitorder="little")
        assert keep[int(rep.tokens[i])]
    lp_g, proc_g, jr_g = run(cuda, True)
    assert np.array_equal(proc_g, proc)
    jr_d, xg = torch.from_numpy(jr_g).to(cuda), x.to(cuda)
    kw = dict(mask_tab=lp_g.tables()[0], counts=lp_g.tables()[1], bias_tab=lp_g.bias_table())
    ops.json_mask(lp_g.json_tables(), jr_d, lp_g.jstate, lp_g.tables()[0], lp_g.n_mask_rows)
    tok_g = ops.sample(xg, temp.to(cuda), None, None, seeds.to(cuda), step.to(cuda), proc=pd_c.to(cuda), **kw)
    _same(tok_g, rep, msg)
    ops.json_advance(lp_g.json_tables(), jr_d, tok_g, lp_g.jstate)
    for j, (i, slot) in enumerate(jr_g.tolist()):
        want = ref.json_advance_ref(ref.json_walk(jm.START_STATE, texts[j]), int(tok_g[i]), table)
        assert jm.record_state(lp_g.jstate[slot].cpu().numpy()) == want and want[0] != jm.DEAD
    # the same batch without the JSON rows: every other row draws the same token
    lp_n, proc_n, jr_n = run(cuda, False)
    assert jr_n is None
    tok_n = ops.sample(xg, temp.to(cuda), None, None, seeds.to(cuda), step.to(cuda),
                       proc=torch.from_numpy(proc_n).to(cuda), mask_tab=lp_n.tables()[0], counts=lp_n.tables()[1],
                       bias_tab=lp_n.bias_table())
    others = [i for i in range(B) if i not in jrow_ids]
    assert torch.equal(tok_n[others], tok_g[others]) and not torch.equal(tok_n[jrow_ids], tok_g[jrow_ids])


def test_engine_eager_and_graphs_emit_json(cuda):
    """tiny-llama with two steps in flight (async scheduling), eager and with hipGraphs. The engine's own logits are
    recorded at every sampler launch, and every greedy JSON row's token must equal the CPU reference's choice on those
    logits: the argmax (first index) under ``json_mask_ref`` of the reference state, which is seeded where the plan
    seeds it and advanced by ``json_advance_ref``. (The CPU engine draws its random weights from another generator,
    so its tokens are not comparable; its sampler and automaton are, on the same logits.) The graphed engine on the
    same weights emits the same tokens, runs JSON steps eagerly and replays the others."""
    g = torch.Generator().manual_seed(3)
    prompts = [[128000] + torch.randint(0, 5000, (m,), generator=g).tolist() for m in (17, 23, 9, 30)]
    n = 12
    js = SamplingParams(temperature=0.0, max_tokens=n, json_mode=True, ignore_eos=True)
    sps = [js, SamplingParams(temperature=0.0, max_tokens=n, ignore_eos=True), js,
           SamplingParams(temperature=1.0, seed=7, max_tokens=n, json_mode=True, ignore_eos=True)]
    cfg = dict(model="tiny-llama", device="cuda:0", num_kv_blocks=256, max_model_len=2048)
    eager = LLMEngine(EngineConfig(**cfg))
    eager.runner.fixed_decode_items = True  # the graph engine's decode split, so both sum in the same order
    assert eager.cfg.async_scheduling
    table = eager._json_table()
    records, orig = [], eager.runner.sample_device

    def sample_device(logits, sp):
        toks = orig(logits, sp)
        records.append((logits.clone(), sp, toks.clone()))  # (read after the run: nothing waits for the GPU here)
        return toks

    eager.runner.sample_device = sample_device
    got = eager.generate(prompts, sps)
    eager.runner.sample_device = orig
    for j in (0, 2, 3):
        assert len(got[j]) == n
        alive_prefixes(table, got[j], eager.eos)
    assert eager.stats["planned_ahead"] > 0 and eager.runner.lp.stats["json_seeds"] == 3
    assert eager.stats.get("grammar_rollbacks", 0) == 0
    state, checked = {}, 0
    for logits, sp, toks in records:
        if sp.upd is not None:
            for slot, rec in zip(sp.upd.json_slots.tolist(), sp.upd.json_states):
                state[slot] = jm.record_state(rec)
        if sp.json_rows is None:
            continue
        x, toks = logits.float().cpu(), toks.cpu()
        for i, slot in sp.json_rows.tolist():
            keep = torch.from_numpy(np.unpackbits(ref.json_mask_ref(state[slot], table).view(np.uint8),
                                                  bitorder="little")[:table.V].astype(bool))
            t = int(toks[i])
            assert keep[t], (i, slot, t)
            if sp.temp[i] == 0:
                row = x[i].masked_fill(~keep, float("-inf"))
                assert t == int(torch.nonzero(row == row.max())[0]), (i, slot, t)
                checked += 1
            state[slot] = ref.json_advance_ref(state[slot], t, table)
    assert checked >= 2 * n - 2
    graphed = LLMEngine(EngineConfig(**cfg, use_graphs=True), model=eager.model)
    got_g = graphed.generate(prompts, sps)
    assert not graphed.runner.graphs.disabled and got_g == got
    # a step with JSON rows runs eagerly; without them the decode steps replay
    more = graphed.generate(prompts[:2], [sps[1], sps[1]])
    assert graphed.runner.graphs.stats["replays"] > 0 and more[1] == got[1]


def test_engine_logit_bias_closes_and_preemption_resumes(cuda):
    from kafka_llm_service_amd.engine.tokenizer import tokenizer_for_model

    eng = LLMEngine(EngineConfig(model="tiny-llama", device="cuda:0", num_kv_blocks=256, max_model_len=2048))
    tok = tokenizer_for_model(eng.model_cfg)
    table = eng._json_table()
    push = {tok.encode(s)[0]: 40.0 for s in ('"', ":", "}")}
    for seed in (3, 4):
        sp = SamplingParams(temperature=1.0, seed=seed, max_tokens=64, json_mode=True, logit_bias=push)
        seq = eng.add_request(f"bias-{seed}", [128000, 60, 61], sp)
        while not seq.finished:
            eng.step()
        assert seq.finish_reason == "stop" and seq.output_ids[-1] in eng.eos
        assert alive_prefixes(table, seq.output_ids, eng.eos) == (jm.DONE, 0, 0)
        assert isinstance(json.loads(tok.decode(seq.output_ids)), dict)
    # preemption: a KV-starved engine on the same weights re-prefills JSON sequences and continues from the seeded state
    g = torch.Generator().manual_seed(5)
    prompts = [[128000] + torch.randint(0, 5000, (50,), generator=g).tolist() for _ in range(4)]
    sp = SamplingParams(temperature=0.0, max_tokens=20, json_mode=True, ignore_eos=True)
    small = LLMEngine(EngineConfig(model="tiny-llama", device="cuda:0", num_kv_blocks=12, max_model_len=2048),
                      model=eng.model)
    got = small.generate(prompts, sp)
    assert small.sched.num_preemptions > 0 and small.runner.lp.stats["json_seeds"] > 4
    for o in got:
        assert len(o) == 20
        alive_prefixes(table, o, eng.eos)
