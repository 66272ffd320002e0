"""``logit_bias`` without a GPU: the request schema, the host-side bias rows of ``LogitsProcessor`` (content keys, LRU,
bounds), the TP wire format, the fp32 reference (``(x - penalties) + b``, then the grammar mask) and the whole path on
the CPU engine and through the chat route (a +100 bias forces its token, a -100 bias bans the greedy one, logprobs stay
those of the raw logits, an id outside the vocabulary is a 400)."""
import json
import pickle
import re
from pathlib import Path

import numpy as np
import pytest
import torch
from fastapi.testclient import TestClient
from pydantic import ValidationError

from kafka_llm_service_amd import ops
from kafka_llm_service_amd.db.local import MemoryDBClient
from kafka_llm_service_amd.engine import step_plan
from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
from kafka_llm_service_amd.engine.logits_proc import BIAS_ROWS, LogitsProcessor, pack_bits
from kafka_llm_service_amd.engine.sequence import SamplingParams, Sequence
from kafka_llm_service_amd.engine.step_plan import BIAS_ROW_INTS, LOGIT_BIAS_MAX, HostStep, ProcUpdates, SampleParams
from kafka_llm_service_amd.kafka.types import ChatCompletionRequest
from kafka_llm_service_amd.ops import reference as ref
from kafka_llm_service_amd.server.app import _sampling_kwargs, create_app
from kafka_llm_service_amd.server.state import ServerConfig, ServerState

MSG = [{"role": "user", "content": "hi"}]


def test_one_constant():
    """LOGIT_BIAS_MAX of the kernel header, the reference, the ops module, the plan and the schema agree."""
    hdr = (Path(ops.__file__).parent / "csrc" / "kafka_abi.h").read_text()
    n = int(re.search(r"constexpr int LOGIT_BIAS_MAX = (\d+);", hdr).group(1))
    from kafka_llm_service_amd.kafka import types

    assert n == 300 == LOGIT_BIAS_MAX == ref.LOGIT_BIAS_MAX == ops.LOGIT_BIAS_MAX == types.LOGIT_BIAS_MAX
    assert BIAS_ROW_INTS == 2 * n and BIAS_ROW_INTS * 4 % 16 == 0 and BIAS_ROWS == 512


# ---- schema -----------------------------------------------------------------------------------------------------------
def test_schema():
    req = ChatCompletionRequest(model="m", messages=MSG, logit_bias={"12": 5, "7": -100, "9": 100.0})
    assert _sampling_kwargs(req)["logit_bias"] == {12: 5.0, 7: -100.0, 9: 100.0}
    for bad in ({"12": 101}, {"12": -100.5}, {"x": 1}, {"-1": 1}, {"1.5": 1}, {"": 1}, {" 3": 1}, {"3": float("nan")},
                {"3": float("inf")}, {str(i): 1 for i in range(301)}, {"7": 1, "07": 2}):
        with pytest.raises(ValidationError):
            ChatCompletionRequest(model="m", messages=MSG, logit_bias=bad)
    ChatCompletionRequest(model="m", messages=MSG, logit_bias={str(i): 1 for i in range(300)})
    # 300 non-zero entries are the bound: zero entries beside them do not count
    big = {str(i): (1 if i < 300 else 0) for i in range(400)}
    assert len(_sampling_kwargs(ChatCompletionRequest(model="m", messages=MSG, logit_bias=big))["logit_bias"]) == 300
    for none in (None, {}, {"5": 0, "6": 0.0}):
        kw = _sampling_kwargs(ChatCompletionRequest(model="m", messages=MSG, logit_bias=none))
        assert "logit_bias" not in kw


def test_schema_is_422_on_the_route():
    from kafka_llm_service_amd.llm.stub import ScriptedProvider

    st = ServerState(ServerConfig(backend="stub", sandbox="none"), llm_provider=ScriptedProvider([{"text": "hi"}] * 2),
                     db=MemoryDBClient())
    with TestClient(create_app(state=st)) as c:
        body = {"model": "kafka", "messages": MSG}
        for bad in ({"12": 101}, {"x": 1}, {"-1": 1}, {str(i): 1 for i in range(301)}):
            assert c.post("/v1/chat/completions", json=dict(body, logit_bias=bad)).status_code == 422
        r = c.post("/v1/chat/completions", content=json.dumps(dict(body, logit_bias={"3": 1})).replace("1}", "NaN}"),
                   headers={"content-type": "application/json"})
        # (the schema refuses it, test_schema; the framework cannot echo a NaN in the 422 body it builds, and the
        # app's ValueError handler then answers 400 — as for a NaN in any other numeric field)
        assert r.status_code in (400, 422)
        # the stub provider ignores the field
        r = c.post("/v1/chat/completions", json=dict(body, logit_bias={"12": 50}))
        assert r.status_code == 200 and r.json()["choices"][0]["message"]["content"] == "hi"


def test_sampling_params_field():
    assert SamplingParams().logit_bias is None and SamplingParams(logit_bias={}).logit_bias is None
    assert SamplingParams(logit_bias={4: 0.0}).logit_bias is None
    p = SamplingParams(logit_bias={9: 1.5, 3: -2, 5: 0})
    assert p.logit_bias == ((3, -2.0), (9, 1.5)) and pickle.loads(pickle.dumps(p)).logit_bias == p.logit_bias
    assert SamplingParams(logit_bias=[(9, 1.5), (3, -2.0)]).logit_bias == p.logit_bias
    for bad in ({-1: 1.0}, {3: 100.5}, {3: float("nan")}, [(3, 1.0), (3, 2.0)], {i: 1.0 for i in range(301)}):
        with pytest.raises(ValueError):
            SamplingParams(logit_bias=bad)


# ---- LogitsProcessor --------------------------------------------------------------------------------------------------
def _seq(i, **kw):
    return Sequence(f"r{i}", [1], SamplingParams(**kw))


def _row_pairs(tab, proc_row):
    r, n = int(proc_row[5]), int(proc_row[6])
    w = tab[r].numpy()
    return tuple(zip(w[:n].tolist(), w[LOGIT_BIAS_MAX:LOGIT_BIAS_MAX + n].view(np.float32).tolist()))


def test_equal_objects_share_one_row():
    V = 1000
    lp = LogitsProcessor("cpu", V, max_slots=8)
    bias = {7: 2.5, 999: -100.0, 0: 0.125}
    seqs = [_seq(0, logit_bias=bias), _seq(1), _seq(2, logit_bias=dict(reversed(list(bias.items())))),
            _seq(3, presence_penalty=0.5), _seq(4, logit_bias={7: 2.5})]
    rows = [(i, s, None) for i, s in enumerate(seqs) if i != 1]
    proc, upd = lp.build(rows, 5)
    assert proc[0, 5] == proc[2, 5] and proc[0, 6] == proc[2, 6] == 3 and proc[4, 6] == 1 and proc[4, 5] != proc[0, 5]
    assert upd.bias_rows.tolist() == [proc[0, 5], proc[4, 5]] and upd.bias_words.shape == (2, BIAS_ROW_INTS)
    assert lp.stats["bias_uploads"] == 2 and lp.stats["bias_rows_used"] == 3
    # rows without a bias keep ints 5..7 zero (the untouched row 1 and the penalty-only row 3)
    assert (proc[[1, 3], 5:8] == 0).all() and (proc[:, 7] == 0).all()
    assert proc[3, 2] >= 0 and (proc[[0, 2, 4], 2] == -1).all() and (proc[:, 0] == 0).all()
    lp.apply(upd, torch.from_numpy)
    assert lp.tables()[0] is lp.mask_tab and len(lp.tables()) == 2
    tab = lp.bias_table()
    assert tab.shape == (BIAS_ROWS, BIAS_ROW_INTS) and tab.dtype == torch.int32
    assert _row_pairs(tab, proc[0]) == ((0, 0.125), (7, 2.5), (999, -100.0)) and _row_pairs(tab, proc[4]) == ((7, 2.5),)
    # the next turn of the same threads: indices only, nothing to upload
    proc2, upd2 = lp.build(rows, 5)
    assert (proc2 == proc).all() and upd2.bias_rows.size == 0 and lp.stats["bias_uploads"] == 2


def test_513_sets_evict_the_least_recently_used_row():
    V = 2048
    lp = LogitsProcessor("cpu", V, max_slots=8)
    tab = lp.bias_table()
    sets = [{i: 1.0, 1000 + i: -0.5} for i in range(513)]

    def step(ids):
        proc, upd = lp.build([(j, _seq(j, logit_bias=sets[i]), None) for j, i in enumerate(ids)], len(ids))
        lp.apply(upd, torch.from_numpy)
        assert len(set(proc[:, 5].tolist())) == len(set(ids))  # a row used by this step is never given away in it
        for j, i in enumerate(ids):  # and after the step's updates every row holds its own pairs
            assert _row_pairs(tab, proc[j]) == tuple(sorted(sets[i].items()))
        return proc, upd

    step(range(0, 256))
    p_b, _ = step(range(256, 512))
    assert lp.stats["bias_uploads"] == 512 and len(lp._brows) == 512
    # set 0 is touched first (now the most recent), set 512 is new: it takes the row of set 1, the least recent
    key = lambda i: ("B", tuple(sorted((t, float(b)) for t, b in sets[i].items())))
    row1 = lp._brows[key(1)]
    proc, upd = step([0, 512, 300])
    assert upd.bias_rows.tolist() == [row1] and proc[1, 5] == row1 and key(1) not in lp._brows
    assert key(0) in lp._brows and proc[2, 5] == p_b[300 - 256, 5] and lp.stats["bias_uploads"] == 513
    # the evicted set comes back as a new row (evicting set 2), with its own pairs again
    step([1, 512])
    assert key(2) not in lp._brows and lp.stats["bias_uploads"] == 514
    # a small table whose rows are all in use by the step: the eviction skips them
    small = LogitsProcessor("cpu", V, max_slots=8, bias_rows=4)
    tab, lp = small.bias_table(), small
    step([0, 1, 2, 3])
    step([0, 1, 4, 5])
    step([5, 6, 0, 7])
    with pytest.raises(RuntimeError):
        lp.build([(j, _seq(j, logit_bias=sets[10 + j]), None) for j in range(5)], 5)


def test_bounds_raise():
    V = 500
    lp = LogitsProcessor("cpu", V, max_slots=8)
    lp.build([(0, _seq(0, logit_bias={V - 1: 1.0}), None)], 1)
    with pytest.raises(ValueError):
        lp.build([(0, _seq(0, logit_bias={V: 1.0}), None)], 1)
    s = _seq(0)
    s.params.logit_bias = tuple((i, 1.0) for i in range(LOGIT_BIAS_MAX + 1))  # past SamplingParams' own check
    with pytest.raises(ValueError):
        lp.build([(0, s, None)], 1)
    s.params.logit_bias = ((-1, 1.0),)
    with pytest.raises(ValueError):
        lp.build([(0, s, None)], 1)
    s.params.logit_bias = ((3, 1.0), (3, 2.0))
    with pytest.raises(ValueError):
        lp.build([(0, s, None)], 1)
    # apply: rows and words must fit the table
    for rows, words in (([BIAS_ROWS], np.zeros((1, BIAS_ROW_INTS), np.int32)), ([0], np.zeros((1, 8), np.int32)),
                        ([-1], np.zeros((1, BIAS_ROW_INTS), np.int32))):
        with pytest.raises(ValueError):
            lp.apply(ProcUpdates(bias_rows=np.asarray(rows, np.int32), bias_words=words), torch.from_numpy)
    # the op: bias entries without a table are an error, not a read through a null pointer
    proc = torch.zeros(1, 8, dtype=torch.int32)
    proc[0, 2], proc[0, 6] = -1, 1
    with pytest.raises(ValueError):
        ops.sample(torch.zeros(1, 16), proc=proc, mask_tab=torch.zeros(1, 1, dtype=torch.int32))


# ---- wire format ------------------------------------------------------------------------------------------------------
def _plan(upd, n=3, proc=True):
    h = HostStep(B=n, T=n, n_rows=n)
    h.i64 = np.arange(3 * n + n, dtype=np.int64)
    h.i32 = np.arange(1 + n, dtype=np.int32)
    p = np.zeros((n, 8), np.int32) if proc else None
    if proc:
        p[:, 2] = -1
        p[1, 5:7] = (4, 2)
    sp = SampleParams(np.full(n, 0.7, np.float32), np.ones(n, np.float32), np.zeros(n, np.int32),
                      np.arange(n, dtype=np.int64), p, False, upd)
    return h, sp


def test_wire_format_round_trip_and_unchanged_without_bias():
    words = np.zeros((2, BIAS_ROW_INTS), np.int32)
    words[0, :2], words[0, LOGIT_BIAS_MAX:LOGIT_BIAS_MAX + 2] = (5, 9), np.array([1.5, -100], np.float32).view(np.int32)
    words[1, 0], words[1, LOGIT_BIAS_MAX] = 77, np.array([100], np.float32).view(np.int32)[0]
    old = dict(mask_rows=np.array([3], np.int32), mask_words=np.arange(5, dtype=np.int32).reshape(1, 5),
               zero_slots=np.array([2, 6], np.int32), dec=np.array([[1, 40]], np.int32))
    h, sp = _plan(ProcUpdates(**old, bias_rows=np.array([4, 511], np.int32), bias_words=words))
    hdr, payload = step_plan.pack_plan(h, sp)
    h2, sp2 = step_plan.unpack_plan(hdr, payload)
    assert np.array_equal(sp2.upd.bias_rows, [4, 511]) and np.array_equal(sp2.upd.bias_words, words)
    assert sp2.upd.bias_words.dtype == np.int32 and np.array_equal(sp2.proc, sp.proc)
    for f in old:
        assert np.array_equal(getattr(sp2.upd, f), old[f])
    assert np.array_equal(h2.i64, h.i64) and np.array_equal(h2.i32, h.i32)
    k = 1 + len(step_plan._PLAN_SCALARS)
    assert step_plan.PLAN_HDR == 32 and step_plan.PLAN_PAYLOAD_IDX == k + 4 and int(hdr[k + 10]) == 2
    # without bias updates: the ten words where they were, the new word 0, the rest of the header 0 and the payload
    # exactly the old sections' bytes
    h, sp = _plan(ProcUpdates(**old))
    hdr0, payload0 = step_plan.pack_plan(h, sp)
    n = 3
    want = h.i64.nbytes + h.i32.nbytes + 4 * n * 3 + 8 * n + 4 * 8 * n + 4 * (1 + 5 + 2 + 2)
    assert payload0.size == want == int(hdr0[step_plan.PLAN_PAYLOAD_IDX]) and not hdr0[k + 10:].any()
    assert hdr0[k:k + 10].tolist() == [h.i64.size, h.i32.size, n, 0, want, n, 1, 5, 2, 1]
    assert payload.size == want + 4 * (2 + 2 * BIAS_ROW_INTS) and np.array_equal(payload[:want], payload0)
    _, sp3 = step_plan.unpack_plan(hdr0, payload0)
    assert sp3.upd.bias_rows.size == 0 and sp3.upd.bias_words.shape == (0, BIAS_ROW_INTS)
    # a step whose only update is a bias row still ships it; one with none ships no update record
    _, sp4 = step_plan.unpack_plan(*step_plan.pack_plan(*_plan(ProcUpdates(bias_rows=np.array([1], np.int32),
                                                                            bias_words=words[:1]))))
    assert sp4.upd is not None and sp4.upd.bias_rows.tolist() == [1]
    assert step_plan.unpack_plan(*step_plan.pack_plan(*_plan(None, proc=False)))[1].upd is None


# ---- reference --------------------------------------------------------------------------------------------------------
def _bias_tab(rows: dict, n_rows=4):
    tab = torch.zeros(n_rows, BIAS_ROW_INTS, dtype=torch.int32)
    for r, pairs in rows.items():
        pairs = sorted(pairs)
        tab[r, :len(pairs)] = torch.tensor([t for t, _ in pairs], dtype=torch.int32)
        tab[r, LOGIT_BIAS_MAX:LOGIT_BIAS_MAX + len(pairs)] = torch.tensor([b for _, b in pairs]).view(torch.int32)
    return tab


def test_reference_formula_elementwise():
    V = 77
    g = torch.Generator().manual_seed(4)
    x = torch.randn(3, V, generator=g) * 3
    counts = torch.zeros(2, 80, dtype=torch.int32)
    counts[1, :V] = torch.randint(0, 3, (V,), generator=g).int()
    keep = torch.rand(V, generator=g) < 0.6
    keep[5], keep[40], keep[33] = False, True, True
    mask_tab = torch.zeros(2, 3, dtype=torch.int32)
    mask_tab[1] = torch.from_numpy(pack_bits(keep.numpy(), 3))
    pairs = [(0, 0.3), (5, 100.0), (40, -7.25), (V - 1, 1e-3), (33, 100.0)]
    tab = _bias_tab({2: pairs})
    pres, freq = 0.7, 0.3
    proc = torch.zeros(3, 8, dtype=torch.int32)
    proc[:, 2] = -1
    proc[0, :3] = torch.tensor([1, 1, 1], dtype=torch.int32)
    proc[0, 3:5] = torch.tensor([pres, freq]).view(torch.int32)
    proc[0, 5:7] = torch.tensor([2, len(pairs)], dtype=torch.int32)
    proc[2, 5:7] = torch.tensor([2, len(pairs)], dtype=torch.int32)  # bias alone; row 1: nothing
    y, forced = ref.process_logits(x, proc, mask_tab, counts, tab)
    b = dict(pairs)
    f32 = np.float32
    for i in range(V):
        c = int(counts[1, i])
        want = (f32(x[0, i]) - (f32(freq) * f32(c) + (f32(pres) if c > 0 else f32(0)))) + f32(b.get(i, 0.0))
        if keep[i]:
            assert f32(y[0, i]) == want, i
        else:
            assert y[0, i] == float("-inf")
        assert f32(y[2, i]) == f32(x[2, i]) + f32(b.get(i, 0.0))
    assert y[0, 5] == float("-inf") and not keep[5]  # +100 on a masked-out token stays -inf
    assert torch.equal(y[1], x[1]) and (forced == -1).all()
    # greedy sampling sees it: the allowed +100 token wins row 0 whatever the logits, a banned one never does
    assert keep[33] and ref.sample(x, None, proc=proc, mask_tab=mask_tab, counts=counts.clone(),
                                   bias_tab=tab).tolist()[0] == 33
    rep = ref.sample_replay(x, torch.full((3,), 0.8), proc=proc, mask_tab=mask_tab, counts=counts.clone(), bias_tab=tab)
    assert rep.tokens[0] == 33 and int(rep.tokens[2]) in (5, 33)
    # a forced row ignores its bias; a count above the bound is clamped like the kernel clamps it
    proc[2, 0], proc[2, 1] = 2, 11
    assert ref.sample(x, None, proc=proc, mask_tab=mask_tab, counts=counts.clone(), bias_tab=tab).tolist()[2] == 11
    with pytest.raises(ValueError):
        ref.process_logits(x, proc, mask_tab, counts, None)


# ---- CPU engine -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    return LLMEngine(EngineConfig(model="tiny-llama", device="cpu", num_kv_blocks=64, max_model_len=2048)).model


def _engine(model, **kw):
    return LLMEngine(EngineConfig(model="tiny-llama", device="cpu", num_kv_blocks=512, max_model_len=2048, **kw),
                     model=model)


@pytest.mark.parametrize("async_on", [False, True])
def test_engine_forces_and_bans(model, async_on):
    g = torch.Generator().manual_seed(11)
    prompts = [torch.randint(0, 5000, (n,), generator=g).tolist() for n in (9, 21, 14, 14)]
    kw = dict(max_tokens=5, ignore_eos=True)
    free = LLMEngine.generate(_engine(model), [prompts[2]], SamplingParams(temperature=0.0, **kw))[0]
    t, gtok = 4242, free[0]
    eng = _engine(model, async_scheduling=async_on)
    outs = eng.generate(prompts, [SamplingParams(temperature=0.0, logit_bias={t: 100}, **kw),
                                  SamplingParams(temperature=1.0, seed=3, logit_bias={t: 100.0, 17: -100.0}, **kw),
                                  SamplingParams(temperature=0.0, logit_bias={gtok: -100}, **kw),
                                  SamplingParams(temperature=0.0, **kw)])
    assert outs[0] == [t] * 5 and outs[1] == [t] * 5
    assert outs[2][0] != gtok and gtok not in outs[2]
    assert outs[3] == LLMEngine.generate(_engine(model), [prompts[3]], SamplingParams(temperature=0.0, **kw))[0]
    st = eng.runner.lp.stats
    assert st["bias_uploads"] == 3 and st["bias_rows_used"] >= 15  # three objects, a row index from then on


def test_engine_logprobs_stay_raw(model):
    g = torch.Generator().manual_seed(12)
    prompt = torch.randint(0, 5000, (12,), generator=g).tolist()
    t = 4242
    eng = _engine(model)
    seq = eng.add_request("r", prompt, SamplingParams(temperature=0.0, max_tokens=3, ignore_eos=True, logprobs=True,
                                                      top_logprobs=2, logit_bias={t: 100}))
    recs = []
    while eng.has_unfinished():
        for o in eng.step():
            recs += o.logprobs or []
    assert seq.output_ids == [t] * 3 and [r[0] for r in recs] == [t] * 3
    # the forced token's RAW logprob (a random-init model: about -log V), not the ~0 of the biased distribution, and
    # the alternatives are the raw top tokens, not the biased one
    assert all(r[1] < -5.0 for r in recs) and all(t not in r[2] and r[3][0] > r[1] for r in recs)


# ---- API --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def api():
    st = ServerState(ServerConfig(backend="engine", model="tiny-llama", sandbox="none", max_model_len=8192,
                                  default_max_tokens=12, prompt_sections=["intro"], warm_prefix=False,
                                  engine_kwargs={"device": "cpu", "num_kv_blocks": 1024}), db=MemoryDBClient())
    with TestClient(create_app(state=st)) as c:
        yield c, st


BODY = {"model": "tiny-llama", "messages": [{"role": "user", "content": "Tell me about MI355X."}], "temperature": 0,
        "max_tokens": 6, "seed": 7, "tool_choice": "none"}


def test_api_string_keys_force_ban_and_raw_logprobs(api):
    c, st = api
    tok = st.llm.tok
    t = tok.encode(" hello")[-1]
    piece = tok.decode([t], False)
    for temp in (0, 1):
        r = c.post("/v1/chat/completions", json=dict(BODY, temperature=temp, logit_bias={str(t): 100},
                                                     logprobs=True, top_logprobs=1))
        assert r.status_code == 200, r.text
        ch = r.json()["choices"][0]
        assert ch["message"]["content"] == piece * 6
        entries = ch["logprobs"]["content"]
        assert [e["token"] for e in entries] == [piece] * 6
        assert all(e["logprob"] < -5.0 and e["top_logprobs"][0]["logprob"] > e["logprob"] for e in entries)
    base = c.post("/v1/chat/completions", json=dict(BODY, logprobs=True)).json()["choices"][0]
    first = base["logprobs"]["content"][0]
    g = tok.encode(first["token"])
    assert len(g) == 1 and tok.decode(g, False) == first["token"]
    banned = c.post("/v1/chat/completions", json=dict(BODY, logprobs=True, logit_bias={str(g[0]): -100}))
    assert banned.status_code == 200
    assert banned.json()["choices"][0]["logprobs"]["content"][0]["token"] != first["token"]
    # the thread route takes the field too, and a stream carries the forced text
    raw = c.post("/v1/chat/completions", json=dict(BODY, stream=True, logit_bias={str(t): 100})).text
    text = "".join(json.loads(b[6:])["choices"][0]["delta"].get("content") or ""
                   for b in raw.split("\n\n") if b.startswith("data: {") and '"choices"' in b)
    assert text == piece * 6
    # an empty / all-zero object is "no bias": the reply of a request without the field
    for none in ({}, {str(t): 0}):
        same = c.post("/v1/chat/completions", json=dict(BODY, logit_bias=none)).json()["choices"][0]["message"]
        assert same["content"] == base["message"]["content"]


def test_api_out_of_vocabulary_id_is_400(api):
    c, st = api
    V = st.engine_client.model_cfg.vocab_size
    before = st.engine_client.health()["replica0"]
    r = c.post("/v1/chat/completions", json=dict(BODY, logit_bias={"5": 1, str(V): 1}))
    assert r.status_code == 400 and str(V) in r.json()["detail"] and "vocabulary" in r.json()["detail"]
    assert st.engine_client.health()["replica0"] == before  # nothing was submitted
    assert c.post("/v1/chat/completions", json=dict(BODY, logit_bias={str(V - 1): 1})).status_code == 200
    tid = c.post("/v1/threads", json={}).json()["thread_id"]
    r = c.post(f"/v1/threads/{tid}/chat/completions", json=dict(BODY, logit_bias={str(V + 7): -1}))
    assert r.status_code == 400 and str(V + 7) in r.json()["detail"]


def test_remote_provider_forwards_the_field():
    from kafka_llm_service_amd.llm.remote import RemoteOpenAIProvider

    p = RemoteOpenAIProvider.__new__(RemoteOpenAIProvider)
    p.model, p.default_max_tokens = "m", 16
    body = p._body([], None, None, None, None, {"logit_bias": {12: 5.0, 7: -100.0}, "seed": 3})
    assert body["logit_bias"] == {"12": 5.0, "7": -100.0} and body["seed"] == 3
    assert "logit_bias" not in p._body([], None, None, None, None, {"seed": 3})
