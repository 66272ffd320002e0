"""``repetition_penalty`` without a GPU: the request schema and ``SamplingParams``, the host tables (prompt flags in the
count table, the slot's ``(r, 1 / r)`` row of ``rep_tab``), the wire format, ``ref.process_logits`` against the
definition written out in numpy, rollback, the CPU engine against a hand loop over the dense oracle, and the replay's
distribution.

The definition: for a row with penalty r != 1 let S be the distinct ids of the sequence's prompt plus every generated
token that still counts. The fp32 logit x_i becomes x_i if i is not in S, x_i * inv_r if x_i > 0 and x_i * r otherwise,
with r = float32(r) and inv_r = float32(1) / float32(r) — one fp32 multiply, within one fp32 ulp of x_i / r — and the
existing processing (presence / frequency on the generated count, bias, mask) then runs on the result."""
import pickle

import numpy as np
import pytest
import torch
from fastapi.testclient import TestClient
from pydantic import ValidationError

from kafka_llm_service_amd.db.local import MemoryDBClient
from kafka_llm_service_amd.engine import step_plan
from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
from kafka_llm_service_amd.engine.logits_proc import LogitsProcessor, pack_bits, rep_factors
from kafka_llm_service_amd.engine.sequence import SamplingParams, Sequence
from kafka_llm_service_amd.engine.step_plan import COUNT_SEEN_PROMPT, HostStep, ProcUpdates, SampleParams
from kafka_llm_service_amd.kafka.types import ChatCompletionRequest
from kafka_llm_service_amd.llm.stub import ScriptedProvider
from kafka_llm_service_amd.models.oracle import dense_logits
from kafka_llm_service_amd.ops import reference as ref
from kafka_llm_service_amd.server.app import _sampling_kwargs, create_app
from kafka_llm_service_amd.server.state import ServerConfig, ServerState

MSG = [{"role": "user", "content": "hi"}]
FLAG = 1 << 30
f32 = np.float32


def penalise(x: np.ndarray, seen: np.ndarray, r: float) -> np.ndarray:
    """The definition on fp32 logits ``x`` ([..., V]) with the bool set ``seen``."""
    x = np.asarray(x, dtype=np.float32)
    r32 = f32(r)
    inv = f32(1) / r32
    with np.errstate(all="ignore"):
        return np.where(seen, np.where(x > 0, x * inv, x * r32), x).astype(np.float32)


def _seq(i, prompt=(1,), **kw):
    return Sequence(f"r{i}", list(prompt), SamplingParams(**kw))


def _apply(lp, upd):
    lp.apply(upd, lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(lp.device))


def test_constants_agree():
    import re
    from pathlib import Path

    import kafka_llm_service_amd.ops as ops_pkg

    hdr = (Path(ops_pkg.__file__).parent / "csrc" / "kafka_abi.h").read_text()
    assert re.search(r"constexpr int COUNT_SEEN_PROMPT = 1 << 30;", hdr)
    assert FLAG == COUNT_SEEN_PROMPT == ref.COUNT_SEEN_PROMPT


# ---- 1. schema and SamplingParams -------------------------------------------------------------------------------------
def test_schema_bounds_are_422():
    for bad in (0.09, 10.01, -1, 0, float("nan"), float("inf"), True, False, "2", "x"):
        with pytest.raises(ValidationError):
            ChatCompletionRequest(model="m", messages=MSG, repetition_penalty=bad)
    for ok in (0.1, 1, 1.3, 10):
        assert ChatCompletionRequest(model="m", messages=MSG, repetition_penalty=ok).repetition_penalty == ok
    assert _sampling_kwargs(ChatCompletionRequest(model="m", messages=MSG, repetition_penalty=1.3)) \
        == {"repetition_penalty": 1.3}
    for off in ({}, dict(repetition_penalty=1), dict(repetition_penalty=1.0), dict(repetition_penalty=None)):
        assert "repetition_penalty" not in _sampling_kwargs(ChatCompletionRequest(model="m", messages=MSG, **off))
    st = ServerState(ServerConfig(backend="stub", sandbox="none"), llm_provider=ScriptedProvider([{"text": "hi"}] * 2),
                     db=MemoryDBClient())
    with TestClient(create_app(state=st)) as c:
        body = {"model": "kafka", "messages": MSG}
        for bad in (0.05, 10.5, "x", "2", True):
            assert c.post("/v1/chat/completions", json=dict(body, repetition_penalty=bad)).status_code == 422
        assert c.post("/v1/chat/completions", json=dict(body, repetition_penalty=2)).status_code == 200


def test_sampling_params_validation():
    assert SamplingParams().repetition_penalty == 1.0 and SamplingParams(repetition_penalty=2).repetition_penalty == 2.0
    p = SamplingParams(repetition_penalty=1.3, presence_penalty=0.5)
    q = pickle.loads(pickle.dumps(p))  # (the DP / TP pipes)
    assert q.repetition_penalty == 1.3 and q == p
    assert SamplingParams(**{k: v for k, v in p.__dict__.items() if k != "allowed_tokens_fn"}) == p  # the workers' dict
    for bad in (0.0999, 10.0001, 0, -2, float("nan"), float("inf"), "2", None, True):
        with pytest.raises(ValueError):
            SamplingParams(repetition_penalty=bad)
    for bad in (0.05, 11, float("nan"), True):
        with pytest.raises(ValueError):
            rep_factors(bad)


def test_penalty_one_is_a_request_without_the_field():
    V = 100
    kws = [dict(presence_penalty=0.5), dict(logit_bias={7: 2.5}), dict(temperature=0.8, min_p=0.1), {}]
    out = []
    for extra in ({}, dict(repetition_penalty=1), dict(repetition_penalty=1.0)):
        lp = LogitsProcessor("cpu", V, max_slots=4)
        proc, upd = lp.build([(i, _seq(i, (3, 4, 5), **kw, **extra), None) for i, kw in enumerate(kws)], 4)
        out.append((proc, upd, lp.stats["rep_rows"], lp.stats["seen_uploads"]))
    for proc, upd, rows, ups in out:
        assert np.array_equal(proc, out[0][0]) and rows == 0 and ups == 0
        assert upd.seen_slots.size == 0 and upd.seen_ids.size == 0 and upd.rep_vals.shape == (0, 2)
        assert upd.seen_off.tolist() == [0] and np.array_equal(upd.zero_slots, out[0][1].zero_slots)


class _Recording(ScriptedProvider):
    def __init__(self, script):
        super().__init__(script)
        self.kwargs = []

    async def stream_completion(self, messages, **kwargs):
        self.kwargs.append(dict(kwargs))
        async for ch in super().stream_completion(messages, **kwargs):
            yield ch


def test_chat_route_hands_the_field_to_the_provider():
    prov = _Recording([{"text": "hi"}] * 4)
    st = ServerState(ServerConfig(backend="stub", sandbox="none"), llm_provider=prov, db=MemoryDBClient())
    with TestClient(create_app(state=st)) as c:
        body = {"model": "kafka", "messages": MSG}
        assert c.post("/v1/chat/completions", json=dict(body, repetition_penalty=1.3)).status_code == 200
        assert prov.kwargs[-1]["repetition_penalty"] == 1.3
        assert c.post("/v1/chat/completions", json=dict(body, repetition_penalty=0.5, stream=True)).status_code == 200
        assert prov.kwargs[-1]["repetition_penalty"] == 0.5
        tid = c.post("/v1/threads", json={}).json()["thread_id"]
        assert c.post(f"/v1/threads/{tid}/chat/completions", json=dict(body, repetition_penalty=2)).status_code == 200
        assert prov.kwargs[-1]["repetition_penalty"] == 2.0
        for off in ({}, dict(repetition_penalty=1)):
            assert c.post("/v1/chat/completions", json=dict(body, **off)).status_code == 200
            assert "repetition_penalty" not in prov.kwargs[-1]


def test_chat_route_reaches_the_engines_sampling_params():
    st = ServerState(ServerConfig(backend="engine", model="tiny-llama", sandbox="none", max_model_len=8192,
                                  default_max_tokens=12, prompt_sections=["intro"], warm_prefix=False,
                                  engine_kwargs={"device": "cpu", "num_kv_blocks": 1024}), db=MemoryDBClient())
    body = {"model": "tiny-llama", "messages": [{"role": "user", "content": "Tell me about MI355X."}],
            "temperature": 0, "max_tokens": 4, "seed": 7, "tool_choice": "none"}
    with TestClient(create_app(state=st)) as c:
        client, got = st.llm.client, []
        orig = client.generate

        def spy(request_id, prompt_ids, params, routing_key=None):
            got.append(params)
            return orig(request_id, prompt_ids, params, routing_key)

        client.generate = spy
        try:
            plain = c.post("/v1/chat/completions", json=body)
            pen = c.post("/v1/chat/completions", json=dict(body, repetition_penalty=2.0))
        finally:
            client.generate = orig
        assert plain.status_code == 200 and pen.status_code == 200, pen.text
        assert [p.repetition_penalty for p in got] == [1.0, 2.0]
        lp = client.async_engine.engine.runner.lp
        assert 1 <= lp.stats["rep_rows"] <= 4 and lp.stats["seen_uploads"] == 1


def test_remote_provider_forwards_only_when_set():
    from kafka_llm_service_amd.llm.remote import RemoteOpenAIProvider

    p = RemoteOpenAIProvider.__new__(RemoteOpenAIProvider)
    p.model, p.default_max_tokens = "m", 16
    assert p._body([], None, None, None, None, {"repetition_penalty": 1.3})["repetition_penalty"] == 1.3
    for kw in ({}, {"repetition_penalty": None}, {"repetition_penalty": 1}, {"repetition_penalty": 1.0}):
        assert "repetition_penalty" not in p._body([], None, None, None, None, dict(kw))


# ---- 2. LogitsProcessor.build / apply ---------------------------------------------------------------------------------
def test_build_seeds_the_prompt_and_apply_writes_the_tables():
    V = 45  # (cnt_ld 48)
    lp = LogitsProcessor("cpu", V, max_slots=4)
    mask_tab, counts = lp.tables()
    assert lp.rep_table().shape == (4, 2) and lp.rep_table().dtype == torch.float32 and bool((lp.rep_table() == 1).all())
    a = _seq(0, (7, 3, 7, 44, 0, 3, 45, 99), repetition_penalty=1.3)  # 45 and 99 lie outside the vocabulary
    b = _seq(1, (5, 6), presence_penalty=0.5)
    c = _seq(2, (9, 9, 9), repetition_penalty=0.5, frequency_penalty=0.25)
    d = _seq(3, (2,), temperature=0.7)
    proc, upd = lp.build([(0, a, None), (1, b, None), (2, c, None)], 4)
    assert proc.shape == (4, 8) and proc.dtype == np.int32
    assert lp.live_rep_table() is None  # no slot holds a factor yet: the sampler runs without the table
    sa, sb, sc = (int(proc[i, 2]) for i in range(3))
    assert len({sa, sb, sc}) == 3 and proc[3, 2] == -1 and sorted(upd.zero_slots.tolist()) == sorted([sa, sb, sc])
    assert upd.seen_slots.tolist() == [sa, sc] and upd.seen_off.tolist() == [0, 4, 5]
    assert upd.seen_ids.tolist() == [0, 3, 7, 44, 9] and upd.seen_ids.dtype == np.int32
    assert upd.rep_vals.dtype == np.float32
    assert np.array_equal(upd.rep_vals, np.array([[f32(1.3), f32(1) / f32(1.3)], [f32(0.5), f32(2)]], np.float32))
    assert proc[0, 3:5].tolist() == [0, 0] and proc[2, 3:5].view(np.float32).tolist() == [0.0, 0.25]
    assert lp.stats["rep_rows"] == 2 and lp.stats["seen_uploads"] == 2 and lp.stats["penalty_rows"] == 2
    counts[sa].fill_(5)  # stale words of an earlier owner
    lp.rep_table()[sb] = torch.tensor([3.0, 1 / 3])
    _apply(lp, upd)
    want = torch.zeros_like(counts)
    want[sa, [0, 3, 7, 44]] = FLAG
    want[sc, 9] = FLAG
    assert torch.equal(counts, want)  # exactly the distinct prompt ids, nothing in the presence-only slot
    assert bool((counts[sb] == 0).all())
    rt = lp.rep_table()
    assert rt[sa].tolist() == [float(f32(1.3)), float(f32(1) / f32(1.3))] and rt[sc].tolist() == [0.5, 2.0]
    assert rt[sb].tolist() == [1.0, 1.0]  # a slot given to a sequence without the penalty is reset
    assert lp.live_rep_table() is rt
    # the next step of the same sequences: no slot is new, nothing is seeded again (as after a preemption)
    proc2, upd2 = lp.build([(0, a, None), (1, b, None), (2, c, None), (3, d, None)], 4)
    assert upd2.empty and np.array_equal(proc2[:3], proc[:3]) and lp.stats["seen_uploads"] == 2
    # a recycled slot: its flags go and its factor is (1, 1) again
    for s in (a, b, c):
        s.status = type(s.status).FINISHED
    lp2_seqs = [_seq(10 + i, (20 + i,), presence_penalty=1.0) for i in range(4)]
    proc3, upd3 = lp.build([(i, s, None) for i, s in enumerate(lp2_seqs)], 4)
    assert sorted(upd3.zero_slots.tolist()) == [0, 1, 2, 3] and upd3.seen_slots.size == 0
    _apply(lp, upd3)
    assert bool((counts == 0).all()) and bool((lp.rep_table() == 1).all()) and lp.live_rep_table() is None


def test_table_is_live_only_while_a_penalised_request_is():
    """A finished request's slot is cleared with the next step's updates (not only when it is needed again), and the
    sampler then gets no table; a second LogitsProcessor fed the same updates (a TP follower) agrees at every step."""
    V = 45
    lead, follow = LogitsProcessor("cpu", V, max_slots=8), LogitsProcessor("cpu", V, max_slots=8)
    a = _seq(0, (7, 3), repetition_penalty=1.3)
    b = _seq(1, (5, 6), presence_penalty=0.5)

    def step(rows):
        proc, upd = lead.build(rows, len(rows))
        for lp in (lead, follow):
            _apply(lp, upd)
        assert (lead.live_rep_table() is None) == (follow.live_rep_table() is None)
        return proc, upd

    step([(0, b, None)])
    assert lead.live_rep_table() is None
    proc, _ = step([(0, a, None), (1, b, None)])
    assert lead.live_rep_table() is not None and torch.equal(lead.rep_table(), follow.rep_table())
    a.status = type(a.status).FINISHED
    _, upd = step([(0, b, None)])
    assert upd.zero_slots.tolist() == [int(proc[0, 2])] and lead.live_rep_table() is None
    assert bool((lead.tables()[1] == 0).all()) and torch.equal(lead.tables()[1], follow.tables()[1])
    c = _seq(2, (9,), repetition_penalty=2.0)
    _, upd = step([(0, b, None), (1, c, None)])
    assert lead.live_rep_table() is not None and upd.zero_slots.tolist() == upd.seen_slots.tolist()


def test_apply_validates_bounds():
    lp = LogitsProcessor("cpu", 45, max_slots=4)
    ok = dict(seen_slots=np.array([1], np.int32), seen_off=np.array([0, 2], np.int32),
              seen_ids=np.array([3, 44], np.int32), rep_vals=np.array([[2, 0.5]], np.float32))
    _apply(lp, ProcUpdates(**ok))
    assert lp.tables()[1][1, [3, 44]].tolist() == [FLAG, FLAG] and lp.rep_table()[1].tolist() == [2.0, 0.5]
    for bad in (dict(seen_slots=np.array([4], np.int32)), dict(seen_slots=np.array([-1], np.int32)),
                dict(seen_ids=np.array([3, 45], np.int32)), dict(seen_ids=np.array([-1, 4], np.int32)),
                dict(seen_off=np.array([0, 1], np.int32)), dict(seen_off=np.array([0, 2, 2], np.int32)),
                dict(rep_vals=np.array([[2, 0.5], [1, 1]], np.float32)),
                dict(rep_vals=np.array([[np.nan, 0.5]], np.float32)), dict(rep_vals=np.array([[0, 0.5]], np.float32))):
        with pytest.raises(ValueError):
            _apply(lp, ProcUpdates(**dict(ok, **bad)))


# ---- 3. wire format ---------------------------------------------------------------------------------------------------
def _plan(upd, n=3):
    h = HostStep(B=n, T=n, n_rows=n)
    h.i64 = np.arange(3 * n + n, dtype=np.int64)
    h.i32 = np.arange(1 + n, dtype=np.int32)
    p = np.zeros((n, 8), np.int32)
    p[:, 2] = [1, -1, 5]
    return h, SampleParams(np.full(n, 0.7, np.float32), np.ones(n, np.float32), np.zeros(n, np.int32),
                           np.arange(n, dtype=np.int64), p, False, upd)


def test_wire_round_trip_and_unchanged_without_seeding():
    old = dict(mask_rows=np.array([3], np.int32), mask_words=np.arange(5, dtype=np.int32).reshape(1, 5),
               zero_slots=np.array([1, 5], np.int32), dec=np.array([[1, 40]], np.int32))
    new = dict(seen_slots=np.array([1, 5], np.int32), seen_off=np.array([0, 3, 3], np.int32),
               seen_ids=np.array([2, 9, 31], np.int32), rep_vals=np.stack([rep_factors(1.3), rep_factors(0.5)]))
    hdr, payload = step_plan.pack_plan(*_plan(ProcUpdates(**old, **new)))
    h2, sp2 = step_plan.unpack_plan(hdr, payload)
    for f, v in {**old, **new}.items():
        got = getattr(sp2.upd, f)
        assert np.array_equal(got, v) and got.dtype == v.dtype, f
    k = 1 + len(step_plan._PLAN_SCALARS)
    assert step_plan.PLAN_HDR == 32 and int(hdr[k + 11]) == 2 and int(hdr[k + 10]) == 0
    # without seeding updates: byte-equal to the plan whose new fields are left at their defaults, header count 0
    hdr0, payload0 = step_plan.pack_plan(*_plan(ProcUpdates(**old)))
    none = dict(seen_slots=np.zeros(0, np.int32), seen_off=np.zeros(1, np.int32), seen_ids=np.zeros(0, np.int32),
                rep_vals=np.zeros((0, 2), np.float32))
    hdr1, payload1 = step_plan.pack_plan(*_plan(ProcUpdates(**old, **none)))
    assert np.array_equal(hdr0, hdr1) and np.array_equal(payload0, payload1) and not hdr0[k + 10:].any()
    h, _ = _plan(None)
    n = 3
    want = h.i64.nbytes + h.i32.nbytes + 4 * n * 3 + 8 * n + 4 * 8 * n + 4 * (1 + 5 + 2 + 2)  # the sections before
    assert payload0.size == want == int(hdr0[step_plan.PLAN_PAYLOAD_IDX])
    assert payload.size == want + 4 * (2 + 3 + 4 + 3) and np.array_equal(payload[:want], payload0)
    sp3 = step_plan.unpack_plan(hdr0, payload0)[1]
    assert sp3.upd.seen_slots.size == 0 and sp3.upd.seen_off.tolist() == [0] and sp3.upd.rep_vals.shape == (0, 2)
    # a step whose only update is a seeding still ships it; ``empty`` accounts for the new sections
    assert ProcUpdates().empty and not ProcUpdates(**new).empty
    sp4 = step_plan.unpack_plan(*step_plan.pack_plan(*_plan(ProcUpdates(**new))))[1]
    assert sp4.upd is not None and sp4.upd.seen_ids.tolist() == [2, 9, 31]
    with pytest.raises(ValueError):
        step_plan.pack_plan(*_plan(ProcUpdates(**dict(new, seen_off=np.array([0, 3, 4], np.int32)))))


# ---- 4. process_logits against the definition -------------------------------------------------------------------------
def test_process_logits_against_the_definition():
    V = 45
    g = torch.Generator().manual_seed(4)
    x = torch.randn(5, V, generator=g) * 3
    x[:, 1], x[:, 2], x[:, 3], x[:, 4] = 0.0, -0.0, float("-inf"), -2.5
    x[:, 5], x[:, 6], x[:, 7] = 3.25, 1e-3, 7.0
    counts = torch.zeros(3, 48, dtype=torch.int32)
    prompt_only, gen_only, both = [1, 3, 5, 20, 44], [2, 4, 6, 21], [0, 7, 22]
    counts[1, prompt_only] = FLAG
    counts[1, gen_only] = torch.tensor([1, 2, 3, 1], dtype=torch.int32)
    counts[1, both] = FLAG + torch.tensor([1, 4, 2], dtype=torch.int32)
    counts[2] = counts[1]
    rep_tab = torch.ones(3, 2)
    rep_tab[1] = torch.from_numpy(rep_factors(1.3))
    rep_tab[2] = torch.from_numpy(rep_factors(0.5))
    keep = torch.rand(V, generator=g) < 0.6
    keep[5], keep[7], keep[4] = False, True, True
    mask_tab = torch.zeros(2, 2, dtype=torch.int32)
    mask_tab[1] = torch.from_numpy(pack_bits(keep.numpy(), 2))
    from test_logit_bias import _bias_tab

    pairs = [(0, 0.3), (5, 100.0), (4, -7.25), (V - 1, 1e-3), (30, 2.0)]
    tab = _bias_tab({2: pairs})
    pres, freq = 0.7, 0.3
    proc = torch.zeros(5, 8, dtype=torch.int32)
    proc[:, 2] = torch.tensor([1, 1, 2, 1, -1], dtype=torch.int32)
    proc[1, 3:5] = torch.tensor([pres, freq]).view(torch.int32)          # row 1: + presence / frequency
    proc[2, 3:5] = torch.tensor([pres, freq]).view(torch.int32)          # row 2: r = 0.5, + bias + mask
    proc[2, 5:7] = torch.tensor([2, len(pairs)], dtype=torch.int32)
    proc[2, 0], proc[2, 1] = 1, 1
    proc[3, 0], proc[3, 1] = 2, 11                                       # row 3: forced; row 4: no slot
    y, forced = ref.process_logits(x, proc, mask_tab, counts, tab, rep_tab)
    word = counts[1, :V].numpy()
    seen, c = word != 0, (word & (FLAG - 1)).astype(np.float32)
    assert seen.sum() == 12 and not seen[[8, 9, 10]].any()
    pen = (f32(freq) * c + np.where(c > 0, f32(pres), f32(0))).astype(np.float32)  # the count excludes the flag
    assert c[prompt_only].tolist() == [0] * 5 and c[both].tolist() == [1, 4, 2]
    y0 = penalise(x[0].numpy(), seen, 1.3)
    assert np.array_equal(y[0].numpy(), y0)
    assert y0[1] == 0 and y0[2] == 0 and np.signbit(y0[2]) and y0[3] == -np.inf            # zero, -0.0, -inf
    assert y0[4] == f32(-2.5) * f32(1.3) and y0[5] == f32(3.25) * (f32(1) / f32(1.3))      # negative, positive
    assert abs(float(y0[7]) - 7.0 / float(f32(1.3))) <= float(np.spacing(y0[7]))            # one ulp of x / r
    assert np.array_equal(y0[[8, 9, 10]], x[0, [8, 9, 10]].numpy())                         # unseen: untouched
    with np.errstate(invalid="ignore"):
        assert np.array_equal(y[1].numpy(), (penalise(x[1].numpy(), seen, 1.3) - pen).astype(np.float32))
        b = np.zeros(V, np.float32)
        for t, v in pairs:
            b[t] = v
        want2 = ((penalise(x[2].numpy(), seen, 0.5) - pen).astype(np.float32) + b).astype(np.float32)
    want2[~keep.numpy()] = -np.inf
    assert np.array_equal(y[2].numpy(), want2) and y[2, 5] == float("-inf")
    assert penalise(x[2].numpy(), seen, 0.5)[7] == 14.0  # r < 1 rewards: a seen positive logit doubles
    assert torch.equal(y[3], x[3]) and forced.tolist() == [-1, -1, -1, 11, -1] and torch.equal(y[4], x[4])
    # off: no table, or a (1, 1) row — bit for bit the processing without the feature, flags or not
    y_off, _ = ref.process_logits(x, proc, mask_tab, counts, tab)
    y_one, _ = ref.process_logits(x, proc, mask_tab, counts, tab, torch.ones(3, 2))
    plain = counts & (FLAG - 1)
    y_old, _ = ref.process_logits(x, proc, mask_tab, plain, tab)
    assert torch.equal(y_off, y_one) and torch.equal(y_off, y_old)
    # the samplers see it: greedy takes the best penalised logit, forced rows their token
    tok = ref.sample(x, None, proc=proc, mask_tab=mask_tab, counts=counts.clone(), bias_tab=tab, rep_tab=rep_tab)
    rep = ref.sample_replay(x, None, proc=proc, mask_tab=mask_tab, counts=counts.clone(), bias_tab=tab, rep_tab=rep_tab)
    assert tok.tolist() == rep.tokens.tolist() == [int(np.argmax(y0)), int(y[1].argmax()), int(y[2].argmax()), 11,
                                                   int(x[4].argmax())]


# ---- 5. rollback ------------------------------------------------------------------------------------------------------
def test_rolled_back_token_is_unseen_unless_the_prompt_holds_it():
    V = 45
    lp = LogitsProcessor("cpu", V, max_slots=2)
    s = _seq(0, (3, 7), repetition_penalty=2.0)
    proc, upd = lp.build([(0, s, None)], 1)
    _apply(lp, upd)
    mask_tab, counts = lp.tables()
    slot = int(proc[0, 2])
    pt = torch.from_numpy(proc)
    x = torch.full((1, V), -1.0)

    def draw(tok):  # greedy: the only positive logit wins, and the sampler counts it
        xx = x.clone()
        xx[0, tok] = 9.0
        got = ref.sample(xx, None, proc=pt, mask_tab=mask_tab, counts=counts, rep_tab=lp.rep_table())
        assert got.tolist() == [tok]

    def seen_now():
        y, _ = ref.process_logits(torch.ones(1, V), pt, mask_tab, counts, None, lp.rep_table())
        return set(torch.nonzero(y[0] != 1).flatten().tolist())

    assert seen_now() == {3, 7}
    draw(20)  # a token the prompt does not hold
    assert seen_now() == {3, 7, 20} and int(counts[slot, 20]) == 1
    lp.uncount(s, 20)
    _apply(lp, lp.build([(0, s, None)], 1)[1])
    assert seen_now() == {3, 7} and int(counts[slot, 20]) == 0
    draw(7)  # a prompt token
    assert int(counts[slot, 7]) == FLAG + 1
    lp.uncount(s, 7)
    _apply(lp, lp.build([(0, s, None)], 1)[1])
    assert seen_now() == {3, 7} and int(counts[slot, 7]) == FLAG  # still seen, its generated count back at zero
    draw(20)
    draw(20)  # drawn before: one rollback leaves it seen
    lp.uncount(s, 20)
    _apply(lp, lp.build([(0, s, None)], 1)[1])
    assert seen_now() == {3, 7, 20} and int(counts[slot, 20]) == 1


# ---- 6. CPU engine ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    return LLMEngine(EngineConfig(model="tiny-llama", device="cpu", num_kv_blocks=64, max_model_len=2048)).model


def _engine(model, **kw):
    return LLMEngine(EngineConfig(model="tiny-llama", device="cpu", num_kv_blocks=512, max_model_len=2048, **kw),
                     model=model)


def hand_loop(model, prompt, n, r, fp32=False):
    """Greedy tokens of the dense oracle under the definition over prompt + output so far, and per step (top-1 / top-2
    margin of the penalised row, the raw row's standard deviation, the penalised runner-up)."""
    out, margins = [], []
    for _ in range(n):
        row = dense_logits(model, prompt + out, fp32=fp32)[-1].float().cpu().numpy()
        seen = np.zeros(row.size, dtype=bool)
        seen[[t for t in prompt + out if t < row.size]] = True
        y = penalise(row, seen, r) if r != 1 else row
        top = np.sort(y)[-2:]
        margins.append((float(top[1] - top[0]), float(row.std()), float(top[0])))
        out.append(int(np.argmax(y)))
    return out, margins


# The paged CPU engine and the dense oracle sum in different orders: tests/test_engine_cpu.py allows a greedy token
# 0.05 below the oracle's maximum. With r = 2 a positive logit is multiplied by 1 or 1 / 2, so a penalised row whose two
# best logits are positive carries at most that difference, and is decided when they lie more than 0.05 apart.
ENGINE_MARGIN = 0.05


def penalised_prompt(model, n):
    """The first prompt of a fixed list whose penalised hand loop is decided at every step and differs from its
    unpenalised one (both read off the oracle alone)."""
    for pseed in range(21, 41):
        g = torch.Generator().manual_seed(pseed)
        prompt = torch.randint(0, 5000, (17,), generator=g).tolist()
        pen, m = hand_loop(model, prompt, n, 2.0)
        if min(d for d, _, _ in m) > ENGINE_MARGIN and min(second for _, _, second in m) > 0 \
                and pen != hand_loop(model, prompt, n, 1.0)[0]:
            return prompt, pen
    pytest.fail("no prompt of the list has a decided penalised run that differs from the plain one")


@pytest.mark.parametrize("async_on", [False, True])
def test_engine_matches_the_hand_loop(model, async_on):
    n = 6
    prompt, pen = penalised_prompt(model, n)
    kw = dict(temperature=0.0, max_tokens=n, ignore_eos=True)
    eng = _engine(model, async_scheduling=async_on)
    outs = eng.generate([prompt, prompt], [SamplingParams(repetition_penalty=2.0, **kw), SamplingParams(**kw)])
    assert outs[0] == pen
    assert outs[1] != outs[0]  # (the penalty changes this run: the comparison above is not vacuous)
    st = eng.runner.lp.stats
    assert st["rep_rows"] == n and st["seen_uploads"] == 1
    slot = eng.runner.lp._slots and next(iter(eng.runner.lp._slots.values()))[0]
    word = eng.runner.lp.tables()[1][slot]
    assert set(torch.nonzero(word & FLAG).flatten().tolist()) == set(prompt)
    assert int((word & (FLAG - 1)).sum()) == n


# ---- 7. sample_replay -------------------------------------------------------------------------------------------------
def _chi2_sf(chi2: float, df: int) -> float:
    return float(torch.special.gammaincc(torch.tensor(df / 2.0, dtype=torch.float64),
                                         torch.tensor(chi2 / 2.0, dtype=torch.float64)))


def _fits(tokens: np.ndarray, q: np.ndarray, n: int, what: str):
    """Pearson chi-square of the draws against q (bins with expected count below 5 merged, p > 1e-4)."""
    obs = np.bincount(tokens, minlength=q.size).astype(np.float64)
    order = np.argsort(q)
    e, o = (q * n)[order], obs[order]
    small = int((e < 5).sum())
    if small:
        while small < e.size and e[:small].sum() < 5:
            small += 1
        e = np.concatenate([[e[:small].sum()], e[small:]])
        o = np.concatenate([[o[:small].sum()], o[small:]])
    chi2 = float(((o - e) ** 2 / e).sum())
    pv = _chi2_sf(chi2, e.size - 1)
    assert pv > 1e-4, f"{what}: chi2 {chi2:.1f} over {e.size} bins, p = {pv:.3g}"


def test_replay_and_reference_draw_from_the_penalised_distribution():
    """One row of 64 logits, 4096 draws with distinct seeds through one seeded slot: the replay (the kernel's stream)
    and ``ref.sample`` both fit softmax(y / T) of the penalised row, and not that of the raw row."""
    V, N, T, r = 64, 4096, 0.8, 2.0
    x = torch.randn(1, V, generator=torch.Generator().manual_seed(1234)) * 2
    counts = torch.zeros(1, V, dtype=torch.int32)
    order = torch.argsort(x[0], descending=True)
    counts[0, order[0:8:2]] = FLAG  # four of the eight likeliest tokens: prompt, generated, both
    counts[0, order[1]] = 2
    counts[0, order[3]] = FLAG + 1
    counts[0, order[40:44]] = 1
    rep_tab = torch.from_numpy(rep_factors(r))[None]
    proc = torch.zeros(N, 8, dtype=torch.int32)
    i = torch.arange(N, dtype=torch.long)
    temp = torch.full((N,), T)
    y = penalise(x[0].numpy(), (counts[0] != 0).numpy(), r).astype(np.float64) / T
    q = np.exp(y - y.max())
    q /= q.sum()
    raw = np.exp(x[0].double().numpy() / T - float(x.max()) / T)
    raw /= raw.sum()
    assert np.abs(q - raw).max() > 0.05  # the penalty moves the distribution
    rp = ref.sample_replay(x.expand(N, V), temp, seeds=i * 2654435761 + 17, step=i % 4, proc=proc,
                           counts=counts.clone(), nsplit=3, rep_tab=rep_tab)
    assert bool(rp.plain.all())
    _fits(rp.tokens.numpy(), q, N, "replay")
    tok = ref.sample(x.expand(N, V), temp, seeds=i, proc=proc, counts=counts.clone(), rep_tab=rep_tab)
    _fits(tok.numpy(), q, N, "ref.sample")
    with pytest.raises(AssertionError):
        _fits(rp.tokens.numpy(), raw, N, "replay against the raw row")
