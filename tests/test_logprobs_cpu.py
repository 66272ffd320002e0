"""Per-token logprobs without a GPU: the fp32 reference against float64, the engine plumbing on the CPU engine
(records per token, roll-backs and early stops, no work for steps nobody asked about, the TP wire format) and the
chat API (request fields, streamed and non-streamed ``logprobs``, unchanged replies for requests that do not ask)."""
import json
import math

import numpy as np
import pytest
import torch
from fastapi.testclient import TestClient

from kafka_llm_service_amd import ops
from kafka_llm_service_amd.db.local import MemoryDBClient
from kafka_llm_service_amd.engine import model_runner as mr
from kafka_llm_service_amd.engine.constrained import ToolCallConstraint
from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
from kafka_llm_service_amd.engine.sequence import SamplingParams, StepOutput
from kafka_llm_service_amd.engine.tokenizer import get_tokenizer
from kafka_llm_service_amd.models.oracle import dense_logits
from kafka_llm_service_amd.ops import reference as ref
from kafka_llm_service_amd.server.app import create_app
from kafka_llm_service_amd.server.state import ServerConfig, ServerState


# ---- reference vs float64 -------------------------------------------------------------------------------------------
def _f64(x, toks, k):
    ls = torch.log_softmax(x.double(), -1)
    vals, ids = torch.sort(ls, dim=-1, descending=True, stable=True)
    return ls.gather(1, toks[:, None])[:, 0], vals[:, :k], ids[:, :k]


@pytest.mark.parametrize("V", [8, 1003, 128256])
def test_reference_matches_float64(V):
    g = torch.Generator().manual_seed(V)
    x = torch.randn(4, V, generator=g) * 4
    x[1] = x[1].to(torch.bfloat16).float()  # ties
    x[2] = 0.75                             # all equal: ids 0..K-1, logprob -log V
    toks = torch.randint(0, V, (4,), generator=g)
    for k in (0, 5, 20):
        tl, pl, pi = ref.token_logprobs(x, toks, None, k)
        wl, wp, wi = _f64(x, toks, k)
        n = min(k, V)
        assert tl.dtype == pl.dtype == torch.float32 and pi.dtype == torch.int32 and pl.shape == pi.shape == (4, k)
        assert torch.equal(pi[:, :n].long(), wi) and (pi[:, n:] == -1).all() and torch.isinf(pl[:, n:]).all()
        assert (tl.double() - wl).abs().max() <= 1e-4
        if n:
            assert (pl[:, :n].double() - wp).abs().max() <= 1e-4
            assert pi[2, :n].tolist() == list(range(n)) and abs(tl[2].item() + math.log(V)) <= 1e-4
    # rows: a subset in the caller's order; bf16 input
    tl, pl, pi = ref.token_logprobs(x.to(torch.bfloat16), toks, [3, 0], 5)
    wl, wp, wi = _f64(x.to(torch.bfloat16), toks, min(5, V))
    assert torch.equal(pi[:, :min(5, V)].long(), wi[[3, 0]]) and (tl.double() - wl[[3, 0]]).abs().max() <= 1e-4
    # the op on CPU tensors is the reference, written through the packed record buffer
    buf = ops.logprob_records(2, 5, "cpu")
    got = ops.token_logprobs(x.to(torch.bfloat16), toks, [3, 0], 5, out=ops.unpack_logprob_records(buf, 5))
    assert torch.equal(got[0], tl) and torch.equal(got[2], pi) and buf.shape == (2, 11)


def test_sampling_params_fields():
    assert SamplingParams().logprobs is False and SamplingParams().top_logprobs == 0
    SamplingParams(logprobs=True, top_logprobs=20)
    for bad in (dict(top_logprobs=3), dict(logprobs=True, top_logprobs=21), dict(logprobs=True, top_logprobs=-1)):
        with pytest.raises(ValueError):
            SamplingParams(**bad)
    assert StepOutput("r", [1], False).logprobs is None


# ---- CPU engine -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    return LLMEngine(EngineConfig(model="tiny-llama", device="cpu", num_kv_blocks=64, max_model_len=2048)).model


def _engine(model, **kw):
    return LLMEngine(EngineConfig(model="tiny-llama", device="cpu", num_kv_blocks=512, max_model_len=2048, **kw),
                     model=model)


def _run(eng, prompts, sps):
    """Every StepOutput per request, in order."""
    seqs = [eng.add_request(f"r{i}", p, sp) for i, (p, sp) in enumerate(zip(prompts, sps))]
    outs: dict = {s.request_id: [] for s in seqs}
    while eng.has_unfinished():
        for o in eng.step():
            outs[o.request_id].append(o)
    return seqs, outs


def _records_consistent(outs, asking: bool):
    recs = []
    for o in outs:
        if not asking:
            assert o.logprobs is None
            continue
        assert (o.logprobs or []) == o.logprobs or not o.new_token_ids
        assert len(o.logprobs or []) == len(o.new_token_ids)  # no token without a record, no record without a token
        for t, r in zip(o.new_token_ids, o.logprobs or []):
            assert isinstance(r, tuple) and r[0] == t
            recs.append(r)
    return recs


@pytest.mark.parametrize("async_on", [False, True])
def test_engine_records(model, async_on):
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(0, 5000, (n,), generator=g).tolist() for n in (9, 30, 17, 22)]
    kw = dict(temperature=0.0, max_tokens=6, ignore_eos=True)
    sps = [SamplingParams(**kw, logprobs=True, top_logprobs=5), SamplingParams(**kw),
           SamplingParams(**kw, logprobs=True), SamplingParams(**kw)]
    eng = _engine(model, async_scheduling=async_on)
    seqs, outs = _run(eng, prompts, sps)
    for i, s in enumerate(seqs):
        recs = _records_consistent(outs[s.request_id], asking=i in (0, 2))
        if i not in (0, 2):
            continue
        assert [r[0] for r in recs] == s.output_ids and len(recs) == 6
        k = sps[i].top_logprobs
        # the bound the CPU engine tests put on the engine's logits against the dense oracle (test_engine_cpu.py: 0.05)
        ls = torch.log_softmax(dense_logits(model, prompts[i] + s.output_ids).float(), -1)
        for j, (t, lp, ids, lps) in enumerate(recs):
            row = ls[len(prompts[i]) - 1 + j]
            assert lp <= 0 and abs(lp - row[t].item()) < 0.05
            assert len(ids) == len(lps) == k
            assert all(a >= b for a, b in zip(lps, lps[1:]))
            if k:
                assert ids[0] == t  # greedy: the emitted id leads the alternatives
                assert lps[0] == lp
                assert all(abs(v - row[i2].item()) < 0.05 for i2, v in zip(ids, lps))
    # picklable as it is (the DP / worker pipes)
    import pickle

    o = outs["r0"][0]
    assert pickle.loads(pickle.dumps(o)).logprobs == o.logprobs


class _NarrowStrings(ToolCallConstraint):
    """The roll-back construction of tests/test_logits_proc.py: free strings over three string-safe tokens, so the
    plan-ahead guess "the pending token does not close the string" breaks every few tokens."""

    def __init__(self, tok, tools, choice):
        import types

        super().__init__(tok, tools, choice)
        base = self.cls
        narrow = np.zeros_like(base.str_safe)
        narrow[np.flatnonzero(base.str_safe)[200:203]] = True
        self.cls = types.SimpleNamespace(str_safe=narrow, digits=base.digits, digits_nz=base.digits_nz,
                                         digit_range=base.digit_range)


TOOLS = [{"type": "function", "function": {"name": "get_weather", "description": "weather", "parameters": {
    "type": "object", "properties": {"city": {"type": "string"}, "days": {"type": "integer"}},
    "required": ["city"]}}}]


def test_rollback_and_early_stop_keep_tokens_and_records_paired(model):
    tok = get_tokenizer("llama3")
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(0, 5000, (n,), generator=g).tolist() for n in (11, 26, 19)]
    eng = _engine(model, async_scheduling=True)
    free = SamplingParams(temperature=0.0, max_tokens=40, ignore_eos=True).__dict__
    first = LLMEngine.generate(_engine(model), [prompts[2]], SamplingParams(**free))[0]
    sps = [SamplingParams(temperature=0.9, max_tokens=70, ignore_eos=True, seed=40, logprobs=True, top_logprobs=2,
                          allowed_tokens_fn=_NarrowStrings(tok, TOOLS, "required")),
           SamplingParams(temperature=0.9, max_tokens=70, ignore_eos=True, seed=41, logprobs=True,
                          frequency_penalty=0.9, allowed_tokens_fn=_NarrowStrings(tok, TOOLS, "required")),
           # stops early: its 5th greedy token is a stop token, with the next step already in flight
           SamplingParams(temperature=0.0, max_tokens=40, ignore_eos=True, logprobs=True, top_logprobs=1,
                          stop_token_ids=[first[4]])]
    seqs, outs = _run(eng, prompts, sps)
    assert eng.stats.get("grammar_rollbacks", 0) > 0, eng.stats
    for s in seqs:
        recs = _records_consistent(outs[s.request_id], asking=True)
        assert [r[0] for r in recs] == s.output_ids
        assert all(r[1] <= 0 or math.isnan(r[1]) for r in recs)
    assert len(seqs[2].output_ids) <= 5 and seqs[2].finish_reason == "stop"
    # a grammar-forced token (known on the host at launch) still has its true raw logprob: not 0, the model's own
    forced = [r for r in _records_consistent(outs["r0"], True)][0]
    assert forced[0] == tok.special_id("<|python_tag|>") and forced[1] < -1.0


def test_no_asking_row_no_call(model, monkeypatch):
    calls = []
    orig = ops.token_logprobs
    monkeypatch.setattr(ops, "token_logprobs", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    g = torch.Generator().manual_seed(8)
    prompts = [torch.randint(0, 5000, (n,), generator=g).tolist() for n in (9, 14)]
    plain = SamplingParams(temperature=0.0, max_tokens=4, ignore_eos=True)
    eng = _engine(model)
    _, outs = _run(eng, prompts, [plain, plain])
    assert not calls and all(o.logprobs is None for os_ in outs.values() for o in os_)
    assert eng.runner._lp_host is None
    # one request asks for 3 tokens, the other runs on for 8: only the steps with the asking row call the op
    ask = SamplingParams(temperature=0.0, max_tokens=3, ignore_eos=True, logprobs=True)
    long = SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True)
    _run(_engine(model, async_scheduling=False), prompts, [ask, long])
    assert len(calls) == 3


def test_plan_wire_format_unchanged(model):
    """pack_plan / unpack_plan round-trip a step with logprob rows exactly as one without: the wire format stays, and
    a follower's SampleParams carry no logprob rows (followers never compute logprobs)."""
    eng = _engine(model)
    g = torch.Generator().manual_seed(9)
    prompts = [torch.randint(0, 5000, (n,), generator=g).tolist() for n in (9, 14)]
    payloads = []
    for ask in (False, True):
        seqs = [eng.add_request(f"w{int(ask)}{i}", p, SamplingParams(temperature=0.7, seed=i, max_tokens=2,
                                                                       logprobs=ask, top_logprobs=4 if ask else 0))
                for i, p in enumerate(prompts)]
        batch = eng.sched.schedule()
        host, sampled = eng.runner.build_host(batch)
        sp = eng.runner.sample_params(sampled)
        assert (sp.lp_rows is not None) == ask and sp.lp_k == (4 if ask else 0)
        hdr, payload = mr.pack_plan(host, sp)
        h2, sp2 = mr.unpack_plan(hdr, payload)
        assert sp2.lp_rows is None and sp2.lp_k == 0
        assert np.array_equal(h2.i64, host.i64) and np.array_equal(sp2.seeds, sp.seeds)
        assert np.array_equal(sp2.temp, sp.temp) and sp2.greedy == sp.greedy
        payloads.append((hdr.shape, payload.size, hdr[1:20].tolist()))
        for s in seqs:
            eng.abort(s.request_id)
    assert payloads[0] == payloads[1] and mr.PLAN_HDR == 32


# ---- API --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def api():
    st = ServerState(ServerConfig(backend="engine", model="tiny-llama", sandbox="none", max_model_len=8192,
                                  default_max_tokens=12, prompt_sections=["intro"], warm_prefix=False,
                                  engine_kwargs={"device": "cpu", "num_kv_blocks": 1024}), db=MemoryDBClient())
    with TestClient(create_app(state=st)) as c:
        yield c


def _frames(text):
    out = []
    for block in text.split("\n\n"):
        if block.startswith("data: "):
            out.append(block[6:] if block[6:] == "[DONE]" else json.loads(block[6:]))
    return out


BODY = {"model": "tiny-llama", "messages": [{"role": "user", "content": "Tell me about MI355X."}], "temperature": 0,
        "max_tokens": 10, "seed": 7, "tool_choice": "none"}


def _check_entries(entries, content, n_top=3):
    assert entries
    for e in entries:
        assert set(e) == {"token", "logprob", "bytes", "top_logprobs"}
        assert isinstance(e["token"], str) and e["logprob"] <= 0 and all(0 <= b < 256 for b in e["bytes"])
        assert len(e["top_logprobs"]) == n_top
        for a in e["top_logprobs"]:
            assert set(a) == {"token", "logprob", "bytes"}
        lps = [a["logprob"] for a in e["top_logprobs"]]
        assert lps == sorted(lps, reverse=True)
    text = b"".join(bytes(e["bytes"]) for e in entries).decode("utf-8", errors="replace")
    assert text.startswith(content), (text, content)


def test_api_logprobs_stream_and_json(api):
    r = api.post("/v1/chat/completions", json=dict(BODY, logprobs=True, top_logprobs=3))
    assert r.status_code == 200, r.text
    ch = r.json()["choices"][0]
    assert set(ch["logprobs"]) == {"content", "refusal"} and ch["logprobs"]["refusal"] is None
    entries = ch["logprobs"]["content"]
    _check_entries(entries, ch["message"]["content"])
    assert entries[0]["top_logprobs"][0]["token"] == entries[0]["token"]  # greedy
    # streamed: the frames' entries, concatenated, are the non-streamed list (same seed, temperature 0)
    fr = _frames(api.post("/v1/chat/completions", json=dict(BODY, logprobs=True, top_logprobs=3, stream=True)).text)
    assert fr[-1] == "[DONE]"
    got, text = [], ""
    for f in fr[:-1]:
        for c in f["choices"]:
            assert c["delta"].get("content") is None or isinstance(c["delta"]["content"], str)
            text += c["delta"].get("content") or ""
            if c.get("logprobs"):
                got += c["logprobs"]["content"]
    assert text == ch["message"]["content"]
    assert [(e["token"], e["bytes"]) for e in got] == [(e["token"], e["bytes"]) for e in entries]
    assert all(abs(a["logprob"] - b["logprob"]) < 1e-4 for a, b in zip(got, entries))
    assert [[t["token"] for t in e["top_logprobs"]] for e in got] == \
        [[t["token"] for t in e["top_logprobs"]] for e in entries]


def test_api_logprobs_validation(api):
    assert api.post("/v1/chat/completions", json=dict(BODY, top_logprobs=3)).status_code in (400, 422)
    assert api.post("/v1/chat/completions", json=dict(BODY, logprobs=True, top_logprobs=21)).status_code in (400, 422)
    assert api.post("/v1/chat/completions", json=dict(BODY, logprobs=False, top_logprobs=2)).status_code in (400, 422)
    r = api.post("/v1/chat/completions", json=dict(BODY, logprobs=True))
    assert r.status_code == 200 and all(e["top_logprobs"] == [] for e in r.json()["choices"][0]["logprobs"]["content"])


def test_api_unchanged_without_the_fields(api):
    """No ``logprobs`` key where none appears today, and the content frames are the pre-formatted fast-path bytes."""
    j = api.post("/v1/chat/completions", json=BODY).json()
    assert set(j["choices"][0]) == {"index", "message", "finish_reason"}
    assert set(j) == {"id", "object", "created", "model", "choices", "usage"}
    raw = api.post("/v1/chat/completions", json=dict(BODY, stream=True)).text
    assert "logprobs" not in raw
    fr = _frames(raw)
    for f in fr[:-1]:
        assert set(f) == {"id", "object", "created", "model", "choices"}
        for c in f["choices"]:
            assert set(c) == {"index", "delta", "finish_reason"} and set(c["delta"]) == {"role", "content",
                                                                                         "tool_calls"}
    assert "".join(c["delta"]["content"] or "" for f in fr[:-1] for c in f["choices"]) == \
        j["choices"][0]["message"]["content"]
    blocks = [b for b in raw.split("\n\n") if '"content":"' in b]
    assert blocks and all(b.endswith(',"tool_calls":null},"finish_reason":null}]}') for b in blocks)


def test_api_logprobs_with_stop_string(api):
    base = api.post("/v1/chat/completions", json=dict(BODY, max_tokens=12)).json()["choices"][0]["message"]["content"]
    assert len(base) > 6
    stop = base[4:7]
    for stream in (False, True):
        r = api.post("/v1/chat/completions", json=dict(BODY, max_tokens=12, logprobs=True, top_logprobs=3,
                                                       stop=[stop], stream=stream))
        assert r.status_code == 200
        if stream:
            fr = _frames(r.text)
            assert fr[-1] == "[DONE]" and not any("error" in f for f in fr[:-1])
            entries = [e for f in fr[:-1] for c in f["choices"] if c.get("logprobs") for e in c["logprobs"]["content"]]
            content = "".join(c["delta"].get("content") or "" for f in fr[:-1] for c in f["choices"])
        else:
            ch = r.json()["choices"][0]
            entries, content = ch["logprobs"]["content"], ch["message"]["content"]
        assert stop not in content and base.startswith(content)
        _check_entries(entries, content)  # the entries may run a few characters past the stop-string cut


def test_stub_provider_ignores_the_fields():
    from kafka_llm_service_amd.llm.stub import ScriptedProvider

    st = ServerState(ServerConfig(backend="stub", sandbox="none"), llm_provider=ScriptedProvider([{"text": "hi"}] * 2),
                     db=MemoryDBClient())
    with TestClient(create_app(state=st)) as c:
        body = {"model": "kafka", "messages": [{"role": "user", "content": "x"}], "logprobs": True, "top_logprobs": 2}
        j = c.post("/v1/chat/completions", json=body).json()
        assert j["choices"][0]["message"]["content"] == "hi" and j["choices"][0]["logprobs"] is None
        assert "logprobs" not in c.post("/v1/chat/completions", json=dict(body, stream=True)).text
