"""JSON mode on the CPU: the automaton against ``json.loads``, masks against the byte walk, the plumbing (schema, pipe,
TP wire format, state seeding) and the CPU engine end to end. Everything compared is an integer: equalities only.
The corpus, the synthetic vocabulary and the helpers are shared with tests/test_json_mode_gpu.py."""
from __future__ import annotations

import json
import pickle

import numpy as np
import pytest
import torch
from fastapi.testclient import TestClient
from pydantic import ValidationError

from kafka_llm_service_amd import ops
from kafka_llm_service_amd.db.local import MemoryDBClient
from kafka_llm_service_amd.engine import json_mode as jm
from kafka_llm_service_amd.engine import step_plan
from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
from kafka_llm_service_amd.engine.logits_proc import LogitsProcessor
from kafka_llm_service_amd.engine.sequence import SamplingParams, Sequence
from kafka_llm_service_amd.engine.step_plan import HostStep, ProcUpdates, SampleParams
from kafka_llm_service_amd.kafka.types import ChatCompletionRequest
from kafka_llm_service_amd.llm.stub import ScriptedProvider
from kafka_llm_service_amd.ops import reference as ref
from kafka_llm_service_amd.server.app import _sampling_kwargs, create_app
from kafka_llm_service_amd.server.state import ServerConfig, ServerState

MSG = [{"role": "user", "content": "hi"}]


def _nest(levels: int) -> bytes:
    """An object whose deepest container is at level ``levels`` (the object itself is level 1), arrays and objects
    alternating."""
    s, close = b'{"k":', b"}"
    for i in range(levels - 1):
        s, close = (s + b"[", b"]" + close) if i % 2 == 0 else (s + b'{"d":', b"}" + close)
    inner = s[-1:]
    return s + (b"" if inner == b"[" else b"1") + close if levels > 1 else b'{"k":1}'


VALID = [
    b"{}", b'{"a":1}', b'{"":""}', b'{"a":{}}', b'{"a":[]}', b'{"a":[[],{},[{}]]}', b'{"a":[1,2,3],"b":{"c":null}}',
    b'{"t":true,"f":false,"n":null}', b'{"a":0}', b'{"a":-0}', b'{"a":10}', b'{"a":-12.5}', b'{"a":0.0}',
    b'{"a":1e5}', b'{"a":1E5}', b'{"a":1e+5}', b'{"a":1.25e-7}', b'{"a":-0.5E+10}', b'{"a":[0,-1,2.5,3e2,4E-1]}',
    b'{"a":123456789012345678901234567890}', b'{"e":"\\"\\\\\\/\\b\\f\\n\\r\\t"}', b'{"u":"\\u00e9\\u20AC\\uD83D\\ude00"}',
    b'{"\\u0041":"x"}', '{"k":"é€😀"}'.encode(), '{"ключ":"値","𝄞":["é"]}'.encode(), b'{"del":"\x7f"}',
    b'{ }', b'{ "a" : 1 }', b'{\n\t"a"\r\n:\n[ 1 , 2 ]\n,\n"b" : { } }', b'{"a":[ ]}', b'{"a":1 }', b'{"a":[1 ,2]}',
    b'{"a":"  spaces  inside  "}', b'{"a":"{[,:]}"}', b'{"a":"true","true":null}', b'{"a":1,"a":2}',
    b'{"a":[[[[1]]]],"b":[{"c":[{"d":{}}]}]}', b'{"a":[true,false,null,"x",1,{},[]]}',
    _nest(2), _nest(5), _nest(31), _nest(32),
]
INVALID = [
    b"", b"[]", b"[1]", b"1", b'"a"', b"true", b"null", b" {}", b"\n{}", b"{} ", b"{}\n", b"{}{}", b"{}x",
    b'{"a":1,}', b'{,}', b'{"a":[1,]}', b'{"a":[,1]}', b'{"a"}', b'{"a":}', b'{"a" 1}', b'{a:1}', b"{'a':1}",
    b'{1:2}', b'{"a":1 "b":2}', b'{"a":[1 2]}', b'{"a":01}', b'{"a":-}', b'{"a":+1}', b'{"a":1.}', b'{"a":.5}',
    b'{"a":1e}', b'{"a":1e+}', b'{"a":0x10}', b'{"a":-01}', b'{"a":tru}', b'{"a":True}', b'{"a":nul}', b'{"a":NaN}',
    b'{"a":Infinity}', b'{"a":"\n"}', b'{"a":"\t"}', b'{"a":"\x00"}', b'{"a":"\\x41"}', b'{"a":"\\u12G4"}',
    b'{"a":"\\u12"}', b'{"a":"x}', b'{"a":[1}', b'{"a":{"b":1]}', b'{"a":1]', b'{"a":"\xed\xa0\x80"}',
    b'{"a":"\xc0\xaf"}', b'{"a":"\xe0\x80\xaf"}', b'{"a":"\xf0\x80\x80\xaf"}', b'{"a":"\xf4\x90\x80\x80"}',
    b'{"a":"\xff"}', b'{"a":"\x80"}', b'{"a":"\xc3"}', b'{"a":"\xe2\x82"}', b'{"\xc3":1}', _nest(33), _nest(40),
]


def _depth(o) -> int:
    if isinstance(o, dict):
        return 1 + max((_depth(v) for v in o.values()), default=0)
    if isinstance(o, list):
        return 1 + max((_depth(v) for v in o), default=0)
    return 0


def _reject_constant(name):
    raise ValueError(name)  # (json.loads reads NaN / Infinity, which RFC 8259 does not have)


def oracle(data: bytes) -> bool:
    """The text is strictly decoded UTF-8, begins with ``{`` and ends with ``}`` (JSON mode allows no whitespace
    around the document), ``json.loads`` reads it as an object, and no container lies deeper than 32 levels."""
    try:
        text = data.decode("utf-8")
        obj = json.loads(text, parse_constant=_reject_constant)
    except (ValueError, RecursionError):
        return False
    return isinstance(obj, dict) and text[:1] == "{" and text[-1:] == "}" and _depth(obj) <= jm.JSON_MAX_DEPTH


def corpus_states() -> list[tuple[int, int, int]]:
    """Every distinct state reached on the valid documents, byte by byte, in order of first appearance (START first,
    DONE among them)."""
    seen = {}
    for doc in VALID:
        st = jm.START_STATE
        seen.setdefault(st)
        for i in range(len(doc)):
            st = ref.json_walk(st, doc[i:i + 1])
            seen.setdefault(st)
    return list(seen)


_POOL = [b"{", b'"', b"a" * 64, b"", b"}", b'{"', b'":', b'",', b'"}', b"}}", b"]]", b"[[", b"[{", b"}]", b'{"a":[',
         b"null", b"tru", b"e,", b"\\u", b"00e9", b"\xc3", b"\xa9", b"\xe2\x82", b"\xac", b"\xf0\x9f", b"\x98\x80",
         b"  ", b" \n", b"1.5e", b"+3", b"-0", b"[[[[{", b'"}]]', b"]]]]}", b'":{"', b"0,", b", ", b'":"', b"\\n"]


def synthetic_table(V: int) -> jm.JsonTable:
    """A vocabulary of V ids: the pool above (1-byte, 2-byte, a 64-byte and an empty token, tokens that open and close
    several levels, split UTF-8), then every single byte, then two-byte fillers. The last id is the EOS; from V = 31 up
    id 10 is a second EOS and id 3 (the empty token) a special without bytes."""
    pieces = list(_POOL) + [bytes([b]) for b in range(256) if bytes([b]) not in _POOL]
    i = 0
    while len(pieces) < V:
        pieces.append(bytes([0x20 + i % 0x5F, 0x20 + (i // 0x5F) % 0x5F]))
        i += 1
    pieces = pieces[:V]
    return jm.JsonTable.from_byte_strings(pieces, [V - 1] if V < 31 else [V - 1, 10])


def tokenize(table: jm.JsonTable, data: bytes) -> list[int]:
    """Greedy longest match over the table's tokens (every single byte is a token from V = 295 up)."""
    by_bytes = {}
    for i in range(table.V):
        b = table.bytes_of(i)
        if b:
            by_bytes.setdefault(b, i)
    longest = max(len(b) for b in by_bytes)
    out, p = [], 0
    while p < len(data):
        for n in range(min(longest, len(data) - p), 0, -1):
            t = by_bytes.get(data[p:p + n])
            if t is not None:
                out.append(t)
                p += n
                break
        else:
            raise ValueError(f"byte {data[p]} has no token")
    return out


def unpack(words: np.ndarray, V: int) -> np.ndarray:
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:V].astype(bool)


# ---- the automaton ------------------------------------------------------------------------------------------------------
def test_table_shape_and_abi_constants():
    assert jm.TRANS.shape == (64, 256) and jm.TRANS.dtype == np.uint8 and jm.N_STATES < 64
    assert (jm.TRANS[jm.DONE] & 63 == jm.DEAD).all() and (jm.TRANS[jm.N_STATES:] & 63 == jm.DEAD).all()
    assert (jm.TRANS[jm.START] & 63 != jm.DEAD).sum() == 1  # only "{": no whitespace before the document
    # the ids the kernels name (ops/csrc/kafka_abi.h)
    abi = open(ops.__file__.replace("__init__.py", "csrc/kafka_abi.h")).read()
    assert (f"JSON_EXPECT_KEY = {jm.EXPECT_KEY}, JSON_EXPECT_VALUE = {jm.EXPECT_VALUE}, JSON_DONE = {jm.DONE};" in abi
            and f"JSON_MAX_DEPTH = {jm.JSON_MAX_DEPTH};" in abi and f"JSON_STATE_INTS = {jm.JSON_STATE_INTS};" in abi
            and step_plan.JSON_STATE_INTS == jm.JSON_STATE_INTS)


def test_corpus_sizes_and_oracle_split():
    assert len(VALID) >= 40 and len(INVALID) >= 40
    assert all(oracle(d) for d in VALID), [d for d in VALID if not oracle(d)]
    assert not any(oracle(d) for d in INVALID), [d for d in INVALID if oracle(d)]
    assert _depth(json.loads(_nest(32))) == 32 and _depth(json.loads(_nest(33))) == 33


@pytest.mark.parametrize("doc", VALID + INVALID, ids=lambda d: repr(d[:24]))
def test_walk_reaches_done_iff_json_object(doc):
    st = jm.START_STATE
    alive = []
    for i in range(len(doc)):
        st = ref.json_walk(st, doc[i:i + 1])
        alive.append(st[0] != jm.DEAD)
    assert (st[0] == jm.DONE) == oracle(doc), (doc, jm.STATE_NAMES[st[0]])
    assert ref.json_walk(jm.START_STATE, doc) == st  # (byte by byte and at once agree)
    if oracle(doc):
        assert all(alive) and st == (jm.DONE, 0, 0)  # every prefix of a valid document is alive
    else:
        assert st[0] != jm.DONE


def test_depth_limit_and_stack_bits():
    st = ref.json_walk(jm.START_STATE, _nest(32)[:-32])
    assert st[1] == 32 and st[2] >> 31 == 0 and st[2] & 1 == 1  # level 32 is an array here, level 1 the object
    for b in (b"[", b"{"):
        assert ref.json_walk(st, b)[0] == jm.DEAD  # a 33rd level
    assert ref.json_walk(ref.json_walk(jm.START_STATE, b'{"a":[{'), b"}]}") == (jm.DONE, 0, 0)
    rec = jm.state_record((jm.AFTER_VALUE, 32, 0xFFFFFFFF))
    assert rec.dtype == np.int32 and rec[2] == -1 and jm.record_state(rec) == (jm.AFTER_VALUE, 32, 0xFFFFFFFF)


# ---- masks and advance ----------------------------------------------------------------------------------------------------
def test_mask_iff_advance_survives_on_every_corpus_state():
    table = synthetic_table(330)
    states = corpus_states()
    assert len(states) > 150 and jm.START_STATE in states and (jm.DONE, 0, 0) in states
    eos = set(table.eos_ids.tolist())
    for st in states:
        keep = unpack(ref.json_mask_ref(st, table), table.V)
        for t in range(table.V):
            nxt = ref.json_advance_ref(st, t, table)
            want = (t in eos) if st[0] == jm.DONE else nxt[0] != jm.DEAD
            assert bool(keep[t]) == want, (st, t, table.bytes_of(t))
        # the EOS ids and the special without bytes are allowed in DONE only / never
        assert all(bool(keep[e]) == (st[0] == jm.DONE) for e in eos) and not keep[3]
    done = ref.json_mask_ref((jm.DONE, 0, 0), table)
    assert unpack(done, table.V).sum() == len(eos)
    assert ref.json_advance_ref((jm.DONE, 0, 0), 0, table) == (jm.DONE, 0, 0)  # a forced id leaves DONE alone
    assert not ref.json_mask_ref((jm.DEAD, 0, 0), table).any()


@pytest.mark.parametrize("V", [1, 31, 64, 65])
def test_mask_ragged_tails_have_clear_surplus_bits(V):
    table = synthetic_table(V)
    for st in [jm.START_STATE, (jm.DONE, 0, 0), ref.json_walk(jm.START_STATE, b'{"a')]:
        words = ref.json_mask_ref(st, table)
        assert words.dtype == np.uint32 and words.shape == (-(-V // 32),)
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")
        assert not bits[V:].any()


def test_real_table_matches_the_detokeniser():
    from kafka_llm_service_amd.engine.tokenizer import get_tokenizer

    tok = get_tokenizer()
    table = jm.table_for(tok, tok.eos_ids)
    assert table is jm.table_for(tok, tok.eos_ids) and table.V == 128256
    for i in (0, 1, 100, 5000, 127999, 128000, 128009, 128255):
        assert table.bytes_of(i) == tok.token_bytes(i)
    assert not table.lens[128000:].any()  # the specials have no bytes
    ids = tok.encode('{"answer": [1, 2.5, "é"], "ok": true}')
    assert b"".join(table.bytes_of(t) for t in ids).decode() == tok.decode(ids)
    st = jm.START_STATE
    for t in ids:
        assert unpack(ref.json_mask_ref(st, table), table.V)[t]
        st = ref.json_advance_ref(st, t, table)
    assert st == (jm.DONE, 0, 0)
    assert np.flatnonzero(unpack(ref.json_mask_ref(st, table), table.V)).tolist() == sorted(tok.eos_ids)


def test_cpu_ops_go_through_the_reference():
    table = synthetic_table(330)
    tabs = ops.JsonTables(table, "cpu")
    states = corpus_states()[:40]
    k, row0 = len(states), 3
    state = torch.zeros(k + 2, 4, dtype=torch.int32)
    slots = list(range(k + 1, 1, -1))  # (a slot is not its row's index)
    for s, st in zip(slots, states):
        state[s] = torch.from_numpy(jm.state_record(st))
    rows = torch.tensor([[i, s] for i, s in enumerate(slots)], dtype=torch.int32)
    mask_tab = torch.full((row0 + k + 2, table.W), 0x5A5A5A5A, dtype=torch.int32)
    ops.json_mask(tabs, rows, state, mask_tab, row0)
    for s, st in zip(slots, states):
        assert np.array_equal(mask_tab[row0 + s].numpy().view(np.uint32), ref.json_mask_ref(st, table))
    assert (mask_tab[:row0 + 2] == 0x5A5A5A5A).all()
    toks = tokenize(table, b'{"a":[')
    sampled = torch.tensor([toks[0]] * k, dtype=torch.int64)
    ops.json_advance(tabs, rows, sampled, state)
    for s, st in zip(slots, states):
        assert jm.record_state(state[s].numpy()) == ref.json_advance_ref(st, toks[0], table)
    with pytest.raises(ValueError):
        ops.json_mask(tabs, torch.tensor([[0, k + 2]], dtype=torch.int32), state, mask_tab, row0)


# ---- plumbing -------------------------------------------------------------------------------------------------------------
def test_schema_and_422():
    ok = ChatCompletionRequest(model="m", messages=MSG, response_format={"type": "json_object"})
    assert ok.json_mode and _sampling_kwargs(ok)["response_format"] == {"type": "json_object"}
    for off in ({}, dict(response_format=None), dict(response_format={"type": "text"})):
        req = ChatCompletionRequest(model="m", messages=MSG, **off)
        assert not req.json_mode and "response_format" not in _sampling_kwargs(req)
    with pytest.raises(ValidationError, match="json_object"):
        ChatCompletionRequest(model="m", messages=MSG, response_format={"type": "json_schema", "json_schema": {}})
    tools = [{"type": "function", "function": {"name": "f", "parameters": {}}}]
    for bad in (dict(response_format={"type": "xml"}), dict(response_format={}), dict(response_format="json_object"),
                dict(response_format={"type": "json_object"}, tools=tools),
                dict(response_format={"type": "json_object"}, tools=tools, tool_choice="auto")):
        with pytest.raises(ValidationError):
            ChatCompletionRequest(model="m", messages=MSG, **bad)
    assert ChatCompletionRequest(model="m", messages=MSG, response_format={"type": "json_object"}, tools=tools,
                                 tool_choice="none").json_mode
    assert not ChatCompletionRequest(model="m", messages=MSG, response_format={"type": "text"}, tools=tools).json_mode


class _Recording(ScriptedProvider):
    def __init__(self, script):
        super().__init__(script)
        self.kwargs = []

    async def stream_completion(self, messages, **kwargs):
        self.kwargs.append(dict(kwargs))
        async for ch in super().stream_completion(messages, **kwargs):
            yield ch


def test_chat_routes_validate_and_forward_response_format():
    prov = _Recording([{"text": "{}"}] * 6)
    st = ServerState(ServerConfig(backend="stub", sandbox="none"), llm_provider=prov, db=MemoryDBClient())
    jf = {"type": "json_object"}
    with TestClient(create_app(state=st)) as c:
        body = {"model": "kafka", "messages": MSG}
        tid = c.post("/v1/threads", json={}).json()["thread_id"]
        for url in ("/v1/chat/completions", f"/v1/threads/{tid}/chat/completions"):
            r = c.post(url, json=dict(body, response_format={"type": "json_schema", "json_schema": {"name": "x"}}))
            assert r.status_code == 422 and "json_object" in r.text
            assert c.post(url, json=dict(body, response_format={"type": "yaml"})).status_code == 422
            tools = [{"type": "function", "function": {"name": "f", "parameters": {}}}]
            assert c.post(url, json=dict(body, response_format=jf, tools=tools)).status_code == 422
            r = c.post(url, json=dict(body, response_format=jf))
            assert r.status_code == 200 and prov.kwargs[-1]["response_format"] == jf
            assert r.json()["choices"][0]["message"]["content"] == "{}"  # (the stub provider ignores the field)
            assert c.post(url, json=dict(body, response_format={"type": "text"})).status_code == 200
            assert "response_format" not in prov.kwargs[-1]
        assert c.post("/v1/chat/completions", json=dict(body, response_format=jf, stream=True)).status_code == 200
        assert prov.kwargs[-1]["response_format"] == jf


def test_remote_provider_forwards_json_object_only():
    from kafka_llm_service_amd.llm.remote import RemoteOpenAIProvider

    p = RemoteOpenAIProvider.__new__(RemoteOpenAIProvider)
    p.model, p.default_max_tokens = "m", 16
    assert p._body([], None, None, None, None, {"response_format": {"type": "json_object"}})["response_format"] == \
        {"type": "json_object"}
    for kw in ({}, {"response_format": None}, {"response_format": {"type": "text"}}):
        assert "response_format" not in p._body([], None, None, None, None, dict(kw))


def test_sampling_params_and_pipe():
    assert SamplingParams().json_mode is False
    p = SamplingParams(json_mode=True, temperature=0.5)
    assert pickle.loads(pickle.dumps(p)) == p and SamplingParams(**dict(p.__dict__)).json_mode is True  # (the pipes)
    for bad in (1, "true", None):
        with pytest.raises(ValueError):
            SamplingParams(json_mode=bad)
    with pytest.raises(ValueError):
        SamplingParams(json_mode=True, allowed_tokens_fn=lambda ids: None)
    with pytest.raises(ValueError):
        SamplingParams(json_mode=True, tool_grammar={"tools": []})


def test_wire_round_trip():
    n = 4
    h = HostStep(B=n, T=n, n_rows=n)
    h.i64 = np.arange(4 * n, dtype=np.int64)
    h.i32 = np.arange(1 + n, dtype=np.int32)
    proc = np.zeros((n, 8), np.int32)
    proc[:, 2] = -1
    proc[[1, 3], 0], proc[[1, 3], 1] = 1, [512 + 7, 512 + 2]
    upd = ProcUpdates(json_slots=np.array([7], np.int32),
                      json_states=jm.state_record((jm.AFTER_VALUE, 32, 0x80000001))[None])
    jrows = np.array([[1, 7], [3, 2]], np.int32)
    sp = SampleParams(np.full(n, 0.7, np.float32), np.ones(n, np.float32), np.zeros(n, np.int32),
                      np.arange(n, dtype=np.int64), proc, False, upd, json_rows=jrows)
    hdr, payload = step_plan.pack_plan(h, sp)
    _, sp2 = step_plan.unpack_plan(hdr, payload)
    assert np.array_equal(sp2.json_rows, jrows) and sp2.json_rows.dtype == np.int32 and np.array_equal(sp2.proc, proc)
    assert np.array_equal(sp2.upd.json_slots, upd.json_slots) and np.array_equal(sp2.upd.json_states, upd.json_states)
    assert jm.record_state(sp2.upd.json_states[0]) == (jm.AFTER_VALUE, 32, 0x80000001)
    # rows without a seed, a seed-free and row-free plan: nothing rides along
    sp.upd = None
    _, sp3 = step_plan.unpack_plan(*step_plan.pack_plan(h, sp))
    assert np.array_equal(sp3.json_rows, jrows) and sp3.upd is None
    sp.json_rows = None
    hdr0, payload0 = step_plan.pack_plan(h, sp)
    _, sp4 = step_plan.unpack_plan(hdr0, payload0)
    assert sp4.json_rows is None and sp4.upd is None and payload0.size == payload.size - 4 * (1 + 4 + 4)
    bad = ProcUpdates(json_slots=np.array([1, 2], np.int32), json_states=np.zeros((1, 4), np.int32))
    with pytest.raises(ValueError):
        step_plan.pack_plan(h, SampleParams(sp.temp, sp.topp, sp.topk, sp.seeds, proc, False, bad))


def test_slot_seeding_on_admission_and_re_prefill():
    table = synthetic_table(330)
    lp = LogitsProcessor("cpu", table.V, max_slots=4, mask_rows=8, json_slots=4)
    lp.set_json_table(table)
    a = Sequence("a", [1], SamplingParams(json_mode=True))
    b = Sequence("b", [1], SamplingParams(json_mode=True, presence_penalty=0.5))
    plain = Sequence("c", [1], SamplingParams(presence_penalty=0.5))
    # admission: both are sampled from a prefill (behind zero decode rows) -> START records
    proc, upd = lp.build([(0, a, None), (1, b, None), (2, plain, None)], 3, n_decode=0)
    ja, jb = int(proc[0, 1]) - 8, int(proc[1, 1]) - 8
    assert proc[:2, 0].tolist() == [1, 1] and {ja, jb} == {0, 1} and proc[2, 0] == 0 and proc[1, 2] >= 0
    assert sorted(upd.json_slots.tolist()) == [0, 1] and (upd.json_states == jm.state_record(jm.START_STATE)).all()
    assert lp.json_rows(proc).tolist() == [[0, ja], [1, jb]] and lp.json_rows(proc[2:]) is None
    lp.apply(upd, torch.from_numpy)
    # the states then move on the device only: decode rows seed nothing, carry no guard and name the same rows
    doc = tokenize(table, b'{"a":[[{"b":"x\\u00e9"}],1.5e+3')
    tabs = ops.JsonTables(table, "cpu")
    rows = torch.from_numpy(lp.json_rows(proc))
    for t in doc:
        a.output_ids.append(t)
        proc2, upd2 = lp.build([(0, a, None), (1, b, None)], 2, n_decode=2)
        assert upd2.json_slots.size == 0 and np.array_equal(proc2[:, :2], proc[:2, :2])
        ops.json_advance(tabs, rows[:1], torch.tensor([t]), lp.jstate)
    walked = jm.record_state(lp.jstate[ja].numpy())
    assert walked == ref.json_walk(jm.START_STATE, b'{"a":[[{"b":"x\\u00e9"}],1.5e+3') and walked[1] == 2
    # a preemption: the device record is lost to a re-prefill, the host seeds the state after the output ids so far
    lp.jstate[ja] = 0
    proc3, upd3 = lp.build([(0, b, None), (1, a, None)], 2, n_decode=1)  # (b decodes, a is re-prefilled)
    assert upd3.json_slots.tolist() == [ja] and jm.record_state(upd3.json_states[0]) == walked
    lp.apply(upd3, torch.from_numpy)
    assert jm.record_state(lp.jstate[ja].numpy()) == walked and jm.record_state(lp.jstate[jb].numpy()) == jm.START_STATE
    a.output_ids.append(-1)  # (a pending token cannot be walked: seeding needs landed tokens)
    with pytest.raises(RuntimeError):
        lp.build([(0, a, None)], 1, n_decode=0)
    with pytest.raises(ValueError):  # the two masks are not intersected
        lp.build([(0, b, [1, 2])], 1)
    # a processor without JSON slots keeps its tables as they were
    mt, _ = LogitsProcessor("cpu", 100, max_slots=2, mask_rows=8).tables()
    assert mt.shape[0] == 8 and lp.tables()[0].shape[0] == 12


# ---- the CPU engine end to end ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine():
    return LLMEngine(EngineConfig(model="tiny-llama", device="cpu", num_kv_blocks=256, max_model_len=2048))


def alive_prefixes(table, out: list[int], eos) -> tuple[int, int, int]:
    """Walks a reply token by token: every prefix must be alive; returns the last state."""
    st = jm.START_STATE
    for i, t in enumerate(out):
        if st[0] == jm.DONE:  # (only an EOS id is allowed; with ignore_eos the row keeps drawing it)
            assert t in eos, (i, t)
            continue
        st = ref.json_advance_ref(st, t, table)
        assert st[0] != jm.DEAD, (i, t, table.bytes_of(t))
    return st


def test_engine_every_prefix_is_alive(engine):
    table = engine._json_table()
    prompts = [[128000, 40, 41, 42], [128000, 50, 51]]
    sps = [SamplingParams(temperature=1.0, seed=s, max_tokens=12, json_mode=True) for s in (11, 12)]
    outs = engine.generate(prompts, sps)
    for o in outs:
        assert 1 <= len(o) <= 12
        alive_prefixes(table, o, engine.eos)
        assert table.bytes_of(o[0])[:1] == b"{"
    assert engine.runner.lp.stats["json_rows"] >= 2 and engine.runner.lp.stats["json_seeds"] == 2
    # a plain request beside a JSON one is not masked: it equals its run alone
    plain = SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True)
    alone = engine.generate([prompts[1]], plain)[0]
    mixed = engine.generate(prompts, [sps[0], plain])
    assert mixed[1] == alone and mixed[0] == outs[0]


def test_engine_logit_bias_closes_the_document(engine):
    from kafka_llm_service_amd.engine.tokenizer import tokenizer_for_model

    tok = tokenizer_for_model(engine.model_cfg)
    table = engine._json_table()
    push = {tok.encode(s)[0]: 40.0 for s in ('"', ":", "}")}
    assert len(push) == 3 and all(len(tok.encode(s)) == 1 for s in ('"', ":", "}"))
    for seed in (3, 4):
        sp = SamplingParams(temperature=1.0, seed=seed, max_tokens=64, json_mode=True, logit_bias=push)
        seq = engine.add_request(f"bias-{seed}", [128000, 60, 61], sp)
        while not seq.finished:
            engine.step()
        out = seq.output_ids
        assert seq.finish_reason == "stop" and out[-1] in engine.eos
        assert alive_prefixes(table, out, engine.eos) == (jm.DONE, 0, 0)
        text = tok.decode(out)
        assert isinstance(json.loads(text), dict), text
    cut = engine.add_request("cut", [128000, 60, 61], SamplingParams(temperature=1.0, seed=5, max_tokens=3,
                                                                     json_mode=True))
    while not cut.finished:
        engine.step()
    assert cut.finish_reason in ("length", "stop") and (cut.finish_reason == "length") == (cut.output_ids[-1] not in
                                                                                            engine.eos)


def test_engine_preemption_resumes_from_the_right_state(engine):
    g = torch.Generator().manual_seed(5)
    prompts = [[128000] + torch.randint(0, 5000, (50,), generator=g).tolist() for _ in range(4)]
    sp = SamplingParams(temperature=0.0, max_tokens=20, json_mode=True, ignore_eos=True)
    want = LLMEngine(EngineConfig(model="tiny-llama", device="cpu", num_kv_blocks=256, max_model_len=2048),
                     model=engine.model).generate(prompts, sp)
    small = LLMEngine(EngineConfig(model="tiny-llama", device="cpu", num_kv_blocks=12, max_model_len=2048),
                      model=engine.model)
    got = small.generate(prompts, sp)
    assert small.sched.num_preemptions > 0 and small.runner.lp.stats["json_seeds"] > 4
    assert got == want
    for o in got:
        alive_prefixes(engine._json_table(), o, engine.eos)
