"""The opt-in automaton tool grammar on the CPU (engine/tool_automaton.py, ops/reference.py tool_mask_ref /
tool_advance_ref, the plan section, the logits processor and the engine). Everything is integer work: every comparison
is equality."""
import json
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from kafka_llm_service_amd import ops
from kafka_llm_service_amd.engine import json_mode as jm
from kafka_llm_service_amd.engine import json_schema as js
from kafka_llm_service_amd.engine import step_plan
from kafka_llm_service_amd.engine import tool_automaton as ta
from kafka_llm_service_amd.engine.chat_template import parse_tool_calls
from kafka_llm_service_amd.engine.constrained import Mask, ToolCallConstraint
from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
from kafka_llm_service_amd.engine.logits_proc import LogitsProcessor
from kafka_llm_service_amd.engine.scheduler import Scheduler
from kafka_llm_service_amd.engine.sequence import PENDING, SamplingParams, Sequence, SeqStatus
from kafka_llm_service_amd.engine.step_plan import HostStep, ProcUpdates, SampleParams
from kafka_llm_service_amd.engine.tokenizer import get_tokenizer
from kafka_llm_service_amd.ops import reference as ref


def fn(name, params):
    return {"type": "function", "function": {"name": name, "parameters": params}}


WEATHER = fn("get_weather", {
    "type": "object", "required": ["location", "days", "units", "tags", "deep", "opt"],
    "properties": {"location": {"type": "string", "minLength": 1}, "days": {"type": "integer", "minimum": 1},
                   "units": {"type": "string", "enum": ["c", "f"]},
                   "tags": {"type": "array", "items": {"type": "string"}, "minItems": 1},
                   "deep": {"type": "boolean"}, "opt": {"type": ["null", "number"], "minimum": 3, "maximum": 40},
                   "ignored": {"type": "string"}}})
SHELL = fn("shell_exec", {"type": "object", "properties": {"shell_id": {"type": "string"},
                                                           "command": {"type": "string", "pattern": "^.+$"},
                                                           "timeout": {"type": "integer"}},
                          "required": ["shell_id", "command"]})
TOOL_SETS = {
    "weather": [WEATHER, fn("get", {"type": "object", "properties": {}}),
                fn("idle", {"type": "object", "properties": {"summary": {"type": "string"}}, "required": ["summary"]})],
    "shell": [SHELL, fn("create_shell", {"type": "object", "properties": {"shell_id": {"type": "string"}},
                                         "required": ["shell_id"]})],
    "nested": [fn("plan", {"type": "object", "required": ["step", "meta"], "properties": {
        "step": {"type": "integer"}, "meta": {"type": "object", "required": ["kind", "ok", "xs"], "properties": {
            "kind": {"enum": ["a", "ab", "b"]}, "ok": {"type": "boolean"}, "nothing": {"type": "null"},
            "xs": {"type": "array", "items": {"type": "number"}}}}}}),
        fn("noop", {})],
}
# enum, boolean and null leaves only: a finite language
FINITE = [fn("switch", {"type": "object", "required": ["room", "on", "why"], "properties": {
    "room": {"enum": ["hall", "kitchen"]}, "on": {"type": "boolean"}, "why": {"type": "null"}}}),
    fn("mode", {"type": "object", "required": ["m"], "properties": {"m": {"enum": ["eco", "max", 3]}}})]
FAMILIES = {"llama3": 128256, "mistral": 32000}


@pytest.fixture(scope="module", params=list(FAMILIES))
def fam(request):
    tok = get_tokenizer(request.param, FAMILIES[request.param])
    return request.param, tok, jm.table_for(tok, tok.eos_ids, tok.vocab_size)


# ---- strictify -----------------------------------------------------------------------------------------------------------
def server_tools():
    from kafka_llm_service_amd.server_tools import (NotebookTools, PlannerTools, ShellTools, count_tool,
                                                    get_weather_tool)

    tools = [get_weather_tool, count_tool] + PlannerTools(None).tools + ShellTools(None).tools + \
        NotebookTools(None).tools
    return [fn(t.name, t.parameters) for t in tools]


def test_strictify_rules():
    s = ta.strictify(WEATHER["function"]["parameters"])
    assert list(s["properties"]) == s["required"] == ["location", "days", "units", "tags", "deep", "opt"]
    assert s["additionalProperties"] is False and s["properties"]["location"] == {"type": "string"}
    assert s["properties"]["days"] == {"type": "integer"} and s["properties"]["tags"] == {
        "type": "array", "items": {"type": "string"}}
    assert s["properties"]["opt"] == {"type": ["null", "number"]}
    assert s["properties"]["units"] == {"type": "string", "enum": ["c", "f"]}
    # optional properties go, a missing type is a string, unions and $ref stay
    odd = {"type": "object", "required": ["b", "a", "gone"], "properties": {
        "a": {"pattern": "x+"}, "b": {"anyOf": [{"type": "integer", "maximum": 3}, {"format": "date"}]},
        "c": {"type": "string"}}, "$defs": {"p": {"type": "integer", "minimum": 0}}}
    so = ta.strictify(odd)
    assert so == {"type": "object", "properties": {"b": {"anyOf": [{"type": "integer"}, {"type": "string"}]},
                                                  "a": {"type": "string"}},
                  "required": ["b", "a"], "additionalProperties": False, "$defs": {"p": {"type": "integer"}}}
    ref_s = ta.strictify({"type": "object", "required": ["n"], "properties": {"n": {"$ref": "#/$defs/p"}},
                          "$defs": {"p": {"type": "integer", "minimum": 0}}})
    assert ref_s["properties"]["n"] == {"$ref": "#/$defs/p"}
    assert ta.strictify({}) == {"type": "string"} and ta.strictify({"type": "object"}) == {
        "type": "object", "properties": {}, "required": [], "additionalProperties": False}
    for sch in (s, so, ref_s):  # idempotent, unchanged when strict, and json_schema compiles it
        assert ta.strictify(sch) == sch
        js.compile_schema(sch)
    strict = {"type": "object", "properties": {"x": {"type": "integer", "description": "d"}}, "required": ["x"],
              "additionalProperties": False}
    assert ta.strictify(strict) == strict


def test_strictify_on_the_servers_own_tools():
    tools = server_tools()
    assert len(tools) >= 8
    for t in tools:
        s = ta.strictify(t["function"]["parameters"])
        assert ta.strictify(s) == s
        js.compile_schema(s)
    for family in FAMILIES:
        d = ta.compile_tool_body(tools, [t["function"]["name"] for t in tools], family)
        assert d.S <= js.SCHEMA_MAX_STATES and d.nbytes <= js.SCHEMA_TAB_BYTES


# ---- the language ----------------------------------------------------------------------------------------------------------
def conforms(v, sch, defs=None) -> bool:
    """A small conformance check of a value against a strict schema, independent of the automaton."""
    defs = sch.get("$defs", {}) if defs is None else defs
    if "$ref" in sch:
        return conforms(v, defs[sch["$ref"][8:]], defs)
    if "anyOf" in sch:
        return any(conforms(v, a, defs) for a in sch["anyOf"])
    if "enum" in sch:
        return any(type(v) is type(e) and v == e for e in sch["enum"])
    types = sch["type"] if isinstance(sch["type"], list) else [sch["type"]]
    for t in types:
        if t == "string" and isinstance(v, str) or t == "null" and v is None or t == "boolean" and isinstance(v, bool):
            return True
        if t == "integer" and isinstance(v, int) and not isinstance(v, bool):
            return True
        if t == "number" and isinstance(v, (int, float)) and not isinstance(v, bool):
            return True
        if t == "array" and isinstance(v, list) and all(conforms(x, sch["items"], defs) for x in v):
            return True
        if t == "object" and isinstance(v, dict) and list(v) == sch["required"] and all(
                conforms(v[k], sch["properties"][k], defs) for k in v):
            return True
    return False


def valid_call(data: bytes, tools, names, family) -> bool:
    """json.loads (bytes from 0x80 up are opaque string content: the language takes them one by one), the compact
    shape, the name and the arguments."""
    try:
        text = data.decode("utf-8", "surrogateescape")
        # (json.loads takes "-0", "1e5" and the like as the grammar does; it also takes NaN / Infinity, which no
        # substitution of one byte can spell here)
        obj = json.loads(text)
    except (ValueError, RecursionError):
        return False
    if not compact(text):
        return False
    if family == "mistral":
        if not (isinstance(obj, list) and len(obj) == 1):
            return False
        obj = obj[0]
    key = "parameters" if family == "llama3" else "arguments"
    if not (isinstance(obj, dict) and list(obj) == ["name", key] and isinstance(obj["name"], str)):
        return False
    if obj["name"] not in names or '"name":"' + obj["name"] + '"' not in text:
        return False
    table = ta.tool_table(tools)
    return conforms(obj[key], ta.strictify(table[obj["name"]] or {"type": "object"}))


def compact(text: str) -> bool:
    """No whitespace outside strings: the only freedom json.loads grants that the body's shape does not."""
    in_str = esc = False
    for ch in text:
        if in_str:
            if esc:
                esc = False
            elif ch == "\\":
                esc = True
            elif ch == '"':
                in_str = False
        elif ch == '"':
            in_str = True
        elif ch in " \t\n\r":
            return False
    return True


CALLS = {
    "weather": [('get_weather', {"location": "Paris é", "days": 12, "units": "c", "tags": [], "deep": True,
                                 "opt": None}),
                ('get_weather', {"location": "a\\\"b", "days": -3, "units": "f", "tags": ["x", "y z"], "deep": False,
                                 "opt": 3.5e2}),
                ("get", {}), ("idle", {"summary": "a much longer summary than twelve tokens " * 4})],
    "nested": [("plan", {"step": 0, "meta": {"kind": "ab", "ok": True, "xs": [1, 2.5, -7]}}), ("noop", {})],
}


def body(name, args, family) -> bytes:
    call = {"name": name, "parameters" if family == "llama3" else "arguments": args}
    return json.dumps(call if family == "llama3" else [call], ensure_ascii=False, separators=(",", ":")).encode()


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("which", list(CALLS))
def test_hand_written_calls_and_one_byte_mutations(family, which):
    tools = TOOL_SETS[which]
    names = [t["function"]["name"] for t in tools]
    dfa = ta.compile_tool_body(tools, names, family)
    subs = b' "\\,:{}[]0-9.eatn\x7f\x80\xc3\xff'
    n_ok = 0
    for name, args in CALLS[which]:
        doc = body(name, args, family)
        assert valid_call(doc, tools, names, family)
        assert ref.schema_walk(js.START, doc, dfa) == js.DONE, doc
        muts = [doc[:i] + doc[i + 1:] for i in range(len(doc))]
        muts += [doc[:i] + bytes([b]) + doc[i + 1:] for i in range(len(doc)) for b in subs if b != doc[i]]
        for m in muts:
            got = ref.schema_walk(js.START, m, dfa) == js.DONE
            assert got == valid_call(m, tools, names, family), m
            n_ok += got
    assert n_ok > 0  # (some mutations stay calls: a digit for a digit, a letter in a string)
    # a named choice admits that tool alone
    one = ta.compile_tool_body(tools, names[-1:], family)
    assert ref.schema_walk(js.START, body(*CALLS[which][-1], family), one) == js.DONE
    assert ref.schema_walk(js.START, body(*CALLS[which][0], family), one) == js.DEAD


def gen_ids(spec):
    return list(np.flatnonzero(spec.base)) + list(spec.extra) if isinstance(spec, Mask) else list(spec)


@pytest.mark.parametrize("which", list(TOOL_SETS))
def test_superset_of_the_generator(fam, which):
    """Seeded random walks through ToolCallConstraint, any allowed token at each step: every token the generator allows
    is allowed by tool_mask_ref, the same ids through tool_advance_ref end in TOOL_CLOSED when the generator is done."""
    family, tok, table = fam
    tools = TOOL_SETS[which]
    for seed in range(40):
        rng = random.Random(1000 * len(which) + seed)
        choice = rng.choice(["required", "auto", {"type": "function", "function": {
            "name": rng.choice(tools)["function"]["name"]}}])
        c = ToolCallConstraint(tok, tools, choice)
        plan = ta.plan_for(tok, tools, choice)
        assert (plan.open, plan.close) == (c.start, c.end)
        rec = ta.tool_record(js.START, plan.phase0, 3)
        out = []
        while len(out) < 400:
            spec = c(out) if out or choice != "auto" else [c.start]  # (auto: the walk opens a call)
            if out == [] and choice == "auto":
                assert c([]) is None
            if spec is None:
                break
            ids = gen_ids(spec)
            keep = ref.tool_mask_ref(rec, plan.open, plan.close, plan.dfa, table)
            # the whole allowed set at a sample of the steps (a 128k-id mask per step is the cost), the drawn id always
            t = int(rng.choice(ids))
            if len(ids) <= 64 or len(out) % 7 == 0:
                assert keep[np.asarray(ids)].all(), (out, [i for i in ids if not keep[i]][:5])
            assert keep[t]
            rec = ref.tool_advance_ref(rec, t, plan.open, plan.close, plan.dfa, table)
            assert rec[0] != js.DEAD and rec[3] == 4
            out.append(t)
        assert c.done and rec.tolist() == [js.DONE, ta.TOOL_CLOSED, 0, 4]
        assert parse_tool_calls(tok.decode(out))


def test_mask_iff_advance_survives(fam):
    family, tok, table = fam
    tools = TOOL_SETS["weather"]
    plan = ta.plan_for(tok, tools, "required")
    rng = np.random.default_rng(5)
    doc = body(*CALLS["weather"][1], family)
    recs = [ta.tool_record(js.START, ta.TOOL_OPEN, 0), ta.tool_record(js.START, ta.TOOL_FREE, 0),
            ta.tool_record(7, ta.TOOL_TEXT, 0), ta.tool_record(js.DONE, ta.TOOL_CLOSED, 0),
            ta.tool_record(js.DONE, ta.TOOL_BODY, 0), ta.tool_record(js.DEAD, ta.TOOL_BODY, 0)]
    for cut in (0, 9, 30, len(doc) // 2, len(doc) - 1):
        recs.append(ta.tool_record(ref.schema_walk(js.START, doc[:cut], plan.dfa), ta.TOOL_BODY, 0))
    probe = np.unique(np.concatenate([rng.integers(0, table.V, 300), [plan.open, plan.close, 0, table.V - 1],
                                      table.eos_ids]))
    for rec in recs:
        keep = ref.tool_mask_ref(rec, plan.open, plan.close, plan.dfa, table)
        assert np.array_equal(np.unpackbits(ref.tool_mask_words(rec, plan.open, plan.close, plan.dfa, table)
                                            .view(np.uint8), bitorder="little")[:table.V].astype(bool), keep)
        for t in probe.tolist():
            nxt = ref.tool_advance_ref(rec, t, plan.open, plan.close, plan.dfa, table)
            if rec[1] == ta.TOOL_CLOSED:  # (the envelope's table: only close is allowed, the record stays whatever comes)
                assert nxt.tolist() == rec.tolist() and keep[t] == (t == plan.close)
                continue
            assert keep[t] == (nxt[0] != js.DEAD), (rec, t)
            if rec[1] == ta.TOOL_BODY and rec[0] not in (js.DONE, js.DEAD) and table.lens[t]:
                assert nxt[0] == ref.schema_walk(int(rec[0]), table.bytes_of(t), plan.dfa)  # the definition
    with pytest.raises(ValueError):
        ref.tool_mask_ref(np.array([0, 5, 0, 1]), plan.open, plan.close, plan.dfa, table)
    with pytest.raises(ValueError):
        ref.tool_mask_ref(recs[0], table.V, plan.close, plan.dfa, table)


def test_tables_are_deterministic_across_processes_and_cached():
    code = ("import hashlib, sys; sys.path.insert(0, %r); import tests.test_tool_automaton as t; "
            "from kafka_llm_service_amd.engine import tool_automaton as ta; "
            "print([hashlib.sha256(ta.compile_tool_body(t.TOOL_SETS[k], [x['function']['name'] for x in "
            "t.TOOL_SETS[k]], f).tobytes()).hexdigest() for k in t.TOOL_SETS for f in t.FAMILIES])")
    import hashlib
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = [subprocess.run([sys.executable, "-c", code % root], capture_output=True, text=True, check=True,
                           cwd=root, env=dict(os.environ, PYTHONHASHSEED=str(h))).stdout for h in (1, 2)]
    mine = [hashlib.sha256(ta.compile_tool_body(TOOL_SETS[k], [x["function"]["name"] for x in TOOL_SETS[k]], f)
                           .tobytes()).hexdigest() for k in TOOL_SETS for f in FAMILIES]
    assert outs[0] == outs[1] == str(mine) + "\n"
    names = [x["function"]["name"] for x in TOOL_SETS["shell"]]
    assert ta.compile_tool_body(TOOL_SETS["shell"], names, "llama3") is ta.compile_tool_body(
        json.loads(json.dumps(TOOL_SETS["shell"])), names, "llama3")
    assert ta.compile_tool_body(TOOL_SETS["shell"], names[::-1], "llama3") is not ta.compile_tool_body(
        TOOL_SETS["shell"], names, "llama3")
    # the builder's new switches default to json_schema's tables
    sch = ta.strictify(WEATHER["function"]["parameters"])
    js._CACHE.clear()
    assert hashlib.sha256(js.compile_schema(sch).tobytes()).hexdigest() == hashlib.sha256(
        js.compile_schema(json.loads(json.dumps(sch))).tobytes()).hexdigest()


def test_limits_and_their_error_texts():
    wide = {"type": "object", "required": [f"k{i}" for i in range(40)],
            "properties": {f"k{i}": {"enum": [("v%d_" % j) * 12 for j in range(20)]} for i in range(40)}}
    with pytest.raises(ValueError, match=r"tool 'big': schema: .*exceeds the limit of (8192 states|262144 bytes)"):
        ta.compile_tool_body([fn("ok", {}), fn("big", wide)], ["ok", "big"], "llama3")
    with pytest.raises(ValueError, match=r"tool 'e': schema: `enum` at #/properties/x/enum/0 holds a value"):
        ta.compile_tool_body([fn("e", {"type": "object", "required": ["x"], "properties": {"x": {"enum": [[1]]}}})],
                             ["e"], "mistral")
    with pytest.raises(ValueError, match=r"tool 'r': schema: `\$ref`"):
        ta.compile_tool_body([fn("r", {"type": "object", "required": ["x"], "properties": {
            "x": {"$ref": "#/$defs/none"}}})], ["r"], "llama3")
    with pytest.raises(ValueError, match="unknown tool 'nope'"):
        ta.compile_tool_body([fn("ok", {})], ["nope"], "llama3")
    with pytest.raises(ValueError, match="mode must be one of program, automaton"):
        ta.grammar_mode({"mode": "fast"})
    assert ta.grammar_mode({}) == ta.grammar_mode(None) == "program" and ta.grammar_mode({}, "automaton") == "automaton"
    tok = get_tokenizer("llama3")
    assert ta.plan_for(tok, TOOL_SETS["shell"], "none") is None
    with pytest.raises(ValueError):
        ta.plan_for(tok, TOOL_SETS["shell"], {"type": "function", "function": {"name": "nope"}})


def test_sampling_params_modes():
    g = {"tools": TOOL_SETS["shell"], "tool_choice": "required"}
    assert SamplingParams(tool_grammar=g).tool_plan is None
    SamplingParams(tool_grammar={**g, "mode": "automaton"})
    SamplingParams(tool_grammar={**g, "mode": "program"}, allowed_tokens_fn=lambda ids: None)
    for bad in (dict(tool_grammar={**g, "mode": "automaton"}, allowed_tokens_fn=lambda ids: None),
                dict(tool_grammar={**g, "mode": "automaton"}, json_mode=True),
                dict(tool_grammar={**g, "mode": "automaton"}, json_schema='{"type":"object"}'),
                dict(tool_grammar={**g, "mode": "fast"})):
        with pytest.raises(ValueError):
            SamplingParams(**bad)


# ---- the wire format ---------------------------------------------------------------------------------------------------------
def _step(n=4):
    h = HostStep(B=n, T=n, n_rows=n)
    h.i64 = np.arange(4 * n, dtype=np.int64)
    h.i32 = np.arange(1 + n, dtype=np.int32)
    proc = np.zeros((n, 8), np.int32)
    proc[:, 2] = -1
    return h, proc, (np.full(n, 0.7, np.float32), np.ones(n, np.float32), np.zeros(n, np.int32),
                     np.arange(n, dtype=np.int64))


def test_plan_bytes_unchanged_when_absent_and_round_trip_when_present():
    h, proc, arrays = _step()
    names = [x["function"]["name"] for x in TOOL_SETS["shell"]]
    d1, d2 = ta.compile_tool_body(TOOL_SETS["shell"], names, "llama3"), js.compile_schema(
        {"type": "object", "properties": {}, "required": [], "additionalProperties": False})
    srows = np.array([[1, 7, 4]], np.int32)
    old_upd = lambda: ProcUpdates(json_slots=np.array([7], np.int32), json_states=js.state_record(5, 4)[None],
                                  schema_tabs=[(4, d2.cls, d2.trans)])
    base = SampleParams(*arrays, proc, False, old_upd(), schema_rows=srows)
    h0, p0 = step_plan.pack_plan(h, base)
    explicit = SampleParams(*arrays, proc, False, old_upd(), schema_rows=srows, tool_rows=None)
    explicit.upd.tool_tabs, explicit.upd.tool_slots = [], np.zeros(0, np.int32)
    h1, p1 = step_plan.pack_plan(h, explicit)
    assert np.array_equal(h0, h1) and p0.tobytes() == p1.tobytes() and 0 < h0[31] < 1 << 32
    plain = step_plan.pack_plan(h, SampleParams(*arrays, None, False))[0]
    assert plain[31] == 0 and step_plan.PLAN_HDR == 32
    # with tool rows: behind the schema section, counted in the upper half of the same header word
    trows = np.array([[0, 3, 2, 128010, 128008], [2, 1, 2, 5, 2]], np.int32)
    upd = old_upd()
    upd.tool_tabs = [(2, d1.cls, d1.trans)]
    upd.tool_slots, upd.tool_states = np.array([3], np.int32), ta.tool_record(js.START, ta.TOOL_OPEN, 2)[None]
    sp = SampleParams(*arrays, proc, False, upd, schema_rows=srows, tool_rows=trows)
    hdr, payload = step_plan.pack_plan(h, sp)
    n_tool = int(hdr[31]) >> 32
    assert int(hdr[31]) & 0xFFFFFFFF == int(h0[31]) and n_tool > 0 and payload.size == p0.size + 4 * n_tool
    assert payload[:p0.size].tobytes() == p0.tobytes() and np.array_equal(hdr[:31], h0[:31] + (
        np.arange(31) == step_plan.PLAN_PAYLOAD_IDX) * 4 * n_tool)
    _, sp2 = step_plan.unpack_plan(hdr, payload)
    assert np.array_equal(sp2.tool_rows, trows) and sp2.tool_rows.dtype == np.int32
    assert np.array_equal(sp2.schema_rows, srows) and sp2.upd.tool_slots.tolist() == [3]
    assert sp2.upd.tool_states.tolist() == [[0, ta.TOOL_OPEN, 0, 3]] and len(sp2.upd.schema_tabs) == 1
    (i, c, t), = sp2.upd.tool_tabs
    assert i == 2 and np.array_equal(c, d1.cls) and np.array_equal(t, d1.trans) and t.dtype == np.uint16
    # rows alone, a table alone, seeds alone
    for u, r in ((None, trows), (ProcUpdates(tool_tabs=[(2, d1.cls, d1.trans)]), None),
                 (ProcUpdates(tool_slots=upd.tool_slots, tool_states=upd.tool_states), None)):
        _, sp3 = step_plan.unpack_plan(*step_plan.pack_plan(h, SampleParams(*arrays, proc, False, u, tool_rows=r)))
        assert (sp3.tool_rows is None) == (r is None) and (sp3.upd is None) == (u is None) and sp3.schema_rows is None
    with pytest.raises(ValueError):
        step_plan.pack_plan(h, SampleParams(*arrays, proc, False, None, tool_rows=np.zeros((1, 3), np.int32)))


# ---- the logits processor ------------------------------------------------------------------------------------------------------
def _seq(tok, tools, choice, name="s"):
    return Sequence(name, [1], SamplingParams(tool_plan=ta.plan_for(tok, tools, choice)))


def test_seeding_replay_slots_and_the_auto_drop(fam):
    family, tok, table = fam
    lp = LogitsProcessor("cpu", table.V, max_slots=4, mask_rows=8, json_slots=3)
    lp.set_json_table(table)
    a, b = _seq(tok, TOOL_SETS["weather"], "required", "a"), _seq(tok, TOOL_SETS["weather"], "auto", "b")
    c = Sequence("c", [1], SamplingParams(json_schema=js.canonical_text(ta.strictify({"type": "object"}))))
    plan = a.params.tool_plan
    assert plan.key == b.params.tool_plan.key and plan.key != plan.dfa.text and isinstance(plan.key, tuple)
    proc, upd = lp.build([(0, a, None), (1, b, None), (2, c, None)], 3, n_decode=0)
    assert len(upd.tool_tabs) == 1 and len(upd.schema_tabs) == 1  # one body for both rows, beside the schema's table
    buf = upd.tool_tabs[0][0]
    sa, sb, sc = (int(proc[i, 1]) - 8 for i in range(3))
    assert lp.tool_rows(proc).tolist() == [[0, sa, buf, plan.open, plan.close], [1, sb, buf, plan.open, plan.close]]
    assert lp.schema_rows(proc).tolist() == [[2, sc, upd.schema_tabs[0][0]]] and lp.json_rows(proc) is None
    assert dict(zip(upd.tool_slots.tolist(), upd.tool_states.tolist())) == {
        sa: [js.START, ta.TOOL_OPEN, 0, buf + 1], sb: [js.START, ta.TOOL_FREE, 0, buf + 1]}
    lp.apply(upd, torch.from_numpy)
    assert lp.stats["tool_seeds"] == 2 and lp.stats["tool_rows"] == 2 and lp.stats["schema_table_uploads"] == 2
    # decode steps: the ops move the records, the host seeds nothing — also past a PENDING id
    tabs, pool = lp.json_tables(), lp.schema_pool()
    doc = [plan.open] + [t for t in _tokens(table, body(*CALLS["weather"][0], family))]
    for t in doc[:9]:
        proc2, upd2 = lp.build([(0, a, None), (1, b, None)], 2, n_decode=2)
        rows = torch.from_numpy(lp.tool_rows(proc2))
        assert upd2.empty
        ops.tool_mask(tabs, pool, rows, 2, lp.jstate, lp.tables()[0], lp.n_mask_rows)
        for sl in (sa, sb):
            want = ref.tool_mask_words(lp.jstate[sl].numpy(), plan.open, plan.close, plan.dfa, table)
            assert np.array_equal(lp.tables()[0][8 + sl].numpy().view(np.uint32), want)
        ops.tool_advance(tabs, pool, rows, torch.tensor([t, t]), lp.jstate)
        a.output_ids.append(PENDING)
        b.output_ids.append(PENDING)
        lp.build([(0, a, None), (1, b, None)], 2, n_decode=2)  # (planned ahead: nothing on the host reads the id)
        a.output_ids[-1] = b.output_ids[-1] = t
    walked = ref.schema_walk(js.START, b"".join(table.bytes_of(t) for t in doc[1:9]), plan.dfa)
    assert lp.jstate[sa].tolist() == lp.jstate[sb].tolist() == [walked, ta.TOOL_BODY, 0, buf + 1]
    # a preemption: the re-prefill replays the landed ids
    lp.jstate[sa] = 0
    _, upd3 = lp.build([(0, a, None)], 1, n_decode=0)
    assert upd3.tool_slots.tolist() == [sa] and upd3.tool_states.tolist() == [[walked, ta.TOOL_BODY, 0, buf + 1]]
    assert not upd3.tool_tabs
    lp.apply(upd3, torch.from_numpy)
    assert lp.jstate[sa].tolist() == [walked, ta.TOOL_BODY, 0, buf + 1]
    # auto that does not open a call: a tool row while the first id is pending, none once it has landed as text
    d = _seq(tok, TOOL_SETS["weather"], "auto", "d")
    a.status = SeqStatus.FINISHED
    d.output_ids = [PENDING]
    assert ta.tool_row_live(d.params.tool_plan, d.output_ids)
    d.output_ids = [17]
    assert not ta.tool_row_live(d.params.tool_plan, d.output_ids) and ta.tool_row_live(b.params.tool_plan, b.output_ids)
    proc4, upd4 = lp.build([(0, d, None)], 1, n_decode=1)
    assert lp.tool_rows(proc4) is None and proc4[0, 0] == 0 and upd4.empty
    # finished sequences give slots and references back; a bad record is refused
    b.status = c.status = SeqStatus.FINISHED
    e = _seq(tok, TOOL_SETS["shell"], "required", "e")
    _, upd5 = lp.build([(0, e, None)], 1, n_decode=0)
    assert len(upd5.tool_tabs) == 1 and lp._stab_refs[buf] == 0
    with pytest.raises(ValueError):
        lp.build([(0, e, [1, 2])], 1)
    for rec in ([0, 5, 0, 1], [0, 1, 1, 1], [js.SCHEMA_MAX_STATES, 2, 0, 1], [0, 2, 0, 0]):
        with pytest.raises(ValueError):
            lp.apply(ProcUpdates(tool_slots=np.array([0], np.int32), tool_states=np.array([rec], np.int32)),
                     torch.from_numpy)


def _tokens(table, data: bytes) -> list[int]:
    """A greedy longest-match tokenisation over the table's byte strings."""
    by = {}
    for i in np.flatnonzero(table.lens > 0).tolist():
        by.setdefault(table.bytes_of(i), i)
    out, o = [], 0
    while o < len(data):
        for n in range(min(16, len(data) - o), 0, -1):
            t = by.get(data[o:o + n])
            if t is not None:
                out.append(t)
                o += n
                break
        else:
            raise AssertionError(data[o:o + 4])
    return out


def test_cpu_ops_skip_rules(fam):
    family, tok, table = fam
    plan = ta.plan_for(tok, TOOL_SETS["shell"], "required")
    tabs, pool = ops.JsonTables(table, "cpu"), ops.SchemaTables(2, "cpu")
    pool.load(1, plan.dfa.cls, plan.dfa.trans)
    state = torch.zeros(3, 4, dtype=torch.int32)
    state[0] = torch.from_numpy(ta.tool_record(js.START, ta.TOOL_OPEN, 1))
    state[1] = torch.tensor([0, 7, 0, 2], dtype=torch.int32)
    state[2] = torch.from_numpy(js.state_record(js.START, 0))
    bad = [[0, 3, 1, plan.open, plan.close], [2, 0, 1, plan.open, plan.close], [0, 0, 0, plan.open, plan.close],
           [0, 0, 2, plan.open, plan.close], [0, 1, 1, plan.open, plan.close], [0, 2, 1, plan.open, plan.close],
           [0, 0, 1, table.V, plan.close], [0, 0, 1, plan.open, -1]]
    mask_tab = torch.full((5, table.W), 0x5A5A5A5A, dtype=torch.int32)
    before = state.clone()
    ops.tool_mask(tabs, pool, torch.tensor(bad, dtype=torch.int32), 2, state, mask_tab, 1)
    ops.tool_advance(tabs, pool, torch.tensor(bad, dtype=torch.int32), torch.tensor([plan.open, 0]), state)
    assert (mask_tab == 0x5A5A5A5A).all() and torch.equal(state, before)
    good = torch.tensor([[0, 0, 1, plan.open, plan.close]], dtype=torch.int32)
    ops.tool_mask(tabs, pool, good, 2, state, mask_tab, 1)
    assert np.flatnonzero(np.unpackbits(mask_tab[1].numpy().view(np.uint8), bitorder="little")).tolist() == [plan.open]
    ops.tool_advance(tabs, pool, good, torch.tensor([plan.open, 0]), state)
    assert state[0].tolist() == [js.START, ta.TOOL_BODY, 0, 2]


# ---- scheduling and the CPU engine ------------------------------------------------------------------------------------------------
def longest_body(dfa) -> int:
    """The longest path START -> DONE in bytes; the language is finite iff the reachable graph has no cycle."""
    memo, on = {}, set()

    def go(s):
        if s == js.DONE:
            return 0
        if s in memo:
            return memo[s]
        assert s not in on, "the language is not finite"
        on.add(s)
        best = max(1 + go(int(n)) for n in set(dfa.trans[s].tolist()) if n != js.DEAD)
        on.discard(s)
        memo[s] = best
        return best
    return go(js.START)


@pytest.fixture(scope="module")
def engine():
    return LLMEngine(EngineConfig(model="tiny-llama", device="cpu", num_kv_blocks=256, max_model_len=2048))


def check_call(tok, out, tools, plan, family="llama3"):
    assert out[0] == plan.open and out[-1] == plan.close, tok.decode(out, False)
    data = b"".join(tok.token_bytes(t) for t in out[1:-1])
    names = [t["function"]["name"] for t in tools]
    assert valid_call(data, tools, names, family), data
    calls = parse_tool_calls(tok.decode(out))
    assert calls and len(calls) == 1 and calls[0]["function"]["name"] in names
    return calls[0]["function"]


def test_engine_required_named_and_auto(engine, monkeypatch):
    from kafka_llm_service_amd.engine.tokenizer import tokenizer_for_model

    tok = tokenizer_for_model(engine.model_cfg)
    prompt = tok.encode("switch the hall light on")
    named = {"type": "function", "function": {"name": "mode"}}
    lp = engine.runner.lp
    for choice, temp, seed in (("required", 0.0, 1), ("required", 1.0, 2), (named, 1.0, 3)):
        plan = ta.plan_for(tok, FINITE, choice)
        bound = 2 + longest_body(plan.dfa)  # open, at most one token per byte, close
        sp = SamplingParams(temperature=temp, max_tokens=bound, seed=seed,
                            tool_grammar={"tools": FINITE, "tool_choice": choice, "mode": "automaton"})
        seq = engine.add_request(f"t-{seed}", prompt, sp)
        assert seq.params.tool_plan is not None and seq.params.allowed_tokens_fn is None
        assert plan.close in seq.params.stop_token_ids
        while not seq.finished:
            engine.step()
        assert seq.finish_reason == "stop", tok.decode(seq.output_ids, False)
        f = check_call(tok, seq.output_ids, FINITE, plan)
        assert choice == "required" or f["name"] == "mode"
    assert lp.stats["tool_rows"] > 0 and lp.stats["tool_seeds"] == 3 and lp.stats["forced_rows"] == 0
    # auto: free text unless the first token opens a call; the row equals the unconstrained one and leaves the tool rows
    plain = SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True)
    auto = SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True,
                          tool_grammar={"tools": FINITE, "tool_choice": "auto", "mode": "automaton"})
    rows0 = lp.stats["tool_rows"]
    want = engine.generate([prompt], plain)[0]
    assert want[0] != ta.plan_for(tok, FINITE, "auto").open
    assert engine.generate([prompt], auto)[0] == want and 1 <= lp.stats["tool_rows"] - rows0 <= 2
    # auto that opens a call (the open token biased up) is held to the body
    plan = ta.plan_for(tok, FINITE, "auto")
    sp = SamplingParams(temperature=0.0, max_tokens=2 + longest_body(plan.dfa), logit_bias={plan.open: 100.0},
                        tool_grammar={"tools": FINITE, "tool_choice": "auto", "mode": "automaton"})
    out = engine.generate([prompt], sp)[0]
    check_call(tok, out, FINITE, plan)
    # the engine's default comes from the environment; "none" keeps the host mask; a bad tool set is refused
    monkeypatch.setenv("KAFKA_TOOL_GRAMMAR", "automaton")
    s1 = engine.add_request("env", prompt, SamplingParams(max_tokens=1, tool_grammar={"tools": FINITE,
                                                                                      "tool_choice": "required"}))
    s2 = engine.add_request("none", prompt, SamplingParams(max_tokens=1, tool_grammar={"tools": FINITE,
                                                                                       "tool_choice": "none"}))
    assert s1.params.tool_plan is not None and s2.params.tool_plan is None and s2.params.allowed_tokens_fn is not None
    with pytest.raises(ValueError, match="tool 'e'"):
        engine.add_request("bad", prompt, SamplingParams(tool_grammar={"tools": [fn("e", {"enum": [[1]]})],
                                                                       "tool_choice": "required"}))
    monkeypatch.delenv("KAFKA_TOOL_GRAMMAR")
    s3 = engine.add_request("dflt", prompt, SamplingParams(max_tokens=1, tool_grammar={"tools": FINITE,
                                                                                       "tool_choice": "required"}))
    assert s3.params.tool_plan is None and isinstance(s3.params.allowed_tokens_fn, ToolCallConstraint)
    while engine.has_unfinished():
        engine.step()


def test_a_pending_automaton_row_is_scheduled(engine):
    """No plan_state for such rows: with its last token PENDING the row is planned ahead, where a generator row in a
    choice state sits the step out."""
    from kafka_llm_service_amd.engine.tokenizer import tokenizer_for_model

    tok = tokenizer_for_model(engine.model_cfg)
    prompt = tok.encode("pick a mode")
    g = {"tools": FINITE, "tool_choice": "required"}
    bound = 2 + longest_body(ta.plan_for(tok, FINITE, "required").dfa)
    sa = engine.add_request("auto-row", prompt, SamplingParams(temperature=0.0, max_tokens=bound, tool_grammar={
        **g, "mode": "automaton"}))
    sg = engine.add_request("gen-row", prompt, SamplingParams(temperature=0.0, max_tokens=40, tool_grammar=g))
    ahead = engine.stats["planned_ahead"]
    seen_a = seen_g_out = 0
    for _ in range(12):
        engine.step()
        if engine._inflight is None or sa.finished or sg.finished:
            continue
        if sa.output_ids[-1:] == [PENDING]:
            batch = engine.sched.schedule(speculative=True)
            seen_a += sa in batch.decode
            if sg.output_ids[-1:] == [PENDING] and not Scheduler._grammar_plannable(sg):
                seen_g_out += sg not in batch.decode
    assert seen_a > 0 and seen_g_out > 0
    assert not hasattr(sa.params.tool_plan, "plan_state") and sa.params.allowed_tokens_fn is None
    while engine.has_unfinished():
        engine.step()
    assert engine.stats["planned_ahead"] > ahead
    check_call(tok, sa.output_ids, FINITE, sa.params.tool_plan)


def test_engine_preemption_resumes_with_the_same_tokens(engine):
    from kafka_llm_service_amd.engine.tokenizer import tokenizer_for_model

    tok = tokenizer_for_model(engine.model_cfg)
    g = torch.Generator().manual_seed(5)
    prompts = [[128000] + torch.randint(0, 5000, (50,), generator=g).tolist() for _ in range(4)]
    sp = SamplingParams(temperature=0.0, max_tokens=20, ignore_eos=True,
                        tool_grammar={"tools": TOOL_SETS["shell"], "tool_choice": "required", "mode": "automaton"})
    mk = lambda nb: LLMEngine(EngineConfig(model="tiny-llama", device="cpu", num_kv_blocks=nb, max_model_len=2048),
                              model=engine.model)
    want = mk(256).generate(prompts, sp)
    small = mk(12)
    got = small.generate(prompts, sp)
    assert small.sched.num_preemptions > 0 and small.runner.lp.stats["tool_seeds"] > 4
    assert got == want
    plan, table = ta.plan_for(tok, TOOL_SETS["shell"], "required"), engine._json_table()
    for o in got:
        rec = ta.tool_record(js.START, ta.TOOL_OPEN, 0)
        for t in o:
            assert ref.tool_mask_ref(rec, plan.open, plan.close, plan.dfa, table)[t]
            rec = ref.tool_advance_ref(rec, t, plan.open, plan.close, plan.dfa, table)
            if rec[1] == ta.TOOL_CLOSED:
                break


def test_server_config_and_provider_forward_the_mode(monkeypatch):
    from kafka_llm_service_amd.server.__main__ import FLAGS
    from kafka_llm_service_amd.server.state import ServerConfig

    assert FLAGS["tool_grammar"] == "KAFKA_TOOL_GRAMMAR"
    monkeypatch.setenv("KAFKA_TOOL_GRAMMAR", "automaton")
    assert ServerConfig.from_env().engine_kwargs["tool_grammar"] == "automaton"
    monkeypatch.delenv("KAFKA_TOOL_GRAMMAR")
    assert "tool_grammar" not in ServerConfig.from_env().engine_kwargs
    assert EngineConfig(model="tiny-llama", tool_grammar="automaton").tool_grammar == "automaton"
