"""Structured outputs on the CPU: the schema compiler against hand-written documents and an independent validator, masks
against the byte walk, random documents and random walks, the compiler's properties and errors, the wire format, the
table pool of the logits processor and the chat API. Everything compared is an integer or a byte string: equalities
only. The schema table, the validator and the generators are shared with tests/test_json_schema_gpu.py."""
from __future__ import annotations

import hashlib
import json
import random
import re
import subprocess
import sys
from collections import deque

import numpy as np
import pytest
import torch
from fastapi.testclient import TestClient
from pydantic import ValidationError

from kafka_llm_service_amd import ops
from kafka_llm_service_amd.db.local import MemoryDBClient
from kafka_llm_service_amd.engine import json_schema as js
from kafka_llm_service_amd.engine import step_plan
from kafka_llm_service_amd.engine.logits_proc import LogitsProcessor
from kafka_llm_service_amd.engine.sequence import SamplingParams, SeqStatus, Sequence
from kafka_llm_service_amd.engine.step_plan import HostStep, ProcUpdates, SampleParams
from kafka_llm_service_amd.kafka.types import ChatCompletionRequest
from kafka_llm_service_amd.ops import reference as ref
from kafka_llm_service_amd.server.app import _sampling_kwargs, create_app
from kafka_llm_service_amd.server.state import ServerConfig, ServerState
from test_json_mode import MSG, _Recording, synthetic_table, tokenize, unpack


def obj(props: dict, **extra) -> dict:
    return dict({"type": "object", "properties": props, "required": list(props), "additionalProperties": False},
                **extra)


def arr(items) -> dict:
    return {"type": "array", "items": items}


STR, INT, NUM, BOOL, NULL = ({"type": t} for t in ("string", "integer", "number", "boolean", "null"))
_POINT = obj({"x": INT, "y": INT})

# name -> (schema, conforming documents, near misses as (alive prefix, the byte that kills it + anything))
SCHEMAS: dict[str, tuple[dict, list[bytes], list[tuple[bytes, bytes]]]] = {
    "empty": (obj({}), [b"{}", b"{ }", b"{\n\t}"], [(b"{}", b" "), (b"{", b'"a":1}'), (b"", b" {}"), (b"", b"[]")]),
    "scalars": (obj({"s": STR, "i": INT, "n": NUM, "b": BOOL, "z": NULL}),
                [b'{"s":"x","i":-12,"n":1.5e3,"b":true,"z":null}',
                 b'{ "s" : "\\u00e9\\n\\ud83d" ,\n"i":0, "n" : -0.5E+10 ,"b":false\t,"z": null\r\n}',
                 '{"s":"é€😀\x7f","i":123456789012345678901234567890,"n":7,"b":true,"z":null}'.encode()],
                [(b'{"', b'i":1'),                                          # wrong key order
                 (b'{"s":"x","i":1,"n":1,"b":true', b"}"),                   # a missing key
                 (b'{"s":"x","i":1,"n":1,"b":true,"z":null', b',"q":1}'),    # an extra key
                 (b'{"s":', b"1"), (b'{"s":"x","i":', b'"1"'), (b'{"s":"x","i":1,"n":1,"b":', b"null"),  # wrong types
                 (b'{"s":"x","i":0', b"1"), (b'{"s":"x","i":-', b"a"), (b'{"s":"x","i":1', b".5"),
                 (b'{"s":"x","i":1', b"e5"), (b'{"s":"x","i":1,"n":1.', b","), (b'{"s":"', b"\xc0\xaf"),
                 (b'{"s":"\xe0', b"\x80\xaf"), (b'{"s":"\xed', b"\xa0\x80"), (b'{"s":"', b"\n"), (b'{"s":"\\', b"x"),
                 (b'{"s":"x","i":1,"n":1,"b":true,"z":null}', b" "), (b'{"s":"x","i":1,"n":1,"b":true,"z":null}', b"}")]),
    "nested": (obj({"a": obj({"b": obj({"c": INT})}), "d": arr(obj({"x": STR, "y": arr(NUM)}))}),
               [b'{"a":{"b":{"c":1}},"d":[]}', b'{"a":{"b":{"c":-7}},"d":[{"x":"","y":[]},{"x":"q","y":[1,2.5,-3e2]}]}',
                b'{ "a" : { "b" : { "c" : 1 } } , "d" : [ { "x" : "s" , "y" : [ 1 , 2 ] } ] }'],
               [(b'{"a":{"b":{"c":1}', b',"z'), (b'{"a":{"b":{"c":1}},"d":[', b","), (b'{"a":{"b":{"c":1}},"d":[{"x":"","y":[1,', b"]"),
                (b'{"a":{"b":{"c":1}},"d":[{"x":"","y":[]}', b"}"), (b'{"a":{"b":{"c":1}},"d":[]', b"]")]),
    "union_shapes": (obj({"v": {"anyOf": [obj({"kind": {"const": "a"}, "x": INT}),
                                          obj({"kind": {"const": "b"}, "y": STR})]}}),
                     [b'{"v":{"kind":"a","x":5}}', b'{"v":{"kind":"b","y":"t"}}', b'{"v": {"kind" :"b" , "y": ""} }'],
                     [(b'{"v":{"kind":"a","', b"y"), (b'{"v":{"kind":"b","y":', b"5"), (b'{"v":{"kind":"', b"c"),
                      (b'{"v":{"', b"x")]),
    "enum_prefix": (obj({"e": {"enum": ["a", "ab", "abc"]}}), [b'{"e":"a"}', b'{"e":"ab"}', b'{"e": "abc" }'],
                    [(b'{"e":"a', b"c"), (b'{"e":"abc', b"d"), (b'{"e":"', b'"'), (b'{"e":"ab', b"\\"),
                     (b'{"e":', b"a")]),
    "nullable": (obj({"s": {"type": ["string", "null"]}}), [b'{"s":null}', b'{"s":"null"}', b'{"s" : "x"}'],
                 [(b'{"s":n', b"i"), (b'{"s":', b"1"), (b'{"s":nul', b"}")]),
    "ref_twice": ({"$defs": {"P": _POINT}, **obj({"a": {"$ref": "#/$defs/P"}, "b": {"$ref": "#/$defs/P"}})},
                  [b'{"a":{"x":1,"y":2},"b":{"x":-3,"y":0}}', b'{"a":{ "x":1,"y":2 },"b":{"x":3 ,"y":4}}'],
                  [(b'{"a":{"x":1,"y":2},"b":{"', b"y"), (b'{"a":{"x":1', b"}")]),
    "arrays": (obj({"a": arr(INT), "b": arr(arr(BOOL))}),
               [b'{"a":[],"b":[]}', b'{"a":[1,-2,30],"b":[[],[true],[false,true]]}', b'{"a":[ 1 , 2 ],"b":[ [ ] ]}'],
               [(b'{"a":[1,', b"]"), (b'{"a":[', b","), (b'{"a":[1 ', b"2"), (b'{"a":[1', b".5"),
                (b'{"a":[],"b":[', b"true")]),
    "enum_mixed": (obj({"e": {"enum": [1, 12, -5, True, None, "x", "é\"q"]}}),
                   [b'{"e":1}', b'{"e":12}', b'{"e":-5}', b'{"e":true}', b'{"e":null}', b'{"e":"x"}',
                    '{"e":"é\\"q" }'.encode()],
                   [(b'{"e":1', b"3"), (b'{"e":12', b"0"), (b'{"e":', b"f"), (b'{"e":-', b"1"), (b'{"e":"', b"y")]),
    "consts": (obj({"c": {"const": "fixed"}, "n": {"const": 42}, "t": {"type": "string", "enum": ["u", "v"]}}),
               [b'{"c":"fixed","n":42,"t":"u"}', b'{"c": "fixed" ,"n": 42 , "t":"v"}'],
               [(b'{"c":"fixe', b'"'), (b'{"c":"fixed","n":4', b","), (b'{"c":"fixed","n":42', b"0")]),
    "anyof_scalars": (obj({"v": {"anyOf": [INT, STR, arr(NULL)]}, "w": {"type": ["integer", "number"]}}),
                      [b'{"v":1,"w":1}', b'{"v":"1","w":1.5}', b'{"v":[null,null],"w":-2e-3}', b'{"v":[ ],"w":0}'],
                      [(b'{"v":1', b"."), (b'{"v":[', b"1"), (b'{"v":', b"t")]),
    "odd_keys": (obj({"ключ": STR, "a/b": INT, 'q"uote': BOOL, "": NULL}),
                 ['{"ключ":"v","a/b":1,"q\\"uote":true,"":null}'.encode()],
                 [('{"клю'.encode(), b"x"), ('{"ключ":"v","a'.encode(), b"~"), ('{"ключ":"v","a/b":1,"q'.encode(), b'"')]),
    "object_or_null": (obj({"o": {"type": ["object", "null"], "properties": {"k": INT}, "required": ["k"],
                                  "additionalProperties": False}, "l": arr({"type": ["object", "null"],
                                                                            "properties": {}, "additionalProperties": False})}),
                       [b'{"o":null,"l":[]}', b'{"o":{"k":1},"l":[{},null,{ }]}'],
                       [(b'{"o":{', b"}"), (b'{"o":null,"l":[{', b'"')]),
    "numbers": (obj({"n": arr(NUM)}), [b'{"n":[0,-0,10,-12.5,0.0,1e5,1E5,1e+5,1.25e-7,-0.5E+10]}'],
                [(b'{"n":[0', b"0"), (b'{"n":[1e', b","), (b'{"n":[', b".5"), (b'{"n":[-', b"]"),
                 (b'{"n":[1.5', b"."), (b'{"n":[', b"+1")]),
    "annotated": ({"$schema": "https://json-schema.org/draft/2020-12/schema", "$id": "x", "title": "T",
                   **obj({"a": {"type": "integer", "title": "A", "description": "d", "default": 1, "examples": [1]}},
                         description="root")},
                  [b'{"a":5}'], [(b'{"a":', b'"')]),
    "pydantic_like": ({"$defs": {"Color": {"enum": ["red", "green"], "title": "Color", "type": "string"},
                                 "Item": obj({"name": STR, "color": {"$ref": "#/$defs/Color"},
                                              "qty": {"anyOf": [INT, NULL], "default": None}}, title="Item")},
                       **obj({"items": arr({"$ref": "#/$defs/Item"}), "ok": BOOL}, title="Order")},
                      [b'{"items":[{"name":"n","color":"red","qty":null},{"name":"","color":"green","qty":3}],"ok":true}',
                       b'{"items":[],"ok":false}'],
                      [(b'{"items":[{"name":"n","color":"', b"b"), (b'{"items":[{"name":"n","color":"red","qty":', b'"')]),
}


# ---- the independent validator: the semantics of the subset, stated over json.loads --------------------------------
class Pairs(list):
    """An object's (key, value) pairs in document order, duplicates kept."""


class Num(str):
    """A number's own text (so -0, 1.0 and 1e0 stay apart)."""


def _reject_constant(name):
    raise ValueError(name)


def parse(data: bytes):
    """The parsed document, or None: strict UTF-8, strict JSON, ``{`` first and ``}`` last (no whitespace around)."""
    try:
        text = data.decode("utf-8")
        v = json.loads(text, object_pairs_hook=Pairs, parse_int=Num, parse_float=Num, parse_constant=_reject_constant)
    except (ValueError, RecursionError):
        return None
    return v if isinstance(v, Pairs) and text[:1] == "{" and text[-1:] == "}" else None


def _literal(v, want) -> bool:
    """``v`` is the enum member ``want`` in its canonical spelling."""
    if isinstance(want, bool) or want is None:
        return v is want
    if isinstance(want, int):
        return isinstance(v, Num) and str(v) == str(want)
    return type(v) is str and v == want


def validate(s: dict, v, root: dict) -> bool:
    if "$ref" in s:
        return validate(root["$defs"][s["$ref"].split("/")[-1]], v, root)
    if "anyOf" in s:
        return any(validate(a, v, root) for a in s["anyOf"])
    if "enum" in s or "const" in s:
        return any(_literal(v, w) for w in (s["enum"] if "enum" in s else [s["const"]]))
    for t in s["type"] if isinstance(s["type"], list) else [s["type"]]:
        if t == "string" and type(v) is str or t == "null" and v is None or t == "boolean" and isinstance(v, bool):
            return True
        if t == "integer" and isinstance(v, Num) and re.fullmatch(r"-?\d+", v):
            return True
        if t == "number" and isinstance(v, Num):
            return True
        if t == "array" and isinstance(v, list) and not isinstance(v, Pairs):
            if all(validate(s["items"], x, root) for x in v):
                return True
        if t == "object" and isinstance(v, Pairs):
            props = s.get("properties", {})
            if [k for k, _ in v] == list(props) and all(validate(props[k], x, root) for k, x in v):
                return True
    return False


def conforms(schema: dict, data: bytes) -> bool:
    v = parse(data)
    return v is not None and validate(schema, v, schema)


# ---- generators -----------------------------------------------------------------------------------------------------------
_CHARS = ["a", "Z", "0", " ", "{", "}", "[", ",", ":", "é", "€", "😀", "\x7f", "\\n", '\\"', "\\\\", "\\u00e9", "\\/"]


def gen(s: dict, root: dict, rng: random.Random) -> str:
    """A random conforming document of ``s`` as text, whitespace at random where the grammar allows it."""
    ws = lambda: rng.choice(["", "", "", " ", "\n", " \t"])
    if "$ref" in s:
        return gen(root["$defs"][s["$ref"].split("/")[-1]], root, rng)
    if "anyOf" in s:
        return gen(rng.choice(s["anyOf"]), root, rng)
    if "enum" in s or "const" in s:
        return json.dumps(rng.choice(s["enum"]) if "enum" in s else s["const"], ensure_ascii=False, separators=(",", ":"))
    t = rng.choice(s["type"]) if isinstance(s["type"], list) else s["type"]
    if t == "string":
        return '"' + "".join(rng.choice(_CHARS) for _ in range(rng.randrange(5))) + '"'
    if t == "integer":
        return rng.choice(["0", "-0", "7", "-12", "1234567890123"])
    if t == "number":
        return rng.choice(["0", "-1", "2.5", "1e5", "-0.5E+10", "3E-2", "10.01"])
    if t == "boolean":
        return rng.choice(["true", "false"])
    if t == "null":
        return "null"
    if t == "array":
        return "[" + ws() + ("," + ws()).join(gen(s["items"], root, rng) + ws() for _ in range(rng.randrange(4))) + "]"
    parts = [json.dumps(k, ensure_ascii=False) + ws() + ":" + ws() + gen(sub, root, rng) + ws()
             for k, sub in s.get("properties", {}).items()]
    return "{" + ws() + ("," + ws()).join(parts) + "}"


def distances(dfa) -> np.ndarray:
    """Edges to DONE per state, by a BFS over the reversed automaton (-1: DONE is out of reach)."""
    rev = [[] for _ in range(dfa.S)]
    for s in range(dfa.S):
        for t in set(dfa.trans[s].tolist()) - {js.DEAD}:
            rev[t].append(s)
    dist = np.full(dfa.S, -1, dtype=np.int64)
    dist[js.DONE] = 0
    todo = deque([js.DONE])
    while todo:
        t = todo.popleft()
        for s in rev[t]:
            if dist[s] < 0:
                dist[s] = dist[t] + 1
                todo.append(s)
    return dist


def complete(dfa, dist, s: int) -> bytes:
    """The bytes of a shortest path from state ``s`` to DONE."""
    out = b""
    while s != js.DONE:
        nxt = dfa.trans[s, dfa.cls].astype(np.int64)  # (per byte)
        b = int(np.argmin(np.where(nxt == js.DEAD, 1 << 30, dist[np.minimum(nxt, dfa.S - 1)])))
        assert nxt[b] != js.DEAD and dist[nxt[b]] < dist[s]
        out, s = out + bytes([b]), int(nxt[b])
    return out


def doc_states(dfa, docs) -> list[int]:
    """Every distinct state the documents reach, byte by byte, in order of first appearance."""
    seen = {js.START: None}
    for d in docs:
        s = js.START
        for i in range(len(d)):
            s = ref.schema_walk(s, d[i:i + 1], dfa)
            seen.setdefault(s)
    return list(seen)


@pytest.fixture(scope="module")
def table():
    return synthetic_table(1000)


NAMES = list(SCHEMAS)


# ---- the compiler --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_hand_written_documents(name):
    schema, good, bad = SCHEMAS[name]
    dfa = js.compile_schema(schema)
    assert dfa.cls.dtype == np.uint8 and dfa.cls.shape == (256,) and dfa.trans.dtype == np.uint16
    assert dfa.trans.shape == (dfa.S, dfa.C) and int(dfa.cls.max()) == dfa.C - 1 and (dfa.trans[js.DONE] == js.DEAD).all()
    for d in good:
        assert conforms(schema, d), d  # (the validator agrees the document is one)
        s = js.START
        for i in range(len(d)):
            s = ref.schema_walk(s, d[i:i + 1], dfa)
            assert s != js.DEAD, (d, i)
            assert (s == js.DONE) == (i == len(d) - 1), (d, i)
        assert ref.schema_walk(js.START, d, dfa) == js.DONE
    for prefix, rest in bad:
        s = ref.schema_walk(js.START, prefix, dfa)
        assert s != js.DEAD, (prefix, rest)
        assert ref.schema_walk(s, rest[:1], dfa) == js.DEAD, (prefix, rest)
        assert ref.schema_walk(js.START, prefix + rest, dfa) == js.DEAD and not conforms(schema, prefix + rest)


def test_the_table_covers_the_constructs():
    assert len(SCHEMAS) >= 15
    assert js.compile_schema(SCHEMAS["empty"][0]).trans.shape[0] == 3  # START, DONE and "after {": the smallest table
    assert (js.START, js.DONE, js.DEAD) == (0, 1, 0xFFFF)


@pytest.mark.parametrize("name", NAMES)
def test_random_documents_and_one_byte_mutations(name, table):
    schema = SCHEMAS[name][0]
    dfa = js.compile_schema(schema)
    rng = random.Random(name)
    masks: dict[int, np.ndarray] = {}
    rejected = accepted = stuck = 0
    dist = distances(dfa)
    for _ in range(200):
        doc = gen(schema, schema, rng).encode("utf-8")
        assert conforms(schema, doc), doc
        s = js.START
        for t in tokenize(table, doc):
            if s not in masks:
                masks[s] = unpack(ref.schema_mask_ref(s, dfa, table), table.V)
            assert masks[s][t], (doc, t, table.bytes_of(t))
            s = ref.schema_advance_ref(s, t, dfa, table)
        assert s == js.DONE, doc
        p = rng.randrange(len(doc) + 1)
        b = bytes([rng.randrange(256)])
        mut = doc[:p] + b + (doc[p:] if rng.random() < 0.5 else doc[p + 1:])
        end = ref.schema_walk(js.START, mut, dfa)
        if conforms(schema, mut):
            accepted += 1
            assert end == js.DONE, (doc, mut)
        else:
            rejected += 1
            # DEAD at or before the end — unless the mutation cut the document short (the closing brace became
            # whitespace, say): then the text is a proper prefix of a conforming document, alive and not DONE, and
            # the shortest way on from its state must end in one
            if end != js.DEAD:
                stuck += 1
                assert end != js.DONE and conforms(schema, mut + complete(dfa, dist, end)), (doc, mut)
    assert rejected > 100 and stuck < rejected // 4


@pytest.mark.parametrize("name", NAMES)
def test_random_walks_end_in_conforming_documents(name, table):
    schema = SCHEMAS[name][0]
    dfa = js.compile_schema(schema)
    dist = distances(dfa)
    rng = np.random.default_rng(len(name))
    nxt_cache: dict[int, tuple[np.ndarray, np.ndarray]] = {}
    for _ in range(12):
        s, out = js.START, b""
        for step in range(100000):
            if s == js.DONE:
                break
            if s not in nxt_cache:
                ids = np.flatnonzero(unpack(ref.schema_mask_ref(s, dfa, table), table.V))
                nxt_cache[s] = (ids, np.array([ref.schema_advance_ref(s, int(t), dfa, table) for t in ids]))
            ids, nxt = nxt_cache[s]
            assert ids.size and (nxt != js.DEAD).all()
            j = int(rng.integers(ids.size)) if step < 40 else int(np.argmin(dist[nxt]))
            assert step < 40 or dist[nxt[j]] < dist[s]  # (every single byte is a token: the walk ends)
            out += table.bytes_of(int(ids[j]))
            s = int(nxt[j])
        assert s == js.DONE and conforms(schema, out), out
    done = unpack(ref.schema_mask_ref(js.DONE, dfa, table), table.V)
    assert np.flatnonzero(done).tolist() == sorted(table.eos_ids.tolist())
    assert not ref.schema_mask_ref(js.DEAD, dfa, table).any() and not ref.schema_mask_ref(dfa.S, dfa, table).any()
    assert ref.schema_advance_ref(js.DONE, 0, dfa, table) == js.DONE
    for t in (3, table.V, -1, int(table.eos_ids[0])):  # no bytes, outside the vocabulary, an EOS before the end
        assert ref.schema_advance_ref(js.START, t, dfa, table) == js.DEAD


@pytest.mark.parametrize("name", NAMES)
def test_every_state_reaches_done_and_the_compile_is_deterministic(name):
    schema = SCHEMAS[name][0]
    dfa = js.compile_schema(schema)
    assert (distances(dfa) >= 0).all()
    reach, todo = {js.START}, [js.START]
    while todo:
        for t in set(dfa.trans[todo.pop()].tolist()) - {js.DEAD}:
            if t not in reach:
                reach.add(t)
                todo.append(t)
    assert len(reach) == dfa.S  # nothing unreachable
    js._CACHE.clear()
    again = js.compile_schema(json.loads(json.dumps(schema)))
    assert again is not dfa and again.tobytes() == dfa.tobytes() and again.text == dfa.text == js.canonical_text(schema)
    assert js.compile_schema(schema) is again and js.compile_text(dfa.text) is again  # (the cache)


def test_a_fresh_process_compiles_the_same_bytes():
    code = ("import sys, json, hashlib; sys.path.insert(0, %r); from test_json_schema import SCHEMAS\n"
            "from kafka_llm_service_amd.engine import json_schema as js\n"
            "print(json.dumps({n: hashlib.sha256(js.compile_schema(s[0]).tobytes()).hexdigest() "
            "for n, s in SCHEMAS.items()}))") % __file__.rsplit("/", 1)[0]
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True,
                         env={**__import__("os").environ, "PYTHONHASHSEED": "12345"}).stdout
    here = {n: hashlib.sha256(js.compile_schema(s[0]).tobytes()).hexdigest() for n, s in SCHEMAS.items()}
    assert json.loads(out.strip().splitlines()[-1]) == here


def test_property_order_is_meaning_and_the_cache_is_a_small_lru():
    a, b = obj({"x": INT, "y": INT}), obj({"y": INT, "x": INT})
    assert js.compile_schema(a).text != js.compile_schema(b).text
    assert ref.schema_walk(0, b'{"y":1,"x":2}', js.compile_schema(b)) == js.DONE
    assert ref.schema_walk(0, b'{"y":1,"x":2}', js.compile_schema(a)) == js.DEAD
    first = js.compile_schema(a)
    for i in range(js._CACHE_MAX + 1):
        js.compile_schema(obj({f"k{i}": NULL}))
    assert len(js._CACHE) == js._CACHE_MAX and js.compile_schema(a) is not first


# ---- errors and limits -------------------------------------------------------------------------------------------------------
def _deep(levels: int) -> dict:
    """Objects in objects with an integer at nesting level ``levels`` (the root is level 1)."""
    s = INT
    for _ in range(levels - 1):
        s = obj({"n": s})
    return s


UNSUPPORTED = [
    (obj({"a": {"type": "string", "pattern": "x"}}), "pattern", "#/properties/a/pattern"),
    (obj({"a": {"type": "string", "format": "date"}}), "format", "#/properties/a/format"),
    (obj({"a": {"type": "string", "minLength": 1}}), "minLength", "#/properties/a/minLength"),
    (obj({"a": {"type": "integer", "minimum": 0}}), "minimum", "#/properties/a/minimum"),
    (obj({"a": {"type": "array", "items": INT, "minItems": 1}}), "minItems", "#/properties/a/minItems"),
    (obj({"a": {"oneOf": [INT]}}), "oneOf", "#/properties/a/oneOf"),
    (obj({"a": {"allOf": [INT]}}), "allOf", "#/properties/a/allOf"),
    (obj({"a": {"not": INT}}), "not", "#/properties/a/not"),
    (obj({"a": INT}, patternProperties={}), "patternProperties", "#/patternProperties"),
    (obj({"a": {}}), "type", "#/properties/a"),
    (obj({"a": {"title": "untyped"}}), "type", "#/properties/a"),
    (obj({"a": {"type": "array"}}), "items", "#/properties/a"),
    (obj({"a": {"enum": [1.5]}}), "enum", "#/properties/a/enum/0"),
    (obj({"a": {"const": {"k": 1}}}), "const", "#/properties/a/const"),
    (obj({"a": {"type": "string", "enum": [1]}}), "enum", "#/properties/a/enum/0"),
    (obj({"a": {"type": "float"}}), "type", "#/properties/a/type"),
    ({"type": "object", "properties": {"a": INT}, "required": [], "additionalProperties": False}, "required", "#/required"),
    ({"type": "object", "properties": {"a": INT}, "required": ["a"]}, "additionalProperties", "#/additionalProperties"),
    ({"type": "object", "properties": {"a": INT}, "required": ["a"], "additionalProperties": True},
     "additionalProperties", "#/additionalProperties"),
    (obj({"a": arr(obj({"b": {"type": "string", "maxLength": 3}}))}), "maxLength",
     "#/properties/a/items/properties/b/maxLength"),
    ({"type": "array", "items": INT}, "type", "#/type"),
    ({"$defs": {"A": obj({"b": {"$ref": "#/$defs/B"}}), "B": obj({"a": {"$ref": "#/$defs/A"}})},
      **obj({"r": {"$ref": "#/$defs/A"}})}, "$ref", "#/$defs/B/properties/a/$ref"),
    (obj({"r": {"$ref": "#/$defs/missing"}}), "$ref", "#/properties/r/$ref"),
    (obj({"r": {"$ref": "other.json"}}), "$ref", "#/properties/r/$ref"),
]


@pytest.mark.parametrize("schema,kw,ptr", UNSUPPORTED, ids=[f"{k}@{p}" for _, k, p in UNSUPPORTED])
def test_unsupported_schemas_name_keyword_and_pointer(schema, kw, ptr):
    with pytest.raises(js.SchemaError) as e:
        js.compile_schema(schema)
    assert f"`{kw}`" in str(e.value) and ptr in str(e.value), str(e.value)
    assert isinstance(e.value, ValueError)


def _ab_enum(k: int) -> dict:
    """An enum of k distinct 20-letter strings over two letters: thousands of states, nine byte classes."""
    return obj({"e": {"enum": ["".join("ab"[(i * 2654435761 % (1 << 20) >> j) & 1] for j in range(20))
                               for i in range(k)]}})


def _wide_enum(k: int) -> dict:
    """An enum of k strings over many distinct bytes beside a free string: thousands of states, ~60 classes."""
    rng = random.Random(1)
    abc = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"
    return obj({"s": STR, "e": {"enum": sorted({"".join(rng.choice(abc) for _ in range(10)) for _ in range(k)})}})


def test_limits_each_with_a_schema_just_over():
    pad = lambda n: obj({"a": INT}, description="d" * n)
    base = len(js.canonical_text(pad(0)))
    assert js.compile_schema(pad(js.SCHEMA_MAX_TEXT - base)).S > 0  # exactly 64 KiB of canonical text
    with pytest.raises(js.SchemaError, match="65536 bytes"):
        js.compile_schema(pad(js.SCHEMA_MAX_TEXT - base + 1))
    assert js.compile_schema(_deep(32)).S > 0
    with pytest.raises(js.SchemaError, match="32 levels"):
        js.compile_schema(_deep(33))
    # states: 651 members give exactly 8192 states (nine byte classes keep the table under its own limit)
    last = js.compile_schema(_ab_enum(651))
    assert last.S == js.SCHEMA_MAX_STATES and last.nbytes <= js.SCHEMA_TAB_BYTES
    with pytest.raises(js.SchemaError, match="8192 states"):
        js.compile_schema(_ab_enum(652))
    # table bytes: a wide alphabet beside a free string reaches 256 KiB long before 8192 states
    wide = js.compile_schema(_wide_enum(188))
    assert wide.S < js.SCHEMA_MAX_STATES and js.SCHEMA_TAB_BYTES - 10 * wide.C * 2 <= wide.nbytes <= js.SCHEMA_TAB_BYTES
    with pytest.raises(js.SchemaError, match="262144 bytes"):
        js.compile_schema(_wide_enum(189))
    for bad in (None, [], "x"):
        with pytest.raises(js.SchemaError):
            js.compile_schema(bad)


# ---- ops on the CPU, the wire format, the logits processor ------------------------------------------------------------------
def test_cpu_ops_go_through_the_reference(table):
    tabs = ops.JsonTables(table, "cpu")
    pool = ops.SchemaTables(3, "cpu")
    names = ["scalars", "empty"]
    dfas = [js.compile_schema(SCHEMAS[n][0]) for n in names]
    for buf, d in zip((2, 0), dfas):
        pool.load(buf, d.cls, d.trans)
    assert pool.kinds() == (1, (dfas[0].nbytes + 15) & ~15) and pool.sdim.tolist() == [[3, dfas[1].C], [0, 0], [dfas[0].S, dfas[0].C]]
    sts = doc_states(dfas[0], SCHEMAS["scalars"][1])[:30]
    k, row0 = len(sts), 2
    state = torch.zeros(k + 2, 4, dtype=torch.int32)
    slots = list(range(k + 1, 1, -1))
    for sl, s in zip(slots, sts):
        state[sl] = torch.from_numpy(js.state_record(s, 2))
    state[0] = torch.from_numpy(js.state_record(js.START, 0))
    rows = torch.tensor([[i, sl, 2] for i, sl in enumerate(slots)] + [[k, 0, 0]], dtype=torch.int32)
    mask_tab = torch.full((row0 + k + 3, table.W), 0x5A5A5A5A, dtype=torch.int32)
    ops.schema_mask(tabs, pool, rows, k + 1, state, mask_tab, row0)
    for sl, s in zip(slots, sts):
        assert np.array_equal(mask_tab[row0 + sl].numpy().view(np.uint32), ref.schema_mask_ref(s, dfas[0], table))
    assert np.array_equal(mask_tab[row0].numpy().view(np.uint32), ref.schema_mask_ref(js.START, dfas[1], table))
    assert (mask_tab[:row0] == 0x5A5A5A5A).all() and (mask_tab[row0 + 1] == 0x5A5A5A5A).all()
    t = tokenize(table, b'{"')[0]
    ops.schema_advance(tabs, pool, rows, torch.full((k + 1,), t, dtype=torch.int64), state)
    for sl, s in zip(slots, sts):
        assert state[sl].tolist() == [ref.schema_advance_ref(s, t, dfas[0], table), 0, 0, 3]
    assert state[0].tolist() == [ref.schema_advance_ref(js.START, t, dfas[1], table), 0, 0, 1]
    for bad in ([[0, k + 2, 2]], [[k + 1, 2, 2]], [[0, 2, 1]], [[0, 2, 3]]):  # slot, sampled row, unloaded / no table
        with pytest.raises(ValueError):
            ops.schema_mask(tabs, pool, torch.tensor(bad, dtype=torch.int32), k + 1, state, mask_tab, row0)
    broken = dfas[0].trans.copy()
    broken[5, 0] = dfas[0].S
    with pytest.raises(ValueError):
        pool.load(1, dfas[0].cls, broken)
    with pytest.raises(ValueError):
        pool.load(3, dfas[0].cls, dfas[0].trans)


def _step(n=4):
    h = HostStep(B=n, T=n, n_rows=n)
    h.i64 = np.arange(4 * n, dtype=np.int64)
    h.i32 = np.arange(1 + n, dtype=np.int32)
    proc = np.zeros((n, 8), np.int32)
    proc[:, 2] = -1
    return h, proc, (np.full(n, 0.7, np.float32), np.ones(n, np.float32), np.zeros(n, np.int32),
                     np.arange(n, dtype=np.int64))


def test_wire_round_trip_and_unchanged_bytes_without_schema_rows():
    h, proc, arrays = _step()
    proc[[1, 3], 0], proc[[1, 3], 1] = 1, [512 + 7, 512 + 2]
    d1, d2 = js.compile_schema(SCHEMAS["scalars"][0]), js.compile_schema(SCHEMAS["empty"][0])
    assert (d2.S * d2.C) % 2 == 0 and (d1.S * d1.C) % 2 in (0, 1)
    odd = js.SchemaDfa(d2.cls.copy(), d2.trans[:, :3].copy(), "")  # (an odd number of entries: the padding word)
    upd = ProcUpdates(json_slots=np.array([7], np.int32), json_states=js.state_record(5, 4)[None],
                      schema_tabs=[(4, d1.cls, d1.trans), (0, odd.cls, odd.trans)])
    srows = np.array([[1, 7, 4], [3, 2, 0]], np.int32)
    sp = SampleParams(*arrays, proc, False, upd, schema_rows=srows)
    hdr, payload = step_plan.pack_plan(h, sp)
    assert hdr.size == step_plan.PLAN_HDR == 32 and hdr[31] > 0 and payload.size < 4 << 20
    _, sp2 = step_plan.unpack_plan(hdr, payload)
    assert np.array_equal(sp2.schema_rows, srows) and sp2.schema_rows.dtype == np.int32 and sp2.json_rows is None
    assert sp2.upd.json_states.tolist() == [[5, 0, 0, 5]] and len(sp2.upd.schema_tabs) == 2
    for (i, c, t), (i2, c2, t2) in zip(upd.schema_tabs, sp2.upd.schema_tabs):
        assert i == i2 and np.array_equal(c, c2) and np.array_equal(t, t2) and t2.dtype == np.uint16
    # the largest table fits the 4 MiB plan slot
    big = np.zeros((js.SCHEMA_TAB_BYTES // 2 // 16, 16), np.uint16)
    sp_big = SampleParams(*arrays, proc, False, ProcUpdates(schema_tabs=[(1, d1.cls, big)]), schema_rows=srows)
    assert step_plan.pack_plan(h, sp_big)[1].size < 4 << 20
    # a table without rows, rows without a table
    for u, r in ((ProcUpdates(schema_tabs=[(4, d1.cls, d1.trans)]), None), (None, srows)):
        _, sp3 = step_plan.unpack_plan(*step_plan.pack_plan(h, SampleParams(*arrays, proc, False, u, schema_rows=r)))
        assert (sp3.schema_rows is None) == (r is None) and (sp3.upd is None) == (u is None)
    # a step without either: header word 31 is 0 and the payload is what it is with the new fields left at their defaults
    jrows = np.array([[1, 7], [3, 2]], np.int32)
    old_upd = ProcUpdates(json_slots=np.array([7], np.int32), json_states=np.array([[6, 1, 1, 0]], np.int32))
    with_fields = SampleParams(*arrays, proc, False, ProcUpdates(json_slots=old_upd.json_slots,
                                                                json_states=old_upd.json_states, schema_tabs=[]),
                               json_rows=jrows, schema_rows=None)
    defaulted = SampleParams(*arrays, proc, False, old_upd, json_rows=jrows)
    (h1, p1), (h0, p0) = step_plan.pack_plan(h, with_fields), step_plan.pack_plan(h, defaulted)
    assert h1[31] == 0 and np.array_equal(h1, h0) and p1.tobytes() == p0.tobytes()
    assert p1.size == step_plan.pack_plan(h, sp)[1].size - 4 * int(hdr[31]) + 4 * 2 * 2  # (sp carries no JSON rows)
    with pytest.raises(ValueError):
        step_plan.pack_plan(h, SampleParams(*arrays, proc, False, None, schema_rows=np.zeros((1, 2), np.int32)))


def _seq(name, schema=None, **kw):
    text = js.canonical_text(schema) if schema is not None else None
    return Sequence(name, [1], SamplingParams(json_schema=text, **kw))


def test_sampling_params():
    text = js.canonical_text(SCHEMAS["scalars"][0])
    p = SamplingParams(json_schema=text, temperature=0.5)
    assert SamplingParams().json_schema is None and SamplingParams(**dict(p.__dict__)) == p
    for bad in (dict(json_schema=text, json_mode=True), dict(json_schema=text, tool_grammar={"tools": []}),
                dict(json_schema=text, allowed_tokens_fn=lambda ids: None), dict(json_schema={"type": "object"}),
                dict(json_schema='{"type":"array","items":{}}'), dict(json_schema="{")):
        with pytest.raises(ValueError):
            SamplingParams(**bad)


def test_logits_processor_tables_slots_and_reseeding(table):
    A, B, C = (SCHEMAS[n][0] for n in ("scalars", "enum_prefix", "nullable"))
    lp = LogitsProcessor("cpu", table.V, max_slots=4, mask_rows=8, json_slots=2)
    lp.set_json_table(table)
    assert lp.spool is None
    a, b = _seq("a", A), Sequence("b", [1], SamplingParams(json_mode=True))
    proc, upd = lp.build([(0, a, None), (1, b, None)], 3, n_decode=0)
    assert lp.spool is None and len(upd.schema_tabs) == 1  # (the pool is allocated when a table is applied)
    buf, cls, trans = upd.schema_tabs[0]
    dfa = js.compile_schema(A)
    assert np.array_equal(trans, dfa.trans) and np.array_equal(cls, dfa.cls)
    # JSON-mode and schema sequences share the slot pool and tell their rows apart
    sa, sb = int(proc[0, 1]) - 8, int(proc[1, 1]) - 8
    assert {sa, sb} == {0, 1} and lp.schema_rows(proc).tolist() == [[0, sa, buf]] and lp.json_rows(proc).tolist() == [[1, sb]]
    recs = dict(zip(upd.json_slots.tolist(), upd.json_states.tolist()))
    assert recs[sa] == [js.START, 0, 0, buf + 1] and recs[sb][3] == 0
    lp.apply(upd, torch.from_numpy)
    assert lp.spool is not None and lp.spool.strans.shape == (2, js.SCHEMA_TAB_BYTES // 2)
    assert lp.stats["schema_table_uploads"] == 1 and lp.stats["schema_seeds"] == 1 and lp.stats["schema_rows"] == 1
    # decode steps seed nothing; the state moves through the ops alone
    tabs, doc = lp.json_tables(), tokenize(table, b'{"s":"x\\u00e9","i":-1')
    rows = torch.from_numpy(lp.schema_rows(proc))
    for t in doc:
        a.output_ids.append(t)
        proc2, upd2 = lp.build([(0, a, None), (1, b, None)], 2, n_decode=2)
        assert upd2.empty and np.array_equal(proc2[:, :2], proc[:2, :2])
        ops.schema_mask(tabs, lp.schema_pool(), rows, 2, lp.jstate, lp.tables()[0], lp.n_mask_rows)
        assert unpack(lp.tables()[0][8 + sa].numpy().view(np.uint32), table.V)[t]
        ops.schema_advance(tabs, lp.schema_pool(), rows, torch.tensor([t, 0]), lp.jstate)
    walked = ref.schema_walk(js.START, b'{"s":"x\\u00e9","i":-1', dfa)
    assert lp.jstate[sa].tolist() == [walked, 0, 0, buf + 1] and walked not in (js.DEAD, js.DONE)
    # a preemption: the re-prefill seeds the state after the landed ids, over the same resident table
    lp.jstate[sa] = 0
    proc3, upd3 = lp.build([(0, b, None), (1, a, None)], 2, n_decode=1)
    assert upd3.json_slots.tolist() == [sa] and upd3.json_states.tolist() == [[walked, 0, 0, buf + 1]]
    assert not upd3.schema_tabs and lp.stats["schema_seeds"] == 2
    lp.apply(upd3, torch.from_numpy)
    assert lp.jstate[sa].tolist() == [walked, 0, 0, buf + 1]
    # the same schema in a later turn reuses the resident table; finished sequences give slots and references back
    a.status = b.status = SeqStatus.FINISHED
    assert a.finished and b.finished
    a2, c = _seq("a2", A), _seq("c", B)
    proc4, upd4 = lp.build([(0, a2, None), (1, c, None)], 2, n_decode=0)
    assert [t[0] for t in upd4.schema_tabs] == [1 - buf] and lp.stats["schema_table_uploads"] == 2
    assert sorted(lp.schema_rows(proc4)[:, 2].tolist()) == [0, 1] and lp.json_rows(proc4) is None
    lp.apply(upd4, torch.from_numpy)
    # LRU: both buffers hold unreferenced tables once a2 and c finish; a third schema takes the least recently used
    a2.status = c.status = a.status
    d = _seq("d", C)
    _, upd5 = lp.build([(0, d, None)], 1, n_decode=0)
    assert [t[0] for t in upd5.schema_tabs] == [buf] and list(lp._stabs) == [js.canonical_text(B), js.canonical_text(C)]
    lp.apply(upd5, torch.from_numpy)
    e = _seq("e", B)  # B is still resident: no upload
    _, upd6 = lp.build([(0, e, None)], 1, n_decode=0)
    assert not upd6.schema_tabs and lp.stats["schema_table_uploads"] == 3
    with pytest.raises(RuntimeError):  # two live sequences hold both slots
        lp.build([(0, _seq("f", A), None)], 1, n_decode=0)
    with pytest.raises(ValueError):
        lp.build([(0, d, [1, 2])], 1)
    bad = ProcUpdates(json_slots=np.array([0], np.int32), json_states=np.array([[js.SCHEMA_MAX_STATES, 0, 0, 1]], np.int32))
    with pytest.raises(ValueError):
        lp.apply(bad, torch.from_numpy)


# ---- the API ---------------------------------------------------------------------------------------------------------------
def _fmt(schema, **extra):
    return {"type": "json_schema", "json_schema": dict({"schema": schema}, **extra)}


def test_request_schema_and_422():
    A = SCHEMAS["pydantic_like"][0]
    ok = ChatCompletionRequest(model="m", messages=MSG, response_format=_fmt(A, name="order_v1", strict=False,
                                                                            description="an order"))
    assert ok.json_schema == A and not ok.json_mode
    assert _sampling_kwargs(ok)["response_format"] == _fmt(A, name="order_v1", strict=False, description="an order")
    assert ChatCompletionRequest(model="m", messages=MSG, response_format={"type": "json_object"}).json_schema is None
    for legacy in ({"type": "json_schema", "json_schema": {}}, {"type": "json_schema", "json_schema": {"name": "x"}},
                   {"type": "json_schema"}):
        with pytest.raises(ValidationError, match="json_object"):
            ChatCompletionRequest(model="m", messages=MSG, response_format=legacy)
    for name in ("", "a b", "x" * 65, 5, "é"):
        with pytest.raises(ValidationError, match="name"):
            ChatCompletionRequest(model="m", messages=MSG, response_format=_fmt(A, name=name))
    for schema, kw, ptr in UNSUPPORTED[:6] + UNSUPPORTED[-3:]:
        with pytest.raises(ValidationError) as e:
            ChatCompletionRequest(model="m", messages=MSG, response_format=_fmt(schema))
        assert kw in str(e.value) and ptr in str(e.value)
    for over, word in ((_deep(33), "32 levels"), (obj({"a": INT}, description="d" * 70000), "65536 bytes")):
        with pytest.raises(ValidationError, match=word):
            ChatCompletionRequest(model="m", messages=MSG, response_format=_fmt(over))
    tools = [{"type": "function", "function": {"name": "f", "parameters": {}}}]
    for tc in ({}, {"tool_choice": "auto"}):
        with pytest.raises(ValidationError, match="tools"):
            ChatCompletionRequest(model="m", messages=MSG, response_format=_fmt(A), tools=tools, **tc)
    assert ChatCompletionRequest(model="m", messages=MSG, response_format=_fmt(A), tools=tools,
                                 tool_choice="none").json_schema == A


def test_chat_routes_forward_the_schema_and_answer_422():
    prov = _Recording([{"text": '{"e":"ab"}'}] * 4)
    st = ServerState(ServerConfig(backend="stub", sandbox="none"), llm_provider=prov, db=MemoryDBClient())
    E = SCHEMAS["enum_prefix"][0]
    with TestClient(create_app(state=st)) as c:
        body = {"model": "kafka", "messages": MSG}
        tid = c.post("/v1/threads", json={}).json()["thread_id"]
        for url in ("/v1/chat/completions", f"/v1/threads/{tid}/chat/completions"):
            r = c.post(url, json=dict(body, response_format=_fmt(E, name="e")))
            assert r.status_code == 200 and prov.kwargs[-1]["response_format"] == _fmt(E, name="e")
            assert list(prov.kwargs[-1]["response_format"]["json_schema"]["schema"]["properties"]) == ["e"]
            for legacy in ({}, {"name": "x"}):
                r = c.post(url, json=dict(body, response_format={"type": "json_schema", "json_schema": legacy}))
                assert r.status_code == 422 and "json_object" in r.text
            r = c.post(url, json=dict(body, response_format=_fmt(obj({"a": {"type": "string", "pattern": "x"}}))))
            assert r.status_code == 422 and "pattern" in r.text and "#/properties/a/pattern" in r.text
            tools = [{"type": "function", "function": {"name": "f", "parameters": {}}}]
            assert c.post(url, json=dict(body, response_format=_fmt(E), tools=tools)).status_code == 422
        assert c.post("/v1/chat/completions", json=dict(body, response_format=_fmt(E), stream=True)).status_code == 200


def test_remote_provider_forwards_the_schema():
    from kafka_llm_service_amd.llm.remote import RemoteOpenAIProvider

    p = RemoteOpenAIProvider.__new__(RemoteOpenAIProvider)
    p.model, p.default_max_tokens = "m", 16
    f = _fmt(SCHEMAS["nullable"][0], name="n")
    assert p._body([], None, None, None, None, {"response_format": f})["response_format"] == f


# ---- end to end: the chat route streams a schema request through the real engine (CPU) ---------------------------------
def test_chat_route_streams_a_conforming_document_from_the_engine():
    """What a ``curl`` against ``/v1/chat/completions`` with ``stream: true`` sees: the engine provider on a tiny model,
    a finite-language schema, whitespace-only tokens biased away so the random-init model cannot idle; the streamed
    content validates and the last choice says "stop"."""
    from kafka_llm_service_amd.engine import json_mode as jm
    from kafka_llm_service_amd.engine.tokenizer import get_tokenizer

    tok = get_tokenizer()
    table = jm.table_for(tok, tok.eos_ids)
    ws = [i for i in range(table.V) if table.lens[i] and not table.bytes_of(i).strip(b" \t\n\r")]
    assert 0 < len(ws) <= 300
    schema = obj({"ok": BOOL})
    st = ServerState(ServerConfig(backend="engine", model="tiny-llama", sandbox="none", max_model_len=8192,
                                  default_max_tokens=12, prompt_sections=["intro"], warm_prefix=False,
                                  engine_kwargs={"device": "cpu", "num_kv_blocks": 1024}), db=MemoryDBClient())
    body = {"model": "tiny-llama", "messages": MSG, "temperature": 0, "max_tokens": 40, "seed": 7,
            "logit_bias": {str(i): -100 for i in ws}, "response_format": _fmt(schema, name="ok"), "stream": True}
    with TestClient(create_app(state=st)) as c:
        r = c.post("/v1/chat/completions", json=body)
        assert r.status_code == 200, r.text
        frames = [json.loads(b[6:]) for b in r.text.split("\n\n") if b.startswith("data: ") and b[6:] != "[DONE]"]
        text = "".join(f["choices"][0]["delta"].get("content") or "" for f in frames if f.get("choices"))
        reasons = [f["choices"][0].get("finish_reason") for f in frames if f.get("choices")]
        assert conforms(schema, text.encode()), text
        assert reasons[-1] == "stop" and r.text.rstrip().endswith("data: [DONE]")
