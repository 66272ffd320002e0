"""The opt-in automaton tool grammar (``tool_grammar["mode"] == "automaton"``): a tool call's body as one byte-level
automaton over the tools' own schemas, walked on the device (ops/csrc/table_grammar.hip), inside an envelope of two
special tokens that have no bytes.

The generator-based constraint (engine/constrained.py) stays the default. It bounds a string to 12 tokens, a number to
one digit token and an array to one item, and its state lives on the host; this module compiles the same call shape

    llama3:  <|python_tag|> {"name":"<tool>","parameters":<object>} <|eom_id|>
    mistral: [TOOL_CALLS] [{"name":"<tool>","arguments":<object>}] </s>

with engine/json_schema.py's NFA, builder and determiniser into a ``SchemaDfa`` whose table lives in the schema pool,
so strings, numbers and arrays are the schema's own and the row's state is a record on the device.

``strictify`` maps a tool's ``parameters`` into the subset json_schema compiles:

* an object keeps the properties its ``required`` names, in the order ``required`` lists them (what the generator
  emits), and gets ``additionalProperties: false``;
* an array keeps its ``items`` (a string where it has none);
* ``type`` lists and ``anyOf`` stay unions, ``$ref`` and the root ``$defs`` stay, ``enum`` / ``const`` stay (an empty
  ``enum`` is dropped);
* every keyword outside the subset is dropped (``minimum``, ``maximum``, ``pattern``, ``format``, ``minLength``,
  ``minItems``, ...); the annotations json_schema ignores (``title``, ``description``, ...) stay;
* a schema without ``type``, ``enum``, ``const``, ``anyOf`` or ``$ref``, or with a type json_schema does not know,
  becomes ``{"type": "string"}``.
A schema already in the subset comes back equal.

The body is compact — no insignificant whitespace, the ``json.dumps(..., separators=(",", ":"))`` shape — and its
strings take bytes from 0x80 up one by one: byte-level BPE tokens split UTF-8 sequences and the generator admits such
tokens, so well-formedness of UTF-8 is left to the model as it is today. For tools whose schemas use ``type``,
``enum``, ``properties`` and ``items`` only, every token sequence the generator allows is in this language.

The envelope is the record ``(state, phase, 0, table + 1)`` of the row's slot in ``jstate``; ``ops/reference.py``
(``tool_mask_ref`` / ``tool_advance_ref``) defines the phases' masks and moves.
"""
from __future__ import annotations

import json
from collections import OrderedDict
from dataclasses import dataclass

import numpy as np

from kafka_llm_service_amd.engine import json_schema as js

TOOL_FREE, TOOL_OPEN, TOOL_BODY, TOOL_TEXT, TOOL_CLOSED = 0, 1, 2, 3, 4  # (kafka_abi.h)
TOOL_PHASES = 5
MODES = ("program", "automaton")

_KEEP = ("type", "enum", "const") + js._IGNORED


def strictify(parameters) -> dict:
    """``parameters`` of a tool in json_schema's subset (the module's rule); idempotent."""
    if not isinstance(parameters, dict):
        return {"type": "string"}
    out = _strict(parameters)
    defs = parameters.get("$defs")
    if isinstance(defs, dict):
        out["$defs"] = {k: _strict(v) for k, v in defs.items()}
    return out


def _strict(sch) -> dict:
    if not isinstance(sch, dict):
        return {"type": "string"}
    notes = {k: sch[k] for k in js._IGNORED if k in sch}
    if "$ref" in sch:
        return {**notes, "$ref": sch["$ref"]}
    if isinstance(sch.get("anyOf"), list) and sch["anyOf"]:
        return {**notes, "anyOf": [_strict(a) for a in sch["anyOf"]]}
    enum = sch.get("enum")
    if (isinstance(enum, list) and enum) or "const" in sch:
        out = {k: sch[k] for k in sch if k in _KEEP and not (k == "enum" and not enum)}
        if "enum" in out and "const" in out:
            del out["const"]
        return out
    t = sch.get("type")
    types = t if isinstance(t, list) else [t]
    types = [x for x in types if isinstance(x, str) and x in js._TYPES]
    types = list(dict.fromkeys(types))
    if not types:
        return {**notes, "type": "string"}
    res = {**notes, "type": types if isinstance(t, list) and len(types) > 1 else types[0]}
    if "object" in types:
        props = sch.get("properties") if isinstance(sch.get("properties"), dict) else {}
        req = sch.get("required") if isinstance(sch.get("required"), list) else []
        req = list(dict.fromkeys(k for k in req if isinstance(k, str) and k in props))
        res["properties"] = {k: _strict(props[k]) for k in req}
        res["required"] = req
        res["additionalProperties"] = False
    if "array" in types:
        res["items"] = _strict(sch["items"]) if isinstance(sch.get("items"), dict) else {"type": "string"}
    return res


def tool_table(tools: list[dict]) -> dict:
    """name -> ``parameters`` of the function tools of an OpenAI ``tools`` list (as ToolCallConstraint reads it)."""
    return {t["function"]["name"]: t["function"].get("parameters") or {} for t in tools
            if t.get("type", "function") == "function" and "function" in t}


def _frame(family: str) -> tuple[bytes, bytes, bytes]:
    if family == "llama3":
        return b'{"name":"', b'","parameters":', b"}"
    return b'[{"name":"', b'","arguments":', b"}]"


def _build(schemas: list[tuple[str, dict]], family: str) -> tuple[np.ndarray, np.ndarray]:
    head, mid, tail = _frame(family)
    nfa = js._Nfa(compact=True, utf8=False)
    start, accept, named = nfa.new(), nfa.new(), nfa.new()
    nfa.lit(start, head, named)
    for name, sch in schemas:
        bld = js._Builder(sch, nfa)
        v_in, v_out = nfa.new(), nfa.new()
        nfa.lit(named, name.encode("utf-8") + mid, v_in)
        try:
            bld.value(sch, "#", v_in, v_out, 1)
        except js.SchemaError as e:
            raise ValueError(f"tool {name!r}: {e}") from None
        except RecursionError:
            raise ValueError(f"tool {name!r}: schema: nesting exceeds the limit of {js.SCHEMA_MAX_NESTING} "
                             f"levels") from None
        nfa.lit(v_out, tail, accept)
    return js._determinise(nfa, start, accept)


_CACHE: OrderedDict = OrderedDict()
_CACHE_MAX = 64


def body_text(schemas: list[tuple[str, dict]], family: str) -> str:
    """The canonical text a compiled body is cached and keyed by: family, the admitted names in order, their strict
    schemas."""
    return json.dumps({"family": family, "tools": [[n, s] for n, s in schemas]}, sort_keys=False,
                      separators=(",", ":"))


def compile_tool_body(tools, names: list[str], family: str) -> js.SchemaDfa:
    """The automaton of one call body over the tools ``names`` admits (``tools``: an OpenAI ``tools`` list, or a dict
    name -> parameters). ``ValueError`` naming the tool for a schema outside what ``strictify`` can mend (an ``enum``
    of objects, an unknown ``$ref``) and for json_schema's limits (8,192 states, 256 KiB)."""
    table = tools if isinstance(tools, dict) else tool_table(tools)
    if family not in ("llama3", "mistral"):
        raise ValueError(f"tool grammar: unknown tokenizer family {family!r}")
    if not names:
        raise ValueError("tool grammar: no tool to call")
    schemas = []
    for n in names:
        if n not in table:
            raise ValueError(f"tool grammar: unknown tool {n!r}")
        if not isinstance(n, str) or not n or any(ord(c) < 0x20 or c in '"\\' for c in n):
            raise ValueError(f"tool {n!r}: the name needs JSON escapes")
        schemas.append((n, strictify(table[n] or {"type": "object"})))
    text = body_text(schemas, family)
    hit = _CACHE.get(text)
    if hit is not None:
        _CACHE.move_to_end(text)
        return hit
    if len(text.encode("utf-8")) > js.SCHEMA_MAX_TEXT * max(1, len(schemas)):
        raise ValueError(f"tool {names[0]!r}: schema: the canonical text exceeds the limit of {js.SCHEMA_MAX_TEXT} "
                         f"bytes")
    try:
        cls, trans = _build(schemas, family)
    except js.SchemaError as e:  # a limit of the whole alternation: name the first tool that breaks it alone
        who = None
        if len(schemas) > 1:
            for one in schemas:
                try:
                    _build([one], family)
                except ValueError:
                    who = one[0]
                    break
        who = repr(who or schemas[0][0]) if who or len(schemas) == 1 else \
            ", ".join(repr(n) for n, _ in schemas) + " together"
        raise ValueError(f"tool {who}: {e}") from None
    dfa = js.SchemaDfa(cls, trans, text)
    _CACHE[text] = dfa
    while len(_CACHE) > _CACHE_MAX:
        _CACHE.popitem(last=False)
    return dfa


def tool_record(state: int, phase: int, table: int) -> np.ndarray:
    """A tool row's int32 [4] record of the device state table: (state, phase, 0, table index + 1)."""
    if not (0 <= state < js.SCHEMA_MAX_STATES or state == js.DEAD) or not 0 <= phase < TOOL_PHASES or table < 0:
        raise ValueError(f"not a tool automaton record: state {state}, phase {phase}, table {table}")
    return np.array([state, phase, 0, table + 1], dtype=np.int32)


@dataclass(frozen=True)
class ToolPlan:
    """What the engine needs of an automaton tool request: the body, the envelope's tokens, the phase a fresh row
    starts in, and the pool key of the table (a tuple: it cannot equal a schema's text)."""
    dfa: js.SchemaDfa
    open: int
    close: int
    phase0: int

    @property
    def key(self) -> tuple:
        return ("tool", self.dfa.text)

    @property
    def auto(self) -> bool:
        return self.phase0 == TOOL_FREE


def tool_row_live(plan: ToolPlan, output_ids: list[int]) -> bool:
    """Is the sequence still a tool row? Under ``auto``, once the first output id has landed and opens no call, the
    row is free text for good (its device record says TOOL_TEXT) and the host stops listing it."""
    return not (plan.auto and output_ids and output_ids[0] >= 0 and output_ids[0] != plan.open)


def grammar_mode(grammar: dict | None, default: str = "program") -> str:
    """The mode of a ``tool_grammar`` dict: its ``"mode"`` key, else ``default``."""
    mode = (grammar or {}).get("mode") or default or "program"
    if mode not in MODES:
        raise ValueError(f"tool grammar mode must be one of {', '.join(MODES)}, not {mode!r}")
    return mode


def plan_for(tok, tools: list[dict], tool_choice) -> ToolPlan | None:
    """The plan of a request, or None for ``tool_choice: "none"`` (one static host mask row: nothing to gain).
    ``open`` / ``close`` and the admitted names are ToolCallConstraint's."""
    from kafka_llm_service_amd.engine.constrained import ToolCallConstraint

    c = ToolCallConstraint(tok, tools, tool_choice)
    if c.mode == "none":
        return None
    dfa = compile_tool_body(c.tools, c.names, "llama3" if c.llama else "mistral")
    V = tok.vocab_size
    if not (0 <= c.start < V and 0 <= c.end < V):
        raise ValueError("tool grammar: the envelope's tokens lie outside the vocabulary")
    return ToolPlan(dfa, int(c.start), int(c.end), TOOL_FREE if c.mode == "auto" else TOOL_OPEN)
