"""Structured outputs (``response_format: {"type": "json_schema", ...}``): a compiler from a JSON Schema to a byte-level
deterministic automaton without a stack.

A non-recursive schema of the supported subset is a regular language, so one transition table does what JSON mode
(engine/json_mode.py) needs a table and a stack for. ``compile_schema`` works in three steps:

1. *Validate* the subset and raise ``SchemaError`` naming the keyword and its JSON pointer. Supported: a root of
   ``type: "object"``; objects whose ``properties`` are emitted in declared order, all of them ``required``, with
   ``additionalProperties: false``; ``string`` (JSON mode's string rules: every escape, ``\\uXXXX``, well-formed UTF-8,
   no raw control bytes), ``integer`` (``-?(0|[1-9][0-9]*)``), ``number`` (JSON mode's grammar), ``boolean``, ``null``;
   ``array`` with one ``items`` schema and any length; ``enum`` / ``const`` over strings, integers, booleans and null
   (each alternative is the bytes of ``json.dumps(v, ensure_ascii=False, separators=(",", ":"))``); ``type`` as a list
   and ``anyOf`` (unions); ``$ref: "#/$defs/NAME"`` expanded in place. ``title``, ``description``, ``default``,
   ``examples``, ``$schema`` and ``$id`` are ignored; every other keyword is refused. A property name is matched as
   the bytes ``json.dumps`` writes for it, no other spelling of the same string.
2. *Build* a byte-level NFA with ε-edges the way JSON mode's table is written: whitespace wherever RFC 8259 allows it
   inside the document (none before the opening ``{``, none after the closing ``}``), a number ends at the byte that may
   follow a value (its final states have an ε-edge to whatever follows), unions and enums are plain alternation.
3. *Determinise* by the subset construction over byte classes: two bytes share a class iff no NFA edge tells them
   apart, so a state has a few dozen columns instead of 256.

The result (``SchemaDfa``): ``cls`` uint8 [256] byte -> class, ``trans`` uint16 [S, C] next state with the fixed ids
``START = 0``, ``DONE = 1`` and ``DEAD = 0xFFFF``. DONE has no outgoing edge, and every state other than DEAD can reach
DONE (every NFA state lies on a path to the accepting one, so every subset does). States are numbered in order of
discovery and classes by their first byte, so equal schema texts give equal bytes in every process: TP ranks rely on
it. ``ops/reference.py`` (``schema_walk`` / ``schema_mask_ref`` / ``schema_advance_ref``) defines the walk;
``ops/csrc/table_grammar.hip`` agrees with it bit for bit.

Limits (each a ``SchemaError`` that states the limit): canonical text <= 64 KiB, nesting <= 32 after ``$ref``
expansion (the root is level 1; every ``properties`` / ``items`` / ``anyOf`` descent adds one), at most
``SCHEMA_MAX_STATES`` states and ``S * C * 2 <= SCHEMA_TAB_BYTES``.
"""
from __future__ import annotations

import json
import re
from collections import OrderedDict

import numpy as np

SCHEMA_MAX_STATES = 8192         # states of one compiled automaton (kafka_abi.h)
SCHEMA_TAB_BYTES = 256 * 1024    # bytes of one transition table, S * C * 2 (kafka_abi.h)
SCHEMA_LDS_BYTES = 20 * 1024 - 256  # a table up to this size is staged in LDS by the mask kernel (kafka_abi.h)
SCHEMA_MAX_TEXT = 64 * 1024      # bytes of the canonical schema text
SCHEMA_MAX_NESTING = 32
START, DONE, DEAD = 0, 1, 0xFFFF

_IGNORED = ("title", "description", "default", "examples", "$schema", "$id")
_TYPES = ("object", "array", "string", "integer", "number", "boolean", "null")
_NAME = re.compile(r"[A-Za-z0-9_-]{1,64}\Z")
# NFA states before the subset step is even tried. 64 KiB of schema text without $ref builds fewer (a state costs at
# least a byte of text), so only a schema that multiplies through $ref stops here — after a few tens of milliseconds,
# which matters because the chat route compiles inside request validation
_NFA_MAX = 8 * SCHEMA_MAX_STATES

_WS = b" \t\n\r"
_DIGITS = b"0123456789"
_HEX = b"0123456789abcdefABCDEF"


class SchemaError(ValueError):
    """A schema outside the supported subset or over a limit; the message names the keyword and its JSON pointer."""


def _mask(bs) -> int:
    m = 0
    for b in bs:
        m |= 1 << b
    return m


_M_WS, _M_DIGITS, _M_19, _M_HEX = _mask(_WS), _mask(_DIGITS), _mask(b"123456789"), _mask(_HEX)
_M_PLAIN = _mask(b for b in range(0x20, 0x80) if b not in b'"\\')
_M_CONT = _mask(range(0x80, 0xC0))


def canonical_text(schema: dict) -> str:
    """The text a compiled schema is cached and shipped by. Property order is meaning: keys are not sorted."""
    return json.dumps(schema, sort_keys=False, separators=(",", ":"))


def check_name(name) -> None:
    if not isinstance(name, str) or not _NAME.match(name):
        raise SchemaError("json_schema.name must match [A-Za-z0-9_-]{1,64}")


class _Nfa:
    """States are integers; ``edges[s]`` is a list of (byte-set as a 256-bit int, target), ``eps[s]`` of targets."""

    def __init__(self, compact: bool = False, utf8: bool = True):
        self.edges: list[list[tuple[int, int]]] = []
        self.eps: list[list[int]] = []
        # engine/tool_automaton.py: ``compact`` leaves out every whitespace loop (the json.dumps(separators=(",", ":"))
        # shape); without ``utf8`` a string takes the bytes from 0x80 up one by one (byte-level BPE tokens split UTF-8
        # sequences). The defaults build the tables of response_format json_schema
        self.compact, self.utf8 = compact, utf8

    def new(self) -> int:
        if len(self.edges) >= _NFA_MAX:
            raise SchemaError(f"schema: the compiled automaton exceeds the limit of {SCHEMA_MAX_STATES} states")
        self.edges.append([])
        self.eps.append([])
        return len(self.edges) - 1

    def edge(self, a: int, m: int, b: int) -> None:
        self.edges[a].append((m, b))

    def ws(self, a: int) -> int:
        if not self.compact:
            self.edges[a].append((_M_WS, a))
        return a

    def lit(self, a: int, data: bytes, b: int) -> None:
        """``data`` (at least one byte) from a to b."""
        for i, c in enumerate(data):
            nxt = b if i == len(data) - 1 else self.new()
            self.edges[a].append((1 << c, nxt))
            a = nxt

    def string(self, a: int, b: int) -> None:
        """JSON mode's string (engine/json_mode.py, the V_* states) from the opening quote at a to b."""
        if not self.utf8:
            return self._byte_string(a, b)
        n = self.new
        st, esc, u1, u2, u3, u4 = n(), n(), n(), n(), n(), n()
        c1, c2, c3, e0, ed, f0, f4 = n(), n(), n(), n(), n(), n(), n()
        e = self.edge
        e(a, 1 << 0x22, st)
        e(st, _M_PLAIN, st)
        e(st, 1 << 0x22, b)
        e(st, 1 << 0x5C, esc)
        e(esc, _mask(b'"\\/bfnrt'), st)
        e(esc, 1 << 0x75, u1)
        for x, y in ((u1, u2), (u2, u3), (u3, u4), (u4, st)):
            e(x, _M_HEX, y)
        e(st, _mask(range(0xC2, 0xE0)), c1)
        e(st, 1 << 0xE0, e0)
        e(st, _mask(x for x in range(0xE1, 0xF0) if x != 0xED), c2)
        e(st, 1 << 0xED, ed)
        e(st, 1 << 0xF0, f0)
        e(st, _mask(range(0xF1, 0xF4)), c3)
        e(st, 1 << 0xF4, f4)
        e(c1, _M_CONT, st)
        e(c2, _M_CONT, c1)
        e(c3, _M_CONT, c2)
        e(e0, _mask(range(0xA0, 0xC0)), c1)
        e(ed, _mask(range(0x80, 0xA0)), c1)
        e(f0, _mask(range(0x90, 0xC0)), c2)
        e(f4, _mask(range(0x80, 0x90)), c2)

    def _byte_string(self, a: int, b: int) -> None:
        """The same string with every byte from 0x80 up taken as it comes."""
        st, esc, u1, u2, u3, u4 = (self.new() for _ in range(6))
        e = self.edge
        e(a, 1 << 0x22, st)
        e(st, _M_PLAIN | _mask(range(0x80, 0x100)), st)
        e(st, 1 << 0x22, b)
        e(st, 1 << 0x5C, esc)
        e(esc, _mask(b'"\\/bfnrt'), st)
        e(esc, 1 << 0x75, u1)
        for x, y in ((u1, u2), (u2, u3), (u3, u4), (u4, st)):
            e(x, _M_HEX, y)

    def number(self, a: int, b: int, integer: bool) -> None:
        """-?(0|[1-9][0-9]*) and, for a number, (\\.[0-9]+)?([eE][+-]?[0-9]+)? — it ends where b's bytes begin."""
        n, e = self.new, self.edge
        minus, zero, int_ = n(), n(), n()
        e(a, 1 << 0x2D, minus)
        for s in (a, minus):
            e(s, 1 << 0x30, zero)
            e(s, _M_19, int_)
        e(int_, _M_DIGITS, int_)
        ends = [zero, int_]
        if not integer:
            dot, frac, ee, esign, exp = n(), n(), n(), n(), n()
            for s in (zero, int_):
                e(s, 1 << 0x2E, dot)
            e(dot, _M_DIGITS, frac)
            e(frac, _M_DIGITS, frac)
            for s in (zero, int_, frac):
                e(s, _mask(b"eE"), ee)
            e(ee, _mask(b"+-"), esign)
            e(ee, _M_DIGITS, exp)
            e(esign, _M_DIGITS, exp)
            e(exp, _M_DIGITS, exp)
            ends += [frac, exp]
        for s in ends:
            self.eps[s].append(b)


def _dumps(v) -> bytes:
    return json.dumps(v, ensure_ascii=False, separators=(",", ":")).encode("utf-8")


class _Builder:
    def __init__(self, root: dict, nfa: "_Nfa | None" = None):
        self.nfa = nfa if nfa is not None else _Nfa()
        self.defs = root.get("$defs", {})
        if not isinstance(self.defs, dict):
            raise SchemaError("schema: `$defs` at #/$defs must be an object")
        self.open_refs: list[str] = []

    def fail(self, kw: str, ptr: str, why: str):
        raise SchemaError(f"schema: `{kw}` at {ptr or '#'} {why}")

    def check_keys(self, sch: dict, ptr: str, allowed) -> None:
        for k in sch:
            if k not in allowed and k not in _IGNORED and not (k == "$defs" and ptr == "#"):
                self.fail(k, f"{ptr}/{k}", "is not supported")

    def value(self, sch, ptr: str, a: int, b: int, depth: int) -> None:
        """Edges that spell every value of ``sch`` on the paths from a to b (neither gets a loop of its own)."""
        if not isinstance(sch, dict):
            self.fail(ptr.rsplit("/", 1)[-1] or "schema", ptr, "must be a schema object")
        if depth > SCHEMA_MAX_NESTING:
            raise SchemaError(f"schema: nesting at {ptr} exceeds the limit of {SCHEMA_MAX_NESTING} levels")
        if "$ref" in sch:
            self.check_keys(sch, ptr, ("$ref",))
            ref = sch["$ref"]
            if not isinstance(ref, str) or not ref.startswith("#/$defs/") or ref[8:] not in self.defs:
                self.fail("$ref", f"{ptr}/$ref", 'must be "#/$defs/NAME" with NAME defined in the root `$defs`')
            if ref in self.open_refs:
                self.fail("$ref", f"{ptr}/$ref", f"closes a reference cycle through {ref} (recursive schemas are "
                                                 f"not supported)")
            self.open_refs.append(ref)
            self.value(self.defs[ref[8:]], ref, a, b, depth)
            self.open_refs.pop()
            return
        if "anyOf" in sch:
            self.check_keys(sch, ptr, ("anyOf",))
            alts = sch["anyOf"]
            if not isinstance(alts, list) or not alts:
                self.fail("anyOf", f"{ptr}/anyOf", "must be a non-empty list of schemas")
            for i, alt in enumerate(alts):
                self.value(alt, f"{ptr}/anyOf/{i}", a, b, depth + 1)
            return
        if "enum" in sch or "const" in sch:
            kw = "enum" if "enum" in sch else "const"
            self.check_keys(sch, ptr, ("enum", "const", "type"))
            if "enum" in sch and "const" in sch:
                self.fail("const", f"{ptr}/const", "cannot stand beside `enum`")
            vals = sch[kw] if kw == "enum" else [sch[kw]]
            if not isinstance(vals, list) or not vals:
                self.fail(kw, f"{ptr}/{kw}", "must be a non-empty list")
            types = sch.get("type")
            types = None if types is None else self.type_list(types, ptr)
            for i, v in enumerate(vals):
                at = f"{ptr}/{kw}" + (f"/{i}" if kw == "enum" else "")
                if isinstance(v, bool):
                    t = "boolean"
                elif v is None:
                    t = "null"
                elif isinstance(v, int):
                    t = "integer"
                elif isinstance(v, str):
                    t = "string"
                else:
                    self.fail(kw, at, "holds a value that is no string, integer, boolean or null")
                if types is not None and t not in types and not (t == "integer" and "number" in types):
                    self.fail(kw, at, f"holds a {t}, which `type` excludes")
                self.nfa.lit(a, _dumps(v), b)
            return
        if "type" not in sch:
            self.check_keys(sch, ptr, ())  # (an unsupported keyword is the better message)
            self.fail("type", ptr, "is missing: a schema needs `type`, `enum`, `const`, `anyOf` or `$ref`")
        types = self.type_list(sch["type"], ptr)
        allowed = {"type"}
        if "object" in types:
            allowed |= {"properties", "required", "additionalProperties"}
        if "array" in types:
            allowed |= {"items"}
        self.check_keys(sch, ptr, allowed)
        for t in types:
            self.typed(t, sch, ptr, a, b, depth)

    def type_list(self, t, ptr: str) -> list[str]:
        types = t if isinstance(t, list) else [t]
        if not types or any(not isinstance(x, str) or x not in _TYPES for x in types) or len(set(types)) != len(types):
            self.fail("type", f"{ptr}/type", f"must be one of {', '.join(_TYPES)} or a list of distinct ones")
        return types

    def typed(self, t: str, sch: dict, ptr: str, a: int, b: int, depth: int) -> None:
        nfa = self.nfa
        if t == "string":
            nfa.string(a, b)
        elif t in ("integer", "number"):
            nfa.number(a, b, t == "integer")
        elif t == "boolean":
            nfa.lit(a, b"true", b)
            nfa.lit(a, b"false", b)
        elif t == "null":
            nfa.lit(a, b"null", b)
        elif t == "array":
            if "items" not in sch:
                self.fail("items", ptr, "is missing: an array needs one `items` schema")
            first, v_in, v_out, more = nfa.ws(nfa.new()), nfa.new(), nfa.ws(nfa.new()), nfa.ws(nfa.new())
            nfa.edge(a, 1 << 0x5B, first)
            nfa.edge(first, 1 << 0x5D, b)
            nfa.eps[first].append(v_in)
            nfa.eps[more].append(v_in)
            self.value(sch["items"], f"{ptr}/items", v_in, v_out, depth + 1)
            nfa.edge(v_out, 1 << 0x2C, more)
            nfa.edge(v_out, 1 << 0x5D, b)
        else:
            props = sch.get("properties", {})
            if not isinstance(props, dict):
                self.fail("properties", f"{ptr}/properties", "must be an object")
            if sch.get("additionalProperties") is not False:
                self.fail("additionalProperties", f"{ptr}/additionalProperties", "must be present and false")
            req = sch.get("required", [])
            if not isinstance(req, list) or any(not isinstance(r, str) for r in req) or set(req) != set(props) \
                    or len(req) != len(props):
                self.fail("required", f"{ptr}/required", "must name every property exactly once (an optional "
                                                         "property is a union with null)")
            cur = nfa.ws(nfa.new())
            nfa.edge(a, 1 << 0x7B, cur)
            if not props:
                nfa.edge(cur, 1 << 0x7D, b)
            for i, (key, sub) in enumerate(props.items()):
                colon, v_in, v_out = nfa.ws(nfa.new()), nfa.ws(nfa.new()), nfa.ws(nfa.new())
                nfa.lit(cur, _dumps(key), colon)
                nfa.edge(colon, 1 << 0x3A, v_in)
                esc = key.replace("~", "~0").replace("/", "~1")
                self.value(sub, f"{ptr}/properties/{esc}", v_in, v_out, depth + 1)
                if i == len(props) - 1:
                    nfa.edge(v_out, 1 << 0x7D, b)
                else:
                    cur = nfa.ws(nfa.new())
                    nfa.edge(v_out, 1 << 0x2C, cur)


class SchemaDfa:
    """``cls`` uint8 [256], ``trans`` uint16 [S, C] (START 0, DONE 1, DEAD 0xFFFF) and the canonical ``text``."""

    def __init__(self, cls: np.ndarray, trans: np.ndarray, text: str):
        self.cls, self.trans, self.text = cls, trans, text
        self.S, self.C = trans.shape
        self.cls.setflags(write=False)
        self.trans.setflags(write=False)

    @property
    def nbytes(self) -> int:
        return self.S * self.C * 2

    def tobytes(self) -> bytes:
        return self.cls.tobytes() + self.trans.tobytes()


def check_tables(cls: np.ndarray, trans: np.ndarray) -> None:
    """What the kernels trust of a table: its shape, the limits, classes below C and next states below S or DEAD."""
    if cls.shape != (256,) or cls.dtype != np.uint8 or trans.ndim != 2 or trans.dtype != np.uint16:
        raise ValueError("schema table: cls must be uint8 [256] and trans uint16 [S, C]")
    S, C = trans.shape
    if not 2 <= S <= SCHEMA_MAX_STATES or not 1 <= C <= 256 or S * C * 2 > SCHEMA_TAB_BYTES \
            or int(cls.max()) >= C or ((trans >= S) & (trans != DEAD)).any() or (trans[DONE] != DEAD).any():
        raise ValueError("schema table: outside the limits, or an entry names a state or class it does not have")


def _determinise(nfa: _Nfa, start: int, accept: int) -> tuple[np.ndarray, np.ndarray]:
    edges, eps = nfa.edges, nfa.eps
    # byte classes: the signature of a byte is the set of distinct labels that hold it
    labels: dict[int, int] = {}
    for es in edges:
        for m, _ in es:
            labels.setdefault(m, len(labels))
    sig_cls: dict[tuple, int] = {}
    cls = np.zeros(256, dtype=np.uint8)
    lab_list = list(labels)
    for b in range(256):
        sig = tuple(i for i, m in enumerate(lab_list) if (m >> b) & 1)
        cls[b] = sig_cls.setdefault(sig, len(sig_cls))
    C = len(sig_cls)
    lab_classes = [sorted({int(cls[b]) for b in range(256) if (m >> b) & 1}) for m in lab_list]
    # ε-closures, memoised per NFA state
    clo: dict[int, tuple[int, ...]] = {}

    def closure(s: int) -> tuple[int, ...]:
        c = clo.get(s)
        if c is None:
            seen, todo = {s}, [s]
            while todo:
                for t in eps[todo.pop()]:
                    if t not in seen:
                        seen.add(t)
                        todo.append(t)
            c = clo[s] = tuple(seen)
        return c

    ids: dict[tuple[int, ...], int] = {tuple(sorted(closure(start))): START, (accept,): DONE}
    order = list(ids)
    rows: list[dict[int, int]] = []
    i = 0
    while i < len(order):
        by_cls: dict[int, set] = {}
        for s in order[i]:
            for m, t in edges[s]:
                for c in lab_classes[labels[m]]:
                    by_cls.setdefault(c, set()).add(t)
        row = {}
        for c in sorted(by_cls):
            tgt = set()
            for t in by_cls[c]:
                tgt.update(closure(t))
            key = tuple(sorted(tgt))
            if accept in tgt and len(key) > 1:  # (the root's closing brace is the only way in: a guard, not a path)
                raise SchemaError("schema: the document's end is ambiguous")
            j = ids.get(key)
            if j is None:
                if len(order) >= SCHEMA_MAX_STATES:
                    raise SchemaError(f"schema: the compiled automaton exceeds the limit of {SCHEMA_MAX_STATES} "
                                      f"states")
                j = ids[key] = len(order)
                order.append(key)
            row[c] = j
        rows.append(row)
        i += 1
    S = len(order)
    if S * C * 2 > SCHEMA_TAB_BYTES:
        raise SchemaError(f"schema: the transition table ({S} states x {C} byte classes x 2 bytes) exceeds the limit "
                          f"of {SCHEMA_TAB_BYTES} bytes")
    trans = np.full((S, C), DEAD, dtype=np.uint16)
    for s, row in enumerate(rows):
        for c, j in row.items():
            trans[s, c] = j
    return cls, trans


_CACHE: OrderedDict[str, SchemaDfa] = OrderedDict()
_CACHE_MAX = 64


def compile_schema(schema: dict) -> SchemaDfa:
    """The automaton of ``schema``, cached by canonical text (a small LRU). Raises ``SchemaError``."""
    if not isinstance(schema, dict):
        raise SchemaError("schema: `schema` at # must be an object")
    try:
        text = canonical_text(schema)
    except (TypeError, ValueError, RecursionError) as e:
        raise SchemaError(f"schema: not JSON ({e})") from None
    hit = _CACHE.get(text)
    if hit is not None:
        _CACHE.move_to_end(text)
        return hit
    if len(text.encode("utf-8")) > SCHEMA_MAX_TEXT:
        raise SchemaError(f"schema: the canonical text exceeds the limit of {SCHEMA_MAX_TEXT} bytes")
    t = schema.get("type")
    if t != "object":
        raise SchemaError('schema: `type` at #/type must be "object" at the root')
    bld = _Builder(schema)
    start, accept = bld.nfa.new(), bld.nfa.new()
    try:
        bld.value(schema, "#", start, accept, 1)
    except RecursionError:  # (cannot happen below the nesting limit; a guard, not a path)
        raise SchemaError(f"schema: nesting exceeds the limit of {SCHEMA_MAX_NESTING} levels") from None
    cls, trans = _determinise(bld.nfa, start, accept)
    dfa = SchemaDfa(cls, trans, text)
    _CACHE[text] = dfa
    while len(_CACHE) > _CACHE_MAX:
        _CACHE.popitem(last=False)
    return dfa


def compile_text(text: str) -> SchemaDfa:
    """The automaton of a canonical schema text (``SamplingParams.json_schema``; what travels to the engine)."""
    hit = _CACHE.get(text)
    if hit is not None:
        _CACHE.move_to_end(text)
        return hit
    try:
        schema = json.loads(text)
    except (TypeError, ValueError, RecursionError) as e:
        raise SchemaError(f"schema: not JSON ({e})") from None
    return compile_schema(schema)


def state_record(state: int, table: int) -> np.ndarray:
    """A schema row's int32 [4] record of the device state table: (state, 0, 0, table index + 1)."""
    if not (0 <= state < SCHEMA_MAX_STATES or state == DEAD) or table < 0:
        raise ValueError(f"not a schema automaton state: {state} of table {table}")
    return np.array([state, 0, 0, table + 1], dtype=np.int32)
