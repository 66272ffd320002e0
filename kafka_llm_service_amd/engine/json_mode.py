"""JSON mode (``response_format: {"type": "json_object"}``): the byte-level pushdown automaton and the token table.

The automaton is deterministic and reads RFC 8259 JSON text whose top-level value is an object, one byte at a time.
A row's state is a small fixed record ``(state, depth, stack)``:

* ``state``: one of fewer than 64 ids (below); ``DEAD`` (63) once a byte was rejected;
* ``depth``: open containers, 0..``JSON_MAX_DEPTH`` (32) — a byte that would open a 33rd level is rejected;
* ``stack``: one bit per open level, bit ``l - 1`` for level ``l``: 1 = object, 0 = array; bits at and above ``depth``
  are zero, so equal situations are equal records.

``TRANS`` uint8 [64, 256] is the whole grammar: entry ``TRANS[state, byte]`` holds the next state in its low six bits
and an operation in its top two:

    0  plain          state = next
    1  open           depth == 32 rejects; else push (``{``: object bit, ``[``: array bit), state = next
    2  close          the top must be an object for ``}`` and an array for ``]``; pop; state = DONE at depth 0, else
                      AFTER_VALUE
    3  comma          state = EXPECT_KEY if the top is an object, else EXPECT_VALUE

Strings take every JSON escape (``\\uXXXX`` with four hex digits), no raw control bytes, and bytes >= 0x80 only as
well-formed UTF-8 (the standard DFA: no overlongs, no surrogates, nothing above U+10FFFF); a character may be split
across tokens because the states carry it. A number ends when a byte that may follow a value arrives: the number
states that may end copy AFTER_VALUE's entries for whitespace, ``,``, ``}`` and ``]``. Whitespace is allowed wherever
the RFC allows it inside the document, not before the opening ``{`` and not after the closing ``}``; DONE accepts no
byte at all. ``ops/reference.py`` (``json_walk``, ``json_mask_ref``, ``json_advance_ref``) is the definition of how
the table is walked and what a token mask is; ``ops/csrc/json_mask.hip`` agrees with it bit for bit.

``JsonTable`` holds, per tokenizer, the bytes the API's detokeniser emits for every id (``KafkaTokenizer.token_bytes``:
byte-level BPE pieces, the pseudo-words above the trained vocabulary, nothing for special tokens) as a CSR pair
``tok_off`` int32 [V + 1] / ``tok_bytes`` uint8, and the model's ``eos_token_ids``. An id without bytes is never
allowed; the EOS ids are allowed in DONE and only there.
"""
from __future__ import annotations

import numpy as np

JSON_MAX_DEPTH = 32
JSON_STATE_INTS = 4  # a row's record in the device state table: (state, depth, stack bits, 0)
JSON_MAX_EOS = 8     # EOS ids the mask kernel compares a token with in DONE

OP_OPEN, OP_CLOSE, OP_COMMA = 1, 2, 3

_NAMES = (
    "START", "OBJ_START", "EXPECT_KEY", "EXPECT_COLON", "EXPECT_VALUE", "ARR_START", "AFTER_VALUE", "DONE",
    "N_MINUS", "N_ZERO", "N_INT", "N_DOT", "N_FRAC", "N_E", "N_ESIGN", "N_EXP",
    "L_T", "L_TR", "L_TRU", "L_F", "L_FA", "L_FAL", "L_FALS", "L_N", "L_NU", "L_NUL",
    # strings: the key copy, then the value copy in the same order (K_* + STR_STRIDE = V_*)
    "K_STR", "K_ESC", "K_U1", "K_U2", "K_U3", "K_U4", "K_C1", "K_C2", "K_C3", "K_E0", "K_ED", "K_F0", "K_F4",
    "V_STR", "V_ESC", "V_U1", "V_U2", "V_U3", "V_U4", "V_C1", "V_C2", "V_C3", "V_E0", "V_ED", "V_F0", "V_F4",
)
S = {n: i for i, n in enumerate(_NAMES)}
STATE_NAMES = {i: n for n, i in S.items()}
N_STATES = len(_NAMES)
DEAD = 63
STATE_NAMES[DEAD] = "DEAD"
START, DONE, AFTER_VALUE, EXPECT_KEY, EXPECT_VALUE = (S[n] for n in ("START", "DONE", "AFTER_VALUE", "EXPECT_KEY",
                                                                      "EXPECT_VALUE"))
assert N_STATES < DEAD

_WS = b" \t\n\r"
_DIGITS = b"0123456789"
_HEX = b"0123456789abcdefABCDEF"


def _build_trans() -> np.ndarray:
    t = np.full((64, 256), DEAD, dtype=np.uint8)

    def put(state: str, bs, nxt: str, op: int = 0) -> None:
        for b in bs:
            t[S[state], b] = S[nxt] | (op << 6)

    def value_start(state: str) -> None:
        put(state, _WS, state)
        put(state, b"{", "OBJ_START", OP_OPEN)
        put(state, b"[", "ARR_START", OP_OPEN)
        put(state, b'"', "V_STR")
        put(state, b"-", "N_MINUS")
        put(state, b"0", "N_ZERO")
        put(state, b"123456789", "N_INT")
        put(state, b"t", "L_T")
        put(state, b"f", "L_F")
        put(state, b"n", "L_N")

    def after_value(state: str) -> None:
        put(state, _WS, "AFTER_VALUE")
        put(state, b",", "AFTER_VALUE", OP_COMMA)  # (the walk picks EXPECT_KEY / EXPECT_VALUE by the stack top)
        put(state, b"}]", "AFTER_VALUE", OP_CLOSE)

    put("START", b"{", "OBJ_START", OP_OPEN)
    put("OBJ_START", _WS, "OBJ_START")
    put("OBJ_START", b'"', "K_STR")
    put("OBJ_START", b"}", "AFTER_VALUE", OP_CLOSE)
    put("EXPECT_KEY", _WS, "EXPECT_KEY")
    put("EXPECT_KEY", b'"', "K_STR")
    put("EXPECT_COLON", _WS, "EXPECT_COLON")
    put("EXPECT_COLON", b":", "EXPECT_VALUE")
    value_start("EXPECT_VALUE")
    value_start("ARR_START")
    put("ARR_START", b"]", "AFTER_VALUE", OP_CLOSE)
    after_value("AFTER_VALUE")
    # numbers: -?(0|[1-9][0-9]*)(\.[0-9]+)?([eE][+-]?[0-9]+)?
    put("N_MINUS", b"0", "N_ZERO")
    put("N_MINUS", b"123456789", "N_INT")
    put("N_INT", _DIGITS, "N_INT")
    for s in ("N_ZERO", "N_INT"):
        put(s, b".", "N_DOT")
    put("N_DOT", _DIGITS, "N_FRAC")
    put("N_FRAC", _DIGITS, "N_FRAC")
    for s in ("N_ZERO", "N_INT", "N_FRAC"):
        put(s, b"eE", "N_E")
    put("N_E", b"+-", "N_ESIGN")
    put("N_E", _DIGITS, "N_EXP")
    put("N_ESIGN", _DIGITS, "N_EXP")
    put("N_EXP", _DIGITS, "N_EXP")
    for s in ("N_ZERO", "N_INT", "N_FRAC", "N_EXP"):
        after_value(s)
    # literals
    for word in (b"true", b"false", b"null"):
        names = ["L_" + word[:i].decode().upper() for i in range(1, len(word))]
        for a, b, c in zip(names, word[1:], names[1:] + ["AFTER_VALUE"]):
            put(a, bytes([b]), c)
    # strings (key copy ends in EXPECT_COLON, value copy in AFTER_VALUE)
    for p, end in (("K_", "EXPECT_COLON"), ("V_", "AFTER_VALUE")):
        st = p + "STR"
        put(st, [b for b in range(0x20, 0x80) if b not in b'"\\'], st)
        put(st, b'"', end)
        put(st, b"\\", p + "ESC")
        put(p + "ESC", b'"\\/bfnrt', st)
        put(p + "ESC", b"u", p + "U1")
        for a, b in ((p + "U1", p + "U2"), (p + "U2", p + "U3"), (p + "U3", p + "U4"), (p + "U4", st)):
            put(a, _HEX, b)
        # UTF-8 (Unicode table 3-7): lead byte -> continuation states; C1..C3 = that many plain continuations left
        put(st, range(0xC2, 0xE0), p + "C1")
        put(st, [0xE0], p + "E0")
        put(st, [b for b in range(0xE1, 0xF0) if b != 0xED], p + "C2")
        put(st, [0xED], p + "ED")
        put(st, [0xF0], p + "F0")
        put(st, range(0xF1, 0xF4), p + "C3")
        put(st, [0xF4], p + "F4")
        put(p + "C1", range(0x80, 0xC0), st)
        put(p + "C2", range(0x80, 0xC0), p + "C1")
        put(p + "C3", range(0x80, 0xC0), p + "C2")
        put(p + "E0", range(0xA0, 0xC0), p + "C1")  # no overlong three-byte forms
        put(p + "ED", range(0x80, 0xA0), p + "C1")  # no surrogates
        put(p + "F0", range(0x90, 0xC0), p + "C2")  # no overlong four-byte forms
        put(p + "F4", range(0x80, 0x90), p + "C2")  # nothing above U+10FFFF
    return t


TRANS = _build_trans()
TRANS.setflags(write=False)

START_STATE = (START, 0, 0)


def state_record(state) -> np.ndarray:
    """``(state, depth, stack)`` as the int32 [4] record of the device state table (the stack's bit 31 travels as the
    sign bit)."""
    s, d, stk = (int(v) for v in state)
    if not (0 <= s < N_STATES or s == DEAD) or not 0 <= d <= JSON_MAX_DEPTH or not 0 <= stk < (1 << 32) \
            or (d < 32 and stk >> d):
        raise ValueError(f"not a JSON automaton state: {state}")
    return np.array([s, d, stk, 0], dtype=np.uint32).view(np.int32)


def record_state(rec) -> tuple[int, int, int]:
    """The inverse of ``state_record`` (any int32 [>= 3] row of the state table)."""
    r = np.asarray(rec, dtype=np.int32).reshape(-1)
    return int(r[0]), int(r[1]), int(r[2:3].view(np.uint32)[0])


class JsonTable:
    """The bytes of every token id (CSR) and the EOS ids of one tokenizer / model."""

    def __init__(self, tok_off: np.ndarray, tok_bytes: np.ndarray, eos_ids):
        self.tok_off = np.ascontiguousarray(tok_off, dtype=np.int32)
        self.tok_bytes = np.ascontiguousarray(tok_bytes, dtype=np.uint8)
        self.V = self.tok_off.size - 1
        self.eos_ids = np.array(sorted(set(int(e) for e in eos_ids)), dtype=np.int32)
        lens = np.diff(self.tok_off)
        if self.V < 1 or int(self.tok_off[0]) != 0 or (lens < 0).any() or int(self.tok_off[-1]) != self.tok_bytes.size:
            raise ValueError("JSON token table: offsets do not tile the bytes")
        if not 1 <= self.eos_ids.size <= JSON_MAX_EOS or int(self.eos_ids[0]) < 0 or int(self.eos_ids[-1]) >= self.V:
            raise ValueError(f"JSON token table: 1..{JSON_MAX_EOS} EOS ids inside the vocabulary are needed")
        if lens[self.eos_ids].any():
            raise ValueError("JSON token table: an EOS id must have no bytes")
        self.lens = lens.astype(np.int32)
        self.W = -(-self.V // 32)

    @classmethod
    def from_byte_strings(cls, pieces: list[bytes], eos_ids) -> "JsonTable":
        """A table over ``pieces[i]`` = the bytes of id i; the EOS ids lose theirs (they are special tokens)."""
        eos = set(int(e) for e in eos_ids)
        pieces = [b"" if i in eos else bytes(p) for i, p in enumerate(pieces)]
        off = np.zeros(len(pieces) + 1, dtype=np.int64)
        np.cumsum([len(p) for p in pieces], out=off[1:])
        return cls(off, np.frombuffer(b"".join(pieces), dtype=np.uint8), eos_ids)

    @classmethod
    def from_tokenizer(cls, tok, eos_ids, vocab: int | None = None) -> "JsonTable":
        V = int(vocab or tok.vocab_size)
        return cls.from_byte_strings([tok.token_bytes(i) for i in range(V)], eos_ids)

    def bytes_of(self, i: int) -> bytes:
        return self.tok_bytes[self.tok_off[i]:self.tok_off[i + 1]].tobytes()


_TABLES: dict = {}


def table_for(tok, eos_ids, vocab: int | None = None) -> JsonTable:
    """The tokenizer's table, built once (next to ``constrained.vocab_classes``)."""
    key = (id(tok), tuple(sorted(int(e) for e in eos_ids)), int(vocab or tok.vocab_size))
    t = _TABLES.get(key)
    if t is None:
        t = _TABLES[key] = JsonTable.from_tokenizer(tok, eos_ids, vocab)
    return t
