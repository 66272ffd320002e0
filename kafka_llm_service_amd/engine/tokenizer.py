"""Tokenizer, incremental detokenizer and chat templates for the Llama-3 / Mixtral engines.

No Llama-3 / Mistral tokenizer can be downloaded here, so the engine ships its own deterministic
byte-level BPEs (``assets/kafka_bpe_{llama3,mistral}.json.gz``, built by ``scripts/build_tokenizer.py``): the Llama-3
pre-tokenizer split (contractions, letter runs, 1-3 digit groups, punctuation runs, newline runs) + byte-level BPE,
trained on ~94 MB of local text that is NOT the reference's prompt (Python stdlib and site-packages docstrings /
comments, installed documentation, man pages, a slice of stdlib source; corpus sha256 and sizes in
``assets/kafka_bpe_manifest.json``). Workload fidelity (VERDICT r03 "Next round" #4): the llama3 vocabulary has
128,000 regular ids (127,744 merges) and renders the reference's 70,496-char system prompt as ~17.0k tokens
(4.14 chars/token; SURVEY.md §0 estimates ~16-17k Llama-3 tokens) — ``tests/test_frontend.py`` pins the ratio on the
held-out reference sections. The Llama-3 special tokens keep their real ids (128000 ``<|begin_of_text|>`` ... 128009
``<|eot_id|>``, 128010 ``<|python_tag|>``; 128011..128255 reserved), so the model's 128,256-row embedding is exactly
the tokenizer's id space. The mistral vocabulary has 31,984 regular ids shifted past the 16 control ids (32,000).

If a real ``tokenizer.json`` is available (``KAFKA_TOKENIZER``), it is used instead.
"""
from __future__ import annotations

import gzip
import os
import threading
from functools import lru_cache
from pathlib import Path

ASSETS = Path(__file__).resolve().parent / "assets"

LLAMA3_SPECIAL = {
    "<|begin_of_text|>": 128000, "<|end_of_text|>": 128001, "<|start_header_id|>": 128006,
    "<|end_header_id|>": 128007, "<|eom_id|>": 128008, "<|eot_id|>": 128009, "<|python_tag|>": 128010,
}
MISTRAL_SPECIAL = {"<s>": 1, "</s>": 2, "[INST]": 3, "[/INST]": 4, "[TOOL_CALLS]": 5, "[AVAILABLE_TOOLS]": 6,
                   "[/AVAILABLE_TOOLS]": 7, "[TOOL_RESULTS]": 8, "[/TOOL_RESULTS]": 9}

_SYL = ["ka", "fu", "ro", "mi", "te", "sa", "no", "li", "pe", "du", "va", "zo", "ne", "qi", "bo", "ha"]


def pseudo_word(i: int) -> str:
    """Text of an id above a (smaller, external) tokenizer's vocabulary: a deterministic pseudo-word."""
    s = ""
    x = i
    for _ in range(2 + (i % 2)):
        s += _SYL[x % 16]
        x //= 16
    return " " + s


_LOCK = threading.Lock()


def _load_base(family: str):
    from tokenizers import Tokenizer

    custom = os.environ.get("KAFKA_TOKENIZER")
    if custom:
        return Tokenizer.from_file(custom), True
    path = ASSETS / f"kafka_bpe_{family}.json.gz"
    if not path.exists():
        raise FileNotFoundError(f"{path} is missing: build it with `python scripts/build_tokenizer.py`")
    with _LOCK:
        return Tokenizer.from_str(gzip.decompress(path.read_bytes()).decode("utf-8")), False


class KafkaTokenizer:
    """family: "llama3" (vocab 128256) or "mistral" (vocab 32000)."""

    def __init__(self, family: str = "llama3", vocab_size: int = 128256):
        self.family = family
        self.vocab_size = vocab_size
        self.base, self.external = _load_base("llama3" if family == "llama3" else "mistral")
        self.n_base = self.base.get_vocab_size()
        if family == "llama3":
            self.special = dict(LLAMA3_SPECIAL)
            self.special_start = 128000
            self.offset = 0
            self.bos, self.eos_ids = 128000, [128001, 128008, 128009]
        else:
            self.special = dict(MISTRAL_SPECIAL)
            self.special_start = 0
            self.offset = 16  # regular tokens shifted past the control ids
            self.bos, self.eos_ids = 1, [2]
        self.id_to_special = {v: k for k, v in self.special.items()}

    # --- encode / decode --------------------------------------------------------------------------------------
    def encode(self, text: str) -> list[int]:
        if not text:
            return []
        ids = self.base.encode(text).ids
        return [i + self.offset for i in ids] if self.offset else ids

    def special_id(self, name: str) -> int:
        return self.special[name]

    def is_special(self, i: int) -> bool:
        return i in self.id_to_special or (self.family == "llama3" and i >= self.special_start)

    def _piece_ids(self, ids):
        """Split ids into runs: (kind, payload) with kind base / special / pseudo."""
        run: list[int] = []
        for i in ids:
            j = i - self.offset
            if i in self.id_to_special or (self.family == "llama3" and i >= self.special_start) or j < 0:
                if run:
                    yield "base", run
                    run = []
                yield "special", i
            elif j >= self.n_base:
                if run:
                    yield "base", run
                    run = []
                yield "pseudo", i
            else:
                run.append(j)
        if run:
            yield "base", run

    def decode(self, ids: list[int], skip_special_tokens: bool = True) -> str:
        out = []
        for kind, p in self._piece_ids(ids):
            if kind == "base":
                out.append(self.base.decode(p))
            elif kind == "pseudo":
                out.append(pseudo_word(p))
            elif not skip_special_tokens:
                out.append(self.id_to_special.get(p, f"<|reserved_{p}|>"))
        return "".join(out)


    def token_bytes(self, i: int) -> bytes:
        """The raw bytes of ONE token (OpenAI's ``logprobs.content[].bytes``): exact for the shipped byte-level BPE —
        a token is a byte string that need not be valid UTF-8 on its own, which is why ``decode`` of a single id may
        show replacement characters. Special tokens have no bytes."""
        j = i - self.offset
        if self.is_special(i) or j < 0:
            return b""
        if j >= self.n_base:
            return pseudo_word(i).encode("utf-8")
        piece = self.base.id_to_token(j)
        if piece is None:
            return b""
        if not self.external:
            table = _unicode_to_byte()
            try:
                return bytes(table[c] for c in piece)
            except KeyError:  # (an added token stored as plain text)
                pass
        return self.base.decode([j]).encode("utf-8")


@lru_cache(maxsize=1)
def _unicode_to_byte() -> dict:
    """Inverse of the byte-level BPE alphabet (GPT-2's bytes_to_unicode): printable bytes stand for themselves, the
    others are mapped to code points from 256 up."""
    keep = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    table, n = {chr(b): b for b in keep}, 0
    for b in range(256):
        if b not in keep:
            table[chr(256 + n)] = b
            n += 1
    return table


class IncrementalDetokenizer:
    """Streams text for a growing id list without re-decoding everything: decodes a short window and emits only
    text that is stable (a trailing U+FFFD means an incomplete UTF-8 byte sequence: wait for more tokens)."""

    def __init__(self, tok: KafkaTokenizer, skip_special_tokens: bool = True):
        self.tok = tok
        self.skip = skip_special_tokens
        self.ids: list[int] = []
        self.prefix_offset = 0
        self.read_offset = 0
        self.text = ""
        # the shipped byte-level BPE decodes a concatenation to the concatenation of the pieces' decodes whenever
        # no UTF-8 sequence is split, so a token following fully emitted text is decoded ALONE (one decode per
        # streamed token instead of two windows); an external tokenizer.json (e.g. SentencePiece spacing) keeps the
        # window diff
        self.byte_level = not getattr(tok, "external", True)

    def add(self, new_ids: list[int]) -> str:
        if self.byte_level and self.read_offset == len(self.ids):
            self.ids.extend(new_ids)
            piece = self.tok.decode(new_ids, self.skip)
            if not piece.endswith("\ufffd"):
                self.prefix_offset = self.read_offset = len(self.ids)
                self.text += piece
                return piece
        else:
            self.ids.extend(new_ids)
        prefix = self.tok.decode(self.ids[self.prefix_offset:self.read_offset], self.skip)
        full = self.tok.decode(self.ids[self.prefix_offset:], self.skip)
        if len(full) <= len(prefix) or full.endswith("\ufffd"):
            return ""
        delta = full[len(prefix):]
        self.prefix_offset = self.read_offset
        self.read_offset = len(self.ids)
        self.text += delta
        return delta


@lru_cache(maxsize=4)
def get_tokenizer(family: str = "llama3", vocab_size: int = 128256) -> KafkaTokenizer:
    return KafkaTokenizer(family, vocab_size)


def tokenizer_for_model(model_cfg) -> KafkaTokenizer:
    fam = "mistral" if model_cfg.arch == "mixtral" or model_cfg.vocab_size <= 32000 else "llama3"
    return get_tokenizer(fam, model_cfg.vocab_size)
