"""Request / sequence state and sampling parameters of the engine.

``SamplingParams`` carries every OpenAI request knob the reference accepted but dropped on the floor
(/root/reference/src/kafka/types.py:34-38 vs /root/reference/server.py:289-294 — quirk Q7): temperature (0 means
greedy; the reference's ``temperature or 0.7`` coercion, /root/reference/server.py:292, is NOT reproduced — Q6),
top_p, stop, presence/frequency penalties, plus engine-only knobs (top_k, seed, ignore_eos for benchmarks, a logits
processor for constrained tool-call decoding).
"""
from __future__ import annotations

import enum
import itertools
import time
from dataclasses import dataclass, field
from typing import Callable

from kafka_llm_service_amd.engine.step_plan import LOGIT_BIAS_MAX


PENDING = -1  # placeholder of a token still being sampled by the in-flight engine step (async scheduling)


@dataclass
class SamplingParams:
    temperature: float = 1.0
    top_p: float = 1.0
    top_k: int = 0
    max_tokens: int = 256
    stop: list[str] = field(default_factory=list)
    stop_token_ids: list[int] = field(default_factory=list)
    ignore_eos: bool = False
    seed: int | None = None
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    # called with (output_token_ids) -> allowed token ids (list / constrained.Mask) or None for "no constraint"
    allowed_tokens_fn: Callable | None = None
    # picklable tool-call grammar {"tools": [...], "tool_choice": ...}: the engine builds the constraint
    # (engine/constrained.py) on its own side, so it also works through the DP / TP worker pipes
    # An optional key ``"mode"``: "program" (the default: the generator-based constraint) or "automaton" — the call's
    # body compiled from the tools' schemas and masked on the device (engine/tool_automaton.py); the engine's default
    # comes from env KAFKA_TOOL_GRAMMAR
    tool_grammar: dict | None = None
    # set by the engine for an automaton request: engine/tool_automaton.ToolPlan (the body, the envelope's tokens)
    tool_plan: object | None = None
    # OpenAI ``logprobs`` / ``top_logprobs``: the log-probability of every generated token and of the 0..20 most
    # likely tokens at its position, over the model's RAW logits (before temperature, penalties and grammar masks;
    # ops/csrc/logprobs.hip). They ride back in ``StepOutput.logprobs``.
    logprobs: bool = False
    top_logprobs: int = 0
    # OpenAI ``logit_bias``: (token id, bias in [-100, 100]) pairs, at most LOGIT_BIAS_MAX of them, added to the
    # logits inside the sampler kernel after the penalties and before temperature and the grammar mask; normalised
    # here to a tuple sorted by id without zero entries, or None (picklable: it crosses the worker pipes)
    logit_bias: tuple | None = None
    # keep the tokens with p_i >= min_p * p_max (0: off), intersected with top-k / top-p; the sampler kernel tests
    # x_i / T >= max + ln(min_p) per token (engine/logits_proc.py proc[7]). Greedy and forced rows ignore it.
    min_p: float = 0.0
    # multiplicative penalty of HF ``generate`` / vLLM over every token the sequence has SEEN — its prompt and the
    # tokens generated so far — in [0.1, 10] (1: off): a seen logit x becomes x / r if x > 0 and x * r otherwise, before
    # the additive penalties (engine/logits_proc.py, the sampler kernel's rep_tab). Forced rows ignore it.
    repetition_penalty: float = 1.0
    # OpenAI ``response_format: {"type": "json_object"}``: every sampled token keeps the output a prefix of one JSON
    # object (RFC 8259, at most 32 levels deep; engine/json_mode.py), and once the object has closed only an EOS id
    # is allowed. The mask is built on the device from a device-resident automaton state (ops/csrc/json_mask.hip) and
    # applies last, like a tool-call mask; it is not combined with ``allowed_tokens_fn`` / ``tool_grammar``.
    json_mode: bool = False
    # OpenAI ``response_format: {"type": "json_schema", ...}``: the canonical text of a schema of the supported subset
    # (engine/json_schema.py), or None. Every sampled token keeps the output a prefix of one document that conforms to
    # it; after the document only an EOS id is allowed. The schema compiles to a transition table of its own that the
    # device kernels walk (ops/csrc/table_grammar.hip); excludes ``json_mode`` and the token constraints.
    json_schema: str | None = None

    def __post_init__(self):
        if self.tool_grammar is not None and self.tool_grammar.get("mode") is not None:
            from kafka_llm_service_amd.engine.tool_automaton import grammar_mode

            if grammar_mode(self.tool_grammar) == "automaton" and (
                    self.json_mode or self.json_schema is not None or self.allowed_tokens_fn is not None):
                raise ValueError("tool_grammar mode \"automaton\" cannot be combined with json_mode, json_schema or "
                                 "an explicit allowed_tokens_fn")
        if self.json_schema is not None:
            if not isinstance(self.json_schema, str):
                raise ValueError("json_schema must be the canonical text of a schema, or None")
            if self.json_mode or self.allowed_tokens_fn is not None or self.tool_grammar is not None:
                raise ValueError("json_schema cannot be combined with json_mode, a token constraint or a tool grammar")
            from kafka_llm_service_amd.engine.json_schema import compile_text

            compile_text(self.json_schema)  # (SchemaError is a ValueError; the automaton stays cached for the engine)
        if not isinstance(self.json_mode, bool):
            raise ValueError("json_mode must be a bool")
        if self.json_mode and (self.allowed_tokens_fn is not None or self.tool_grammar is not None):
            raise ValueError("json_mode cannot be combined with a token constraint or a tool grammar")
        if isinstance(self.repetition_penalty, bool) or not isinstance(self.repetition_penalty, (int, float)) \
                or not 0.1 <= self.repetition_penalty <= 10.0:  # (a NaN fails both comparisons)
            raise ValueError("repetition_penalty must be a number in [0.1, 10]")
        self.repetition_penalty = float(self.repetition_penalty)
        if isinstance(self.min_p, bool) or not isinstance(self.min_p, (int, float)) \
                or not 0.0 <= self.min_p <= 1.0:  # (a NaN fails both comparisons)
            raise ValueError("min_p must be a number in [0, 1]")
        self.min_p = float(self.min_p)
        if self.logit_bias is not None:
            items = self.logit_bias.items() if isinstance(self.logit_bias, dict) else self.logit_bias
            pairs = tuple(sorted((int(t), float(b)) for t, b in items if float(b) != 0.0))
            ids = [t for t, _ in pairs]
            if any(t < 0 for t in ids) or len(set(ids)) != len(ids):
                raise ValueError("logit_bias token ids must be distinct non-negative integers")
            if any(not -100.0 <= b <= 100.0 for _, b in pairs):  # (a NaN fails both comparisons)
                raise ValueError("logit_bias values must lie in [-100, 100]")
            if len(pairs) > LOGIT_BIAS_MAX:
                raise ValueError(f"logit_bias holds more than {LOGIT_BIAS_MAX} entries")
            self.logit_bias = pairs or None
        if not isinstance(self.top_logprobs, int) or isinstance(self.top_logprobs, bool) \
                or not 0 <= self.top_logprobs <= 20:
            raise ValueError("top_logprobs must be an integer in 0..20")
        if self.top_logprobs > 0 and not self.logprobs:
            raise ValueError("top_logprobs requires logprobs")
        if self.temperature < 0:
            raise ValueError("temperature must be >= 0")
        if not 0 < self.top_p <= 1:
            raise ValueError("top_p must be in (0, 1]")
        if self.max_tokens < 1:
            raise ValueError("max_tokens must be >= 1")
        if isinstance(self.stop, str):
            self.stop = [self.stop]

    @property
    def greedy(self) -> bool:
        return self.temperature == 0.0


class SeqStatus(enum.Enum):
    WAITING = 0
    RUNNING = 1
    FINISHED = 2


_ids = itertools.count(1)


class Sequence:
    __slots__ = ("seq_id", "request_id", "prompt_ids", "output_ids", "params", "status", "num_computed",
                 "num_cached", "arrival", "first_token_time", "finish_reason", "last_token_time", "preemptions",
                 "stop_checker", "meta", "token_times")

    def __init__(self, request_id: str, prompt_ids: list[int], params: SamplingParams, meta: dict | None = None):
        if len(prompt_ids) == 0:
            raise ValueError("empty prompt")
        self.seq_id = next(_ids)
        self.request_id = request_id
        self.prompt_ids = list(prompt_ids)
        self.output_ids: list[int] = []
        self.params = params
        self.status = SeqStatus.WAITING
        self.num_computed = 0
        self.num_cached = 0
        self.arrival = time.perf_counter()
        self.first_token_time: float | None = None
        self.last_token_time: float | None = None
        self.finish_reason: str | None = None
        self.preemptions = 0
        self.stop_checker = None
        self.meta = meta or {}
        self.token_times = None

    @property
    def total_len(self) -> int:
        return len(self.prompt_ids) + len(self.output_ids)

    def token_at(self, i: int) -> int:
        n = len(self.prompt_ids)
        return self.prompt_ids[i] if i < n else self.output_ids[i - n]

    def tokens_range(self, a: int, b: int) -> list[int]:
        n = len(self.prompt_ids)
        if b <= n:
            return self.prompt_ids[a:b]
        if a >= n:
            return self.output_ids[a - n:b - n]
        return self.prompt_ids[a:] + self.output_ids[:b - n]

    def all_ids(self) -> list[int]:
        return self.prompt_ids + self.output_ids

    @property
    def remaining(self) -> int:
        return self.total_len - self.num_computed

    @property
    def finished(self) -> bool:
        return self.status == SeqStatus.FINISHED


@dataclass
class StepOutput:
    request_id: str
    new_token_ids: list[int]
    finished: bool
    finish_reason: str | None = None
    num_prompt_tokens: int = 0
    num_output_tokens: int = 0
    num_cached_tokens: int = 0
    text: str | None = None
    # for a request with ``logprobs``: one plain tuple (token_id, logprob, top_ids, top_lps) per id of new_token_ids
    # (plain tuples: the output stays picklable across the DP / worker pipes); None otherwise
    logprobs: list | None = None
