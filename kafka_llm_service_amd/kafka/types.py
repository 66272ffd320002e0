"""OpenAI-compatible request / response schemas (/root/reference/src/kafka/types.py:13-107).

Same field names and validation bounds (temperature in [0, 2], max_tokens > 0, top_p in [0, 1], penalties in
[-2, 2]). ``usage`` is populated from real engine token counts (quirk Q8); ``stream_options.include_usage`` adds a
final usage chunk like the OpenAI API; ``tool_choice`` / ``tools`` are accepted (the server's own tool set is used,
``tool_choice`` steers constrained decoding); ``logprobs`` / ``top_logprobs`` (0..20, only with ``logprobs: true``)
return per-token log-probabilities of the model's raw logits; ``logit_bias`` maps token ids (JSON string keys) to
biases in [-100, 100], at most 300 of them, added to the logits inside the sampler. Two fields go beyond the OpenAI
schema: ``min_p`` in [0, 1] and ``top_k`` >= 0 (0 turns either off), the sampler's other two truncation rules, and
``repetition_penalty`` in [0.1, 10] (1 or absent: off), the multiplicative penalty of HF ``generate`` / vLLM over the
tokens of the prompt and of the output so far. ``response_format``: ``{"type": "text"}`` (or absent) changes nothing;
``{"type": "json_object"}`` is JSON mode — the reply is one JSON object (the sampler masks every token that would
break RFC 8259, the mask built on the GPU: engine/json_mode.py); ``{"type": "json_schema", "json_schema": {"name"?,
"strict"?, "description"?, "schema": {...}}}`` is structured output — the reply is one JSON document that conforms to
``schema``, a schema of the supported subset (engine/json_schema.py: it is compiled here, so every unsupported
keyword and every limit is a 422 naming the keyword and its JSON pointer); enforcement is always on, whatever
``strict`` says. Any other type is refused, and so is either structured type together with ``tools`` unless
``tool_choice`` is ``"none"``.
"""
from __future__ import annotations

import math
from typing import Any, Optional

from pydantic import BaseModel, Field, field_validator, model_validator

LOGIT_BIAS_MAX = 300  # non-zero entries of one request's logit_bias (the sampler's table row, engine/logits_proc.py)


class ChatMessage(BaseModel):
    role: str
    content: Optional[str] = None
    name: Optional[str] = None
    tool_calls: Optional[list[dict[str, Any]]] = None
    tool_call_id: Optional[str] = None


class StreamOptions(BaseModel):
    include_usage: bool = False


class ChatCompletionRequest(BaseModel):
    model: str
    messages: list[ChatMessage]
    temperature: Optional[float] = Field(None, ge=0, le=2)
    max_tokens: Optional[int] = Field(None, gt=0)
    stream: Optional[bool] = False
    stop: Optional[list[str] | str] = None
    top_p: Optional[float] = Field(None, ge=0, le=1)
    frequency_penalty: Optional[float] = Field(None, ge=-2, le=2)
    presence_penalty: Optional[float] = Field(None, ge=-2, le=2)
    user: Optional[str] = None
    seed: Optional[int] = None
    stream_options: Optional[StreamOptions] = None
    tool_choice: Optional[Any] = None
    tools: Optional[list[dict[str, Any]]] = None
    # per-token log-probabilities of the model's raw logits, and the 0..20 most likely tokens at each position
    logprobs: Optional[bool] = None
    top_logprobs: Optional[int] = Field(None, ge=0, le=20)
    # token id (a base-10 string key, as JSON has it) -> bias in [-100, 100] added to that token's logit
    logit_bias: Optional[dict[str, float]] = None
    # extensions beyond the OpenAI schema, applied inside the sampler: ``min_p`` keeps the tokens whose probability is
    # at least min_p times the most likely token's (0: off); ``top_k`` keeps the k most likely tokens (0: off)
    min_p: Optional[float] = Field(None, ge=0, le=1)
    top_k: Optional[int] = Field(None, ge=0)
    # a logit x of a token the prompt or the output so far holds becomes x / r (x > 0) or x * r (x <= 0); 1: off
    repetition_penalty: Optional[float] = Field(None, ge=0.1, le=10)
    # {"type": "text"} | {"type": "json_object"} (JSON mode: the reply is one JSON object) | {"type": "json_schema",
    # "json_schema": {"schema": {...}}} (the reply conforms to the schema)
    response_format: Optional[dict[str, Any]] = None

    @field_validator("response_format")
    @classmethod
    def _response_format_type(cls, v):
        if v is None:
            return v
        t = v.get("type")
        if t == "json_schema":
            from kafka_llm_service_amd.engine.json_schema import check_name, compile_schema

            js = v.get("json_schema")
            if not isinstance(js, dict) or not isinstance(js.get("schema"), dict):
                raise ValueError('response_format type "json_schema" needs `json_schema.schema`, a schema object; for '
                                 'unconstrained JSON use "json_object"')
            if "name" in js:
                check_name(js["name"])
            compile_schema(js["schema"])  # (SchemaError is a ValueError: a 422 with the keyword and its pointer)
            return v
        if t not in ("text", "json_object"):
            raise ValueError(f'response_format type must be "text", "json_object" or "json_schema", not {t!r}')
        return v

    @field_validator("repetition_penalty", mode="before")
    @classmethod
    def _repetition_penalty_is_a_number(cls, v):
        if isinstance(v, (bool, str)):  # (pydantic would read true as 1.0 and "2" as 2.0)
            raise ValueError("repetition_penalty must be a number in [0.1, 10]")
        return v

    @field_validator("logit_bias")
    @classmethod
    def _logit_bias_bounds(cls, v):
        if v is None:
            return v
        ids = set()
        for k, b in v.items():
            if not (k.isascii() and k.isdigit()):
                raise ValueError(f"logit_bias key {k!r} is not a non-negative base-10 token id")
            if not math.isfinite(b) or not -100 <= b <= 100:
                raise ValueError(f"logit_bias value for token {k} must be a finite number in [-100, 100]")
            if b != 0:
                if int(k) in ids:
                    raise ValueError(f"logit_bias names token {int(k)} twice")
                ids.add(int(k))
        if len(ids) > LOGIT_BIAS_MAX:
            raise ValueError(f"logit_bias holds more than {LOGIT_BIAS_MAX} non-zero entries")
        return v

    @model_validator(mode="after")
    def _top_logprobs_needs_logprobs(self):
        if self.top_logprobs is not None and not self.logprobs:
            raise ValueError("top_logprobs requires logprobs to be true")
        if self.json_mode and self.tools and self.tool_choice != "none":
            raise ValueError('response_format "json_object" cannot be combined with tools unless tool_choice is '
                             '"none" (the JSON mask and the tool-call mask are not intersected)')
        if self.json_schema is not None and self.tools and self.tool_choice != "none":
            raise ValueError('response_format "json_schema" cannot be combined with tools unless tool_choice is '
                             '"none" (the schema mask and the tool-call mask are not intersected)')
        return self

    @property
    def json_schema(self) -> Optional[dict]:
        """The schema object of a ``json_schema`` response format, else None."""
        if self.response_format and self.response_format.get("type") == "json_schema":
            return self.response_format["json_schema"]["schema"]
        return None

    @property
    def json_mode(self) -> bool:
        return bool(self.response_format) and self.response_format.get("type") == "json_object"


class AgentRunRequest(BaseModel):
    messages: list[ChatMessage]
    model: str = "default"
    temperature: float = 0.7
    max_tokens: Optional[int] = None


class CreateThreadRequest(BaseModel):
    system_message: Optional[str] = None
    user_id: Optional[str] = None
    kafka_profile_id: Optional[str] = None
    metadata: Optional[dict[str, Any]] = None


class DeltaContent(BaseModel):
    role: Optional[str] = None
    content: Optional[str] = None
    tool_calls: Optional[list[dict[str, Any]]] = None


class StreamChoice(BaseModel):
    index: int = 0
    delta: DeltaContent
    finish_reason: Optional[str] = None


class StreamChunkResponse(BaseModel):
    id: str
    object: str = "chat.completion.chunk"
    created: int
    model: str
    choices: list[StreamChoice]


class MessageContent(BaseModel):
    role: str = "assistant"
    content: Optional[str] = None
    tool_calls: Optional[list[dict[str, Any]]] = None


class Choice(BaseModel):
    index: int = 0
    message: MessageContent
    finish_reason: Optional[str] = None


class Usage(BaseModel):
    prompt_tokens: int = 0
    completion_tokens: int = 0
    total_tokens: int = 0


class ChatCompletionResponse(BaseModel):
    id: str
    object: str = "chat.completion"
    created: int
    model: str
    choices: list[Choice]
    usage: Optional[Usage] = None
