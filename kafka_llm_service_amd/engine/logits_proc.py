"""Device-side logits processing: grammar bitmasks, forced tokens and presence / frequency penalties run INSIDE the
sampler kernel (``ops/csrc/sampling.hip``, RowProc), so a constrained or penalised thread no longer takes the whole
batch off the fast path (VERDICT r03 "Next round" #3).

The reference accepts ``presence_penalty`` / ``frequency_penalty`` (/root/reference/src/kafka/types.py:34-38; quirk
Q7 of SURVEY.md §2.9: accepted but never forwarded) and its agent loop decodes tool calls
(/root/reference/src/agents/base.py:372-433), which here are grammar-constrained (``engine/constrained.py``).

Per step the host builds one int32 row per sampled sequence (``proc``, 8 ints):
    [0] mode  0 none | 1 bitmask row [1] of ``mask_tab`` | 2 forced token [1] (the kernel writes it, no draw)
    [2] penalty slot: row of ``counts`` holding the sequence's generated-token counts, and of ``rep_tab`` (-1: no
        penalty)
    [3] presence, [4] frequency penalty (fp32 bits)
    [5] row of ``bias_tab`` holding the request's ``logit_bias``, [6] its entry count (0: no bias)
    [7] ``min_p``: the fp32 bits of ``float32(ln(min_p))`` (``min_p_bits``; 0: off, min_p = 1 travels as -0.0)
The kernel computes ``(y - freq * c - (c > 0 ? pres : 0)) + b`` in fp32 and applies the grammar mask after it: a
masked-out token stays -inf whatever its bias. The bias is stateless (nothing to undo on a rollback or a re-prefill).
``repetition_penalty`` r != 1 comes first (vLLM's order): ``y = x`` unless the sequence has SEEN the token — it is in
``seq.prompt_ids``, or it was drawn and not rolled back — then ``y = x * inv_r`` for ``x > 0`` and ``y = x * r``
otherwise, with ``r = float32(r)`` and ``inv_r = float32(1) / float32(r)`` computed once here: the kernel multiplies and
never divides, so ``y`` is within one fp32 ulp of HF's ``x / r``. A slot's factors are its row of ``rep_tab``; prompt
membership is the flag ``COUNT_SEEN_PROMPT`` in the slot's count words, set when the slot is assigned (the generated
count is the word's low 30 bits, "seen" is a non-zero word). Forced rows ignore it; greedy rows honour it.
``min_p`` acts on the processed row under temperature: token i is kept iff ``x_i / T >= max(x / T) + ln(min_p)`` (one
fp32 add of the host's logarithm, so the kernel, its replay and the CPU reference share one threshold bit for bit),
intersected with top-k / top-p; greedy and forced rows ignore it.
The proc rows ride in the step's single H2D upload (and in the TP plan); the two tables live on the device at fixed
addresses (hipGraph-capturable), and so does the bias table:
  * ``mask_tab`` uint32 [MASK_ROWS, ceil(V / 32)]: one row per distinct allowed set (a constraint state's cached
    vocab mask + its extra ids, or an explicit id list), LRU-managed by key; a new set costs one 16 KB row upload,
    after that the same state is a row index;
  * ``counts`` int32 [slots, V]: a slot per penalised live sequence, zeroed on (re)assignment; the sampler bumps
    ``counts[slot][token]`` with every token it draws, so the next step (stream-ordered) sees it without the host;
  * ``bias_tab`` int32 [BIAS_ROWS, 2 * LOGIT_BIAS_MAX]: one row per distinct ``logit_bias`` object — the ids in
    strictly ascending order, then the fp32 bits of their biases — keyed by content and LRU-managed like the mask
    rows: a thread sends the same object every turn, so after one 2.4 KB row upload it is a row index;
  * ``rep_tab`` fp32 [slots, 2]: ``(r, inv_r)`` of the slot's sequence, ``(1, 1)`` for a slot without the penalty.
JSON mode (``SamplingParams.json_mode``; engine/json_mode.py, ops/csrc/json_mask.hip) adds rows the LRU never hands
out: a processor built with ``json_slots`` appends that many rows to ``mask_tab`` and owns ``jstate`` int32
[json_slots, 4], one automaton state record per live JSON sequence. A JSON row is a mode-1 row naming mask row
``n_mask_rows + slot``; the mask kernel fills that row from ``jstate[slot]`` right before the sampler and the advance
kernel moves ``jstate[slot]`` over the drawn token right behind it, so the state never visits the host: such rows
carry no guard and never roll back, and two steps can be in flight. The host seeds a slot's record only when the row
is sampled from a prefill — admission, or the re-prefill after a preemption or an eviction — by walking the output ids
so far (all landed by then) through ``ref.json_advance_ref``.
Structured outputs (``SamplingParams.json_schema``; engine/json_schema.py, ops/csrc/table_grammar.hip) share those slots
and mask rows: a schema row's record is ``(state, 0, 0, table index + 1)``, and its kernels walk the request's own
transition table out of a device pool of ``json_slots`` buffers (``ops.SchemaTables``: 64 MiB at 256 slots, allocated
by the first schema request — schema steps never run inside a graph, so no captured graph needs the address). Tables
are keyed by the schema's canonical text and refcounted by live sequences; unreferenced ones stay resident in LRU
order, so a thread that sends the same schema every turn uploads it once. With as many buffers as state slots a live
sequence always finds one. A new table travels in ``ProcUpdates.schema_tabs`` and is loaded on every TP rank.
The automaton tool grammar (``SamplingParams.tool_plan``; engine/tool_automaton.py, the same kernels) takes a
slot and a mask row from the same space and a buffer of the same pool, under a key no schema text equals; its record is
``(state, phase, 0, table index + 1)``, seeded as TOOL_FREE or TOOL_OPEN and replayed over the landed output ids after a
preemption. Under ``tool_choice: "auto"`` the host drops the row from the tool rows once the first output id has landed
and does not open a call: from then on it is an unconstrained row. New tables, seeds and the row list ride in
``ProcUpdates.tool_tabs`` / ``tool_slots`` / ``tool_states`` and ``SampleParams.tool_rows``.
Table writes (new mask rows, slot zeroing, count decrements of rolled-back tokens) are ``ProcUpdates`` applied on the stream before the step's sampler — on
every TP rank, from the same plan, so every rank samples the same token.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import numpy as np
import torch

# (the update record travels in a step's wire format)
from kafka_llm_service_amd.engine.step_plan import (BIAS_ROW_INTS, COUNT_SEEN_PROMPT, JSON_STATE_INTS, LOGIT_BIAS_MAX,
                                                    ProcUpdates)
from kafka_llm_service_amd.engine.json_schema import DEAD as SCHEMA_DEAD, SCHEMA_MAX_STATES
from kafka_llm_service_amd.engine.tool_automaton import TOOL_PHASES, tool_row_live

MASK_ROWS = 512
BIAS_ROWS = 512


def pack_bits(keep: np.ndarray, words: int) -> np.ndarray:
    """bool [V] -> int32 [words] with bit j of word w = keep[32 w + j] (the kernel's layout)."""
    b = np.zeros(words * 32, dtype=bool)
    b[:keep.shape[0]] = keep
    return np.packbits(b, bitorder="little").view("<u4").view(np.int32)


def spec_forced(spec) -> int | None:
    """The one token a constraint spec allows (a single-id list), else None."""
    if isinstance(spec, (list, tuple)) and len(spec) == 1:
        return int(spec[0])
    return None


def min_p_bits(min_p: float) -> int:
    """``proc[7]`` of a row: the int32 bits of ``float32(ln(min_p))``; 0 for min_p = 0 (off). ln(1) = 0 is sent as
    -0.0 (0x80000000), which keeps "on" apart from "off" and adds the same."""
    if not 0.0 <= min_p <= 1.0:  # (a NaN fails both comparisons)
        raise ValueError("min_p must lie in [0, 1]")
    if min_p == 0.0:
        return 0
    lmp = np.float32(math.log(min_p))
    return int((-np.float32(0.0) if lmp == 0 else lmp).view(np.int32))


def rep_factors(r: float) -> np.ndarray:
    """A slot's ``rep_tab`` row ``(float32(r), float32(1) / float32(r))``: the reciprocal is one fp32 division on the
    host, and the kernel, its replay and the CPU reference multiply by it — within one fp32 ulp of ``x / r``."""
    if isinstance(r, bool) or not 0.1 <= r <= 10.0:  # (a NaN fails both comparisons)
        raise ValueError("repetition_penalty must lie in [0.1, 10]")
    r32 = np.float32(r)
    return np.array([r32, np.float32(1.0) / r32], dtype=np.float32)


class LogitsProcessor:
    def __init__(self, device: torch.device, vocab: int, max_slots: int = 256, mask_rows: int = MASK_ROWS,
                 bias_rows: int = BIAS_ROWS, json_slots: int = 0):
        self.device = torch.device(device)
        self.V = vocab
        self.W = -(-vocab // 32)
        self.cnt_ld = -(-vocab // 8) * 8
        self.n_mask_rows = mask_rows
        self.n_bias_rows = bias_rows
        self.max_slots = max_slots
        self.mask_tab: torch.Tensor | None = None
        self.counts: torch.Tensor | None = None
        self.bias_tab: torch.Tensor | None = None
        self.rep_tab: torch.Tensor | None = None
        self._rows: OrderedDict = OrderedDict()  # key -> mask row (LRU order)
        self._brows: OrderedDict = OrderedDict()  # ("B", ((id, bias), ...)) -> bias row (LRU order)
        self._slots: dict[int, tuple[int, object]] = {}  # seq_id -> (slot, seq)
        self._free: list[int] = list(range(max_slots - 1, -1, -1))
        # slots whose rep_tab row holds r != 1, as apply() has written them: the same on every TP rank
        self._rep_slots: set[int] = set()
        self._rep_seqs: dict[int, object] = {}  # seq_id -> seq of the sequences build() has seeded a slot for
        self._dec: list[tuple[int, int]] = []  # (slot, token) decrements queued by uncount()
        # JSON mode: state-table slots (mask rows n_mask_rows + slot), the token table and its device copy
        self.n_json_slots = json_slots
        self.jstate: torch.Tensor | None = None
        self._jslots: dict[int, tuple[int, object]] = {}  # seq_id -> (slot, seq)
        self._jfree: list[int] = list(range(json_slots - 1, -1, -1))
        self.json_table_fn = None  # () -> engine/json_mode.JsonTable of the model's tokenizer (set by the engine)
        self._json_table = None
        self._json_dev = None
        # json_schema: the table pool (device side: apply(); host side: build()). _stabs: schema text -> buffer, in
        # LRU order of last use; a buffer with _stab_refs 0 may be given to another schema
        self.spool = None
        self._stabs: OrderedDict = OrderedDict()
        self._stab_refs: dict[int, int] = {}
        self._stab_free: list[int] = list(range(json_slots - 1, -1, -1))
        self._sseq: dict[int, int] = {}  # seq_id -> buffer of the sequences that hold a reference
        self._slot_tab = np.full(max(1, json_slots), -1, dtype=np.int32)  # slot -> buffer (-1: a JSON-mode slot)
        # slot -> (open id, close id) of an automaton tool row (engine/tool_automaton.py), -1 for every other slot
        self._slot_tool = np.full((max(1, json_slots), 2), -1, dtype=np.int32)
        self.stats = {"mask_uploads": 0, "proc_steps": 0, "forced_rows": 0, "mask_rows_used": 0, "penalty_rows": 0,
                      "bias_uploads": 0, "bias_rows_used": 0, "min_p_rows": 0, "rep_rows": 0, "seen_uploads": 0,
                      "json_rows": 0, "json_seeds": 0, "schema_rows": 0, "schema_seeds": 0,
                      "schema_table_uploads": 0, "tool_rows": 0, "tool_seeds": 0}

    # ---- tables (allocated together on first use: a captured graph sees every address) --------------------------
    def tables(self) -> tuple[torch.Tensor, torch.Tensor]:
        if self.mask_tab is None:
            self.mask_tab = torch.zeros(self.n_mask_rows + self.n_json_slots, self.W, dtype=torch.int32,
                                        device=self.device)
            self.jstate = torch.zeros(max(1, self.n_json_slots), JSON_STATE_INTS, dtype=torch.int32,
                                      device=self.device)
            self.counts = torch.zeros(self.max_slots, self.cnt_ld, dtype=torch.int32, device=self.device)
            self.bias_tab = torch.zeros(self.n_bias_rows, BIAS_ROW_INTS, dtype=torch.int32, device=self.device)
            self.rep_tab = torch.ones(self.max_slots, 2, dtype=torch.float32, device=self.device)
        return self.mask_tab, self.counts

    def bias_table(self) -> torch.Tensor:
        """The logit-bias table (allocated with the other two)."""
        self.tables()
        return self.bias_tab

    def rep_table(self) -> torch.Tensor:
        """The repetition-penalty table (allocated with the other three)."""
        self.tables()
        return self.rep_tab

    def live_rep_table(self) -> torch.Tensor | None:
        """The table while some slot holds a factor r != 1, else None: the sampler is then launched without it and
        runs the kernel that knows no repetition penalty (a step's updates are applied before its sampler, so the
        answer is the step's, and every TP rank gives the same one)."""
        return self.rep_table() if self._rep_slots else None

    # ---- JSON mode ----------------------------------------------------------------------------------------------
    def set_json_table(self, table) -> None:
        """The token table (engine/json_mode.JsonTable) the JSON rows of this processor are walked over."""
        if table.V != self.V:
            raise ValueError(f"JSON token table holds {table.V} ids, the vocabulary {self.V}")
        if table is not self._json_table:
            self._json_table, self._json_dev = table, None

    def json_table(self):
        if self._json_table is None:
            if self.json_table_fn is None:
                raise RuntimeError("JSON mode needs a token table (LogitsProcessor.set_json_table)")
            self.set_json_table(self.json_table_fn())
        return self._json_table

    def json_tables(self):
        """The device copy of the token table and the automaton (ops.JsonTables), made once."""
        if self._json_dev is None:
            from kafka_llm_service_amd import ops

            self._json_dev = ops.JsonTables(self.json_table(), self.device)
        return self._json_dev

    def grammar_rows(self, proc: np.ndarray | None) -> tuple:
        """The grammar rows of ``proc`` (mode-1 rows naming a mask row behind the LRU-managed ones), split by what
        their slot holds: (JSON int32 [k, 2], schema [k, 3], tool [k, 5]), each the leading columns of (sampled row,
        state slot, table buffer, open id, close id), or None where there is no such row."""
        if proc is None or not self.n_json_slots:
            return None, None, None
        idx = np.flatnonzero((proc[:, 0] == 1) & (proc[:, 1] >= self.n_mask_rows))
        slots = proc[idx, 1] - self.n_mask_rows
        tab, tool = self._slot_tab[slots], self._slot_tool[slots]
        full = np.concatenate([np.stack([idx, slots, tab], axis=1), tool], axis=1).astype(np.int32)
        is_tool = tool[:, 0] >= 0  # (a tool row has a table too, and is not a schema row)
        return tuple(np.ascontiguousarray(full[m, :w]) if m.any() else None
                     for m, w in ((tab < 0, 2), ((tab >= 0) & ~is_tool, 3), (is_tool, 5)))

    def json_rows(self, proc: np.ndarray | None) -> np.ndarray | None:
        """int32 [k, 2] (sampled row, state slot) of the JSON-mode rows of ``proc``, or None."""
        return self.grammar_rows(proc)[0]

    def schema_rows(self, proc: np.ndarray | None) -> np.ndarray | None:
        """int32 [k, 3] (sampled row, state slot, table buffer) of the json_schema rows of ``proc``, or None."""
        return self.grammar_rows(proc)[1]

    def tool_rows(self, proc: np.ndarray | None) -> np.ndarray | None:
        """int32 [k, 5] (sampled row, state slot, table buffer, open id, close id) of the automaton tool rows of
        ``proc``, or None."""
        return self.grammar_rows(proc)[2]

    def _json_reclaim(self) -> None:
        """The slots, and the table references, of sequences that have finished since."""
        for sid in [sid for sid, (_, s) in self._jslots.items() if s.finished]:
            slot = self._jslots.pop(sid)[0]
            self._jfree.append(slot)
            self._slot_tab[slot] = -1
            self._slot_tool[slot] = -1
            buf = self._sseq.pop(sid, None)
            if buf is not None:
                self._stab_refs[buf] -= 1

    def _schema_table(self, seq, new_tabs: list, key=None, dfa=None) -> int:
        """The pool buffer of the sequence's schema; a schema the pool does not hold takes a free buffer or the least
        recently used unreferenced one, and its table joins ``new_tabs``. A tool row's body shares the pool under
        ``key`` (a tuple, so no schema text equals it) with the automaton ``dfa`` it is already compiled to."""
        from kafka_llm_service_amd.engine.json_schema import compile_text

        buf = self._sseq.get(seq.seq_id)
        if buf is not None:
            return buf
        text = seq.params.json_schema if key is None else key
        buf = self._stabs.get(text)
        if buf is None:
            if not self._stab_free:
                self._json_reclaim()
                victim = next((t for t, b in self._stabs.items() if not self._stab_refs.get(b)), None)
                if victim is None:  # (as many buffers as slots, a slot holder references one: cannot happen)
                    raise RuntimeError("logits processor: every schema table buffer is referenced")
                self._stab_free.append(self._stabs.pop(victim))
            buf = self._stab_free.pop()
            dfa = compile_text(text) if dfa is None else dfa
            self._stabs[text] = buf
            new_tabs.append((buf, dfa.cls, dfa.trans))
            self.stats["schema_table_uploads"] += 1
        self._stabs.move_to_end(text)
        self._stab_refs[buf] = self._stab_refs.get(buf, 0) + 1
        self._sseq[seq.seq_id] = buf
        return buf

    @staticmethod
    def _replay(seq, start, step):
        """``start`` moved by ``step(state, id)`` over the sequence's output ids so far — the only place the host
        computes a grammar state (all ids have landed when a prefill is sampled)."""
        st = start
        for t in seq.output_ids:
            if t < 0:
                raise RuntimeError("grammar rows: a state is seeded from landed tokens only")
            st = step(st, t)
        return st

    def json_seed(self, seq) -> np.ndarray:
        """The JSON-mode row's state record after the sequence's output ids so far."""
        from kafka_llm_service_amd.engine import json_mode as jm
        from kafka_llm_service_amd.ops import reference as ref

        table = self.json_table()
        return jm.state_record(self._replay(seq, jm.START_STATE, lambda st, t: ref.json_advance_ref(st, t, table)))

    def schema_seed(self, seq, buf: int) -> np.ndarray:
        """The schema row's record after the sequence's output ids so far."""
        from kafka_llm_service_amd.engine import json_schema as js
        from kafka_llm_service_amd.ops import reference as ref

        table, dfa = self.json_table(), js.compile_text(seq.params.json_schema)
        return js.state_record(self._replay(seq, js.START, lambda st, t: ref.schema_advance_ref(st, t, dfa, table)),
                               buf)

    def tool_seed(self, seq, buf: int) -> np.ndarray:
        """The tool row's record after the sequence's output ids so far: the phase its ``tool_choice`` starts in,
        replayed through ``ref.tool_advance_ref``."""
        from kafka_llm_service_amd.engine import tool_automaton as ta
        from kafka_llm_service_amd.engine.json_schema import START
        from kafka_llm_service_amd.ops import reference as ref

        plan, table = seq.params.tool_plan, self.json_table()
        return self._replay(seq, ta.tool_record(START, plan.phase0, buf),
                            lambda rec, t: ref.tool_advance_ref(rec, t, plan.open, plan.close, plan.dfa, table))

    def schema_pool(self):
        """The device pool of schema tables (ops.SchemaTables), allocated by the first schema step."""
        if self.spool is None:
            from kafka_llm_service_amd import ops

            self.spool = ops.SchemaTables(max(1, self.n_json_slots), self.device)
        return self.spool

    def _json_slot(self, seq) -> tuple[int, bool]:
        e = self._jslots.get(seq.seq_id)
        if e is not None:
            return e[0], False
        if not self._jfree:  # reclaim the slots of sequences that have finished since
            self._json_reclaim()
        if not self._jfree:
            raise RuntimeError(f"logits processor: more than {self.n_json_slots} live JSON-mode sequences")
        slot = self._jfree.pop()
        self._jslots[seq.seq_id] = (slot, seq)
        return slot, True

    def _grammar_row(self, proc: np.ndarray, i: int, seq, kind: str, seed_row: bool, slots: list, states: list,
                     pool: tuple | None = None, envelope: tuple | None = None) -> None:
        """Row ``i`` of ``proc`` becomes the ``kind`` ("json", "schema", "tool") row of ``seq``: a mode-1 row naming
        the mask row of the sequence's state slot. A table row takes its pool buffer through ``pool``, the arguments
        of ``_schema_table`` behind the sequence; a tool row records its ``envelope`` (open id, close id). A slot
        assigned here, or a row sampled from a prefill (``seed_row``), has its record seeded: it joins ``slots`` /
        ``states``."""
        slot, new_slot = self._json_slot(seq)
        seed_args = (seq,)
        if pool is not None:
            buf = self._slot_tab[slot] = self._schema_table(seq, *pool)
            seed_args = (seq, buf)
        if envelope is not None:
            self._slot_tool[slot] = envelope
        if new_slot or seed_row:
            slots.append(slot)
            states.append(getattr(self, kind + "_seed")(*seed_args))
            self.stats[kind + "_seeds"] += 1
        proc[i, 0], proc[i, 1] = 1, self.n_mask_rows + slot
        self.stats[kind + "_rows"] += 1

    # ---- host side ----------------------------------------------------------------------------------------------
    def _table_row(self, lru: OrderedDict, n_rows: int, key, words_fn, upd_rows: list, upd_words: list, used: set,
                   stat: str) -> int:
        """The table row of ``key`` in ``lru`` (a table of ``n_rows`` rows); a new key takes a free row or evicts the
        least recently used one, and its words (``words_fn()``) join the step's updates."""
        r = lru.get(key)
        if r is not None:
            lru.move_to_end(key)
            used.add(r)
            return r
        if len(lru) < n_rows:
            r = len(lru)
        else:  # evict the least recently used key not needed by this step (a step has <= max_slots rows)
            for k in lru:
                if lru[k] not in used:
                    r = lru.pop(k)
                    break
            else:  # pragma: no cover - more distinct sets in one step than table rows
                raise RuntimeError("logits processor: more distinct sets in one step than table rows")
        lru[key] = r
        used.add(r)
        upd_rows.append(r)
        upd_words.append(words_fn())
        self.stats[stat] += 1
        return r

    def _mask_row(self, key, bits_fn, upd_rows: list, upd_words: list, used: set) -> int:
        return self._table_row(self._rows, self.n_mask_rows, key, bits_fn, upd_rows, upd_words, used, "mask_uploads")

    def _bias_row(self, pairs: tuple, upd_rows: list, upd_words: list, used: set) -> int:
        def words(pairs=pairs):
            w = np.zeros(BIAS_ROW_INTS, dtype=np.int32)
            w[:len(pairs)] = [t for t, _ in pairs]
            w[LOGIT_BIAS_MAX:LOGIT_BIAS_MAX + len(pairs)] = np.array([b for _, b in pairs],
                                                                      dtype=np.float32).view(np.int32)
            return w
        return self._table_row(self._brows, self.n_bias_rows, ("B", pairs), words, upd_rows, upd_words, used,
                               "bias_uploads")

    def _slot(self, seq, zero: list) -> tuple[int, bool]:
        """(the sequence's count-table slot, whether this call assigned it — such a slot joins ``zero``)."""
        e = self._slots.get(seq.seq_id)
        if e is not None:
            return e[0], False
        if not self._free:  # reclaim the slots of sequences that have finished since
            for sid in [sid for sid, (_, s) in self._slots.items() if s.finished]:
                self._free.append(self._slots.pop(sid)[0])
        if not self._free:
            raise RuntimeError(f"logits processor: more than {self.max_slots} live penalised sequences")
        slot = self._free.pop()
        self._slots[seq.seq_id] = (slot, seq)
        if slot not in zero:  # (a slot _release_finished_rep freed in this very step is already there)
            zero.append(slot)
        return slot, True

    def _release_finished_rep(self, zero: list) -> None:
        """Frees the slots of finished sequences that had a repetition penalty and clears them with this step's
        updates, so that ``live_rep_table`` turns None — on every rank — as soon as no such request is left, not only
        when the slot is needed again."""
        for sid in [sid for sid, s in self._rep_seqs.items() if s.finished]:
            del self._rep_seqs[sid]
            e = self._slots.pop(sid, None)
            if e is not None:
                self._free.append(e[0])
                zero.append(e[0])

    def uncount(self, seq, token: int) -> None:
        """A drawn token the engine discarded (grammar rollback, engine.py ``_finish_step``): the sampler already
        bumped ``counts[slot][token]``, so the next table update takes it back — otherwise the row keeps penalising a
        token that is not in its output. Queued on the host; applied by the next step that samples a processed row
        (every later sample of a penalised sequence is such a row), before its sampler."""
        e = self._slots.get(seq.seq_id)
        if e is not None and 0 <= int(token) < self.V:
            self._dec.append((e[0], int(token)))

    def build(self, rows: list[tuple[int, object, object]], n: int,
              n_decode: int | None = None) -> tuple[np.ndarray, ProcUpdates]:
        """``rows``: (row, seq, constraint spec) for every sampled row that needs processing (spec None, a list of
        allowed ids, or a constrained.Mask); ``n`` rows in the step, the first ``n_decode`` of them decode rows (None:
        all — only JSON rows care: one sampled from a prefill has its state seeded). Returns (proc int32 [n, 8], table
        updates)."""
        from kafka_llm_service_amd.engine.constrained import Mask

        self.tables()
        proc = np.zeros((n, 8), dtype=np.int32)
        proc[:, 2] = -1
        upd_rows, upd_words, zero, used = [], [], [], set()
        b_rows, b_words, b_used = [], [], set()
        seen = []  # (slot, (r, inv_r), ascending distinct prompt ids) of the slots this step seeds
        j_slots, j_states, s_tabs = [], [], []
        t_slots, t_states, t_tabs = [], [], []
        if self._rep_seqs:
            self._release_finished_rep(zero)
        V, W = self.V, self.W
        for i, s, spec in rows:
            p = s.params
            from_prefill = n_decode is not None and i >= n_decode  # (a grammar row's record is then seeded)
            if spec is not None:
                forced = spec_forced(spec)
                if forced is not None:
                    if not 0 <= forced < V:
                        raise ValueError(f"constraint forces token {forced} outside [0, {V})")
                    proc[i, 0], proc[i, 1] = 2, forced
                    self.stats["forced_rows"] += 1
                elif isinstance(spec, Mask):
                    extra = tuple(sorted(set(int(e) for e in spec.extra)))
                    if any(not 0 <= e < V for e in extra):
                        raise ValueError("constraint mask names a token outside the vocabulary")

                    def bits(m=spec, ex=extra):
                        keep = np.asarray(m.base[:V], dtype=bool).copy()
                        keep[list(ex)] = True
                        return pack_bits(keep, W)
                    proc[i, 0], proc[i, 1] = 1, self._mask_row(("M", spec.key, extra), bits, upd_rows, upd_words,
                                                               used)
                    self.stats["mask_rows_used"] += 1
                else:
                    ids = tuple(sorted(set(int(t) for t in spec)))
                    if not ids or any(not 0 <= t < V for t in ids):
                        raise ValueError(f"constraint allows no token / a token outside [0, {V})")

                    def bits(ids=ids):
                        keep = np.zeros(V, dtype=bool)
                        keep[list(ids)] = True
                        return pack_bits(keep, W)
                    proc[i, 0], proc[i, 1] = 1, self._mask_row(("L",) + ids, bits, upd_rows, upd_words, used)
                    self.stats["mask_rows_used"] += 1
            if getattr(p, "json_mode", False):
                if spec is not None:
                    raise ValueError("JSON mode and a token constraint on one row: the masks are not intersected")
                self._grammar_row(proc, i, s, "json", from_prefill, j_slots, j_states)
            if getattr(p, "json_schema", None) is not None:
                if spec is not None or getattr(p, "json_mode", False):
                    raise ValueError("json_schema and another token mask on one row: the masks are not intersected")
                self._grammar_row(proc, i, s, "schema", from_prefill, j_slots, j_states, (s_tabs,))
            plan = getattr(p, "tool_plan", None)
            if plan is not None and tool_row_live(plan, s.output_ids):
                if spec is not None or getattr(p, "json_mode", False) or getattr(p, "json_schema", None) is not None:
                    raise ValueError("the automaton tool grammar and another token mask on one row: the masks are "
                                     "not intersected")
                if not (0 <= plan.open < V and 0 <= plan.close < V):
                    raise ValueError("tool grammar: the envelope's tokens lie outside the vocabulary")
                self._grammar_row(proc, i, s, "tool", from_prefill, t_slots, t_states, (t_tabs, plan.key, plan.dfa),
                                  (plan.open, plan.close))
            rep = p.repetition_penalty
            if p.presence_penalty or p.frequency_penalty or rep != 1.0:
                proc[i, 2], new_slot = self._slot(s, zero)
                if p.presence_penalty or p.frequency_penalty:
                    proc[i, 3:5] = np.array([p.presence_penalty, p.frequency_penalty], dtype=np.float32).view(np.int32)
                    self.stats["penalty_rows"] += 1
                if rep != 1.0:
                    self.stats["rep_rows"] += 1
                    if new_slot:  # its factors and its prompt's flags (a preempted or re-prefilled sequence keeps
                        # its slot and is not seeded again)
                        ids = np.unique(np.asarray(s.prompt_ids, dtype=np.int64))
                        seen.append((int(proc[i, 2]), rep_factors(rep), ids[(ids >= 0) & (ids < V)].astype(np.int32)))
                        self.stats["seen_uploads"] += 1
                        self._rep_seqs[s.seq_id] = s
            bias = getattr(p, "logit_bias", None)
            if bias:
                pairs = tuple(sorted((int(t), float(b)) for t, b in bias if float(b) != 0.0))
                ids = [t for t, _ in pairs]
                if len(pairs) > LOGIT_BIAS_MAX:
                    raise ValueError(f"logit_bias holds {len(pairs)} entries, more than {LOGIT_BIAS_MAX}")
                if any(not 0 <= t < V for t in ids) or len(set(ids)) != len(ids):
                    raise ValueError(f"logit_bias names a token outside [0, {V}) or names one twice")
                if pairs:
                    proc[i, 5], proc[i, 6] = self._bias_row(pairs, b_rows, b_words, b_used), len(pairs)
                    self.stats["bias_rows_used"] += 1
            min_p = getattr(p, "min_p", 0.0)
            if min_p:
                proc[i, 7] = min_p_bits(float(min_p))
                self.stats["min_p_rows"] += 1
        self.stats["proc_steps"] += 1
        upd = ProcUpdates()
        if upd_rows:
            upd.mask_rows = np.asarray(upd_rows, dtype=np.int32)
            upd.mask_words = np.stack(upd_words).astype(np.int32, copy=False)
        if zero:
            upd.zero_slots = np.asarray(zero, dtype=np.int32)
        if self._dec:
            upd.dec = np.asarray(self._dec, dtype=np.int32).reshape(-1, 2)
            self._dec = []
        if b_rows:
            upd.bias_rows = np.asarray(b_rows, dtype=np.int32)
            upd.bias_words = np.stack(b_words)
        if seen:
            upd.seen_slots = np.asarray([sl for sl, _, _ in seen], dtype=np.int32)
            upd.rep_vals = np.stack([f for _, f, _ in seen])
            upd.seen_off = np.concatenate([[0], np.cumsum([ids.size for _, _, ids in seen])]).astype(np.int32)
            upd.seen_ids = np.concatenate([ids for _, _, ids in seen]).astype(np.int32)
        if j_slots:
            upd.json_slots = np.asarray(j_slots, dtype=np.int32)
            upd.json_states = np.stack(j_states).astype(np.int32)
        upd.schema_tabs = s_tabs
        upd.tool_tabs = t_tabs
        if t_slots:
            upd.tool_slots = np.asarray(t_slots, dtype=np.int32)
            upd.tool_states = np.stack(t_states).astype(np.int32)
        return proc, upd

    # ---- device side ----------------------------------------------------------------------------------------------
    def _write_records(self, what: str, slots: np.ndarray, st, json_ok: bool, phases: int, upload) -> None:
        """The records ``st`` [k, 4] into the slots ``slots`` of the state table, checked first. A record whose word 3
        is 0 is a JSON-mode record (state, depth, stack bits, 0), taken only with ``json_ok``; every other one is a
        table record (state, phase < ``phases``, 0, buffer + 1): a schema record with ``phases`` 1, a tool record with
        TOOL_PHASES."""
        if not slots.size:
            return
        st = np.asarray(st)
        ok = st.shape == (slots.size, JSON_STATE_INTS) and int(slots.min()) >= 0 \
            and int(slots.max()) < self.n_json_slots
        if ok:
            tabrec = st[:, 3] != 0 if json_ok else np.ones(len(st), dtype=bool)
            jm_st, tb = st[~tabrec], st[tabrec]
            ok = not ((jm_st[:, 0] < 0) | (jm_st[:, 0] > 63) | (jm_st[:, 1] < 0) | (jm_st[:, 1] > 32)).any() and not (
                (tb[:, 0] < 0) | ((tb[:, 0] >= SCHEMA_MAX_STATES) & (tb[:, 0] != SCHEMA_DEAD)) | (tb[:, 1] < 0)
                | (tb[:, 1] >= phases) | (tb[:, 2] != 0) | (tb[:, 3] < 1) | (tb[:, 3] > self.n_json_slots)).any()
        if not ok:
            raise ValueError(f"logits processor: {what} update does not fit the state table")
        self.jstate.index_copy_(0, upload(slots.astype(np.int64)), upload(np.ascontiguousarray(st, dtype=np.int32)))

    def apply(self, upd: ProcUpdates | None, upload) -> None:
        """Stream-ordered table writes (``upload``: numpy -> device tensor, e.g. the runner's staging ring)."""
        if upd is None or upd.empty:
            return
        mask_tab, counts = self.tables()
        for buf, cls, trans in (*upd.schema_tabs, *upd.tool_tabs):  # (checked by the pool: the kernels trust a table)
            self.schema_pool().load(int(buf), cls, trans, upload)
        self._write_records("tool record", upd.tool_slots, upd.tool_states, False, TOOL_PHASES, upload)
        self._write_records("JSON state", upd.json_slots, upd.json_states, True, 1, upload)
        if upd.mask_rows.size:
            if int(upd.mask_rows.max()) >= self.n_mask_rows or upd.mask_words.shape[1] != mask_tab.shape[1]:
                raise ValueError("logits processor: mask update does not fit the table")
            rows = upload(upd.mask_rows.astype(np.int64))
            mask_tab.index_copy_(0, rows, upload(upd.mask_words))
        if upd.bias_rows.size:
            bias_tab = self.bias_table()
            if int(upd.bias_rows.min()) < 0 or int(upd.bias_rows.max()) >= bias_tab.shape[0] \
                    or upd.bias_words.shape != (upd.bias_rows.size, bias_tab.shape[1]):
                raise ValueError("logits processor: logit-bias update does not fit the table")
            bias_tab.index_copy_(0, upload(upd.bias_rows.astype(np.int64)), upload(upd.bias_words))
        if upd.dec.size:  # before the zeroing: a recycled slot starts from zero whatever was queued for it
            if int(upd.dec[:, 0].max()) >= counts.shape[0] or int(upd.dec[:, 1].max()) >= counts.shape[1]:
                raise ValueError("logits processor: count decrement outside the count table")
            flat = upd.dec[:, 0].astype(np.int64) * counts.shape[1] + upd.dec[:, 1]
            idx = upload(flat)
            counts.view(-1).index_add_(0, idx, torch.full(idx.shape, -1, dtype=counts.dtype, device=counts.device))
        if upd.zero_slots.size:
            if int(upd.zero_slots.max()) >= counts.shape[0]:
                raise ValueError("logits processor: penalty slot outside the count table")
            slots = upload(upd.zero_slots.astype(np.int64))
            counts.index_fill_(0, slots, 0)
            self.rep_table().index_fill_(0, slots, 1.0)  # a recycled slot inherits no factor: (1, 1) until seeded
            self._rep_slots.difference_update(upd.zero_slots.tolist())
        if upd.seen_slots.size:  # after the zeroing: the prompt's flags, then the slot's (r, inv_r)
            upd.check_seen()
            rep_tab = self.rep_table()
            sl = upd.seen_slots.astype(np.int64)
            if int(sl.min()) < 0 or int(sl.max()) >= min(counts.shape[0], rep_tab.shape[0]) \
                    or (upd.seen_ids.size and (int(upd.seen_ids.min()) < 0 or int(upd.seen_ids.max()) >= self.V)) \
                    or not np.isfinite(upd.rep_vals).all() or (upd.rep_vals <= 0).any():
                raise ValueError("logits processor: repetition-penalty update does not fit the tables")
            if upd.seen_ids.size:
                flat = np.repeat(sl, np.diff(upd.seen_off)) * counts.shape[1] + upd.seen_ids
                counts.view(-1).index_fill_(0, upload(flat), COUNT_SEEN_PROMPT)
            rep_tab.index_copy_(0, upload(sl), upload(np.ascontiguousarray(upd.rep_vals, dtype=np.float32)))
            self._rep_slots.difference_update(sl.tolist())
            self._rep_slots.update(int(s) for s, r in zip(sl, upd.rep_vals[:, 0]) if r != 1.0)
