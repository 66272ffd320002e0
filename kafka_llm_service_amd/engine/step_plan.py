"""Host-side plan of one engine step: the attention work items of its three launches (cascade prefix pass, decode,
prefill tiles), the layout of the two packed buffers that carry it to the device, and the wire format a TP leader
ships to its followers.

Pure arithmetic on lengths and block tables (numpy only): sequences, the KV manager and device tensors stay in
``engine/model_runner.py``, whose ``build_host`` packs tokens and slots and calls ``plan_attention``. The records
below carry the field names of ``ops/csrc/kafka_abi.h`` (AttnWorkItem, DecodeItem). The planning loops build plain
tuples in the records' field order (a NamedTuple costs three times a tuple to make, which a step of a few hundred
tiles notices) and read them by unpacking or through the index records TILE, ITEM and DEC.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import NamedTuple

import numpy as np

ITEM_INTS = 8          # int32 fields of one work item (kafka_abi.h ITEM_INTS): a row of the device items tensors
MAX_ITEM_KEYS = 32000  # key range of one attention work item (page ids of an item are staged in 8 KB of LDS)
MIN_DECODE_KEYS = 256      # smallest key range of one decode work item
# decode workgroups per launch (items x Hkv) the suffix pieces are sized for; 0 = one item per row (no split
# unless a row alone would leave most CUs idle)
# 1,344 with the decode kernel at three workgroups per CU (768 slots): 1,152 was +1.6 % over 768 and 1,344 another
# +0.2-0.4 % over 1,152, same boxes (profiles/r03/decode_occ3/decode_target_ab_*.jsonl; 768 was best at two per CU,
# profiles/r02/decode_items_ab.jsonl)
DECODE_TARGET_ITEMS = 1344  # (768 / 1536 / 2304 lose to it: profiles/r04/bench_ab_decode_target_blas.jsonl)
MAX_PARTIALS = 64           # partial slots per row that the decode kernel's fused merge reads (one lane each)
MAX_PREFIX_CHUNKS = 32
LOGIT_BIAS_MAX = 300                # entries of one request's logit_bias (kafka_abi.h LOGIT_BIAS_MAX)
BIAS_ROW_INTS = 2 * LOGIT_BIAS_MAX  # one row of the sampler's bias table: ids, then the fp32 bits of their biases
COUNT_SEEN_PROMPT = 1 << 30         # flag of a prompt token in the sampler's count table (kafka_abi.h)
JSON_STATE_INTS = 4                 # a JSON-mode row's device state record (kafka_abi.h; engine/json_mode.py)


def cdiv(a, b):
    return -(-a // b)


# ---- records ------------------------------------------------------------------------------------------------------
class Tile(NamedTuple):
    """Query tokens [q0, q0 + count) of the step's prefill rows against keys [lo, extent) of block-table row
    ``bt_row``: ``extent`` = the tile's last position + 1, ``hi`` = key bound of its chunk. ``lo`` > 0: the keys below
    it were attended by the cascade prefix pass, whose partials sit in slots [0, s0) of the tile's rows."""
    q0: int
    count: int
    bt_row: int
    extent: int
    hi: int
    lo: int = 0
    s0: int = 0


class TileItem(NamedTuple):
    """One row of the prefix / prefill items tensors (kafka_abi.h AttnWorkItem)."""
    q_start: int
    q_count: int
    bt_row: int
    kv_lo: int
    kv_hi: int
    split: int    # -1: normalised bf16 rows; >= 0: partial slot
    alt: int = 0  # != 0: the partial goes to the launch's alt buffer (prefill rows riding in the prefix pass)
    pad: int = 0


class Group(NamedTuple):
    """A cascade group: ``rows`` contiguous decode rows whose block tables start with the same ``pages`` pages."""
    rows: int
    pages: int


class DecodeItem(NamedTuple):
    """One row of the decode items tensor (kafka_abi.h DecodeItem): keys [lo, hi) of row b, piece ``split`` of
    ``nsplit`` behind ``npre`` prefix partials; split -1 = null item."""
    b: int
    lo: int
    hi: int
    split: int
    nsplit: int
    npre: int
    pad0: int = 0
    pad1: int = 0


# index of each field: t[TILE.extent], it[ITEM.kv_lo], column DEC.split of an int32 [n, ITEM_INTS] decode items array
TILE = Tile(*range(len(Tile._fields)))
ITEM = TileItem(*range(ITEM_INTS))
DEC = DecodeItem(*range(ITEM_INTS))


# ---- the packed step and its layout -------------------------------------------------------------------------------
@dataclass
class HostStep:
    """Host-side plan of one step: the packed int64 and int32 buffers (sections: ``i64_sections``, ``i32_sections``)
    and the scalars that fix their layout."""
    B: int = 0
    T: int = 0
    nbt: int = 1
    bt_w: int = 1           # block-table columns (pages of the longest row of the step; a bucket under graphs)
    bt_need: int = 0        # columns holding pages (<= bt_w): what a broadcast plan actually ships
    n_rows: int = 0
    s_total: int = 1        # partial slots per decode row (cascade prefix chunks + suffix pieces)
    n_dec_items: int = 0
    n_prefix_items: int = 0
    cascade_prefix: int = 0  # longest cascade prefix of the step (tokens; 0 = no cascade)
    n_items: int = 0
    prefill_splits: int = 0
    n_merge: int = 0        # prefill row ranges whose tiles were split: (lo, hi) pairs of section merge_ranges
    prefix_joined: int = 0  # prefill tiles that ride in the cascade prefix pass (alt partials into prefill_part)
    i64: np.ndarray | None = None
    i32: np.ndarray | None = None
    # (row, seq, position): decode inputs whose token was still being sampled at planning time, filled at launch
    patch: list = field(default_factory=list)
    stats: dict = field(default_factory=dict)
    # rows filled on the device from ModelRunner.tok_buf: destination token rows (section late_dst) and source rows
    # of the previous step's sampler output (late_src), appended at launch
    n_late: int = 0
    late_off: int = 0

    def i32_sections(self) -> dict[str, tuple[int, tuple]]:
        """{section: (offset, shape)} of ``i32``, from the scalars alone; the sections tile the buffer in this order."""
        return _sections(0, (("block_tables", (self.nbt, self.bt_w)), ("q_limit", (self.T,)),
                             ("decode_items", (self.n_dec_items, ITEM_INTS)),
                             ("prefix_items", (self.n_prefix_items, ITEM_INTS)),
                             ("prefill_items", (self.n_items, ITEM_INTS)), ("merge_ranges", (self.n_merge, 2))))

    def i64_sections(self) -> dict[str, tuple[int, tuple]]:
        """As ``i32_sections`` for ``i64``; the late rows exist once ``launch`` has appended them."""
        sec = _sections(0, (("tokens", (self.T,)), ("positions", (self.T,)), ("slots", (self.T,)),
                            ("logit_rows", (self.n_rows,))))
        if self.n_late:
            sec.update(_sections(self.late_off, (("late_dst", (self.n_late,)), ("late_src", (self.n_late,)))))
        return sec


def _sections(off: int, shapes) -> dict[str, tuple[int, tuple]]:
    out = {}
    for name, shape in shapes:
        out[name] = (off, shape)
        off += math.prod(shape)
    return out


def section(buf, sections: dict, name: str):
    """View of one section of ``buf`` (a packed numpy array or torch tensor laid out as ``sections`` says)."""
    o, shape = sections[name]
    v = buf[o:o + math.prod(shape)]
    return v if len(shape) == 1 else v.reshape(shape)


def join(sections: dict, parts: dict, dtype) -> np.ndarray:
    """The packed buffer of ``sections`` from one array (or list of records) per section; a part of another size
    than its section is an error."""
    flat, end = [], 0
    for name, (off, shape) in sections.items():
        if off != end:
            raise ValueError(f"section before {name}: {end - off} elements too many")
        a = parts[name]
        if len(a):
            a = np.asarray(a, dtype=dtype).reshape(-1)
            flat.append(a)
            end += a.size
    if end != off + math.prod(shape):
        raise ValueError(f"section {name}: {end - off} elements for shape {shape}")
    return np.concatenate(flat)


@dataclass
class ProcUpdates:
    """Device table writes a step needs before its sampler runs (identical on every TP rank)."""
    mask_rows: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int32))     # [k] rows of mask_tab
    mask_words: np.ndarray = field(default_factory=lambda: np.zeros((0, 0), np.int32))  # [k, W] their bits
    zero_slots: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int32))    # [z] count rows to clear
    # [d, 2] (slot, token): counts[slot][token] -= 1 — a token the sampler counted and the engine rolled back
    dec: np.ndarray = field(default_factory=lambda: np.zeros((0, 2), np.int32))
    # logit-bias rows: [k] rows of bias_tab and [k, 2 * LOGIT_BIAS_MAX] their words (ascending ids, then fp32 bits)
    bias_rows: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int32))
    bias_words: np.ndarray = field(default_factory=lambda: np.zeros((0, BIAS_ROW_INTS), np.int32))
    # repetition penalty: [k] penalty slots newly given to a sequence with repetition_penalty != 1, [k, 2] fp32 their
    # (r, 1 / r) rows of rep_tab, and the ascending distinct prompt ids of each (CSR: slot j owns
    # seen_ids[seen_off[j]:seen_off[j + 1]], seen_off int32 [k + 1]; [0] without slots) whose count words get
    # COUNT_SEEN_PROMPT
    seen_slots: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int32))
    seen_off: np.ndarray = field(default_factory=lambda: np.zeros(1, np.int32))
    seen_ids: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int32))
    rep_vals: np.ndarray = field(default_factory=lambda: np.zeros((0, 2), np.float32))
    # JSON mode: [k] slots of the device state table the host (re)seeds — on admission and on a re-prefill — and
    # [k, JSON_STATE_INTS] their records (state id, depth, stack bits, 0); every other state change happens on the device
    json_slots: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int32))
    json_states: np.ndarray = field(default_factory=lambda: np.zeros((0, JSON_STATE_INTS), np.int32))
    # json_schema: the tables this step loads into the device pool before its mask kernel runs, as (table index, cls
    # uint8 [256], trans uint16 [S, C]) — a schema the pool does not hold yet (engine/json_schema.py). A schema row's
    # seeded record rides in json_slots / json_states above as (state, 0, 0, table index + 1)
    schema_tabs: list = field(default_factory=list)
    # automaton tool grammar (engine/tool_automaton.py): the call bodies' tables this step loads into the same pool, as
    # schema_tabs; [k] slots the host (re)seeds and [k, JSON_STATE_INTS] their records (state, phase, 0, table index + 1)
    tool_tabs: list = field(default_factory=list)
    tool_slots: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int32))
    tool_states: np.ndarray = field(default_factory=lambda: np.zeros((0, JSON_STATE_INTS), np.int32))

    @property
    def empty(self) -> bool:
        return not (self.mask_rows.size or self.zero_slots.size or self.dec.size or self.bias_rows.size
                    or self.seen_slots.size or self.json_slots.size or self.schema_tabs or self.tool_tabs
                    or self.tool_slots.size)

    def check_seen(self) -> None:
        """The repetition-penalty sections agree with each other (a plan on the wire, a table update)."""
        k, off = self.seen_slots.size, self.seen_off
        if off.shape != (k + 1,) or self.rep_vals.shape != (k, 2) or int(off[0]) != 0 \
                or (np.diff(off) < 0).any() or int(off[-1]) != self.seen_ids.size:
            raise ValueError("plan: repetition-penalty slots, offsets, ids and factors disagree")


@dataclass
class SampleParams:
    temp: np.ndarray
    topp: np.ndarray
    topk: np.ndarray
    seeds: np.ndarray
    # per-row device logits processing (engine/logits_proc.py): int32 [n, 8] or None when no row needs it
    proc: np.ndarray | None
    greedy: bool
    upd: ProcUpdates | None = None  # table writes (new grammar mask rows, penalty slots to clear) before sampling
    known: dict | None = None       # row -> token fixed by the grammar (forced): the host knows it at launch
    # per-token logprobs (ops.token_logprobs): the sampled rows whose request asked (int32, ascending) and the step's
    # largest top_logprobs. NOT part of pack_plan / unpack_plan: only the rank that returns tokens computes them
    lp_rows: np.ndarray | None = None
    lp_k: int = 0
    # JSON mode: int32 [k, 2] (sampled row, state-table slot) of the step's JSON rows, or None. The mask kernel runs
    # over them before the sampler and the advance kernel behind it (ops/csrc/json_mask.hip); part of the plan
    json_rows: np.ndarray | None = None
    # json_schema: int32 [k, 3] (sampled row, state-table slot, table index) of the step's schema rows, or None; the
    # mask and advance kernels of ops/csrc/table_grammar.hip run over them around the sampler; part of the plan
    schema_rows: np.ndarray | None = None
    # automaton tool grammar: int32 [k, TOOL_ROW_INTS] (sampled row, state-table slot, table index, open id, close id)
    # of the step's tool rows, or None; the same kernels run over them in launches of their own; part of the plan
    tool_rows: np.ndarray | None = None


GRAMMARS = ("json", "schema", "tool")  # the ``*_rows`` of SampleParams, in the order of their upload and mask launches


_PLAN_SCALARS = ("B", "T", "nbt", "bt_w", "n_rows", "s_total", "n_dec_items", "n_prefix_items", "cascade_prefix",
                 "n_items", "prefill_splits", "n_merge", "n_late", "late_off", "bt_need", "prefix_joined")
PLAN_HDR = 32  # int64 header of a broadcast step plan
PLAN_PAYLOAD_IDX = 1 + len(_PLAN_SCALARS) + 4  # header word holding the payload size (pack_plan)
PLAN_SCHEMA_IDX = PLAN_HDR - 1  # header word holding the int32 word count of the trailing json_schema section
# the tool grammar section, behind it, has a header word of its own in the upper half of the same int64: words 0..30 are
# taken and the header's size is part of the wire format, while a section's int32 word count fits 31 bits
PLAN_TOOL_SHIFT = 32
TOOL_ROW_INTS = 5  # kafka_abi.h


def _schema_section(rows: np.ndarray, tabs: list) -> np.ndarray:
    """The plan's trailing json_schema section as int32 words; it describes its own parts: [k rows, t tables], the rows
    [k, 3], then per table (index, S, C), cls as 64 words and trans as ceil(S * C / 2) words (zero-padded). The tool
    grammar section is the same with rows of TOOL_ROW_INTS words."""
    parts = [np.array([rows.shape[0], len(tabs)], np.int32), rows.astype(np.int32, copy=False).reshape(-1)]
    for idx, cls, trans in tabs:
        cls, trans = np.ascontiguousarray(cls), np.ascontiguousarray(trans)
        if cls.shape != (256,) or cls.dtype != np.uint8 or trans.ndim != 2 or trans.dtype != np.uint16:
            raise ValueError("plan: a schema table is cls uint8 [256] and trans uint16 [S, C]")
        flat = trans.reshape(-1)
        if flat.size % 2:
            flat = np.concatenate([flat, np.zeros(1, np.uint16)])
        parts += [np.array([idx, trans.shape[0], trans.shape[1]], np.int32), cls.view(np.int32), flat.view(np.int32)]
    return np.concatenate(parts)


def _schema_unsection(words: np.ndarray, row_ints: int = 3) -> tuple[np.ndarray, list]:
    k, t = int(words[0]), int(words[1])
    o = 2 + row_ints * k
    if k < 0 or t < 0 or o > words.size:
        raise ValueError("plan: the json_schema section does not hold its rows")
    rows = words[2:o].reshape(k, row_ints)
    tabs = []
    for _ in range(t):
        idx, S, C = (int(v) for v in words[o:o + 3])
        n = (S * C + 1) // 2
        if S < 1 or C < 1 or o + 3 + 64 + n > words.size:
            raise ValueError("plan: the json_schema section does not hold its tables")
        cls = words[o + 3:o + 67].view(np.uint8).copy()
        trans = words[o + 67:o + 67 + n].view(np.uint16)[:S * C].reshape(S, C).copy()
        tabs.append((idx, cls, trans))
        o += 67 + n
    if o != words.size:
        raise ValueError("plan: the json_schema section is longer than its parts")
    return rows, tabs


def _bt_rewidth(h: HostStep, i32: np.ndarray, w_from: int, w_to: int) -> np.ndarray:
    """``i32`` with its block-table section cut or zero-padded from ``w_from`` to ``w_to`` columns."""
    off, (nbt, _) = h.i32_sections()["block_tables"]
    end = off + nbt * w_from
    bt = np.zeros((nbt, w_to), dtype=np.int32)
    w = min(w_from, w_to)
    bt[:, :w] = i32[off:end].reshape(nbt, w_from)[:, :w]
    return np.concatenate([i32[:off], bt.reshape(-1), i32[end:]])


def pack_plan(h: HostStep, sp: SampleParams) -> tuple[np.ndarray, np.ndarray]:
    """A launched step as (int64 header [PLAN_HDR], uint8 payload): the fixed-layout wire format a TP leader sends its
    followers (two gloo tensor broadcasts per step; no pickling). Everything a follower needs to run the SAME step:
    the layout scalars, the packed int64 / int32 buffers and the sampling parameters with the logits-processing rows
    and table updates (every rank samples the all-gathered logits itself with the same grammar masks and penalty
    counts, so its device copy of the sampled ids — the next step's late decode inputs — is identical to the
    leader's)."""
    n = sp.temp.shape[0]
    i32 = h.i32.astype(np.int32, copy=False)
    if 0 < h.bt_need < h.bt_w:  # ship only the block-table columns that hold pages (followers re-pad with zeros)
        i32 = _bt_rewidth(h, i32, h.bt_w, h.bt_need)
    upd = sp.upd if sp.upd is not None else ProcUpdates()
    proc = sp.proc if sp.proc is not None else np.zeros((0, 8), np.int32)
    parts = [h.i64.astype(np.int64, copy=False), i32,
             sp.temp.astype(np.float32, copy=False), sp.topp.astype(np.float32, copy=False),
             sp.topk.astype(np.int32, copy=False), sp.seeds.astype(np.int64, copy=False),
             proc.astype(np.int32, copy=False), upd.mask_rows.astype(np.int32, copy=False),
             upd.mask_words.astype(np.int32, copy=False), upd.zero_slots.astype(np.int32, copy=False),
             upd.dec.astype(np.int32, copy=False), upd.bias_rows.astype(np.int32, copy=False),
             upd.bias_words.astype(np.int32, copy=False)]
    if upd.bias_rows.size and upd.bias_words.shape != (upd.bias_rows.size, BIAS_ROW_INTS):
        raise ValueError("plan: logit-bias update rows and words disagree")
    upd.check_seen()
    if upd.seen_slots.size:  # behind the bias rows: slots [k], offsets [k + 1], factors [k, 2] fp32, ids
        parts += [upd.seen_slots.astype(np.int32, copy=False), upd.seen_off.astype(np.int32, copy=False),
                  upd.rep_vals.astype(np.float32, copy=False), upd.seen_ids.astype(np.int32, copy=False)]
    if upd.json_states.shape != (upd.json_slots.size, JSON_STATE_INTS):
        raise ValueError("plan: JSON state slots and records disagree")
    jrows = sp.json_rows if sp.json_rows is not None else np.zeros((0, 2), np.int32)
    if jrows.ndim != 2 or jrows.shape[1] != 2:
        raise ValueError("plan: JSON rows must be (sampled row, slot) pairs")
    if upd.json_slots.size or jrows.size:  # last: seeded slots [k], their records [k, 4], the step's JSON rows [j, 2]
        parts += [upd.json_slots.astype(np.int32, copy=False), upd.json_states.astype(np.int32, copy=False),
                  jrows.astype(np.int32, copy=False)]
    srows = sp.schema_rows if sp.schema_rows is not None else np.zeros((0, 3), np.int32)
    if srows.ndim != 2 or srows.shape[1] != 3:
        raise ValueError("plan: schema rows must be (sampled row, slot, table) triples")
    n_schema = 0
    if srows.size or upd.schema_tabs:  # the trailing section; a step without it packs to the bytes it always did
        parts.append(_schema_section(srows, upd.schema_tabs))
        n_schema = parts[-1].size
    trows = sp.tool_rows if sp.tool_rows is not None else np.zeros((0, TOOL_ROW_INTS), np.int32)
    if trows.ndim != 2 or trows.shape[1] != TOOL_ROW_INTS:
        raise ValueError("plan: tool rows must be (sampled row, slot, table, open, close) records")
    if upd.tool_states.shape != (upd.tool_slots.size, JSON_STATE_INTS):
        raise ValueError("plan: tool state slots and records disagree")
    n_tool = 0
    if trows.size or upd.tool_tabs or upd.tool_slots.size:  # the last section: [n seeds], slots [n], records [n, 4],
        # then rows and tables as the json_schema section; a step without it packs to the bytes it always did
        parts += [np.array([upd.tool_slots.size], np.int32), upd.tool_slots.astype(np.int32, copy=False),
                  upd.tool_states.astype(np.int32, copy=False).reshape(-1), _schema_section(trows, upd.tool_tabs)]
        n_tool = sum(p.size for p in parts[-4:])
    payload = np.concatenate([np.ascontiguousarray(a).reshape(-1).view(np.uint8) for a in parts])
    hdr = np.zeros(PLAN_HDR, dtype=np.int64)
    hdr[PLAN_SCHEMA_IDX] = n_schema | (n_tool << PLAN_TOOL_SHIFT)
    hdr[0] = 1
    k = len(_PLAN_SCALARS)
    hdr[1:1 + k] = [getattr(h, f) for f in _PLAN_SCALARS]
    W = upd.mask_words.shape[1] if upd.mask_rows.size else 0
    hdr[1 + k:1 + k + 10] = [h.i64.size, i32.size, n, int(sp.greedy), payload.size, proc.shape[0],
                             upd.mask_rows.size, W, upd.zero_slots.size, upd.dec.shape[0]]
    hdr[1 + k + 10] = upd.bias_rows.size  # (0 and no bytes behind ``dec`` for a step without new bias rows)
    hdr[1 + k + 11] = upd.seen_slots.size  # (likewise: 0 and no bytes without newly seeded repetition-penalty slots)
    hdr[1 + k + 12], hdr[1 + k + 13] = upd.json_slots.size, jrows.shape[0]  # (likewise without JSON rows)
    return hdr, payload


def unpack_plan(hdr: np.ndarray, payload: np.ndarray) -> tuple[HostStep, SampleParams]:
    k = len(_PLAN_SCALARS)
    h = HostStep(**{f: int(v) for f, v in zip(_PLAN_SCALARS, hdr[1:1 + k])})
    n64, n32, n, greedy, _, n_proc, n_mask, W, n_zero, n_dec = (int(v) for v in hdr[1 + k:1 + k + 10])
    n_bias = int(hdr[1 + k + 10])
    n_seen = int(hdr[1 + k + 11])
    n_jseed, n_jrows = int(hdr[1 + k + 12]), int(hdr[1 + k + 13])
    o = 0

    def take(dt, cnt):
        nonlocal o
        nb = np.dtype(dt).itemsize * cnt
        a = payload[o:o + nb].view(dt)
        o += nb
        return a

    h.i64 = take(np.int64, n64)
    h.i32 = take(np.int32, n32)
    if 0 < h.bt_need < h.bt_w:  # re-pad the shipped block-table columns to the step's layout width
        h.i32 = _bt_rewidth(h, h.i32, h.bt_need, h.bt_w)
    sp = SampleParams(take(np.float32, n), take(np.float32, n), take(np.int32, n), take(np.int64, n), None,
                      bool(greedy))
    proc = take(np.int32, n_proc * 8).reshape(n_proc, 8)
    upd = ProcUpdates(take(np.int32, n_mask), take(np.int32, n_mask * W).reshape(n_mask, W),
                      take(np.int32, n_zero), take(np.int32, 2 * n_dec).reshape(n_dec, 2), take(np.int32, n_bias),
                      take(np.int32, n_bias * BIAS_ROW_INTS).reshape(n_bias, BIAS_ROW_INTS))
    if n_seen:
        upd.seen_slots, upd.seen_off = take(np.int32, n_seen), take(np.int32, n_seen + 1)
        upd.rep_vals = take(np.float32, 2 * n_seen).reshape(n_seen, 2)
        upd.seen_ids = take(np.int32, max(0, int(upd.seen_off[-1])))
        upd.check_seen()
    if n_jseed or n_jrows:
        upd.json_slots = take(np.int32, n_jseed)
        upd.json_states = take(np.int32, n_jseed * JSON_STATE_INTS).reshape(n_jseed, JSON_STATE_INTS)
        jrows = take(np.int32, 2 * n_jrows).reshape(n_jrows, 2)
        sp.json_rows = jrows if n_jrows else None
    n_schema = int(hdr[PLAN_SCHEMA_IDX]) & ((1 << PLAN_TOOL_SHIFT) - 1)
    n_tool = int(hdr[PLAN_SCHEMA_IDX]) >> PLAN_TOOL_SHIFT
    if n_schema:
        srows, upd.schema_tabs = _schema_unsection(take(np.int32, n_schema))
        sp.schema_rows = srows if srows.shape[0] else None
    if n_tool:
        words = take(np.int32, n_tool)
        ns = int(words[0]) if words.size else -1
        if ns < 0 or 1 + ns * (1 + JSON_STATE_INTS) > words.size:
            raise ValueError("plan: the tool grammar section does not hold its seeds")
        upd.tool_slots = words[1:1 + ns]
        upd.tool_states = words[1 + ns:1 + ns * (1 + JSON_STATE_INTS)].reshape(ns, JSON_STATE_INTS)
        trows, upd.tool_tabs = _schema_unsection(words[1 + ns * (1 + JSON_STATE_INTS):], TOOL_ROW_INTS)
        sp.tool_rows = trows if trows.shape[0] else None
    sp.proc = proc if n_proc else None
    sp.upd = None if upd.empty else upd
    return h, sp


# ---- key pieces ---------------------------------------------------------------------------------------------------
def key_pieces(lo: int, span: int, hi: int, chunk: int) -> list[tuple[int, int]]:
    """Keys [lo, lo + span) as equal 32-key-aligned pieces (kv_lo, kv_hi) of about ``chunk`` keys, the last one
    bounded by ``hi``."""
    n = max(1, cdiv(span, chunk))
    ps = cdiv(span, n * 32) * 32
    return [(lo + c * ps, min(hi, lo + (c + 1) * ps)) for c in range(cdiv(span, ps))]


def one_round_chunk(chunk: int, spans: list[tuple[int, int]], limit: int, max_keys: int = MAX_ITEM_KEYS) -> int:
    """``chunk`` grown until the (key span, tiles over it) pairs make at most ``limit`` items: per-span rounding up
    can overshoot a launch's target by a few, and a second round of a handful of workgroups doubles the launch (r03
    trace: 272 workgroups for a new turn, 125 us vs ~60)."""
    while chunk < max_keys and sum(t * -(-s // chunk) for s, t in spans) > limit:  # (inline cdiv: up to ~1000 rounds)
        chunk += 32
    return chunk


def plan_prefill_items(tiles: list[tuple], hkv: int, target_wgs: int, min_chunk: int,
                       max_keys: int = MAX_ITEM_KEYS) -> tuple[list[tuple], int, list[tuple[int, int]]]:
    """Work items (``TileItem`` tuples) of the prefill tile kernel from query tiles (``Tile`` tuples; ``lo`` and
    ``s0`` may be left out). A tile with
    ``lo`` > 0 attends only keys [lo, extent) — its keys below lo (a shared system prefix) were attended by the
    step's cascade prefix pass, whose partials sit in slots [0, s0) of the row — so it always writes partials, at
    slots s0, s0 + 1, ...

    The tile kernel's time per workgroup is ~a + b x (32-key blocks), so a launch is as long as its longest item. A
    causal prompt's tiles grow linearly (a 2k prompt: 2 .. 64 blocks) and a new turn's few tiles each span a ~20k-token
    context: when the launch is at most ~two rounds of workgroups, tiles longer than the balanced share
    (sum of extents x Hkv / target_wgs, >= min_chunk) are split into equal key pieces whose (O, lse) partials are
    merged afterwards; shorter tiles still write bf16 rows directly. Larger launches only get longest-first order
    (the dispatcher then packs the tail). Returns (items, partial slots per row, merged row ranges)."""
    if not tiles:
        return [], 0, []
    tiles = [t if len(t) == len(TILE) else tuple(Tile(*t)) for t in tiles]
    spans = [extent - lo for _, _, _, extent, _, lo, _ in tiles]
    if len(tiles) * hkv >= 2 * target_wgs:
        ck = max_keys  # many tiles: split only what exceeds the LDS page-staging bound
    else:
        ck = min(max(min_chunk, cdiv(sum(spans) * hkv, target_wgs * 32) * 32), max_keys)
        if max(spans) < 3 * ck // 2 and max(spans) <= max_keys:
            ck = max_keys  # nothing long enough for a split to shorten the launch by much
        elif min(spans) > ck:
            # every tile is split (new turns against a long cached context): keep the launch to ONE round of
            # workgroups
            ck = one_round_chunk(ck, [(s, 1) for s in spans], target_wgs // hkv, max_keys)
    items, splits, ranges = [], 0, []
    for (q0, count, bt_row, _, hi, lo, s0), span in zip(tiles, spans):
        if span <= ck and lo == 0:
            items.append((q0, count, bt_row, 0, hi, -1, 0, 0))
            continue
        pieces = key_pieces(lo, span, hi, ck)
        items += [(q0, count, bt_row, kv_lo, kv_hi, s0 + c, 0, 0) for c, (kv_lo, kv_hi) in enumerate(pieces)]
        splits = max(splits, s0 + len(pieces))
        if ranges and ranges[-1][1] == q0:
            ranges[-1] = (ranges[-1][0], q0 + count)
        else:
            ranges.append((q0, q0 + count))
    kv_lo, kv_hi = ITEM.kv_lo, ITEM.kv_hi
    items.sort(key=lambda it: it[kv_lo] - it[kv_hi])  # longest key range first
    return items, splits, ranges


def retile(spans: list[tuple[int, int]], tile: int) -> list[tuple[int, int]]:
    """(q0, count) token spans (ascending) -> the same tokens as (q0, count) tiles of at most ``tile`` tokens, contiguous
    spans joined first: 8 new turns of 30 tokens back to back make 4 full tiles, not 8 half-empty ones."""
    runs: list[list[int]] = []
    for q0, cnt in spans:
        if runs and runs[-1][0] + runs[-1][1] == q0:
            runs[-1][1] += cnt
        else:
            runs.append([q0, cnt])
    return [(q0 + t, min(tile, cnt - t)) for q0, cnt in runs for t in range(0, cnt, tile)]


def merge_ranges(ranges: list[tuple[int, int]]) -> list[tuple[int, int]]:
    """Sorted union of half-open row ranges, touching ones joined (one attn_merge launch per range)."""
    out: list[tuple[int, int]] = []
    for lo, hi in sorted(ranges):
        if out and lo <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    return out


def prefix_groups(bt: np.ndarray, nfull: np.ndarray, min_blocks: int) -> tuple[list[int], list[Group]]:
    """Cascade groups of decode rows: rows whose block tables start with the same pages share that KV prefix.

    ``bt`` int32 [B, W] block tables, ``nfull[b]`` = pages of row b that may belong to a shared prefix (full pages
    before the one holding the current token). Returns (order, groups): a permutation of the rows that makes every
    group contiguous, and (row_count, prefix_pages) per group in that order (groups first, then ungrouped rows).
    A set of rows is split by the first page where it disagrees when its common prefix is shorter than
    ``min_blocks`` — e.g. threads on the Kafka system prompt vs threads created with their own system message
    (quirk Q4 of SURVEY.md §2.9) vs stateless /chat/completions traffic each get their own group."""
    groups: list[tuple[list[int], int]] = []
    loose: list[int] = []

    def rec(rows: np.ndarray, d: int) -> None:
        while True:
            if len(rows) < 2:
                loose.extend(rows.tolist())
                return
            lim = int(nfull[rows].min())
            sub = bt[rows, d:lim]
            if sub.shape[1]:
                eq = (sub == sub[0]).all(0)
                j = d + (int(np.argmin(eq)) if not eq.all() else sub.shape[1])
            else:
                j = d
            if j >= min_blocks:
                groups.append((rows.tolist(), j))
                return
            short = nfull[rows] <= j  # rows without a page j: cannot share anything longer
            if short.any():
                loose.extend(rows[short].tolist())
                rows = rows[~short]
                d = j
                continue
            col = bt[rows, j]
            for v in np.unique(col):
                rec(rows[col == v], j + 1)
            return

    rec(np.arange(bt.shape[0]), 0)
    order = [r for rows, _ in groups for r in rows] + loose
    return order, [Group(len(rows), p) for rows, p in groups]


def _pieces_to_items(seq_lens: np.ndarray, kv_start: np.ndarray, npre: np.ndarray, a0: np.ndarray, ns: np.ndarray,
                     block_lo, block_hi) -> np.ndarray:
    """Decode items of rows cut into ``ns[b]`` pieces: piece c of row b covers its 32-key blocks
    [block_lo(b, c), block_hi(b, c)) counted from ``a0[b]``, clipped to [kv_start, len)."""
    rows = np.repeat(np.arange(seq_lens.shape[0]), ns)
    split = np.arange(rows.shape[0]) - np.repeat(np.cumsum(ns) - ns, ns)
    lo = np.maximum(kv_start[rows], a0[rows] + block_lo(rows, split) * 32)
    hi = np.minimum(seq_lens[rows], a0[rows] + block_hi(rows, split) * 32)
    z = np.zeros_like(rows)
    return np.stack(DecodeItem(b=rows, lo=lo, hi=hi, split=split, nsplit=ns[rows], npre=npre[rows], pad0=z, pad1=z),
                    1).astype(np.int32)


def _longest_first(it: np.ndarray) -> np.ndarray:
    return it[np.argsort(it[:, DEC.lo] - it[:, DEC.hi], kind="stable")]


def decode_items(seq_lens: np.ndarray, kv_start: np.ndarray, npre: np.ndarray, hkv: int,
                 target: int = DECODE_TARGET_ITEMS, min_keys: int = MIN_DECODE_KEYS) -> np.ndarray:
    """Work items (``DecodeItem`` rows) of the decode kernel: every row's keys [kv_start, len) in
    32-key-aligned pieces of about ``ch`` keys, ``ch`` chosen so the launch has ~``target`` workgroups (x Hkv) of
    about equal bytes (long histories are split, short ones stay whole); at most MAX_PARTIALS - npre pieces."""
    B = seq_lens.shape[0]
    suffix = np.maximum(seq_lens - kv_start, 1).astype(np.int64)
    # fewer rows than it takes to fill the GPU (B x Hkv < 512 workgroups): split so the launch still has ~512
    target = max(target, 512) if B * hkv < 512 else target
    if target <= 0:
        ch = int(suffix.max())
    else:
        ch = max(min_keys, cdiv(int(suffix.sum()) * hkv, target * 32) * 32)
    a0 = kv_start - kv_start % 32
    nb = (seq_lens - a0 + 31) // 32
    ns = np.minimum(np.maximum(1, cdiv(suffix, ch)), MAX_PARTIALS - npre)
    bps = cdiv(nb, ns)
    ns = cdiv(nb, bps)  # no empty trailing piece
    it = _pieces_to_items(seq_lens, kv_start, npre, a0, ns, lambda r, c: c * bps[r], lambda r, c: (c + 1) * bps[r])
    # longest pieces first: they start while the dispatcher fills the GPU, short ones fill the tail
    return _longest_first(it) if ns.max() > 1 else it


def decode_items_fixed(seq_lens: np.ndarray, kv_start: np.ndarray, npre: np.ndarray, hkv: int,
                       target: int = DECODE_TARGET_ITEMS) -> np.ndarray:
    """``decode_items`` with EXACTLY n = max(B, target // hkv) items (a captured decode graph's launch shape then
    depends on B alone, no padded grid): the n pieces are dealt to the rows in proportion to their 32-key blocks
    (largest remainder, at least one per row, at most MAX_PARTIALS - npre and one per block), each row's blocks split
    evenly; rows too short to take their share leave null items (split -1: the kernel drops them)."""
    B = seq_lens.shape[0]
    n = max(B, target // hkv)
    a0 = kv_start - kv_start % 32
    nb = np.maximum((seq_lens - a0 + 31) // 32, 1).astype(np.int64)
    cap = np.maximum(1, np.minimum(nb, MAX_PARTIALS - npre))
    ns = np.minimum(cap, np.maximum(1, (n * nb) // max(1, int(nb.sum()))))
    while int(ns.sum()) > n:  # the at-least-one floor overshot: take pieces back from the lightest split rows
        more = ns > 1
        if not more.any():
            break
        load = np.where(more, nb / ns, np.inf)
        ns[int(np.argmin(load))] -= 1
    left = n - int(ns.sum())
    while left > 0:  # largest blocks-per-piece first
        room = ns < cap
        if not room.any():
            break
        load = np.where(room, nb / ns, -1.0)
        k = min(left, int(room.sum()))
        for b in np.argsort(-load, kind="stable")[:k]:
            ns[b] += 1
        left = n - int(ns.sum())
    it = _longest_first(_pieces_to_items(seq_lens, kv_start, npre, a0, ns, lambda r, c: (c * nb[r]) // ns[r],
                                         lambda r, c: ((c + 1) * nb[r]) // ns[r]))
    if it.shape[0] < n:
        pad = np.zeros((n - it.shape[0], ITEM_INTS), dtype=np.int32)
        pad[:, DEC.split] = -1
        it = np.concatenate([it, pad])
    return it


# ---- the attention plan of a step ---------------------------------------------------------------------------------
@dataclass(frozen=True)
class PlanConfig:
    tile: int               # tokens per tile work item
    hkv: int
    page: int               # tokens per KV page
    target_wgs: int         # workgroups the prefill / cascade tile launches are balanced for
    prefill_kv_chunk: int
    joins: bool = True      # new-turn prefill chunks may join a cascade group's prefix pass (tile variant 3)
    join_suffix: bool = True  # a joined chunk's own keys (behind the prefix) ride in the cascade launch too
    fixed_decode: bool = False  # decode_items_fixed: the decode grid depends on B alone (graph replay)
    # (a graph layout key: s_total rounded up to a multiple of 8 so a handful of layouts cover every step; the
    # partial buffers' unused slots are never touched)
    round_s_total: bool = False


@dataclass
class AttnPlan:
    """The attention part of a step: the items of its three launches, the prefill rows to merge and the scalars of
    ``HostStep`` they fix."""
    decode_items: np.ndarray | tuple = ()  # int32 [n, ITEM_INTS]
    prefix_items: list[tuple] = field(default_factory=list)   # TileItem tuples
    prefill_items: list[tuple] = field(default_factory=list)
    merge_ranges: list[tuple[int, int]] = field(default_factory=list)
    s_total: int = 1
    cascade_prefix: int = 0
    prefill_splits: int = 0
    prefix_joined: int = 0
    n_groups: int = 0

    @property
    def scalars(self) -> dict:
        """The ``HostStep`` fields this plan sets."""
        return {"s_total": self.s_total, "n_dec_items": len(self.decode_items),
                "n_prefix_items": len(self.prefix_items), "cascade_prefix": self.cascade_prefix,
                "n_items": len(self.prefill_items), "prefill_splits": self.prefill_splits,
                "n_merge": len(self.merge_ranges), "prefix_joined": self.prefix_joined}

    def stats(self, B: int, T: int) -> dict:
        return {"B": B, "T": T, "cascade_prefix": self.cascade_prefix, "cascade_groups": self.n_groups,
                "prefix_joined_tiles": self.prefix_joined, "decode_items": len(self.decode_items),
                "prefix_items": len(self.prefix_items), "s_total": self.s_total,
                "prefill_splits": self.prefill_splits, "prefill_items": len(self.prefill_items)}


def chunk_tiles(chunks: list[tuple[int, int, int]], tile: int) -> list[tuple]:
    """Causal query tiles (``Tile`` tuples) of prefill chunks (a, b, bt_row) = tokens [a, b) of a sequence, packed
    back to back."""
    tiles, q = [], 0
    for a, b, bt_row in chunks:
        for t0 in range(0, b - a, tile):
            count = min(tile, b - a - t0)
            tiles.append((q + t0, count, bt_row, a + t0 + count, b, 0, 0))
        q += b - a
    return tiles


def prefix_joins(bt: np.ndarray, groups: list[Group], chunks: list[tuple[int, int, int]], tiles: list[tuple],
                 page: int) -> dict[int, list[int]]:
    """{group index: prefill tile indices} of the prefill chunks that start at or behind a cascade group's
    shared prefix and whose block table holds the same prefix pages (the groups' rows are contiguous from row
    0 in group order; a tile names its chunk through its block-table row)."""
    starts, r0 = [], 0
    for g in groups:
        starts.append((r0, g.pages))
        r0 += g.rows
    chunk_group: dict[int, int] = {}
    for a, _, bt_row in chunks:
        for gi, (g_row, p) in enumerate(starts):
            if a >= p * page and np.array_equal(bt[bt_row, :p], bt[g_row, :p]):
                chunk_group[bt_row] = gi
                break
    joins: dict[int, list[int]] = {}
    for ti, t in enumerate(tiles):
        gi = chunk_group.get(t[TILE.bt_row])
        if gi is not None:
            joins.setdefault(gi, []).append(ti)
    return joins


def plan_cascade(plan: AttnPlan, B: int, groups: list[Group], joins: dict[int, list[int]], tiles: list[tuple],
                 cfg: PlanConfig) -> tuple[np.ndarray, np.ndarray]:
    """The cascade prefix pass: every group's shared prefix attended once for all its rows by the tile kernel, in
    key chunks whose partials take slots 0 .. nc - 1 of the rows. Joined prefill tiles (``joins``) ride along with
    alt partials and are updated in ``tiles`` (lo = the prefix, s0 = nc); with ``cfg.join_suffix`` their own keys
    behind the prefix are items of this launch too: their partial slots and row ranges go to ``plan.prefill_splits``
    and ``plan.merge_ranges``. Sets ``plan.prefix_items``; returns (kv_start [B], npre [B]) of the decode rows."""
    tile, page = cfg.tile, cfg.page
    # joined tiles' own key spans (behind the prefix)
    spans = {ti: tiles[ti][TILE.extent] - groups[gi].pages * page for gi, js in joins.items() for ti in js} \
        if cfg.join_suffix else {}
    # the joined rows' prefix-pass tiles: the group's joined tokens re-tiled at token granularity (a burst
    # of short new turns fills 64-token tiles instead of one mostly empty tile per turn; every key of the
    # prefix is below every joined token's position, so tokens of different turns share a tile)
    jt = {gi: retile([(tiles[ti][TILE.q0], tiles[ti][TILE.count]) for ti in js], tile) for gi, js in joins.items()}
    # key chunks sized so the prefix pass launches ~target_wgs workgroups over all groups together, in one round
    prefixes = [(g.pages * page, cdiv(g.rows, tile) + len(jt.get(gi, ()))) for gi, g in enumerate(groups)]
    work = sum(P * t for P, t in prefixes) + sum(spans.values())
    want = max(1, cfg.target_wgs // cfg.hkv)
    chunk = min(MAX_ITEM_KEYS, max(256, cdiv(work, want * 32) * 32))
    chunk = one_round_chunk(chunk, prefixes + [(s, 1) for s in spans.values()], want)
    items: list[tuple] = []  # TileItem tuples
    kv_start = np.zeros(B, dtype=np.int64)
    npre = np.zeros(B, dtype=np.int64)
    r0 = 0
    for gi, g in enumerate(groups):
        P = g.pages * page
        nc, ck = cdiv(P, chunk), chunk
        if nc > MAX_PREFIX_CHUNKS:
            ck = cdiv(P, MAX_PREFIX_CHUNKS * 32) * 32
            nc = cdiv(P, ck)
        for c in range(nc):  # chunk-major: the row tiles of one chunk run together (L2 sharing)
            lo, hi = c * ck, min(P, (c + 1) * ck)
            items += [(q0, min(tile, r0 + g.rows - q0), r0, lo, hi, c, 0, 0) for q0 in range(r0, r0 + g.rows, tile)]
            # joined prefill rows: q rows B + q0, fp32 alt partials
            items += [(B + q0, cnt, r0, lo, hi, c, 1, 0) for q0, cnt in jt.get(gi, ())]
        for ti in joins.get(gi, ()):
            q0, count, bt_row, _, t_hi = tiles[ti][:TILE.lo]
            tiles[ti] = tiles[ti][:TILE.lo] + (P, nc)
            if ti in spans:
                # the tile's keys [P, extent) in pieces of ~chunk keys: alt partials at slots nc, nc + 1..
                # (beside its prefix pieces' slots 0..nc-1), so the step needs no separate prefill launch
                # for it; attn_merge combines all of the row's slots as before
                pieces = key_pieces(P, spans[ti], t_hi, chunk)
                items += [(B + q0, count, bt_row, lo, hi, nc + c, 1, 0) for c, (lo, hi) in enumerate(pieces)]
                plan.prefill_splits = max(plan.prefill_splits, nc + len(pieces))
                plan.merge_ranges.append((q0, q0 + count))
        kv_start[r0:r0 + g.rows] = P
        npre[r0:r0 + g.rows] = nc
        r0 += g.rows
    plan.prefix_items = items
    return kv_start, npre


def plan_attention(bt: np.ndarray, seq_lens: np.ndarray, groups: list[Group], chunks: list[tuple[int, int, int]],
                   cfg: PlanConfig) -> AttnPlan:
    """The attention work of one step. ``bt`` int32 [rows, W] block tables, decode rows first; ``seq_lens`` the
    decode rows' lengths in group order (``prefix_groups``: the rows of ``groups`` are contiguous from row 0);
    ``chunks`` the prefill chunks (a, b, bt_row).

    Each group's prefix is attended once for all its rows by the tile kernel (``plan_cascade``), the per-row
    suffixes by the decode kernel in pieces of about equal size, the prefill chunks by the tile kernel
    (``plan_prefill_items``)."""
    B = seq_lens.shape[0]
    groups = [Group(*g) for g in groups]
    plan = AttnPlan(n_groups=len(groups))
    tiles = chunk_tiles(chunks, cfg.tile)
    # new-turn prefill chunks whose block table starts with a cascade group's prefix pages (the ~18k shared
    # system prompt every new turn of a thread re-attends): their tokens join the group's prefix pass — one read
    # of the prefix pages per step for all rows — and their own tiles attend only the keys behind the prefix
    joins = prefix_joins(bt, groups, chunks, tiles, cfg.page) if groups and cfg.joins else {}
    plan.prefix_joined = sum(len(js) for js in joins.values())
    if B:
        kv_start = npre = np.zeros(B, dtype=np.int64)
        if groups:
            kv_start, npre = plan_cascade(plan, B, groups, joins, tiles, cfg)
            plan.cascade_prefix = max(g.pages for g in groups) * cfg.page
        plan.decode_items = (decode_items_fixed if cfg.fixed_decode else decode_items)(seq_lens, kv_start, npre,
                                                                                       cfg.hkv)
        real = plan.decode_items[:, DEC.split] >= 0
        plan.s_total = int((npre[plan.decode_items[real, DEC.b]] + plan.decode_items[real, DEC.nsplit]).max())
        if cfg.round_s_total:
            plan.s_total = min(MAX_PARTIALS, cdiv(plan.s_total, 8) * 8)
    sfx_rows = plan.merge_ranges  # joined tiles whose own keys were planned into the prefix pass
    if sfx_rows:  # (their suffix items are in the prefix pass)
        done = {ti for js in joins.values() for ti in js}
        tiles = [t for ti, t in enumerate(tiles) if ti not in done]
    # long tiles (a new turn against a ~20k-token cached context, the late tiles of a causal prompt) are
    # split along the key range so the launch is balanced; their partials are merged afterwards
    plan.prefill_items, splits, ranges = plan_prefill_items(tiles, cfg.hkv, cfg.target_wgs,
                                                            min(256, cfg.prefill_kv_chunk))
    plan.prefill_splits = max(plan.prefill_splits, splits)
    plan.merge_ranges = merge_ranges(ranges + sfx_rows) if sfx_rows else ranges
    return plan
