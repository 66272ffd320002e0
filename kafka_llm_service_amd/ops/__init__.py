"""Public op API. GPU tensors run the hand-written CDNA4 HIP kernels (``csrc/*.hip``) and nothing else;
CPU tensors run the fp32 PyTorch references in ``reference.py`` (unit tests / CPU-only tooling).

Kernel inventory:
  rmsnorm / fused_add_rmsnorm / silu_mul        csrc/norm_act.hip
  rope_kv_write (RoPE + paged KV write)         csrc/rope_kv.hip
  attn_decode / attn_prefill / attn_merge       csrc/attention.hip   (MFMA 32x32x16 bf16, paged, split-K, cascade)
  sample (greedy / temperature / top-k / top-p) csrc/sampling.hip
  token_logprobs (logprob + top-k alternatives) csrc/logprobs.hip
  json_mask / json_advance (JSON-mode masks)    csrc/json_mask.hip
  schema_mask / schema_advance (json_schema)    csrc/table_grammar.hip
  tool_mask / tool_advance (tool automaton)     csrc/table_grammar.hip
  moe_* / grouped GEMM                          csrc/moe.hip
  custom all-reduce                             csrc/allreduce.hip
"""
from __future__ import annotations

import math
import os
from typing import Callable, NamedTuple

import numpy as np
import torch

from . import reference as ref
from ._ext import ext

PAGE = ref.PAGE
kv_cache_shapes = ref.kv_cache_shapes
kv_page_bytes = ref.kv_page_bytes
is_fp8_cache = ref.is_fp8_cache


def _gpu(t: torch.Tensor) -> bool:
    return t.is_cuda


def is_slab(t: torch.Tensor) -> bool:
    """Split-K partial sums of the decode GEMM: fp32 [S, T, n] (``linear_stream``). The slab-aware ops below
    (fused_add_rmsnorm, silu_mul, rope_kv_write) sum them while loading; ``slab_reduce`` gives the bf16 tensor."""
    return t.dtype == torch.float32 and t.dim() == 3


def rows_of(t: torch.Tensor) -> int:
    return t.shape[1] if is_slab(t) else t.shape[0]


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float, out: torch.Tensor | None = None) -> torch.Tensor:
    if out is None:
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    if _gpu(x):
        ext().rmsnorm(out.view(-1, x.shape[-1]), x.reshape(-1, x.shape[-1]), w, float(eps))
    else:
        out.copy_(ref.rmsnorm(x, w, eps))
    return out


def fused_add_rmsnorm(x: torch.Tensor, residual: torch.Tensor, w: torch.Tensor, eps: float,
                      out: torch.Tensor | None = None) -> torch.Tensor:
    """residual <- x + residual (in place); returns rmsnorm(residual) * w (into ``out`` or a new tensor).
    ``x`` may be a split-K slab [S, T, d] (summed in fp32 before the add)."""
    slab = is_slab(x)
    if out is None:
        out = torch.empty(residual.shape, dtype=residual.dtype, device=x.device)
    if _gpu(x):
        xa = x if slab else x.reshape(-1, x.shape[-1])
        ext().fused_add_rmsnorm(out.view(-1, x.shape[-1]), xa, residual.view(-1, x.shape[-1]), w, float(eps))
    else:
        y, s = ref.fused_add_rmsnorm(x.sum(0) if slab else x, residual, w, eps)
        residual.copy_(s)
        out.copy_(y)
    return out


def silu_mul(x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """silu(x[..., :F]) * x[..., F:] (bf16 out); ``x`` may be a split-K slab [S, T, 2F]."""
    F = x.shape[-1] // 2
    slab = is_slab(x)
    if out is None:
        lead = (x.shape[1],) if slab else x.shape[:-1]
        out = torch.empty(*lead, F, dtype=torch.bfloat16 if slab else x.dtype, device=x.device)
    if _gpu(x):
        ext().silu_mul(out.view(-1, F), x if slab else x.reshape(-1, 2 * F))
    else:
        out.copy_(ref.silu_mul(x.sum(0) if slab else x))
    return out


def rope_kv_write(qkv, positions, cos_sin, q_out, k_cache, v_cache, slot_mapping, Hq: int, Hkv: int) -> None:
    """RoPE on q/k + paged KV write; ``qkv`` is bf16 [T, W] or a split-K slab [S, T, W]."""
    if _gpu(qkv):
        ext().rope_kv_write(qkv, positions, cos_sin, q_out, k_cache, v_cache, slot_mapping, int(Hq), int(Hkv))
    else:
        ref.rope_kv_write(qkv.sum(0) if is_slab(qkv) else qkv, positions, cos_sin, q_out, k_cache, v_cache,
                          slot_mapping, Hq, Hkv)


_TICKETS: dict = {}


def _tickets(dev: torch.device, n: int, pool: str = "decode") -> torch.Tensor:
    """Zeroed int32 counters for a kernel's ticket merge (re-armed by the kernel itself, so one buffer per device and
    pool serves every layer and step; allocated once, large, so graph capture never allocates). Pool "decode":
    decode attention, per row x kv head; pool "logprobs": ``token_logprobs``'s tickets and split partials."""
    t = _TICKETS.get((dev, pool))
    if t is None or t.numel() < n:
        t = _TICKETS[(dev, pool)] = torch.zeros(max(n, 1 << 16), dtype=torch.int32, device=dev)
    return t


def attn_decode_items(q, k_cache, v_cache, block_tables, items, out_part, lse_part, scale: float, out=None,
                      pre_part=None, merge=None) -> None:
    """Paged decode attention over work items (int32 [n, 8]: row b, key range [lo, hi), piece ``split`` of
    ``nsplit``, ``npre`` prefix partials in front). Each item writes its (O, lse2) partial to slot npre + split of
    [B, Hq, S_total, D]; with ``out`` (npre + nsplit <= 64 per row) the rows are instead merged with their prefix
    partials and written as final bf16 — a one-piece row directly, a split row by the last piece to finish (ticket
    counters, no merge kernel). ``pre_part``: bf16 prefix partials written by the tile-v3 cascade (slots < npre,
    out_part's shape) — half the bytes of the fp32 round trip. ``merge`` = (part [rows, Hq, S2, D], lse [rows, Hq,
    S2], out [rows, Hq, D]): other rows' fp32 partials (a step's prefill rows) merged into ``out`` by extra
    workgroups of the same launch, as ``attn_merge`` would."""
    if _gpu(q):
        tk = _tickets(q.device, q.shape[0] * k_cache.shape[1]) if out is not None else None
        mp, ml, mo = merge if merge is not None else (None, None, None)
        ext().attn_decode(q, k_cache, v_cache, block_tables, items, out_part, lse_part, float(scale), out, tk,
                          pre_part, mp, ml, mo)
        return
    ref.attn_decode_items(q, k_cache, v_cache, block_tables, items, out_part, lse_part, scale, out, pre_part)
    if merge is not None:
        ref.attn_merge(*merge)


def uniform_decode_items(seq_lens: torch.Tensor, kv_start: torch.Tensor | None, num_splits: int,
                         split_offset: int) -> torch.Tensor:
    """Decode items splitting every row's keys [kv_start, seq_len) into ``num_splits`` 32-key-aligned pieces, with
    partial slots from ``split_offset`` (built on the tensors' device, no host sync)."""
    B, S = seq_lens.numel(), int(num_splits)
    dev = seq_lens.device
    L = seq_lens.long()
    st = kv_start.long()[:B] if kv_start is not None else torch.zeros_like(L)
    a0 = st - st % 32
    nb = ((L - a0 + 31) // 32).clamp(min=0)
    bps = (nb + S - 1) // S
    b = torch.arange(B, device=dev).repeat_interleave(S)
    s = torch.arange(S, device=dev).repeat(B)
    blo = s * bps[b]
    bhi = torch.minimum(nb[b], blo + bps[b])
    lo = torch.maximum(st[b], a0[b] + blo * 32)
    hi = torch.maximum(lo, torch.minimum(L[b], a0[b] + bhi * 32))
    z = torch.zeros_like(b)
    return torch.stack([b, lo, hi, s, z + S, z + int(split_offset), z, z], 1).to(torch.int32).contiguous()


def attn_decode(q, k_cache, v_cache, block_tables, seq_lens, kv_start, out_part, lse_part, num_splits: int,
                split_offset: int, scale: float, out=None) -> None:
    """Uniform split-K decode (every row's keys [kv_start, seq_len) in ``num_splits`` pieces) on the work-item
    kernel: partials at slots [split_offset, split_offset + num_splits), or with ``out`` merged with the prefix
    partials [0, split_offset) into final bf16 rows (see ``attn_decode_items``)."""
    if out is not None and split_offset + num_splits > 64:
        raise ValueError("fused-merge decode needs <= 64 partials")
    items = uniform_decode_items(seq_lens[:q.shape[0]], kv_start, num_splits, split_offset)
    attn_decode_items(q, k_cache, v_cache, block_tables, items, out_part, lse_part, scale, out)


def attn_prefill(items, q, k_cache, v_cache, block_tables, q_limit, scale: float, out=None, out_part=None,
                 lse_part=None, variant: int = 0, alt_part=None, alt_lse=None, alt_tok_off: int = 0) -> None:
    """Work-item paged attention (chunked prefill / cascade prefix). ``items`` is int32 [n, 8]:
    (q_start, q_count, bt_row, kv_lo, kv_hi, split, alt, 0). Items with ``alt`` set (tile variant 3) write their
    partial into ``alt_part`` / ``alt_lse`` (fp32 [rows, Hq, S2, D], row = token - ``alt_tok_off``) instead of
    ``out_part``: the cascade's prefix pass over a step's new-turn prefill rows."""
    if _gpu(q):
        ext().attn_prefill(items, q, k_cache, v_cache, block_tables, q_limit, out, out_part, lse_part, float(scale),
                           int(variant), alt_part, alt_lse, int(alt_tok_off))
    else:
        ref.attn_prefill_items(items, q, k_cache, v_cache, block_tables, q_limit, scale, out, out_part, lse_part,
                               alt_part, alt_lse, alt_tok_off)


def tile_rows(variant: int = 0) -> int:
    """Query rows ((token, head) pairs of one KV head) per attn_prefill work item for a kernel variant."""
    return 256 if variant in (0, 3) else 128


def attn_merge(part, lse, out, lse_out=None, pre=None, npre: int = 0) -> None:
    """Log-sum-exp merge of the S partials per (row, head) of part f32 [rows, Hq, S, D] -> out bf16; with ``pre``
    (bf16, part's shape) slots [0, npre) are read from it (the cascade's prefix partials)."""
    if _gpu(part):
        ext().attn_merge(part, lse, out, lse_out, pre, int(npre))
    else:
        ref.attn_merge(part, lse, out, lse_out, pre, npre)


_SAMPLE_WS: dict = {}
_SAMPLE_SPLIT = int(__import__("os").environ.get("KAFKA_SAMPLE_SPLIT", "8"))


def _sample_ws(dev: torch.device, n: int) -> torch.Tensor:
    """Sampler workspace: 65536 zeroed per-row tickets (re-armed by the kernel) + split winners; allocated once per
    device, large enough for graph capture never to allocate."""
    t = _SAMPLE_WS.get(dev)
    if t is None or t.numel() < n:
        t = _SAMPLE_WS[dev] = torch.zeros(max(n, 65536 + 2 * 4096 * 8), dtype=torch.int32, device=dev)
    return t


LOGIT_BIAS_MAX = ref.LOGIT_BIAS_MAX  # entries of one request's logit_bias; a bias_tab row is twice as many ints


def sample(logits, temperature=None, top_p=None, top_k=None, seeds=None, step=None, out=None, proc=None,
           mask_tab=None, counts=None, bias_tab=None, rep_tab=None) -> torch.Tensor:
    """Sampled ids [B] (int64). ``proc`` int32 [B, 8] turns on the per-row logits processing of the kernel (grammar
    bitmask rows of ``mask_tab``, forced ids, presence / frequency penalties from ``counts``, which the sampler
    updates with every drawn token, sparse logit biases from rows of ``bias_tab``; engine/logits_proc.py builds all
    four). A ``proc`` row that names bias entries without a ``bias_tab`` is an error. ``rep_tab`` fp32 [slots, 2] holds
    the penalty slots' repetition penalties (r, 1 / r): a row whose slot has r != 1 multiplies the logits of its seen
    tokens (count word != 0; a prompt token carries COUNT_SEEN_PROMPT) by 1 / r if positive, else by r, first of all.
    Flags belong to slots whose ``rep_tab`` row has r != 1 and to no others: for a row without such a factor (or
    without ``rep_tab``) the kernel reads the whole count word as a count, so a flagged word there is a count of 2^30
    (engine/logits_proc.py sets and clears the two together). Passing ``rep_tab`` selects the kernel instantiation
    that knows the penalty; the engine passes it only while some slot holds a factor."""
    B = logits.shape[0]
    if out is None:
        out = torch.empty(B, dtype=torch.long, device=logits.device)
    if proc is not None and bias_tab is None and bool((proc[:B, 6] > 0).any()):  # (the engine always passes the table)
        raise ValueError("sample: proc rows carry logit-bias entries but no bias_tab was given")
    if _gpu(logits):
        V = logits.shape[1]
        nsplit = _SAMPLE_SPLIT if V >= 16384 else 1  # a row over 8 workgroups (greedy / plain temperature)
        ws = _sample_ws(logits.device, 65536 + 2 * B * nsplit) if nsplit > 1 else None
        ext().sample(logits, temperature, top_p, top_k, seeds, step, out, ws, nsplit, proc, mask_tab, counts,
                     bias_tab, rep_tab)
    else:
        ref.sample(logits, temperature, top_p, top_k, seeds, step, out, proc, mask_tab, counts, bias_tab, rep_tab)
    return out


class JsonTables:
    """What the JSON-mode ops read, on one device: the automaton's transition table, the tokens' bytes (CSR) and the
    EOS ids of ``table`` (engine/json_mode.JsonTable, kept for the CPU path). Built once per (table, device)."""

    def __init__(self, table, device):
        from kafka_llm_service_amd.engine import json_mode as jm

        self.table = table
        self.device = torch.device(device)
        self.V = table.V
        self.trans = torch.from_numpy(jm.TRANS.copy()).to(self.device)
        self.tok_off = torch.from_numpy(table.tok_off).to(self.device)
        # (padded: a table whose tokens are all empty still has an address)
        self.tok_bytes = torch.from_numpy(np.concatenate([table.tok_bytes, np.zeros(16, np.uint8)])).to(self.device)
        self.eos = torch.from_numpy(table.eos_ids).to(self.device)


def _json_check(tabs: JsonTables, rows, state, n_sampled: int | None = None) -> None:
    """The device-side values the kernels trust (CPU tensors only: the kernels skip a row that names a slot outside
    the state table)."""
    r = rows.reshape(-1, 2)
    if r.numel() and (int(r[:, 1].min()) < 0 or int(r[:, 1].max()) >= state.shape[0]
                      or (n_sampled is not None and (int(r[:, 0].min()) < 0 or int(r[:, 0].max()) >= n_sampled))):
        raise ValueError("json: a row names a slot outside the state table or a row outside the sampled ids")


def json_mask(tabs: JsonTables, rows, state, mask_tab, json_row0: int) -> None:
    """For every (sampled row, slot) pair of ``rows`` (int32 [k, 2]): row ``json_row0 + slot`` of ``mask_tab`` (int32
    [rows, >= ceil(V / 32)]) becomes the vocabulary mask of the slot's JSON automaton state ``state[slot]`` (int32
    [slots, 4]: state id, depth, stack bits, 0) — ``ref.json_mask_ref`` word for word. Launches and allocates nothing
    for k = 0."""
    if rows.shape[0] == 0:
        return
    if _gpu(mask_tab):
        ext().json_mask(tabs.trans, tabs.tok_off, tabs.tok_bytes, tabs.eos, rows, state, mask_tab, int(json_row0))
        return
    from kafka_llm_service_amd.engine import json_mode as jm

    _json_check(tabs, rows, state)
    W = tabs.table.W
    if json_row0 < 0 or json_row0 + state.shape[0] > mask_tab.shape[0] or mask_tab.shape[1] < W:
        raise ValueError("json_mask: the mask table does not hold the slots' rows")
    for slot in rows[:, 1].tolist():
        words = ref.json_mask_ref(jm.record_state(state[slot].numpy()), tabs.table)
        mask_tab[json_row0 + slot, :W] = torch.from_numpy(words.view(np.int32).copy())


def json_advance(tabs: JsonTables, rows, sampled, state) -> None:
    """Behind the sampler: ``state[slot]`` of every (sampled row, slot) pair advances over the bytes of the id
    ``sampled[row]`` (int64) — ``ref.json_advance_ref``. Launches nothing for k = 0."""
    if rows.shape[0] == 0:
        return
    if _gpu(state):
        ext().json_advance(tabs.trans, tabs.tok_off, tabs.tok_bytes, rows, sampled, state)
        return
    from kafka_llm_service_amd.engine import json_mode as jm

    _json_check(tabs, rows, state, sampled.shape[0])
    for r, slot in rows.tolist():
        st = ref.json_advance_ref(jm.record_state(state[slot].numpy()), int(sampled[r]), tabs.table)
        state[slot] = torch.from_numpy(jm.state_record(st))


SCHEMA_MASK_TOKENS = 1024  # tokens one workgroup of schema_mask_kernel walks per staged table (a multiple of 256; measured)
SCHEMA_MASK_DWORD = True   # token bytes through aligned 4-byte loads


class SchemaTables:
    """The device pool of compiled schema tables (engine/json_schema.SchemaDfa) the structured-output ops read:
    ``strans`` uint16 [n, SCHEMA_TAB_BYTES / 2], ``scls`` uint8 [n, 256], ``sdim`` int32 [n, 2] = (S, C). The host keeps
    each loaded table (``dfas``: the CPU path walks it through the reference) and so knows which kernel instantiations
    a launch needs."""

    def __init__(self, n: int, device):
        from kafka_llm_service_amd.engine import json_schema as js

        if n < 1:
            raise ValueError("schema tables: the pool needs at least one buffer")
        self.n, self.device = int(n), torch.device(device)
        self.strans = torch.zeros(self.n, js.SCHEMA_TAB_BYTES // 2, dtype=torch.uint16, device=self.device)
        self.scls = torch.zeros(self.n, 256, dtype=torch.uint8, device=self.device)
        self.sdim = torch.zeros(self.n, 2, dtype=torch.int32, device=self.device)
        self.dfas: list = [None] * self.n

    def load(self, idx: int, cls, trans, upload=None) -> None:
        """Buffer ``idx`` becomes the table (``cls`` uint8 [256], ``trans`` uint16 [S, C]); ``upload``: numpy ->
        device tensor (default: a plain copy). The table is checked here: the kernels trust its entries."""
        from kafka_llm_service_amd.engine import json_schema as js

        cls, trans = np.array(cls), np.array(trans)  # (own, writable, contiguous copies)
        if not 0 <= int(idx) < self.n:
            raise ValueError(f"schema tables: buffer {idx} outside the pool of {self.n}")
        js.check_tables(cls, trans)
        up = upload or (lambda a: torch.from_numpy(a).to(self.device))
        S, C = trans.shape
        # one H2D copy of (S, C), cls and trans as int32 words, the type every upload path knows (an odd table is padded
        # by one zero entry, still inside its buffer), then three device copies into the pool
        flat = trans.reshape(-1)
        if flat.size % 2:
            flat = np.concatenate([flat, np.zeros(1, np.uint16)])
        dev = up(np.concatenate([np.array([S, C], np.int32), cls.view(np.int32), flat.view(np.int32)]))
        self.sdim[idx].copy_(dev[:2])
        self.scls[idx].view(torch.int32).copy_(dev[2:66])
        self.strans[idx].view(torch.int32)[:flat.size // 2].copy_(dev[66:])
        self.dfas[idx] = js.SchemaDfa(cls, trans, "")

    def kinds(self, used=None) -> tuple[int, int]:
        """(bit 0: a table is staged in LDS; bit 1: one is walked in global memory, the LDS bytes a launch allocates:
        the largest table that fits SCHEMA_LDS_BYTES, rounded up to 16) over the buffers ``used`` — the tables a
        launch's rows name, when the caller knows them on the host — or over every loaded buffer."""
        from kafka_llm_service_amd.engine import json_schema as js

        k = lds = 0
        for d in (self.dfas if used is None else [self.dfas[int(t)] for t in used if 0 <= int(t) < self.n]):
            if d is not None:
                if d.nbytes <= js.SCHEMA_LDS_BYTES:
                    k, lds = k | 1, max(lds, (d.nbytes + 15) & ~15)
                else:
                    k |= 2
        return k, lds


def _table_rows(pool: SchemaTables, rows, width: int, state, n_sampled: int, V: int) -> list:
    """The rows the kernels would not skip (CPU tensors only), as lists of ``width`` ints: 3 (sampled row, slot, table)
    or 5 (... open, close). A bad schema row raises, as ``_json_check``; a bad tool row is left out, as on the GPU."""
    from kafka_llm_service_amd.engine import tool_automaton as ta

    keep = []
    for row in rows.reshape(-1, width).tolist():
        r, slot, t = row[:3]
        ok = (0 <= r < n_sampled and 0 <= slot < state.shape[0] and 0 <= t < pool.n and pool.dfas[t] is not None
              and int(state[slot, 3]) == t + 1)
        if ok and width == 5:
            ok = 0 <= row[3] < V and 0 <= row[4] < V and 0 <= int(state[slot, 1]) < ta.TOOL_PHASES
        if ok:
            keep.append(row)
        elif width == 3:
            raise ValueError("schema: a row names a sampled row, a slot or a table outside its array, or a slot whose "
                             "record belongs to another table")
    return keep


def _table_mask(tabs: JsonTables, pool: SchemaTables, rows, width: int, n_sampled: int, state, mask_tab,
                json_row0: int, tokens, dword, used) -> None:
    """``schema_mask`` (width 3) and ``tool_mask`` (width 5): one kernel pair, one CPU loop over the references."""
    if rows.shape[0] == 0:
        return
    if _gpu(mask_tab):
        kinds, lds = pool.kinds(used)
        head = (pool.strans, pool.scls, pool.sdim, tabs.tok_off, tabs.tok_bytes)
        tail = (lds, int(tokens or SCHEMA_MASK_TOKENS), SCHEMA_MASK_DWORD if dword is None else bool(dword))
        if width == 3:
            ext().schema_mask(*head, tabs.eos, rows, int(n_sampled), state, mask_tab, int(json_row0), kinds, *tail)
        else:
            ext().tool_mask(*head, rows, int(n_sampled), state, mask_tab, int(json_row0), kinds or 2, *tail)
        return
    keep = _table_rows(pool, rows, width, state, n_sampled, tabs.table.V)
    W = tabs.table.W
    if json_row0 < 0 or json_row0 + state.shape[0] > mask_tab.shape[0] or mask_tab.shape[1] < W:
        raise ValueError("the mask table does not hold the slots' rows")
    for _, slot, t, *env in keep:
        if width == 3:
            words = ref.schema_mask_ref(int(state[slot, 0]) & 0xFFFFFFFF, pool.dfas[t], tabs.table)
        else:
            words = ref.tool_mask_words(state[slot].numpy(), *env, pool.dfas[t], tabs.table)
        mask_tab[json_row0 + slot, :W] = torch.from_numpy(words.view(np.int32).copy())


def _table_advance(tabs: JsonTables, pool: SchemaTables, rows, width: int, sampled, state) -> None:
    """``schema_advance`` (width 3) and ``tool_advance`` (width 5)."""
    if rows.shape[0] == 0:
        return
    if _gpu(state):
        launch = ext().schema_advance if width == 3 else ext().tool_advance
        launch(pool.strans, pool.scls, pool.sdim, tabs.tok_off, tabs.tok_bytes, rows, sampled, state)
        return
    for r, slot, t, *env in _table_rows(pool, rows, width, state, sampled.shape[0], tabs.table.V):
        if width == 3:
            state[slot, 0] = ref.schema_advance_ref(int(state[slot, 0]) & 0xFFFFFFFF, int(sampled[r]), pool.dfas[t],
                                                    tabs.table)
        else:
            state[slot] = torch.from_numpy(ref.tool_advance_ref(state[slot].numpy(), int(sampled[r]), *env,
                                                                pool.dfas[t], tabs.table))


def schema_mask(tabs: JsonTables, pool: SchemaTables, rows, n_sampled: int, state, mask_tab, json_row0: int,
                tokens: int | None = None, dword: bool | None = None, used=None) -> None:
    """For every (sampled row, slot, table) of ``rows`` (int32 [k, 3]): row ``json_row0 + slot`` of ``mask_tab`` becomes
    the vocabulary mask of the slot's schema state ``state[slot, 0]`` over table ``table`` of ``pool`` —
    ``ref.schema_mask_ref`` word for word. ``tabs`` supplies the token bytes and the EOS ids. ``used``: the distinct
    table buffers the rows name, if the host knows them (the engine does): the launch's LDS is then sized by those
    tables, not by everything the pool still holds. Launches nothing for k = 0."""
    _table_mask(tabs, pool, rows, 3, n_sampled, state, mask_tab, json_row0, tokens, dword, used)


def schema_advance(tabs: JsonTables, pool: SchemaTables, rows, sampled, state) -> None:
    """Behind the sampler: ``state[slot, 0]`` of every row advances over the bytes of the id ``sampled[row]`` (int64)
    — ``ref.schema_advance_ref``; the record's other words stay. Launches nothing for k = 0."""
    _table_advance(tabs, pool, rows, 3, sampled, state)


def tool_mask(tabs: JsonTables, pool: SchemaTables, rows, n_sampled: int, state, mask_tab, json_row0: int,
              tokens: int | None = None, dword: bool | None = None, used=None) -> None:
    """For every (sampled row, slot, table, open, close) of ``rows`` (int32 [k, 5]): row ``json_row0 + slot`` of
    ``mask_tab`` becomes the vocabulary mask of the slot's tool record ``state[slot]`` — ``ref.tool_mask_ref`` word for
    word (engine/tool_automaton.py: the envelope of a tool call around the body's table ``table`` of ``pool``). ``used``
    as for ``schema_mask``. A row the kernel's skip rules name is left alone. Launches nothing for k = 0."""
    _table_mask(tabs, pool, rows, 5, n_sampled, state, mask_tab, json_row0, tokens, dword, used)


def tool_advance(tabs: JsonTables, pool: SchemaTables, rows, sampled, state) -> None:
    """Behind the sampler: the record ``state[slot]`` of every row moves over the id ``sampled[row]`` (int64) —
    ``ref.tool_advance_ref``; word 3 stays. Launches nothing for k = 0."""
    _table_advance(tabs, pool, rows, 5, sampled, state)


LOGPROBS_MAX_K = 20      # OpenAI's top_logprobs bound; the kernel's register / LDS budget (csrc/logprobs.hip)
_LP_TICKETS = 8192       # LP_MAX_ROWS of csrc/logprobs.hip: ticket counters in front of the partials
_LP_PART = 2 + 2 * LOGPROBS_MAX_K


def logprob_records(R: int, k: int, device) -> torch.Tensor:
    """A packed record buffer for ``token_logprobs``: [R, 1 + 2k] 4-byte words, row = logprob | k top logprobs | k top
    ids (int32 bits), so a step's records are ONE device->host copy. ``unpack_logprob_records`` gives the views."""
    return torch.empty(R, 1 + 2 * k, dtype=torch.float32, device=device)


def unpack_logprob_records(buf: torch.Tensor, k: int) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(tok_lp [R], top_lp [R, k], top_id [R, k] int32): three views of a packed record buffer [R, 1 + 2k] float32
    (on any device, or its pinned host copy) — the ``out`` of ``token_logprobs``."""
    return buf[:, 0], buf[:, 1:1 + k], buf.view(torch.int32)[:, 1 + k:1 + 2 * k]


def logprobs_split(V: int) -> int:
    """Workgroups per row: 8 like the sampler, more when a slice would not fit the kernel's registers (16,384
    entries per workgroup); one below 16,384 entries."""
    if V < 16384:
        return 1
    return min(64, max(_SAMPLE_SPLIT if _SAMPLE_SPLIT > 1 else 8, -(-V // 16384)))


def token_logprobs(logits, tokens, rows=None, k: int = 0, out=None):
    """Log-probabilities of the RAW logits (before temperature, penalties and grammar masks): for every scored row r
    (``rows``: row ids of ``logits``, default all) -> (tok_lp [R] f32 = log softmax at ``tokens[row]``, top_lp [R, k]
    f32 and top_id [R, k] i32 = the k (0..20) most likely tokens in the order (value descending, index ascending)).
    ``tokens`` is indexed by LOGITS row (the sampler's output as it stands). ``out`` = three such tensors sharing a row
    stride, e.g. ``unpack_logprob_records(logprob_records(R, k, device), k)`` (one packed buffer). GPU tensors run csrc/logprobs.hip (one streaming read of
    each row, nothing allocated per call with ``out`` and device ``rows``: graph-safe); CPU tensors the fp32
    reference."""
    k = int(k)
    if not 0 <= k <= LOGPROBS_MAX_K:
        raise ValueError(f"k must be in 0..{LOGPROBS_MAX_K}")
    B, V = logits.shape
    dev = logits.device
    if rows is not None and not isinstance(rows, torch.Tensor):
        ra = np.asarray(rows, dtype=np.int64).reshape(-1)
        if ra.size and (ra.min() < 0 or ra.max() >= B):
            raise ValueError(f"rows must lie in [0, {B})")
        rows = torch.from_numpy(ra.astype(np.int32)).to(dev)
    R = B if rows is None else int(rows.numel())
    if out is None:
        out = unpack_logprob_records(logprob_records(R, k, dev), k)
    tok_lp, top_lp, top_id = out
    if _gpu(logits):
        if rows is not None and rows.dtype != torch.int32:
            rows = rows.to(torch.int32)
        nsplit = logprobs_split(V)
        # a pool of its own (tickets | partials), sized once for 1,024 rows x 8 splits so no call allocates
        ws = _tickets(dev, _LP_TICKETS + max(R * nsplit, 1024 * 8) * _LP_PART, pool="logprobs") if nsplit > 1 else None
        ext().token_logprobs(logits, tokens, rows, k, tok_lp, top_lp, top_id, ws, nsplit)
    else:
        a, b, c = ref.token_logprobs(logits, tokens, rows, k)
        tok_lp[:R].copy_(a)
        if k:
            top_lp[:R, :k].copy_(b)
            top_id[:R, :k].copy_(c)
    return tok_lp, top_lp, top_id


def tile_weight(w: torch.Tensor, glu: bool = False) -> torch.Tensor:
    """Row-major weight [N, K] -> the wave-tiled layout [N/32, K/16, 64, 8] read by the weight-streaming decode GEMM
    (csrc/wstream_gemm.hip): lane l = (r = l % 32, h = l // 32) of tile (nb, kb) holds W[32 nb + r, 16 kb + 8 h : +8].
    ``glu``: W = [gate; up] (N = 2F); the 32-row tiles are interleaved gate_0, up_0, gate_1, up_1, ... so one
    workgroup holds matching gate/up columns and the GEMM can emit silu(gate) * up directly."""
    N, K = w.shape
    t = w.reshape(N // 32, 32, K // 16, 2, 8).permute(0, 2, 3, 1, 4)
    if glu:
        t = t.reshape(2, N // 64, K // 16, 2, 32, 8).transpose(0, 1)
    return t.contiguous().view(N // 32, K // 16, 64, 8)


def untile_weight(wt: torch.Tensor, glu: bool = False) -> torch.Tensor:
    nb, kb = wt.shape[0], wt.shape[1]
    if glu:
        wt = wt.view(nb // 2, 2, kb, 64, 8).transpose(0, 1).reshape(nb, kb, 64, 8)
    return wt.reshape(nb, kb, 2, 32, 8).permute(0, 3, 1, 2, 4).reshape(nb * 32, kb * 16)


# fp8 weights (weight_dtype="fp8"): e4m3 wave tiles uint8 [N/32, K/32, 64, 16] plus fp32 power-of-two row scales [N]
# (layout and quantisation rule: reference.tile_weight_fp8); linear_stream / linear_glu take them with ``scale``.
tile_weight_fp8 = ref.tile_weight_fp8
untile_weight_fp8 = ref.untile_weight_fp8


def is_fp8_weight(wt: torch.Tensor | None) -> bool:
    return wt is not None and wt.dtype == torch.uint8


# MXFP4 weights (weight_dtype="mxfp4"): e2m1 wave tiles float4_e2m1fn_x2 [N/32, K/64, 64, 16] plus the e8m0 block-scale
# image float8_e8m0fnu [N/32, K/64, 32, 2] (layout and quantisation rule: reference.tile_weight_mxfp4 / mxfp4_quant);
# linear_stream / linear_glu take them with ``scale``. The tile dtype tells the three formats apart.
mxfp4_quant = ref.mxfp4_quant
tile_weight_mxfp4 = ref.tile_weight_mxfp4
untile_weight_mxfp4 = ref.untile_weight_mxfp4


_F4 = torch.float4_e2m1fn_x2


def is_mxfp4_weight(wt: torch.Tensor | None) -> bool:
    return wt is not None and wt.dtype == _F4


# ---- weight tile formats of the streaming GEMMs -------------------------------------------------------------------
# The one place that knows them: everything below (and models/llama.py) looks a format up by the TILE dtype
# (WEIGHT_FORMATS) or by its weight_dtype name (WEIGHT_DTYPES) and reads what it needs from the entry.
class WeightFormat(NamedTuple):
    name: str                           # the weight_dtype of enable_stream_weights / EngineConfig
    abi: int                            # csrc/kafka_abi.h WF_*
    vk: int                             # K columns of one 16-B tile vector: tiles are [N/32, K/vk, 64, 32 B / vk elements]
    tile: Callable                      # (w [N, K], glu) -> (tiles, scale or None)
    untile: Callable                    # (tiles, scale, glu) -> row-major bf16 [N, K] (quantised: the dequantised values)
    scale_dtype: torch.dtype | None     # None: the tiles have no scale
    scale_shape: Callable | None        # the tiles' shape -> their scale's (leading expert dims pass through)
    scale_name: str                     # for messages
    raw: bool                           # the extension takes tiles and scale viewed as uint8
    experts: bool                       # the grouped (MoE) kernel takes this format


# (tile / untile go through this module's names at call time, so a test can wrap e.g. ``ops.untile_weight_fp8``)
WEIGHT_FORMATS = {
    torch.bfloat16: WeightFormat("bf16", 0, 16, lambda w, glu=False: (tile_weight(w, glu), None),
                                 lambda wt, scale, glu=False: untile_weight(wt, glu), None, None, "", False, True),
    torch.uint8: WeightFormat("fp8", 1, 32, lambda w, glu=False: tile_weight_fp8(w, glu),
                              lambda wt, scale, glu=False: untile_weight_fp8(wt, scale, glu), torch.float32,
                              lambda s: (*s[:-4], s[-4] * 32), "row scales", False, True),
    _F4: WeightFormat("mxfp4", 2, 64, lambda w, glu=False: tile_weight_mxfp4(w, glu),
                      lambda wt, scale, glu=False: untile_weight_mxfp4(wt, scale, glu), torch.float8_e8m0fnu,
                      lambda s: (*s[:-2], 32, 2), "block-scale image", True, True),
}
WEIGHT_DTYPES = {f.name: f for f in WEIGHT_FORMATS.values()}


def weight_format(weight_dtype: str) -> WeightFormat:
    f = WEIGHT_DTYPES.get(weight_dtype)
    if f is None:
        raise ValueError(f"weight_dtype must be {', '.join(WEIGHT_DTYPES)}, not {weight_dtype!r}")
    return f


def _check_scale(fn: str, f: WeightFormat, wt: torch.Tensor, scale: torch.Tensor | None) -> None:
    """Quantised tiles need the scale tensor their format defines (dtype and shape)."""
    if scale is None:
        raise ValueError(f"{fn}: {f.name} weight tiles need their {f.scale_name} (scale=)")
    if scale.dtype != f.scale_dtype or scale.shape != f.scale_shape(wt.shape):  # (torch.Size compares as a tuple)
        raise ValueError(f"{fn}: the scale of {f.name} tiles {tuple(wt.shape)} must be their {f.scale_dtype} "
                         f"{f.scale_name} {f.scale_shape(wt.shape)}, not {scale.dtype} {tuple(scale.shape)}")


def tiled_dims(wt: torch.Tensor) -> tuple[int, int]:
    """(N, K) of a wave-tiled weight [N/32, K/vk, 64, .] of any format."""
    return wt.shape[0] * 32, wt.shape[1] * WEIGHT_FORMATS[wt.dtype].vk


def tile_weight_as(w: torch.Tensor, weight_dtype: str, glu: bool = False):
    """Row-major [N, K] -> (tiles, scale or None) of the format ``weight_dtype`` ("bf16", "fp8", "mxfp4")."""
    return weight_format(weight_dtype).tile(w, glu)


def untile_weight_as(wt: torch.Tensor, scale: torch.Tensor | None, glu: bool = False) -> torch.Tensor:
    """The row-major bf16 [N, K] weight of tiles of any format (quantised ones dequantised, exactly)."""
    return WEIGHT_FORMATS[wt.dtype].untile(wt, scale, glu)


def tiled_weight_bytes(shape, weight_dtype: str) -> int:
    """Bytes of the tiles and scales of a [..., N, K] weight in the format ``weight_dtype``."""
    f = weight_format(weight_dtype)
    n = math.prod(shape) * 32 // f.vk
    if f.scale_dtype is not None:
        n += math.prod(f.scale_shape((*shape[:-2], shape[-2] // 32, shape[-1] // f.vk, 64, 16))) * f.scale_dtype.itemsize
    return n


def _refuse_quantised(fn: str, wt: torch.Tensor) -> None:
    """The kernels behind ``fn`` read bf16 tiles only: quantised ones are refused instead of misread (the callers test
    the dtype inline: they sit on the decode step's host path)."""
    raise ValueError(f"{fn}: takes bf16 weight tiles only, not {wt.dtype} tiles (use linear_stream / linear_glu)")


# Steps of up to this many rows run the dense projections on the weight-streaming kernel (csrc/wstream_gemm.hip).
# The kernel takes up to 256 rows: one 192-row tile (MT = 6) up to 192, beyond that two row tiles of 128 sharing each
# weight slice through the MALL, where it loses to hipBLASLt (gate_up 101 vs 66 us at 168..248 rows; bench 7,359 vs
# 7,546 tok/s, profiles/r02/stream_max_m_256_rejected.jsonl). The 192-row tile only ties the skinny GEMM + hipBLASLt
# path of 129..192-row steps (8,725 vs 8,732 tok/s, profiles/r06/mt6/), so the default stays 128; tiled-only models
# (no row-major copy for hipBLASLt) stream every step up to 256 rows. Env KAFKA_STREAM_MAX_M (1..256).
STREAM_MAX_M = max(1, min(256, int(os.environ.get("KAFKA_STREAM_MAX_M", "128"))))
STREAM_KERNEL_MAX_M = 256


def stream_plan(M: int, N: int, K: int, max_splits: int = 8) -> tuple[int, int, int] | None:
    """(row tiles, K chunk, splits) of the decode GEMM for a shape, None if unsupported (same rule as
    kafka_wstream_plan in csrc/wstream_gemm.hip, mirrored so CPU runs take the same split decisions)."""
    if M < 1 or M > STREAM_KERNEL_MAX_M or N % 32 or N <= 0:
        return None
    mt = 1 if M <= 32 else (2 if M <= 64 else (3 if M <= 96 else (4 if M <= 128 or M > 192 else 6)))
    kc = 128 if mt >= 4 else 256
    if K % kc or K <= 0:
        return None
    nx, chunks, s = (N + 127) // 128 * ((M + 32 * mt - 1) // (32 * mt)), K // kc, 1
    target = 192
    while s * 2 <= max_splits and s * 2 <= 8 and chunks % (s * 2) == 0 and nx * s < target:
        s *= 2
    return mt, kc, s


SKINNY_MIN_M, SKINNY_MAX_M = 129, 256


def skinny_plan(M: int, N: int, K: int, max_splits: int = 8) -> int:
    """Splits of the skinny GEMM (csrc/skinny_gemm.hip kafka_skinny_plan, mirrored for CPU runs); 0 = unsupported."""
    if M < SKINNY_MIN_M or M > SKINNY_MAX_M or N % 128 or K % 64:
        return 0
    nx, s = N // 128, 1
    while s * 2 <= max_splits and nx * s < 192 and K % (64 * s * 2) == 0 and K // (s * 2) >= 256:
        s *= 2
    return s


def linear_skinny(x: torch.Tensor, wt: torch.Tensor, max_splits: int = 8, glu: bool = False) -> torch.Tensor:
    """y = x @ W^T for 129..256 rows from the wave-tiled weight (mixed decode + prefill steps): bf16 [M, N] (or the
    activated [M, N/2] with ``glu``) for one split, else fp32 split-K slabs [S, M, N] in gate | up order for glu."""
    if wt.dtype != torch.bfloat16:
        _refuse_quantised("linear_skinny", wt)
    M, K = x.shape
    N = wt.shape[0] * 32
    S = skinny_plan(M, N, K, max_splits)
    if S == 0:
        raise ValueError(f"linear_skinny: unsupported shape M={M} N={N} K={K}")
    if _gpu(x):
        if S == 1:
            y = torch.empty(M, N // 2 if glu else N, dtype=x.dtype, device=x.device)
            ext().skinny_gemm(x, wt, y, None, 1, bool(glu))
            return y
        p = torch.empty(S, M, N, dtype=torch.float32, device=x.device)
        ext().skinny_gemm(x, wt, None, p, int(S), bool(glu))
        return p
    w = untile_weight(wt, glu).float()
    y = x.float() @ w.t()
    if S == 1:
        return (ref.silu_mul(y) if glu else y).to(x.dtype)
    p = torch.zeros(S, M, N, dtype=torch.float32)
    p[0] = y
    return p


def linear_stream(x: torch.Tensor, wt: torch.Tensor, max_splits: int = 8, nt: bool = True,
                  glu: bool = False, scale: torch.Tensor | None = None) -> torch.Tensor:
    """y = x @ W^T for decode-sized M (<= 128) from the wave-tiled weight ``wt``: the weight-streaming MFMA kernel.
    Returns bf16 [M, N] when the plan has one split, else the fp32 split-K slabs [S, M, N] (a slab; the consumer
    kernels sum it while loading). ``glu`` (wt tiled with glu=True): a one-split plan returns the ACTIVATED
    silu(gate) * up [M, N/2] (fused epilogue); a split plan returns gate | up slabs as usual (see ``linear_glu``).
    fp8 tiles (uint8 ``wt`` from ``tile_weight_fp8``) need their row scales ``scale``, MXFP4 tiles (``tile_weight_mxfp4``)
    their e8m0 block-scale image; same plans and outputs."""
    M, K = x.shape
    f = WEIGHT_FORMATS[wt.dtype]
    if f.scale_dtype is None:
        scale = None
    else:
        _check_scale("linear_stream", f, wt, scale)
        if not nt:
            raise ValueError(f"linear_stream: {f.name} weight tiles stream non-temporally only (nt=False unsupported)")
        if wt.shape[1] * f.vk != K:
            raise ValueError(f"linear_stream: x has K={K}, the {f.name} tiles K={wt.shape[1] * f.vk}")
    N = wt.shape[0] * 32
    plan = stream_plan(M, N, K, max_splits)
    if plan is None:
        raise ValueError(f"linear_stream: unsupported shape M={M} N={N} K={K}")
    S = plan[2]
    if _gpu(x):
        y = p = None
        if S == 1:
            y = torch.empty(M, N // 2 if glu else N, dtype=x.dtype, device=x.device)
        else:
            p = torch.empty(S, M, N, dtype=torch.float32, device=x.device)
        if f.raw:
            wt, scale = wt.view(torch.uint8), scale.view(torch.uint8)
        ext().wstream_gemm(x, wt, y, p, int(max_splits), bool(nt), bool(glu), scale, f.abi)
        return y if S == 1 else p
    w = f.untile(wt, scale, glu).float()
    xf = x.float()
    if S == 1:
        y = xf @ w.t()
        if glu:
            return ref.silu_mul(y).to(x.dtype)
        return y.to(x.dtype)
    ks = K // S
    return torch.stack([xf[:, s * ks:(s + 1) * ks] @ w[:, s * ks:(s + 1) * ks].t() for s in range(S)])


def linear_glu(x: torch.Tensor, wt: torch.Tensor, max_splits: int = 8,
               scale: torch.Tensor | None = None) -> torch.Tensor:
    """silu(x @ Wg^T) * (x @ Wu^T) from GLU-tiled gate_up weights: fused into the GEMM epilogue when the plan has one
    split, else the GEMM's slabs go through silu_mul. ``scale``: the row scales of fp8 tiles / the block-scale image of
    MXFP4 tiles."""
    N = wt.shape[0] * 32
    plan = stream_plan(x.shape[0], N, x.shape[1], max_splits)
    y = linear_stream(x, wt, max_splits, glu=True, scale=scale)
    return y if plan is not None and plan[2] == 1 else silu_mul(y)


# ---- fused decode layer (csrc/wstream_gemm.hip FIN_*): deferred RMSNorm + split-K finishers ----------------------
# A decode layer runs as qkv(+RoPE/KV write) -> attention -> o(+residual add, next norm) -> gate_up(+row scale,
# SwiGLU) -> down(+residual add, next norm): the RMSNorm and RoPE kernels leave the step. The residual producer writes
# X' = bf16(h * w) and per-128-column partial sums of h^2 (``ss`` fp32 [d/128, T]); the consumer GEMM scales each
# output row by r = rsqrt(sum(ss) / d + eps) — rmsnorm(h) . W^T = r * ((h * w) . W^T).

def fin_row_scale(ss: torch.Tensor | None, M: int, d: int, eps: float) -> torch.Tensor | None:
    """r[m] = rsqrt(sum_j ss[j, m] / d + eps) (fp32 [M]) — the deferred RMSNorm scale; None without partials."""
    if ss is None:
        return None
    return torch.rsqrt(ss[:, :M].float().sum(0) / d + eps)


FIN_POOLS = ("fin", "fin_o", "fin_down", "fin_qkv")


def fin_errors(dev: torch.device) -> int:
    """Error words of the fused GEMM finishers (the last int of each ticket pool; csrc FinArgs::err): nonzero if a
    finisher ran on another XCD than the splits that kept their slabs in their home L2 — the result of that launch is
    unreliable. Checked by the tests, smoke() and the bench (a host sync: not for the hot path)."""
    n = 0
    for pool in FIN_POOLS:
        t = _TICKETS.get((dev, pool))
        if t is not None:
            n |= int(t[-1].item())
    return n


# KAFKA_FIN_STAMPS=<file.json>: every fused GEMM launch records per-workgroup phase stamps (csrc FinArgs::stamps) and
# the anatomy of the last launches per kind is written to that file at exit (benchmarks/fused_bench.py reads the same
# stamps in isolation; this is the in-engine view)
_FIN_STAMPS = os.environ.get("KAFKA_FIN_STAMPS")
_STAMP_LOG: list = []


def _stamps_for(kind: str, grid: int, dev: torch.device):
    if not _FIN_STAMPS:
        return None
    if not _STAMP_LOG:
        import atexit
        atexit.register(_dump_stamps)
    t = torch.zeros(grid * 8 + 8, dtype=torch.long, device=dev)
    _STAMP_LOG.append((kind, grid, t))
    del _STAMP_LOG[:-2000]
    return t


def _dump_stamps() -> None:
    import json
    import statistics
    out: dict = {}
    for kind, grid, t in _STAMP_LOG:
        a = t[:grid * 8].view(grid, 8).cpu().double() / 100.0
        a = a - a[:, 0].min()
        fin = a[:, 4] > 0
        rec = {"loop_max": float((a[:, 1] - a[:, 0]).max()), "last_loop_end": float(a[:, 1].max()),
               "first_start_to_last_start": float(a[:, 0].max())}
        if fin.any():
            rec.update(end=float(a[fin, 4].max()), tail=float(a[fin, 4].max() - a[:, 1].max()),
                       fin_med=float((a[fin, 4] - a[fin, 3]).median()),
                       drain_med=float((a[a[:, 2] > 0, 2] - a[a[:, 2] > 0, 1]).median()) if (a[:, 2] > 0).any() else 0.0,
                       ticket_med=float((a[fin, 3] - a[fin, 2]).median()))
        out.setdefault(f"{kind}/grid{grid}", []).append(rec)
    summary = {k: {f: round(statistics.median(r[f] for r in v if f in r), 2) for f in v[-1]} | {"calls": len(v)}
               for k, v in out.items()}
    with open(_FIN_STAMPS, "w") as f:
        json.dump(summary, f, indent=1)


def _fin_scratch(x: torch.Tensor, N: int, max_splits: int) -> tuple[int, torch.Tensor | None]:
    M, K = x.shape
    plan = stream_plan(M, N, K, max_splits)
    if plan is None or M > 128 or N % 128:
        raise ValueError(f"fused decode GEMM: unsupported shape M={M} N={N} K={K}")
    S = plan[2]
    return S, (torch.empty(S, M, N, dtype=torch.float32, device=x.device) if S > 1 else None)


def linear_res(x: torch.Tensor, wt: torch.Tensor, resid: torch.Tensor, nw: torch.Tensor, xn: torch.Tensor,
               ss_out: torch.Tensor, max_splits: int = 8, pool: str = "fin") -> None:
    """resid <- bf16(resid + x @ W^T) in place; xn <- bf16(resid * nw); ss_out[cb, m] = sum of resid[m, 128 cb:+128]^2
    (the o / down projection with the residual add and the next RMSNorm's producer half, csrc FIN_RES)."""
    if wt.dtype != torch.bfloat16:
        _refuse_quantised("linear_res", wt)
    N = wt.shape[0] * 32
    if _gpu(x):
        S, p = _fin_scratch(x, N, max_splits)
        ext().wstream_fin(1, x, wt, None, p, _tickets(x.device, N // 128 + 1, pool), None, 0.0, resid, nw, xn, ss_out,
                          None, None, None, None, None, None, 0, 0, int(max_splits),
                          _stamps_for(pool, N // 128 * S, x.device))
        return
    M = x.shape[0]
    y = x.float() @ untile_weight(wt).float().t()
    s = (resid.float() + y).to(resid.dtype)
    resid.copy_(s)
    xn.copy_((s.float() * nw.float()).to(xn.dtype))
    ss_out[:, :M] = s.float().pow(2).view(M, N // 128, 128).sum(-1).t()


def linear_qkv_rope(x: torch.Tensor, wt: torch.Tensor, ss_in: torch.Tensor | None, eps: float, positions, cos_sin,
                    q_out, k_cache, v_cache, slot_mapping, Hq: int, Hkv: int, max_splits: int = 8,
                    pool: str = "fin_qkv") -> None:
    """RoPE + paged KV write of r * (x @ Wqkv^T) (r: the deferred RMSNorm of x from ``ss_in``, or 1), in the QKV
    GEMM's split-K finisher (csrc FIN_ROPE); bf16 caches, head dim 128."""
    if wt.dtype != torch.bfloat16:
        _refuse_quantised("linear_qkv_rope", wt)
    N = wt.shape[0] * 32
    M, K = x.shape
    if _gpu(x):
        S, p = _fin_scratch(x, N, max_splits)
        ext().wstream_fin(2, x, wt, None, p, _tickets(x.device, N // 128 + 1, pool), ss_in, float(eps), None, None,
                          None, None, positions, cos_sin, q_out, k_cache, v_cache, slot_mapping, int(Hq), int(Hkv),
                          int(max_splits), _stamps_for(pool, N // 128 * S, x.device))
        return
    y = x.float() @ untile_weight(wt).float().t()
    r = fin_row_scale(ss_in, M, K, eps)
    if r is not None:
        y = y * r[:, None]
    ref.rope_kv_write(y, positions, cos_sin, q_out, k_cache, v_cache, slot_mapping, Hq, Hkv)


def linear_glu_rs(x: torch.Tensor, wt: torch.Tensor, ss_in: torch.Tensor | None, eps: float) -> torch.Tensor:
    """silu(r g) * (r u) with [g | u] = x @ Wgu^T from GLU-tiled weights, one split (csrc FIN_GLU); r as above."""
    if wt.dtype != torch.bfloat16:
        _refuse_quantised("linear_glu_rs", wt)
    N = wt.shape[0] * 32
    M, K = x.shape
    if _gpu(x):
        y = torch.empty(M, N // 2, dtype=x.dtype, device=x.device)
        ext().wstream_fin(3, x, wt, y, None, _tickets(x.device, 1, "fin"), ss_in, float(eps), None, None, None, None,
                          None, None, None, None, None, None, 0, 0, 1, _stamps_for("glu", N // 128, x.device))
        return y
    y = x.float() @ untile_weight(wt, glu=True).float().t()
    r = fin_row_scale(ss_in, M, K, eps)
    if r is not None:
        y = y * r[:, None]
    F = N // 2
    return (torch.nn.functional.silu(y[:, :F]) * y[:, F:]).to(x.dtype)


def fin_supported(M: int, d: int, n_qkv: int, n_gu: int, head_dim: int, kw_gate_up: int = 2) -> bool:
    """Shapes the fused decode layer takes (else the model runs the unfused kernels): one row tile, 128-column heads,
    the gate_up row-scale partials fit its threads."""
    if not (1 <= M <= 128 and head_dim == 128 and d % 128 == 0 and d <= 4096 and n_qkv % 128 == 0 and
            n_gu % 128 == 0):
        return False
    if stream_plan(M, n_gu, d, 1) is None or stream_plan(M, n_qkv, d) is None or stream_plan(M, d, d) is None:
        return False
    mt, kc, _ = stream_plan(M, n_gu, d, 1)
    nth = 256 * (2 if mt == 2 and kc == 256 and d // kc >= 6 else 1)
    ssl, nss, tpr = 4096 // nth, d // 128, 1
    while tpr * ssl < nss:
        tpr *= 2
    return tpr <= 64 and M * tpr <= nth


def tile_experts(w: torch.Tensor, glu: bool = False) -> torch.Tensor:
    """Expert weights [E, N, K] -> wave-tiled [E, N/32, K/16, 64, 8] (``tile_weight`` per expert)."""
    E, N, K = w.shape
    out = torch.empty(E, N // 32, K // 16, 64, 8, dtype=w.dtype, device=w.device)
    for e in range(E):
        out[e].copy_(tile_weight(w[e], glu))
    return out


def untile_experts(wt: torch.Tensor, glu: bool = False) -> torch.Tensor:
    return torch.stack([untile_weight(wt[e], glu) for e in range(wt.shape[0])])


# fp8 expert weights: uint8 [E, N/32, K/32, 64, 16] tiles plus fp32 row scales [E, N] (reference.tile_experts_fp8);
# grouped_stream_glu / grouped_stream_combine take them with ``scale``.
tile_experts_fp8 = ref.tile_experts_fp8
untile_experts_fp8 = ref.untile_experts_fp8


# MXFP4 expert weights: float4_e2m1fn_x2 [E, N/32, K/64, 64, 16] tiles plus the float8_e8m0fnu block-scale images
# [E, N/32, K/64, 32, 2] — the dense MXFP4 images per expert; grouped_stream_glu / grouped_stream_combine take them with
# ``scale``.

def tile_experts_mxfp4(w: torch.Tensor, glu: bool = False):
    """Expert weights [E, N, K] -> (float4_e2m1fn_x2 tiles [E, N/32, K/64, 64, 16], float8_e8m0fnu block-scale images
    [E, N/32, K/64, 32, 2]): ``tile_weight_mxfp4`` per expert (every expert quantised on its own, blocks along K)."""
    return tile_experts_as(w, "mxfp4", glu)


def untile_experts_mxfp4(wt4: torch.Tensor, se: torch.Tensor, glu: bool = False) -> torch.Tensor:
    """The dequantised row-major bf16 [E, N, K] experts of MXFP4 expert tiles (e2m1 * 2^e, exact in bf16)."""
    return untile_experts_as(wt4, se, glu)


def stream_moe_supported(N: int, K: int) -> bool:
    # (every tile format: the kernel's 256- and 128-deep K chunks are 8 and 4 fp8 vectors or 4 and 2 mxfp4 ones)
    return N % 64 == 0 and K % 256 == 0


# weight prefetch of the grouped streaming kernel pinned ahead of its MFMAs (as the dense one; toggled by
# benchmarks/moe_bench.py for its A/B)
GROUPED_PIN = True


def tile_experts_as(w: torch.Tensor, weight_dtype: str, glu: bool = False):
    """Expert weights [E, N, K] -> (tiles [E, ...], scales [E, ...] or None): the format's ``tile`` per expert."""
    f = weight_format(weight_dtype)
    wt = st = None
    for e in range(w.shape[0]):
        t, s = f.tile(w[e], glu)
        if wt is None:
            wt = t.new_empty(w.shape[0], *t.shape)
            st = None if s is None else s.new_empty(w.shape[0], *s.shape)
        wt[e].copy_(t)
        if st is not None:
            st[e].copy_(s)
    return wt, st


def untile_experts_as(wt: torch.Tensor, scale: torch.Tensor | None, glu: bool = False) -> torch.Tensor:
    """Row-major bf16 [E, N, K] experts of expert tiles of any format (quantised ones dequantised)."""
    f = WEIGHT_FORMATS[wt.dtype]
    return torch.stack([f.untile(wt[e], None if scale is None else scale[e], glu) for e in range(wt.shape[0])])


def _expert_format(fn: str, wt: torch.Tensor, scale: torch.Tensor | None):
    """(format, scale to pass on) of expert tiles; quantised ones need their scales."""
    f = WEIGHT_FORMATS[wt.dtype]
    if f.scale_dtype is None:
        return f, None
    _check_scale(fn, f, wt, scale)
    return f, scale


def grouped_stream_glu(x: torch.Tensor, wt: torch.Tensor, r: "MoERouting", e_lo: int = 0,
                       scale: torch.Tensor | None = None) -> torch.Tensor:
    """silu(gate) * up for every routed (token, local expert) entry, rows in expert-sorted order [n_ent, F]: the
    weight-streaming grouped kernel on GLU-tiled expert weights (``tile_experts(w13, glu=True)``, the uint8 tiles
    of ``tile_experts_fp8`` with their row scales ``scale``, or the float4_e2m1fn_x2 tiles of ``tile_experts_mxfp4``
    with their e8m0 block-scale images ``scale``)."""
    f, scale = _expert_format("grouped_stream_glu", wt, scale)
    T = x.shape[0]
    n_ent = r.perm_tok.numel()
    F = wt.shape[1] * 16  # (N / 32 tiles of 32 rows, N = 2 F: every tile format)
    y = torch.empty(n_ent, F, dtype=x.dtype, device=x.device)
    if _gpu(x):
        if f.raw:
            wt, scale = wt.view(torch.uint8), scale.view(torch.uint8)
        ext().wstream_grouped(x, wt, scale, f.abi, r.perm_tok, r.perm_w, r.expert_off, int(e_lo), int(T), True, y,
                              None, GROUPED_PIN)
        return y
    h = ref_grouped(x, untile_experts_as(wt, scale, glu=True), r, e_lo, gather=True)
    y.copy_(ref.silu_mul(h))
    return y


def grouped_stream_combine(a: torch.Tensor, wt: torch.Tensor, r: "MoERouting", T: int, out: torch.Tensor,
                           e_lo: int = 0, scale: torch.Tensor | None = None) -> torch.Tensor:
    """out[token] += w * (a[entry] @ W_e^T) over the local experts' entries (out f32 [T, N], zeroed by the caller).
    ``scale``: the row scales of fp8 expert tiles / the block-scale images of MXFP4 ones."""
    f, scale = _expert_format("grouped_stream_combine", wt, scale)
    if _gpu(a):
        if f.raw:
            wt, scale = wt.view(torch.uint8), scale.view(torch.uint8)
        ext().wstream_grouped(a, wt, scale, f.abi, r.perm_tok, r.perm_w, r.expert_off, int(e_lo), int(T), False, None,
                              out, GROUPED_PIN)
        return out
    ref.grouped_gemm(a, untile_experts_as(wt, scale), r.perm_tok, r.perm_w, r.expert_off, e_lo, False, None, out)
    return out


def ref_grouped(x, w, r, e_lo, gather):
    y = torch.zeros(r.perm_tok.numel(), w.shape[1], dtype=x.dtype)
    ref.grouped_gemm(x, w, r.perm_tok, r.perm_w, r.expert_off, e_lo, gather, y, None)
    return y


def slab_reduce(p: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """bf16 [M, N] = sum of the split-K slabs [S, M, N] (bf16 inputs pass through)."""
    if not is_slab(p):
        return p
    if out is None:
        out = torch.empty(p.shape[1], p.shape[2], dtype=torch.bfloat16, device=p.device)
    if _gpu(p):
        ext().slab_reduce(p, out)
    else:
        out.copy_(p.sum(0))
    return out


rope_cos_sin = ref.rope_cos_sin


class MoERouting:
    """Device-side routing of one MoE layer (csrc/moe.hip ``moe_route``): everything the grouped GEMMs need."""
    __slots__ = ("topk_w", "topk_e", "perm_tok", "perm_w", "expert_off", "tile_off", "num_experts", "max_tiles")

    def __init__(self, topk_w, topk_e, perm_tok, perm_w, expert_off, tile_off, num_experts):
        self.topk_w, self.topk_e = topk_w, topk_e
        self.perm_tok, self.perm_w = perm_tok, perm_w
        self.expert_off, self.tile_off = expert_off, tile_off
        self.num_experts = num_experts
        self.max_tiles = (perm_tok.numel() + GG_BM - 1) // GG_BM + num_experts


GG_BM = 64  # row tile of the grouped GEMM (a routing bound the kernel and the host agree on)


def moe_route(logits: torch.Tensor, k: int) -> MoERouting:
    """softmax -> top-k -> renormalise, then a stable sort of the T*k entries by expert (token order inside)."""
    T, E = logits.shape
    dev = logits.device
    if _gpu(logits):
        tw = torch.empty(T, k, dtype=torch.float32, device=dev)
        te = torch.empty(T, k, dtype=torch.int32, device=dev)
        pt = torch.empty(T * k, dtype=torch.int32, device=dev)
        pw = torch.empty(T * k, dtype=torch.float32, device=dev)
        eo = torch.empty(E + 1, dtype=torch.int32, device=dev)
        to = torch.empty(E + 1, dtype=torch.int32, device=dev)
        ext().moe_route(logits, int(k), GG_BM, tw, te, pt, pw, eo, to)
        return MoERouting(tw, te, pt, pw, eo, to, E)
    tw, te, pt, pw, eo, to = ref.moe_route(logits, k, GG_BM)
    return MoERouting(tw, te, pt, pw, eo, to, E)


def grouped_gemm(x: torch.Tensor, w: torch.Tensor, r: MoERouting, gather: bool, e_lo: int = 0,
                 y: torch.Tensor | None = None, combine_out: torch.Tensor | None = None) -> torch.Tensor:
    """Per expert segment of the routed entries: Y = X_e . W_e^T (W = [E_local, N, K], experts [e_lo, e_lo+E_local)).

    gather=True reads A rows as x[perm_tok[r]] (token activations), else x[r] (expert-sorted rows).
    combine_out (f32 [T, N], zeroed by the caller) receives out[perm_tok[r]] += perm_w[r] * Y[r] instead of Y."""
    n_ent = r.perm_tok.numel()
    if combine_out is not None and combine_out.shape[0] != r.topk_w.shape[0]:
        raise ValueError("combine_out must have one row per routed token")
    if combine_out is None and y is None:
        y = torch.empty(n_ent, w.shape[1], dtype=x.dtype, device=x.device)
    if _gpu(x):
        ext().grouped_gemm(x, w, r.perm_tok, r.perm_w, r.expert_off, r.tile_off, int(e_lo), int(r.max_tiles),
                           bool(gather), y, combine_out)
    else:
        ref.grouped_gemm(x, w, r.perm_tok, r.perm_w, r.expert_off, e_lo, gather, y, combine_out)
    return combine_out if combine_out is not None else y


# ---- expert-parallel all-to-all (csrc/moe.hip ep_*, models/moe.py MoEBlock._a2a) --------------------------------
def ep_layout(T: int, ep: int, k: int, El: int, d: int) -> tuple[int, int, int]:
    """(owned tokens per rank Tl, slot capacity C per destination, metadata rows MR) of the EP send image
    [ep, C + MR, d]: a token's k experts are distinct, so at most min(k, El) of its pairs go to one rank."""
    Tl = max(1, -(-T // ep))
    C = Tl * min(k, El)
    MR = -(-(16 + 4 * C) // (2 * d))
    return Tl, C, MR


def ep_dispatch(x: torch.Tensor, topk_e: torch.Tensor, lo: int, n_own: int, El: int, ep: int, C: int,
                MR: int) -> tuple[torch.Tensor, torch.Tensor]:
    """Send image [ep, C + MR, d] bf16 of the owned (token, expert) pairs + their slot map (int32 [n_own * k]:
    destination block row of each pair), computed on the device."""
    d = x.shape[1]
    k = topk_e.shape[1]
    img = torch.empty(ep, C + MR, d, dtype=x.dtype, device=x.device)
    slot = torch.empty(max(1, n_own * k), dtype=torch.int32, device=x.device)
    te = topk_e if topk_e.dtype == torch.int32 else topk_e.to(torch.int32)
    if _gpu(x):
        ext().ep_dispatch(x, te.contiguous(), int(lo), int(n_own), int(El), int(C), img, slot)
    else:
        img.zero_()
        ref.ep_dispatch(x, te, lo, n_own, El, C, img, slot)
    return img, slot


def ep_recv_route(img: torch.Tensor, C: int, El: int) -> "MoERouting":
    """MoERouting over the rows of a received EP image: valid slots sorted stably by local expert."""
    ep = img.shape[0]
    dev = img.device
    if _gpu(img):
        pt = torch.empty(ep * C, dtype=torch.int32, device=dev)
        pw = torch.empty(ep * C, dtype=torch.float32, device=dev)
        eo = torch.empty(El + 1, dtype=torch.int32, device=dev)
        to = torch.empty(El + 1, dtype=torch.int32, device=dev)
        ext().ep_recv_route(img, int(C), int(El), GG_BM, pt, pw, eo, to)
    else:
        pt, pw, eo, to = ref.ep_recv_route(img, C, El, GG_BM)
    rows = img.shape[0] * img.shape[1]  # combine outputs are indexed by image row (topk_* are not read)
    tw = torch.zeros(rows, 1, dtype=torch.float32, device=dev)
    return MoERouting(tw, tw.to(torch.int32), pt, pw, eo, to, El)


def ep_combine(back: torch.Tensor, slot_map: torch.Tensor, topk_w: torch.Tensor, lo: int, n_own: int,
               out: torch.Tensor) -> torch.Tensor:
    """out[i] = sum_j topk_w[lo + i, j] * back_rows[slot_map[i k + j]] for the owned tokens (bf16)."""
    rows = back.reshape(-1, back.shape[-1])
    if n_own <= 0:
        return out
    if _gpu(back):
        ext().ep_combine(rows, slot_map, topk_w.float().contiguous(), int(lo), int(n_own), out)
    else:
        ref.ep_combine(rows, slot_map, topk_w, lo, n_own, out)
    return out
