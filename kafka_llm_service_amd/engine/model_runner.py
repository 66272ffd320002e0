"""Turns a ScheduledBatch into device tensors, runs the model and samples (one engine step on one GPU/TP rank).

Host->device traffic per step is two packed pinned buffers (one int64: tokens / positions / slots / logit rows;
one int32: block tables / causal limits / decode, cascade and prefill work items) copied with one async H2D each; the only
device->host traffic is the sampled token ids (SURVEY.md §3.2 "device→host: sampled token ids only").

Decode-only batches can be replayed from hipGraphs captured per batch-size bucket (``engine/graphs.py``); mixed
batches run eagerly.
"""
from __future__ import annotations

import bisect
import os
from collections import deque
from dataclasses import dataclass

import numpy as np
import torch

from kafka_llm_service_amd import ops
from kafka_llm_service_amd.engine.logits_proc import LogitsProcessor, spec_forced
from kafka_llm_service_amd.engine.scheduler import ScheduledBatch
from kafka_llm_service_amd.engine.sequence import Sequence
from kafka_llm_service_amd.engine.tool_automaton import tool_row_live
from kafka_llm_service_amd.engine.step_plan import (  # noqa: F401 - the planner's names, importable from here as before
    DECODE_TARGET_ITEMS, MAX_ITEM_KEYS, MAX_PARTIALS, MAX_PREFIX_CHUNKS, MIN_DECODE_KEYS, PLAN_HDR, PLAN_PAYLOAD_IDX,
    _PLAN_SCALARS, HostStep, SampleParams, decode_items, decode_items_fixed, merge_ranges, pack_plan,
    plan_prefill_items, prefix_groups, retile, unpack_plan)
from kafka_llm_service_amd.engine.step_plan import GRAMMARS, PlanConfig, cdiv, join, plan_attention, section
from kafka_llm_service_amd.models.attention import AttnMeta
from kafka_llm_service_amd.models.llama import StepInput, TransformerLM

ROWS_BUCKETS = (64, 96, 128, 256, 1 << 30)  # step-size histogram buckets (decode GEMM row-tile plans, skinny, BLAS)


class CollectiveError(RuntimeError):
    """A TP peer stopped taking part in the custom all-reduce (its waits timed out): the step's tokens were computed
    from stale peer data and the replica must fail (503 + respawn), not stream them."""


@dataclass
class Launched:
    tokens: torch.Tensor            # sampled ids (pinned host buffer on GPU, plain tensor on CPU)
    event: object = None            # completion event of the D2H copy
    dev_tokens: torch.Tensor | None = None  # the sampler's device output (input ids of the next step's decode rows)
    rows: dict | None = None        # seq_id -> row of dev_tokens
    err_idx: int | None = None      # slot of ModelRunner._err_host holding the custom all-reduce error word
    known: dict | None = None       # row -> token the grammar forced (known on the host at launch)
    # (packed records [R, 1 + 2k] float32 — pinned host buffer on GPU —, k, sampled rows [R]) of a step with
    # logprob rows; lands with ``event`` like the tokens
    logprobs: tuple | None = None


def pad_step_rows(T: int) -> int:
    """Token rows of a mixed step whose GEMMs go to hipBLASLt (129..256 rows): measured on MI355X (Llama-3-8B shapes,
    ``benchmarks/gemm_bench.py``, profiles/r02/gemm_sweep_M129_320.log) the library picks slow kernels for 129..152
    rows (QKV 40 vs 26 us) and at multiples of 32 (down-proj at 192 rows: 101 vs 60 us), so the step is padded with
    inert rows (no KV slot, no attention item, no logits) to the next 16 k + 8 >= 168."""
    if T <= ops.STREAM_MAX_M or T > 256:  # (steps the streaming GEMM takes need no padding)
        return T
    t = max(T, 168)
    t += (8 - t % 16) % 16
    return t if t <= 256 else T


_NP2TORCH = {np.dtype(np.int64): torch.int64, np.dtype(np.int32): torch.int32, np.dtype(np.float32): torch.float32}


class _Stager:
    """Per-step host->device uploads through a ring of pinned staging arenas (one arena per launch, bump-allocated):
    no pinned allocation and no pageable copy on the step path, so every upload is a plain async DMA in stream
    order. An arena is reused ``depth`` launches later, when at most two steps can be in flight — its copies have
    executed by then."""

    def __init__(self, device: torch.device, nbytes: int = 8 << 20, depth: int = 4):
        self.device = device
        self.nbytes = nbytes
        self.bufs: list[torch.Tensor | None] = [None] * depth
        self.events: list = [None] * depth  # copies of the arena's last launch (a TP follower is not throttled)
        self.i = 0
        self.off = 0

    def begin(self) -> None:
        if self.device.type == "cuda":
            ev = self.events[self.i]
            if ev is None:
                ev = self.events[self.i] = torch.cuda.Event()
            ev.record()  # after every copy issued from the arena that is being left
        self.i = (self.i + 1) % len(self.bufs)
        self.off = 0
        ev = self.events[self.i]
        if ev is not None:
            ev.synchronize()  # normally long done: the arena's copies ran len(bufs) launches ago

    def upload_many(self, arrays: list[np.ndarray]) -> list[torch.Tensor]:
        """Several arrays staged back to back (256-B aligned) and moved by ONE async copy into one device buffer —
        a step's plan and sampling parameters cost one copy launch instead of one each; returns device views."""
        arrays = [np.ascontiguousarray(a) for a in arrays]
        if self.device.type != "cuda":
            return [torch.from_numpy(a) for a in arrays]
        offs, off = [], 0
        for a in arrays:
            offs.append(off)
            off = (off + a.nbytes + 255) & ~255
        base = (self.off + 255) & ~255
        buf = self.bufs[self.i]
        if buf is None or base + off > buf.numel():
            self.bufs[self.i] = buf = torch.empty(max(self.nbytes, 2 * (base + off)), dtype=torch.uint8,
                                                  pin_memory=True)
        host = buf.numpy()
        for a, o in zip(arrays, offs):
            host[base + o:base + o + a.nbytes] = a.reshape(-1).view(np.uint8)
        self.off = base + off
        dev = torch.empty(off, dtype=torch.uint8, device=self.device)
        dev.copy_(buf[base:base + off], non_blocking=True)
        return [dev[o:o + a.nbytes].view(_NP2TORCH[a.dtype]).view(a.shape) for a, o in zip(arrays, offs)]

    def upload(self, a: np.ndarray) -> torch.Tensor:
        a = np.ascontiguousarray(a)
        if self.device.type != "cuda":
            return torch.from_numpy(a)
        nb = a.nbytes
        off = (self.off + 255) & ~255
        buf = self.bufs[self.i]
        if buf is None or off + nb > buf.numel():
            # (a replaced arena goes back to torch's pinned cache, which waits for its recorded copies)
            self.bufs[self.i] = buf = torch.empty(max(self.nbytes, 2 * (off + nb)), dtype=torch.uint8,
                                                  pin_memory=True)
        stage = buf[off:off + nb]
        stage.numpy()[:] = a.reshape(-1).view(np.uint8)
        self.off = off + nb
        dev = torch.empty(a.size, dtype=_NP2TORCH[a.dtype], device=self.device)
        dev.view(torch.uint8).copy_(stage, non_blocking=True)
        return dev.view(a.shape)

    def upload_into(self, arrays: list[np.ndarray | None], offs: list[int], dst: torch.Tensor) -> None:
        """Arrays staged at their byte offsets of ``dst`` (a uint8 device buffer whose layout the caller fixed) and moved
        by ONE async copy of the whole range — a hipGraph's static inputs refreshed with one copy launch instead of an
        upload plus a device copy per array. Every byte of ``dst`` is written: the ranges of None arrays (and any
        padding) become zeros, never stale bytes of an earlier upload."""
        n = dst.numel()
        if self.device.type != "cuda":
            dst.zero_()
            for a, o in zip(arrays, offs):
                if a is not None:
                    dst[o:o + a.nbytes].copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8)))
            return
        base = (self.off + 255) & ~255
        buf = self.bufs[self.i]
        if buf is None or base + n > buf.numel():
            self.bufs[self.i] = buf = torch.empty(max(self.nbytes, 2 * (base + n)), dtype=torch.uint8, pin_memory=True)
        host = buf.numpy()
        host[base:base + n] = 0
        for a, o in zip(arrays, offs):
            if a is not None:
                a = np.ascontiguousarray(a)
                host[base + o:base + o + a.nbytes] = a.reshape(-1).view(np.uint8)
        self.off = base + n
        dst.copy_(buf[base:base + n], non_blocking=True)


class ModelRunner:
    def __init__(self, model: TransformerLM, k_caches, v_caches, kvm, max_num_seqs: int, max_blocks_per_seq: int,
                 cascade_min_prefix: int = 512, use_cascade: bool = True, target_wgs: int = 256,
                 prefill_kv_chunk: int = 1024):
        self.model = model
        self.k_caches, self.v_caches = k_caches, v_caches
        self.kvm = kvm
        self.device = model.device
        self.max_num_seqs = max_num_seqs
        self.max_blocks = max_blocks_per_seq
        self.G = model.hq // model.hkv
        # tile-kernel variant (ops.tile_rows): 3 = LDS-DMA ring kernel (csrc/attn_tile.hip, 8 waves x 256 query rows,
        # bf16 pages); 0 = register-staged 8 waves x 256 rows (fp8 pages); 1 = 4 waves x 128 rows
        fp8 = bool(k_caches) and ops.is_fp8_cache(k_caches[0])
        self.variant = int(os.environ.get("KAFKA_TILE_VARIANT", "0" if fp8 else "3"))
        if fp8 and self.variant == 3:
            raise ValueError("tile variant 3 reads bf16 KV pages only")
        # mixed steps of 129..256 rows padded away from hipBLASLt's slow sizes (dense TP = 1 GPU models)
        self.pad_rows = (self.device.type == "cuda" and model.tp == 1 and not getattr(model, "tiled_only", False)
                         and os.environ.get("KAFKA_PAD_ROWS", "1") == "1")
        self.tile = ops.tile_rows(self.variant) // self.G  # tokens per attention work item
        # the v3 cascade hands its prefix partials to the decode kernel as bf16 (normalised O, fp32 lse): ~33 MB
        # less HBM traffic per Llama-3-8B layer at 64 threads on an 18k prefix (+1.4 %,
        # profiles/r03/bench_ab_cascade_bf16_partials.jsonl)
        self.cascade_bf16 = self.variant == 3
        self.cascade_min_prefix = cascade_min_prefix
        self.target_wgs = target_wgs  # workgroups the prefill / cascade tile launches are balanced for
        self.prefill_kv_chunk = int(os.environ.get("KAFKA_PREFILL_KV_CHUNK", prefill_kv_chunk))
        self.use_cascade = use_cascade
        self.vocab = model.cfg.vocab_size
        pin = self.device.type == "cuda"
        self._pin = pin
        self.last_stats: dict = {}
        self.recent_stats: deque = deque(maxlen=16)  # stats of the last launched steps (two can be in flight)
        self.rows_hist = [0] * len(ROWS_BUCKETS)  # launched steps by token rows (ROWS_BUCKETS upper bounds)
        self.broadcast = None  # set on a TP leader: callable(HostStep, SampleParams) (engine/tp_worker.py)
        self._tok_host = None  # pinned landing buffers of the sampled ids
        self._lp_host = None   # pinned landing buffers of the logprob records (allocated by the first step that asks)
        self._lp_dev = None    # the running step's packed logprob records on the device (_run -> launch)
        self._err_host = None  # pinned landing slots of the custom all-reduce error word (TP)
        self.stager = _Stager(self.device)
        # every step's sampled ids also land here (fixed address, so hipGraphs can read it): the next step's decode
        # rows whose token was still being sampled at launch gather their input ids from it on the stream
        self.tok_buf = torch.zeros(max_num_seqs * 2 + 64, dtype=torch.int64, device=self.device)
        self.graphs = None  # engine/graphs.py DecodeGraphs when hipGraph decode is enabled
        # decode_items_fixed without graphs too (set by the graph / eager equivalence tests)
        self.fixed_decode_items = False
        # a joined new turn's own keys (its history behind the shared prefix) ride in the cascade launch too
        self.join_suffix = os.environ.get("KAFKA_JOIN_SUFFIX", "1") == "1"
        self.step_events: list | None = None  # (start, end) timing events per launched step when a list is set
        # grammar masks / forced tokens / penalties inside the sampler kernel (tables allocated on first use)
        # (and the JSON-mode rows: a state slot and a device-written mask row per live JSON sequence)
        self.lp = LogitsProcessor(self.device, self.vocab, max_slots=max(256, max_num_seqs),
                                  json_slots=max(256, max_num_seqs))

    # ------------------------------------------------------------------------------------------------------------
    def prepare(self, batch: ScheduledBatch) -> tuple[StepInput, list[Sequence]]:
        host, sample_seqs = self.build_host(batch)
        return self.to_device(host), sample_seqs

    def plan_config(self) -> PlanConfig:
        graphs = self.graphs is not None  # graph replay: the decode grid depends on B alone, s_total is a layout key
        return PlanConfig(tile=self.tile, hkv=self.model.hkv, page=ops.PAGE, target_wgs=self.target_wgs,
                          prefill_kv_chunk=self.prefill_kv_chunk, joins=self.variant == 3,
                          join_suffix=self.join_suffix, fixed_decode=graphs or self.fixed_decode_items,
                          round_s_total=graphs)

    def build_host(self, batch: ScheduledBatch) -> tuple[HostStep, list[Sequence]]:
        """All host-side work of a step: token/slot/page-table packing here, attention work-item planning in
        ``step_plan.plan_attention``. The result is a few numpy arrays + scalars — what a TP leader broadcasts to its
        followers (``engine/tp_worker.py``).

        Decode rows are reordered so that every cascade group (rows sharing a KV prefix of at least
        ``cascade_min_prefix`` tokens, ``prefix_groups``) is contiguous."""
        dec = list(batch.decode)
        B = len(dec)
        pre = batch.prefill
        T_real = B + sum(e - s for _, s, e in pre)
        T = pad_step_rows(T_real) if self.pad_rows else T_real
        nbt = max(1, B + len(pre))
        need = cdiv(max([s.total_len for s in dec] + [b for _, _, b in pre] + [1]), ops.PAGE)  # pages of the longest row
        # under graphs the width is a power-of-two bucket (>= 64 pages): the layout (and so the captured graph)
        # changes only when the longest row crosses a bucket, and the per-step upload / TP broadcast stays small
        bt_w = (min(self.max_blocks, max(64, 1 << (need - 1).bit_length())) if self.graphs is not None
                else min(self.max_blocks, cdiv(need, 16) * 16))
        bt = np.zeros((nbt, bt_w), dtype=np.int32)
        groups: list[tuple[int, int]] = []
        seq_lens = np.fromiter((s.total_len for s in dec), dtype=np.int64, count=B)
        if B:
            self.kvm.fill_block_tables([s.seq_id for s in dec], bt)
            if self.use_cascade and B >= 2:
                nfull = (seq_lens - 1) // ops.PAGE
                order, groups = prefix_groups(bt[:B], nfull, cdiv(self.cascade_min_prefix, ops.PAGE))
                if groups and order != list(range(B)):
                    dec = [dec[i] for i in order]
                    bt[:B] = bt[:B][order]
                    seq_lens = seq_lens[order]
        if pre:
            self.kvm.fill_block_tables([s.seq_id for s, _, _ in pre], bt[B:])
        tokens = np.empty(T, dtype=np.int64)
        positions = np.empty(T, dtype=np.int64)
        slots = np.empty(T, dtype=np.int64)
        q_limit = np.empty(T, dtype=np.int32)
        sample_seqs: list[Sequence] = []
        logit_rows: list[int] = []
        patch = []
        for i, s in enumerate(dec):
            p = s.total_len - 1
            t = s.token_at(p)
            if t < 0:  # PENDING: sampled by the step still in flight (async scheduling)
                patch.append((i, s, p))
            tokens[i] = t
            positions[i] = p
            q_limit[i] = p
            self.kvm.fill_slots(s.seq_id, p, p + 1, slots, i)
            sample_seqs.append(s)
            logit_rows.append(i)
        r = B
        for s, a, b in pre:
            n = b - a
            tokens[r:r + n] = s.tokens_range(a, b)
            positions[r:r + n] = np.arange(a, b)
            q_limit[r:r + n] = np.arange(a, b, dtype=np.int32)
            self.kvm.fill_slots(s.seq_id, a, b, slots, r)
            if b == s.total_len:
                sample_seqs.append(s)
                logit_rows.append(r + n - 1)
            r += n
        if T > T_real:  # inert padding rows: token 0 at position 0, no KV write, not attended, no logits
            tokens[T_real:] = 0
            positions[T_real:] = 0
            slots[T_real:] = -1
            q_limit[T_real:] = 0
        plan = plan_attention(bt, seq_lens, groups, [(a, b, B + j) for j, (_, a, b) in enumerate(pre)],
                              self.plan_config())
        h = HostStep(B=B, T=T, nbt=nbt, bt_w=bt_w, bt_need=min(need, bt_w), n_rows=len(logit_rows), patch=patch,
                     stats=plan.stats(B, T), **plan.scalars)
        h.i64 = join(h.i64_sections(), {"tokens": tokens, "positions": positions, "slots": slots,
                                        "logit_rows": logit_rows}, np.int64)
        h.i32 = join(h.i32_sections(), {"block_tables": bt, "q_limit": q_limit, "decode_items": plan.decode_items,
                                        "prefix_items": plan.prefix_items, "prefill_items": plan.prefill_items,
                                        "merge_ranges": plan.merge_ranges}, np.int32)
        return h, sample_seqs

    def to_device(self, h: HostStep, sp: "SampleParams | None" = None) -> StepInput:
        """One H2D copy of the packed buffers (and of the step's sampling parameters when ``sp`` samples with
        temperature: left in ``self._sp_dev`` for ``sample_device``), then views into it (identical on every TP
        rank)."""
        named = {}  # what rides behind the two packed buffers, in upload order
        if sp is not None and not sp.greedy and sp.temp.shape[0]:
            named.update(f32=np.concatenate([sp.temp, sp.topp]), topk=sp.topk, seeds=sp.seeds)
        if sp is not None and sp.proc is not None:
            named["proc"] = sp.proc
            # (grammar rows are proc rows: behind them, JSON mode, json_schema, then the tool grammar)
            named.update((k, getattr(sp, k + "_rows")) for k in GRAMMARS if getattr(sp, k + "_rows") is not None)
        dev = self.stager.upload_many([h.i64, h.i32, *named.values()])
        if named:
            at = dict(zip(named, dev[2:]))
            self._sp_dev = (sp, at.get("f32"), at.get("topk"), at.get("seeds"), at.get("proc"))
            self._grammar_dev = (sp, {k: at[k] for k in GRAMMARS if k in at})
        return self.views(dev[0], dev[1], h)

    def views(self, d64: torch.Tensor, d32: torch.Tensor, h: HostStep) -> StepInput:
        """StepInput over packed device buffers laid out as ``h`` describes (only h's scalars are read, so a hipGraph
        captured over static buffers replays with any step of the same layout)."""
        B, T = h.B, h.T
        s64, s32 = h.i64_sections(), h.i32_sections()
        t_tokens = section(d64, s64, "tokens")
        meta = AttnMeta(num_decode=B, num_tokens=T, scale=self.model.scale, variant=self.variant)
        meta.block_tables = section(d32, s32, "block_tables")
        meta.q_limit = section(d32, s32, "q_limit")
        Hq, D = self.model.hq, self.model.D
        if B:
            meta.decode_items = section(d32, s32, "decode_items")
            if h.n_prefix_items:
                meta.prefix_items = section(d32, s32, "prefix_items")
            meta.s_total = h.s_total
            meta.part = torch.empty(B, Hq, h.s_total, D, dtype=torch.float32, device=self.device)
            meta.lse = torch.empty(B, Hq, h.s_total, dtype=torch.float32, device=self.device)
            if h.n_prefix_items and self.cascade_bf16:
                meta.pre_part = torch.empty(B, Hq, h.s_total, D, dtype=torch.bfloat16, device=self.device)
            meta.extra["cascade_prefix"] = h.cascade_prefix
        if h.n_items:
            meta.prefill_items = section(d32, s32, "prefill_items")
        if h.prefill_splits:
            Tp = T - B
            meta.prefill_splits = h.prefill_splits
            mr = section(h.i32, s32, "merge_ranges")  # host copy of the plan (every TP rank)
            meta.prefill_merge = [(int(lo), int(hi)) for lo, hi in mr]
            meta.prefill_part = torch.empty(Tp, Hq, h.prefill_splits, D, dtype=torch.float32,
                                            device=self.device)
            meta.prefill_lse = torch.full((Tp, Hq, h.prefill_splits), float("-inf"), dtype=torch.float32,
                                          device=self.device)
            meta.prefix_joined = h.prefix_joined > 0
        if h.n_late:
            t_tokens.index_copy_(0, section(d64, s64, "late_dst"),
                                 self.tok_buf.index_select(0, section(d64, s64, "late_src")))
        return StepInput(t_tokens, section(d64, s64, "positions"), section(d64, s64, "slots"), meta,
                         section(d64, s64, "logit_rows"))

    def _host(self, a: np.ndarray) -> torch.Tensor:
        """Host tensor of ``a`` for an async copy into a device buffer (pinned on GPU hosts)."""
        t = torch.from_numpy(a)
        return t.pin_memory() if self.device.type == "cuda" else t

    def _h2d(self, a: np.ndarray) -> torch.Tensor:
        return self.stager.upload(a)

    # ------------------------------------------------------------------------------------------------------------
    def sample(self, logits: torch.Tensor, seqs: list[Sequence]) -> torch.Tensor:
        return self.sample_device(logits, self.sample_params(seqs))

    def sample_params(self, seqs: list[Sequence], n_decode: int | None = None) -> "SampleParams":
        """Per-row sampling parameters of a step; rows with a token constraint, penalties (presence, frequency,
        repetition), a logit bias or min_p get a logits-processing row (engine/logits_proc.py) that the sampler kernel applies on the device. A constrained row's spec is
        computed from its landed tokens, or past a pending one when the grammar can guess its successor state
        (engine/constrained.py: a wrong guess rolls the row back one token); a forced token is returned in
        ``known`` so the engine writes it at launch. A JSON-mode row (``json_mode``) is a processing row too: its mask
        row is written on the device from its device-resident automaton state (engine/json_mode.py), so it needs no
        landed token; the rows at and behind ``n_decode`` are sampled from a prefill, where such a row's state is
        seeded."""
        n = len(seqs)
        temp = np.empty(n, dtype=np.float32)
        topp = np.empty(n, dtype=np.float32)
        topk = np.empty(n, dtype=np.int32)
        seeds = np.empty(n, dtype=np.int64)
        rows = []  # (row, seq, allowed) for rows that need penalties or a token constraint
        known = None
        lp_rows, lp_k = [], 0
        for i, s in enumerate(seqs):
            p = s.params
            temp[i] = p.temperature
            topp[i] = p.top_p
            topk[i] = p.top_k
            base = p.seed if p.seed is not None else (s.seq_id * 7919)
            seeds[i] = (base * 1000003 + len(s.output_ids)) & 0x7FFFFFFFFFFFFFFF
            if p.logprobs:
                lp_rows.append(i)
                lp_k = max(lp_k, p.top_logprobs)
            allowed = None
            if p.allowed_tokens_fn is not None:
                # (a pending last token is speculated past by the constraint, ToolCallConstraint.__call__)
                allowed = p.allowed_tokens_fn(s.output_ids)
                f = spec_forced(allowed) if allowed is not None else None
                if f is not None:
                    known = known or {}
                    known[i] = f
            # (min_p acts under temperature only: a greedy row needs no processing row for it)
            if allowed is not None or p.presence_penalty or p.frequency_penalty or p.logit_bias \
                    or (p.min_p and p.temperature > 0) or p.repetition_penalty != 1.0 or p.json_mode \
                    or p.json_schema is not None or (p.tool_plan is not None and tool_row_live(p.tool_plan,
                                                                                              s.output_ids)):
                rows.append((i, s, allowed))
        proc = upd = None
        if rows:
            proc, upd = self.lp.build(rows, n, n_decode)
            upd = None if upd.empty else upd
        sp = SampleParams(temp, topp, topk, seeds, proc, not temp.any(), upd, known)
        sp.json_rows, sp.schema_rows, sp.tool_rows = self.lp.grammar_rows(proc)
        if lp_rows:
            sp.lp_rows, sp.lp_k = np.asarray(lp_rows, dtype=np.int32), lp_k
        return sp

    def logprobs_device(self, logits: torch.Tensor, toks: torch.Tensor, sp: "SampleParams") -> torch.Tensor | None:
        """The step's logprob records, launched right behind its sampler: packed [R, 1 + 2k] (ops.logprob_records)
        for the rows of ``sp.lp_rows`` over the RAW logits and the ids the sampler just wrote (a grammar-forced id
        included). A step without such rows launches, copies and allocates nothing."""
        if sp.lp_rows is None:
            return None
        buf = ops.logprob_records(sp.lp_rows.shape[0], sp.lp_k, logits.device)
        ops.token_logprobs(logits, toks, self._h2d(sp.lp_rows), sp.lp_k, out=ops.unpack_logprob_records(buf, sp.lp_k))
        return buf

    def apply_proc_updates(self, sp: "SampleParams") -> None:
        """The step's logits-processor table writes, stream-ordered before its sampler (every TP rank)."""
        if sp.upd is not None:
            self.lp.apply(sp.upd, self._h2d)

    def proc_tables(self, sp: "SampleParams") -> dict:
        if sp.proc is None:
            return {}
        mask_tab, counts = self.lp.tables()
        return {"mask_tab": mask_tab, "counts": counts, "bias_tab": self.lp.bias_table(),
                "rep_tab": self.lp.live_rep_table()}

    def sample_device(self, logits: torch.Tensor, sp: "SampleParams") -> torch.Tensor:
        """The step's sampler launch. A step with JSON rows launches the mask kernel in front of it (the rows' mask
        rows from their device states) and the advance kernel behind it (the states over the drawn ids); a step
        with json_schema or automaton tool rows does the same with the kernels of ops/csrc/table_grammar.hip over the
        requests' own tables (JSON-mode mask, schema mask, tool mask, sampler, then the advances: tool, JSON mode,
        schema); a step without any launches exactly what it always did."""
        pre, self._grammar_dev = getattr(self, "_grammar_dev", None), None
        if all(getattr(sp, k + "_rows") is None for k in GRAMMARS):
            return self._sample_device(logits, sp)
        on_dev = pre[1] if pre is not None and pre[0] is sp else {}  # (uploaded with the step's plan)

        def dev_rows(kind: str):
            rows = getattr(sp, kind + "_rows")
            return None if rows is None else on_dev[kind] if kind in on_dev else self._h2d(rows)

        tabs, mask_tab = self.lp.json_tables(), self.lp.tables()[0]
        jrows = dev_rows("json")
        if jrows is not None:
            ops.json_mask(tabs, jrows, self.lp.jstate, mask_tab, self.lp.n_mask_rows)
        srows = dev_rows("schema")
        if srows is not None:
            ops.schema_mask(tabs, self.lp.schema_pool(), srows, logits.shape[0], self.lp.jstate, mask_tab,
                            self.lp.n_mask_rows, used=np.unique(sp.schema_rows[:, 2]))
        trows = dev_rows("tool")
        if trows is not None:
            ops.tool_mask(tabs, self.lp.schema_pool(), trows, logits.shape[0], self.lp.jstate, mask_tab,
                          self.lp.n_mask_rows, used=np.unique(sp.tool_rows[:, 2]))
        toks = self._sample_device(logits, sp)
        if trows is not None:
            ops.tool_advance(tabs, self.lp.schema_pool(), trows, toks, self.lp.jstate)
        if jrows is not None:
            ops.json_advance(tabs, jrows, toks, self.lp.jstate)
        if srows is not None:
            ops.schema_advance(tabs, self.lp.schema_pool(), srows, toks, self.lp.jstate)
        return toks

    def _sample_device(self, logits: torch.Tensor, sp: "SampleParams") -> torch.Tensor:
        n = logits.shape[0]
        dev = logits.device
        pre, self._sp_dev = getattr(self, "_sp_dev", None), None
        if pre is not None and pre[0] is not sp:
            pre = None
        kw = self.proc_tables(sp)
        if sp.proc is not None:
            kw["proc"] = pre[4] if pre is not None and pre[4] is not None else self._h2d(sp.proc)
        if sp.greedy:
            return ops.sample(logits, torch.zeros(n, device=dev), **kw)
        if pre is not None and pre[2] is not None and pre[2].shape[0] == n:  # uploaded with the step's plan
            _, f32, tk, sd, _ = pre
            return ops.sample(logits, f32[:n], f32[n:], tk, sd, **kw)
        f32 = self._h2d(np.concatenate([sp.temp, sp.topp]))
        return ops.sample(logits, f32[:n], f32[n:], self._h2d(sp.topk), self._h2d(sp.seeds), **kw)

    # ------------------------------------------------------------------------------------------------------------
    @torch.inference_mode()
    def execute(self, batch: ScheduledBatch) -> tuple[list[Sequence], list[int]]:
        host, sample_seqs = self.build_host(batch)
        return sample_seqs, self.collect(self.launch(host, sample_seqs))

    @torch.inference_mode()
    def launch(self, host: HostStep, sample_seqs: list[Sequence], prev: Launched | None = None) -> Launched:
        """Enqueue one step on the GPU without waiting for it: (TP broadcast) -> H2D -> forward -> sample -> async
        D2H of the sampled ids into pinned memory. ``collect`` waits for them.

        Decode rows whose input token was PENDING at planning time are filled from the host if the token has landed
        since, else device-side from ``prev`` (the in-flight step that samples it): one gather + scatter on the
        stream, so the launch never waits for the previous step. Under TP the followers do the same from their own
        copy of the sampled ids (every rank samples the all-gathered logits with the same parameters)."""
        late_dst, late_src = [], []
        for row, s, pos in host.patch:
            t = s.token_at(pos)
            if t >= 0:
                host.i64[row] = t
            else:
                if prev is None or prev.rows is None or s.seq_id not in prev.rows:
                    raise RuntimeError(f"decode row {row}: token {pos} of seq {s.seq_id} is neither landed nor in "
                                       "the in-flight step")
                late_dst.append(row)
                late_src.append(prev.rows[s.seq_id])
        host.patch = []
        if late_dst:
            host.late_off, host.n_late = host.i64.size, len(late_dst)
            host.i64 = np.concatenate([host.i64, np.asarray(late_dst + late_src, dtype=np.int64)])
        self.last_stats = host.stats
        self.recent_stats.append(host.stats)
        self.rows_hist[bisect.bisect_left(ROWS_BUCKETS, host.T)] += 1
        sp = self.sample_params(sample_seqs, host.B)
        self.stager.begin()
        if self.broadcast is not None:  # TP leader: followers run the same step on their shards
            self.broadcast(host, sp)
        ev_s = None
        if self.step_events is not None and self.device.type == "cuda":
            ev_s = torch.cuda.Event(enable_timing=True)
            ev_s.record()
        toks = self._run(host, sp)
        lp, self._lp_dev = self._lp_dev, None
        rows = {s.seq_id: i for i, s in enumerate(sample_seqs)}
        if self.device.type != "cuda":
            return Launched(toks.clone(), None, toks, rows, known=sp.known,
                            logprobs=None if lp is None else (lp, sp.lp_k, sp.lp_rows))
        n = toks.shape[0]
        # a ring of pinned landing buffers: two steps can be in flight, each D2H needs its own
        ring = self._tok_host
        if ring is None or ring[0].shape[0] < n or ring[0].dtype != toks.dtype:
            ring = self._tok_host = [torch.empty(max(n, 256), dtype=toks.dtype, pin_memory=True) for _ in range(3)]
        self._tok_i = (getattr(self, "_tok_i", 0) + 1) % len(ring)
        out = ring[self._tok_i][:n]
        out.copy_(toks, non_blocking=True)
        lp_out = None
        if lp is not None:
            # the records ride back beside the ids: their own pinned ring with the token ring's slot discipline (two
            # steps in flight, one more buffer), one copy of the packed block, the same completion event
            lring, need = self._lp_host, lp.numel()
            if lring is None or lring[0].numel() < need:
                lring = self._lp_host = [torch.empty(max(need, 256 * 41), dtype=torch.float32, pin_memory=True)
                                         for _ in range(len(ring))]
            host_lp = lring[self._tok_i][:need].view(lp.shape)
            host_lp.copy_(lp, non_blocking=True)
            lp_out = (host_lp, sp.lp_k, sp.lp_rows)
        err_idx = None
        car = self._custom_ar()
        if car is not None:  # the error word rides along with the sampled ids (4 bytes, same stream)
            if self._err_host is None:
                self._err_host = torch.zeros(len(ring), dtype=torch.int32, pin_memory=True)
            err_idx = self._tok_i
            car.error_async(self._err_host, err_idx)
        ev = torch.cuda.Event()
        ev.record()
        if ev_s is not None:  # GPU span of the step (plan upload -> token download), read back after the run
            ev_e = torch.cuda.Event(enable_timing=True)
            ev_e.record()
            self.step_events.append((ev_s, ev_e))
        return Launched(out, ev, toks, rows, err_idx, sp.known, lp_out)

    def _custom_ar(self):
        """The IPC collective whose error word rides back with every step's ids: the TP group's custom all-reduce,
        or — data-parallel attention (tp = 1) — the EP group's IPC all-to-all (a peer that stops arriving makes its
        a2a waits time out; without this check the live ranks would stream tokens built from stale expert rows)."""
        if not hasattr(self, "_car"):
            from kafka_llm_service_amd.parallel import comm
            from kafka_llm_service_amd.parallel import state as pstate

            self._car = None
            if self.model.tp > 1:
                self._car = pstate.custom_ar()
            elif getattr(self.model, "dp_attention", False) and self.model.ep > 1 and self.device.type == "cuda":
                self._car = comm.get_custom(pstate.get().ep_group)
        return self._car

    @torch.inference_mode()
    def follower_launch(self, host: HostStep, sp: SampleParams) -> None:
        """A TP follower's copy of the leader's step (``tp_worker.follower_loop``): same forward on this rank's shard,
        same collectives, same sampler — nothing comes back to the host."""
        self.last_stats = host.stats
        self.stager.begin()
        self._run(host, sp)

    def _run(self, host: HostStep, sp: SampleParams) -> torch.Tensor:
        """Forward + sampling of one step (hipGraph replay for eligible decode steps): the sampled ids on the device,
        also left in ``tok_buf`` for the next step's late decode rows."""
        toks = None
        self._lp_dev = None
        self.apply_proc_updates(sp)
        if self.graphs is not None and self.graphs.eligible(host, sp):
            toks = self.graphs.run(host, sp)
        if toks is None:
            inp = self.to_device(host, sp)
            logits = self.model.forward(inp, self.k_caches, self.v_caches)
            toks = self.sample_device(logits, sp)
            self.tok_buf[:toks.shape[0]].copy_(toks)
            self._lp_dev = self.logprobs_device(logits, toks, sp)
        return toks

    def collect(self, h: "Launched") -> list[int]:
        if h.event is not None:
            h.event.synchronize()
        if h.err_idx is not None and int(self._err_host[h.err_idx]) != 0:
            raise CollectiveError("custom all-reduce / all-to-all: a peer did not arrive within 2 s; failing the "
                                  "replica")
        return h.tokens.tolist()

    def collect_logprobs(self, h: "Launched") -> dict:
        """{sampled row: (logprob, top_ids, top_lps)} of a collected step (call after ``collect``: same event)."""
        if h.logprobs is None:
            return {}
        buf, k, rows = h.logprobs
        tl, pl, pi = ops.unpack_logprob_records(buf, k)
        tl, pl, pi = tl.tolist(), pl.tolist(), pi.tolist()
        return {int(r): (tl[j], pi[j], pl[j]) for j, r in enumerate(rows.tolist())}
