"""fp8 (e4m3) expert weights for Mixtral (``weight_dtype="fp8"``): per-expert e4m3 wave tiles with one power-of-two
scale per row of every expert, streamed by the W8 instantiation of the grouped weight-streaming kernel.

As for the dense projections (tests/test_weight_fp8.py) the fp8 model IS the quantised model: row-major ``w13`` / ``w2``
hold the dequantised experts (exact in bf16), so the streamed decode steps, ``ops.grouped_gemm`` on prefill-sized steps,
the CPU reference path and the dense oracle compute with the same weights. Tolerances are the mirrored bf16 tests',
unchanged: the kernel's GLU atol 0.03 / rtol 0.02 and combine 0.02 / 0.01 against the fp32 reference on the
dequantised experts (tests/test_kernels_gpu.py test_wstream_grouped), greedy tokens within 0.15 (CPU) / 0.25 (GPU)
logits of the dense oracle (tests/test_weight_fp8.py). Rows carry power-of-two factors 2^-3..2^3 that differ between
experts, so a scale read for the global instead of the local expert, or for the untiled row, fails."""
import functools

import pytest
import torch
from test_weight_fp8 import _assert_greedy_gap, _close, _weight, _within_fp8

from kafka_llm_service_amd import ops
from kafka_llm_service_amd.ops import reference as ref


def _experts(E, N, K, seed, std=0.05, device="cpu"):
    """bf16 [E, N, K]: the ``_weight`` recipe per expert (other seeds: other row factors), rescaled to ``std``."""
    w = torch.stack([_weight(N, K, seed=seed + 101 * e).float() for e in range(E)]) * (std / 0.05)
    return w.to(torch.bfloat16).to(device)


def _cpu_routing(r):
    return ops.MoERouting(*(t.cpu() for t in (r.topk_w, r.topk_e, r.perm_tok, r.perm_w, r.expert_off, r.tile_off)),
                          r.num_experts)


# ---------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("glu", [False, True])
def test_tile_experts_fp8_roundtrip(glu):
    E, N, K = 3, 128, 512
    w = _experts(E, N, K, seed=1)
    assert not torch.equal(w[0].float().abs().amax(-1), w[1].float().abs().amax(-1))
    wt8, st = ops.tile_experts_fp8(w, glu=glu)
    assert wt8.dtype == torch.uint8 and wt8.shape == (E, N // 32, K // 32, 64, 16) and wt8.is_contiguous()
    assert st.dtype == torch.float32 and st.shape == (E, N) and st.is_contiguous()
    deq = ops.untile_experts_fp8(wt8, st, glu=glu)
    assert deq.dtype == torch.bfloat16 and deq.shape == (E, N, K)
    q, e = ref.fp8_quant(w)  # every row of every expert over its whole K
    exact = q.view(torch.float8_e4m3fn).float() * torch.exp2(e.float())[..., None]
    assert torch.equal(deq.float(), exact)
    assert torch.equal(exact.to(torch.bfloat16).float(), exact)
    _within_fp8(deq.float(), w.float())
    assert not torch.equal(st[0], st[1])  # the experts' scales differ
    for i in range(E):
        t, s = ops.tile_weight_fp8(w[i], glu=glu)
        assert torch.equal(wt8[i], t) and torch.equal(st[i], s)


def test_grouped_stream_fp8_cpu_equals_dequantised():
    """CPU path: fp8 expert tiles + scales == the same call on the bf16 tiles of the dequantised experts."""
    T, d, F, E, e_lo, e_n = 9, 512, 256, 8, 2, 4
    g = torch.Generator().manual_seed(4)
    x = torch.randn(T, d, generator=g).to(torch.bfloat16)
    r = ops.moe_route(torch.randn(T, E, generator=g).to(torch.bfloat16), 2)
    w13, w2 = _experts(e_n, 2 * F, d, seed=5), _experts(e_n, d, F, seed=6)
    w13_8, w13_s = ops.tile_experts_fp8(w13, glu=True)
    w2_8, w2_s = ops.tile_experts_fp8(w2)
    w13_t = ops.tile_experts(ops.untile_experts_fp8(w13_8, w13_s, glu=True), glu=True)
    w2_t = ops.tile_experts(ops.untile_experts_fp8(w2_8, w2_s))
    a8 = ops.grouped_stream_glu(x, w13_8, r, e_lo=e_lo, scale=w13_s)
    a = ops.grouped_stream_glu(x, w13_t, r, e_lo=e_lo)
    eo = r.expert_off.tolist()
    lo, hi = eo[e_lo], eo[e_lo + e_n]
    assert hi > lo and a8.shape == a.shape == (2 * T, F) and a8.dtype == a.dtype
    assert torch.equal(a8[lo:hi], a[lo:hi])
    a[:lo].zero_()  # (rows of the other ranks' experts are undefined: the combine does not read them)
    a[hi:].zero_()
    out8, out = torch.zeros(T, d), torch.zeros(T, d)
    ops.grouped_stream_combine(a, w2_8, r, T, out8, e_lo=e_lo, scale=w2_s)
    ops.grouped_stream_combine(a, w2_t, r, T, out, e_lo=e_lo)
    assert out.abs().max() > 0 and torch.equal(out8, out)
    with pytest.raises(ValueError):
        ops.grouped_stream_glu(x, w13_8, r, e_lo=e_lo)  # uint8 tiles without their scales
    with pytest.raises(ValueError):
        ops.grouped_stream_combine(a, w2_8, r, T, out8, e_lo=e_lo)


def _cpu_cfg(**kw):
    cfg = dict(model="tiny-mixtral", device="cpu", num_kv_blocks=256, max_model_len=2048)
    cfg.update(kw)
    return cfg


def _cpu_prompts(vocab=5000):
    g = torch.Generator().manual_seed(3)
    pre = torch.randint(0, vocab, (70,), generator=g).tolist()
    return [pre + torch.randint(0, vocab, (n,), generator=g).tolist() for n in (5, 17, 40)]


def test_engine_fp8_experts_cpu(tmp_path, monkeypatch):
    from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
    from kafka_llm_service_amd.engine.sequence import SamplingParams
    from kafka_llm_service_amd.models.weights import build_model, save_safetensors

    monkeypatch.delenv("KAFKA_WEIGHT_DTYPE", raising=False)
    monkeypatch.delenv("KAFKA_DECODE_GEMM", raising=False)
    bf16 = LLMEngine(EngineConfig(**_cpu_cfg(decode_gemm="stream")))
    eng = LLMEngine(EngineConfig(**_cpu_cfg(weight_dtype="fp8")))
    m = eng.model
    assert m.stream and not m.tiled_only and m.weight_dtype == "fp8"
    for lw, lb in zip(m.layers, bf16.model.layers):
        E, N13, d = lb.w13.shape
        assert lw.w13_t.dtype == torch.uint8 and lw.w13_t.shape == (E, N13 // 32, d // 32, 64, 16)
        assert lw.w2_t.dtype == torch.uint8 and lw.w2_t.shape == (E, d // 32, N13 // 64, 64, 16)
        assert lw.w13_s.dtype == torch.float32 and lw.w13_s.shape == (E, N13)
        assert lw.w2_s.dtype == torch.float32 and lw.w2_s.shape == (E, d)
        assert torch.equal(lw.w13, ops.untile_experts_fp8(lw.w13_t, lw.w13_s, glu=True))
        assert torch.equal(lw.w2, ops.untile_experts_fp8(lw.w2_t, lw.w2_s))
        assert not torch.equal(lw.w13, lb.w13)  # quantised ...
        _within_fp8(lw.w13.float(), lb.w13.float())  # ... within e4m3 of the same random-init experts
        _within_fp8(lw.w2.float(), lb.w2.float())
        assert lw.router.dtype == torch.bfloat16 and torch.equal(lw.router, lb.router)
        assert lw.qkv_t.dtype == torch.uint8  # (the attention projections as before)
    assert not any(k.endswith("_s") or k.endswith("_t") for k in m.named_tensors())
    prompts = _cpu_prompts()
    sp = SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True)
    outs = eng.generate(prompts, sp)
    assert eng.generate(prompts, sp) == outs  # prefix-cached rerun
    _assert_greedy_gap(m, prompts, outs, 0.15)
    assert m.weight_bytes() < bf16.model.weight_bytes()
    # experts counted as fp8 + scales: one byte per element and 4 per row, against two bytes per element
    exp8 = sum(t.numel() * t.element_size() for lw in m.layers for t in (lw.w13_t, lw.w13_s, lw.w2_t, lw.w2_s))
    exp16 = sum(t.numel() * t.element_size() for lw in bf16.model.layers for t in (lw.w13_t, lw.w2_t))
    assert exp8 < 0.52 * exp16
    assert bf16.model.weight_bytes() - m.weight_bytes() >= exp16 - exp8
    assert m.stream_weight_bytes("fp8") < bf16.model.stream_weight_bytes() * 0.52
    # safetensors export, then build_model: the dequantised experts
    save_safetensors(m, tmp_path / "model.safetensors")
    back = build_model(m.cfg, "cpu", weights=str(tmp_path))
    for i, lw in enumerate(m.layers):
        assert torch.equal(back.layers[i].w13, ops.untile_experts_fp8(lw.w13_t, lw.w13_s, glu=True))
        assert torch.equal(back.layers[i].w2, ops.untile_experts_fp8(lw.w2_t, lw.w2_s))
        assert torch.equal(back.layers[i].router, lw.router)
    # tiled-only mode: the single row-major expert copy stays unquantised bf16
    only = LLMEngine(EngineConfig(**_cpu_cfg(weight_dtype="fp8", decode_gemm="stream_only")))
    for lw, lb in zip(only.model.layers, bf16.model.layers):
        assert only.model.tiled_only and lw.w13_t is None and lw.w2_t is None and lw.w13_s is None and lw.w2_s is None
        assert torch.equal(lw.w13, lb.w13) and torch.equal(lw.w2, lb.w2)
        assert lw.qkv_t.dtype == torch.uint8 and lw.qkv is None


def test_fp8_expert_tiles_of_ep_ranks_are_slices():
    """Every expert-parallel rank quantises its own whole experts: its tiles and scales equal the matching slice of the
    EP = 1 model's (models built directly, no process group)."""
    from kafka_llm_service_amd.models.config import get_config
    from kafka_llm_service_amd.models.weights import build_model

    cfg = get_config("tiny-mixtral")
    full = build_model(cfg, "cpu")
    full.enable_stream_weights(weight_dtype="fp8")
    n = cfg.num_experts // 2
    for rank in (0, 1):
        part = build_model(cfg, "cpu", tp=2, tp_rank=rank)
        part.enable_stream_weights(weight_dtype="fp8")
        e0 = rank * n
        for lw, lf in zip(part.layers, full.layers):
            assert lw.w13_t.shape[0] == n and lw.w13_s.shape == (n, lf.w13_s.shape[1])
            for name in ("w13_t", "w13_s", "w2_t", "w2_s", "w13", "w2"):
                assert torch.equal(getattr(lw, name), getattr(lf, name)[e0:e0 + n]), name


# ---------------------------------------------------------------------------------------------------------------- GPU
@functools.lru_cache(maxsize=None)
def _gpu_experts(e_n, d, F):
    """(w13 tiles, scales, dequantised w13, w2 tiles, scales, dequantised w2), GPU tiles and CPU fp32 dequantised
    experts, built once per shape."""
    dev = torch.device("cuda:0")
    w13 = _experts(e_n, 2 * F, d, seed=d + F, std=d ** -0.5, device=dev)
    w2 = _experts(e_n, d, F, seed=d + F + 7, std=F ** -0.5, device=dev)
    w13_8, w13_s = ops.tile_experts_fp8(w13, glu=True)
    w2_8, w2_s = ops.tile_experts_fp8(w2)
    d13, d2 = ops.untile_experts_fp8(w13_8, w13_s, glu=True), ops.untile_experts_fp8(w2_8, w2_s)
    _within_fp8(d13.float(), w13.float())
    _within_fp8(d2.float(), w2.float())
    assert not torch.equal(w13_s[0], w13_s[-1]) and not torch.equal(w2_s[0], w2_s[-1])
    return w13_8, w13_s, d13.float().cpu(), w2_8, w2_s, d2.float().cpu()


def _check_grouped_fp8(x, logits, d, F, E, e_lo, e_n, msg):
    """Both halves of the expert MLP on fp8 tiles vs the fp32 reference on the dequantised experts. Returns the
    routing (CPU)."""
    T = x.shape[0]
    w13_8, w13_s, d13, w2_8, w2_s, d2 = _gpu_experts(e_n, d, F)
    r = ops.moe_route(logits, 2)
    rc = _cpu_routing(r)
    a = ops.grouped_stream_glu(x, w13_8, r, e_lo=e_lo, scale=w13_s)
    h_ref = torch.zeros(T * 2, 2 * F)
    ref.grouped_gemm(x.cpu().float(), d13, rc.perm_tok, rc.perm_w, rc.expert_off, e_lo, True, h_ref, None)
    eo = rc.expert_off.tolist()
    lo, hi = eo[e_lo], eo[e_lo + e_n]
    _close(a[lo:hi], ref.silu_mul(h_ref[lo:hi]), atol=0.03, rtol=0.02, msg=f"grouped glu fp8 {msg}")
    out = torch.zeros(T, d, device=x.device)
    ops.grouped_stream_combine(a, w2_8, r, T, out, e_lo=e_lo, scale=w2_s)
    out_ref = torch.zeros(T, d)
    ref.grouped_gemm(a.cpu().float(), d2, rc.perm_tok, rc.perm_w, rc.expert_off, e_lo, False, None, out_ref)
    _close(out, out_ref, atol=0.02, rtol=0.01, msg=f"grouped combine fp8 {msg}")
    torch.cuda.synchronize()
    return rc


GROUPED_SHAPES = [(1, 512, 512, 8, 0, 8), (37, 1024, 768, 8, 0, 8), (100, 768, 256, 8, 4, 4),
                  (128, 512, 1024, 8, 2, 4), (300, 1024, 512, 8, 0, 8), (640, 512, 512, 8, 0, 8),
                  (200, 512, 1024, 8, 2, 4), (64, 4096, 1792, 8, 0, 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("T,d,F,E,e_lo,e_n,pin",
                         [s + (True,) for s in GROUPED_SHAPES] + [GROUPED_SHAPES[1] + (False,),
                                                                  GROUPED_SHAPES[4] + (False,)])
def test_wstream_grouped_fp8(cuda, monkeypatch, T, d, F, E, e_lo, e_n, pin):
    """W8 grouped streaming kernel (GLU-tiled w13 with fused SwiGLU, w2 with the fused weighted combine), the routing
    of ``ops.moe_route`` as test_wstream_grouped: every row-tile size (MT = 1 / 2 / 4), 1..16 chunks with odd counts,
    a one-chunk w2, expert-parallel subsets (local-expert indexing of tiles and scales), pinned and unpinned."""
    monkeypatch.setattr(ops, "GROUPED_PIN", pin)
    torch.manual_seed(9)
    x = torch.randn(T, d, device=cuda, dtype=torch.bfloat16)
    logits = torch.randn(T, E, device=cuda).to(torch.bfloat16)
    _check_grouped_fp8(x, logits, d, F, E, e_lo, e_n, f"T={T} d={d} F={F} e_lo={e_lo} pin={pin}")


@pytest.mark.gpu
def test_wstream_grouped_fp8_thirty_row_expert(cuda):
    """MT = 4 (T >= 193) at K = 512 with one expert owning exactly 30 rows — the case the comment above the grouped
    kernel's MFMA loop describes (28..32 rows: row tile 0 only just used, tiles 1..3 computed but never stored)."""
    T, d, F, E, hot = 200, 512, 512, 8, 3
    others = [e for e in range(E) if e != hot]
    logits = torch.full((T, E), -8.0)
    for t in range(T):
        if t < 30:  # the first 30 tokens pick the hot expert and one other, nobody else picks it
            logits[t, hot], logits[t, others[t % 7]] = 4.0, 3.0
        else:
            logits[t, others[t % 7]], logits[t, others[(t + 3) % 7]] = 4.0, 3.0
    torch.manual_seed(10)
    x = torch.randn(T, d, device=cuda, dtype=torch.bfloat16)
    rc = _check_grouped_fp8(x, logits.to(torch.bfloat16).to(cuda), d, F, E, 0, E, "30-row expert")
    eo = rc.expert_off.tolist()
    assert eo[hot + 1] - eo[hot] == 30


@pytest.mark.gpu
@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graphs"])
def test_mixtral_engine_fp8_experts_gpu(cuda, graphs, monkeypatch):
    """tiny-mixtral with fp8 experts vs the dense oracle (which reads the dequantised experts): prefill steps above
    MOE_STREAM_MAX_T run ops.grouped_gemm on them, decode steps the W8 grouped streaming kernel."""
    from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
    from kafka_llm_service_amd.engine.sequence import SamplingParams
    from kafka_llm_service_amd.models import moe

    monkeypatch.delenv("KAFKA_WEIGHT_DTYPE", raising=False)
    monkeypatch.setattr(moe, "MOE_STREAM_MAX_T", 32)
    calls = {"stream": 0, "gemm": 0}
    glu, gemm = ops.grouped_stream_glu, ops.grouped_gemm

    def counted_glu(x, wt, *a, **kw):
        assert wt.dtype == torch.uint8 and kw.get("scale") is not None
        calls["stream"] += 1
        return glu(x, wt, *a, **kw)

    def counted_gemm(*a, **kw):
        calls["gemm"] += 1
        return gemm(*a, **kw)

    monkeypatch.setattr(ops, "grouped_stream_glu", counted_glu)
    monkeypatch.setattr(ops, "grouped_gemm", counted_gemm)
    e = LLMEngine(EngineConfig(model="tiny-mixtral", device=str(cuda), num_kv_blocks=1024, max_model_len=4096,
                               weight_dtype="fp8", use_graphs=graphs))
    lw = e.model.layers[0]
    assert lw.w13_t.dtype == torch.uint8 and lw.w2_t.dtype == torch.uint8
    assert torch.equal(lw.w13, ops.untile_experts_fp8(lw.w13_t, lw.w13_s, glu=True))
    g = torch.Generator().manual_seed(3)  # prompts as tests/test_engine_gpu.py test_mixtral_engine_matches_oracle
    prefix = torch.randint(0, e.model_cfg.vocab_size, (64,), generator=g).tolist()
    prompts = [prefix + torch.randint(0, e.model_cfg.vocab_size, (n,), generator=g).tolist() for n in (5, 40, 130)]
    outs = e.generate(prompts, SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True))
    assert calls["stream"] >= 1 and calls["gemm"] >= 1, calls
    if graphs:
        assert not e.runner.graphs.disabled and e.runner.graphs.stats["replays"] >= 1
    _assert_greedy_gap(e.model, prompts, outs, 0.25)
