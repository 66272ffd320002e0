"""MXFP4 (e2m1, e8m0 block scales) expert weights for Mixtral (``weight_dtype="mxfp4"``): per-expert e2m1 wave tiles with
the dense block-scale image per expert, streamed by the W4 instantiation of the grouped weight-streaming kernel.

The file mirrors tests/test_weight_fp8_moe.py one for one. As there, the mxfp4 model IS the quantised model: row-major
``w13`` / ``w2`` hold the dequantised experts (e2m1 * 2^e, exact in bf16), so the streamed decode steps,
``ops.grouped_gemm`` on prefill-sized steps, the CPU reference path and the dense oracle compute with the same weights.
Tolerances are the mirrored tests', unchanged, because the references run on the same dequantised weights and the error
left is bf16 output rounding plus accumulation order: GLU atol 0.03 / rtol 0.02 and combine 0.02 / 0.01 against the fp32
reference (``_check_grouped_fp8``), greedy tokens within 0.15 (CPU, tests/test_weight_mxfp4.py) / 0.25 (GPU) logits of
the dense oracle. The GLU half is in addition compared BITWISE with the bf16 grouped kernel on the dequantised experts:
the B fragments are the same bf16 values, the MT / KC choice is shared and every accumulator sees the same MFMA sequence
(the combine half adds with float atomics in no fixed order and is not compared bitwise).
Weights carry a random power of two per row AND per 32-column block (tests/test_weight_mxfp4.py ``_weight``) under seeds
that differ between experts, so a scale read for the global instead of the local expert, for another row or for another
block fails. Expert bytes: 4.25 bits per weight against 16, 0.266 (< 0.28)."""
import functools

import pytest
import torch
from test_weight_fp8_moe import GROUPED_SHAPES, _cpu_routing
from test_weight_mxfp4 import E8, F4, _assert_greedy_gap, _close, _u8, _weight, _within_mxfp4

from kafka_llm_service_amd import ops
from kafka_llm_service_amd.ops import reference as ref


def _experts(E, N, K, seed, std=0.05, device="cpu"):
    """bf16 [E, N, K]: the mxfp4 ``_weight`` recipe per expert (other seeds: other row and block factors), rescaled to
    ``std``."""
    w = torch.stack([_weight(N, K, seed=seed + 101 * e).float() for e in range(E)]) * (std / 0.05)
    return w.to(torch.bfloat16).to(device)


def _within(deq, w):
    for e in range(w.shape[0]):
        _within_mxfp4(deq[e].float(), w[e].float())


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_mxfp4_format_has_expert_tiles():
    from kafka_llm_service_amd.models.llama import TransformerLM

    assert ops.weight_format("mxfp4").experts
    assert TransformerLM._expert_dtype("mxfp4") == "mxfp4"


@pytest.mark.parametrize("glu", [False, True])
def test_tile_experts_mxfp4_roundtrip(glu):
    E, N, K = 3, 128, 512
    w = _experts(E, N, K, seed=1)
    wt4, se = ops.tile_experts_as(w, "mxfp4", glu)
    assert wt4.dtype == F4 and wt4.shape == (E, N // 32, K // 64, 64, 16) and wt4.is_contiguous()
    assert se.dtype == E8 and se.shape == (E, N // 32, K // 64, 32, 2) and se.is_contiguous()
    deq = ops.untile_experts_as(wt4, se, glu)
    assert deq.dtype == torch.bfloat16 and deq.shape == (E, N, K)
    _within(deq, w)
    assert not torch.equal(_u8(se)[0], _u8(se)[1])  # the experts' scales differ
    for i in range(E):  # per expert exactly the dense images and the dense dequantisation of that expert alone
        t, s = ops.tile_weight_mxfp4(w[i], glu=glu)
        assert torch.equal(_u8(wt4)[i], _u8(t)) and torch.equal(_u8(se)[i], _u8(s))
        assert torch.equal(deq[i], ops.untile_weight_mxfp4(t, s, glu=glu))
    # the named pair is the same loop
    wt4b, seb = ops.tile_experts_mxfp4(w, glu=glu)
    assert torch.equal(_u8(wt4b), _u8(wt4)) and torch.equal(_u8(seb), _u8(se))
    assert torch.equal(ops.untile_experts_mxfp4(wt4, se, glu=glu), deq)


def test_grouped_stream_mxfp4_cpu_equals_dequantised():
    """CPU path: mxfp4 expert tiles + scale images == the same call on the bf16 tiles of the dequantised experts."""
    T, d, F, E, e_lo, e_n = 9, 512, 256, 8, 2, 4
    g = torch.Generator().manual_seed(4)
    x = torch.randn(T, d, generator=g).to(torch.bfloat16)
    r = ops.moe_route(torch.randn(T, E, generator=g).to(torch.bfloat16), 2)
    w13, w2 = _experts(e_n, 2 * F, d, seed=5), _experts(e_n, d, F, seed=6)
    w13_4, w13_s = ops.tile_experts_mxfp4(w13, glu=True)
    w2_4, w2_s = ops.tile_experts_mxfp4(w2)
    w13_t = ops.tile_experts(ops.untile_experts_mxfp4(w13_4, w13_s, glu=True), glu=True)
    w2_t = ops.tile_experts(ops.untile_experts_mxfp4(w2_4, w2_s))
    a4 = ops.grouped_stream_glu(x, w13_4, r, e_lo=e_lo, scale=w13_s)
    a = ops.grouped_stream_glu(x, w13_t, r, e_lo=e_lo)
    eo = r.expert_off.tolist()
    lo, hi = eo[e_lo], eo[e_lo + e_n]
    assert hi > lo and a4.shape == a.shape == (2 * T, F) and a4.dtype == a.dtype
    assert torch.equal(a4[lo:hi], a[lo:hi])
    a[:lo].zero_()  # (rows of the other ranks' experts are undefined: the combine does not read them)
    a[hi:].zero_()
    out4, out = torch.zeros(T, d), torch.zeros(T, d)
    ops.grouped_stream_combine(a, w2_4, r, T, out4, e_lo=e_lo, scale=w2_s)
    ops.grouped_stream_combine(a, w2_t, r, T, out, e_lo=e_lo)
    assert out.abs().max() > 0 and torch.equal(out4, out)
    with pytest.raises(ValueError):
        ops.grouped_stream_glu(x, w13_4, r, e_lo=e_lo)  # e2m1 tiles without their scale images
    with pytest.raises(ValueError):
        ops.grouped_stream_combine(a, w2_4, r, T, out4, e_lo=e_lo)
    with pytest.raises(ValueError):
        ops.grouped_stream_glu(x, w13_4, r, e_lo=e_lo, scale=torch.ones(e_n, 2 * F))  # fp8-style row scales
    with pytest.raises(ValueError):
        ops.grouped_stream_combine(a, w2_4, r, T, out4, e_lo=e_lo, scale=w2_s[:, :, :-1])  # another K


def _cpu_cfg(**kw):
    cfg = dict(model="tiny-mixtral", device="cpu", num_kv_blocks=256, max_model_len=2048)
    cfg.update(kw)
    return cfg


def _cpu_prompts(vocab=5000):
    g = torch.Generator().manual_seed(3)
    pre = torch.randint(0, vocab, (70,), generator=g).tolist()
    return [pre + torch.randint(0, vocab, (n,), generator=g).tolist() for n in (5, 17, 40)]


def _nbytes(*ts):
    return sum(t.numel() * t.element_size() for t in ts)


def test_engine_mxfp4_experts_cpu(tmp_path, monkeypatch):
    from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
    from kafka_llm_service_amd.engine.sequence import SamplingParams
    from kafka_llm_service_amd.models.weights import build_model, save_safetensors

    monkeypatch.delenv("KAFKA_WEIGHT_DTYPE", raising=False)
    monkeypatch.delenv("KAFKA_DECODE_GEMM", raising=False)
    bf16 = LLMEngine(EngineConfig(**_cpu_cfg(decode_gemm="stream")))
    eng = LLMEngine(EngineConfig(**_cpu_cfg(weight_dtype="mxfp4")))
    m = eng.model
    assert m.stream and not m.tiled_only and m.weight_dtype == "mxfp4"
    for lw, lb in zip(m.layers, bf16.model.layers):
        E, N13, d = lb.w13.shape
        assert lw.w13_t.dtype == F4 and lw.w13_t.shape == (E, N13 // 32, d // 64, 64, 16)
        assert lw.w2_t.dtype == F4 and lw.w2_t.shape == (E, d // 32, N13 // 128, 64, 16)
        assert lw.w13_s.dtype == E8 and lw.w13_s.shape == (E, N13 // 32, d // 64, 32, 2)
        assert lw.w2_s.dtype == E8 and lw.w2_s.shape == (E, d // 32, N13 // 128, 32, 2)
        assert torch.equal(lw.w13, ops.untile_experts_mxfp4(lw.w13_t, lw.w13_s, glu=True))
        assert torch.equal(lw.w2, ops.untile_experts_mxfp4(lw.w2_t, lw.w2_s))
        assert not torch.equal(lw.w13, lb.w13)  # quantised ...
        _within(lw.w13, lb.w13)  # ... within the mxfp4 rule of the same random-init experts
        _within(lw.w2, lb.w2)
        assert lw.router.dtype == torch.bfloat16 and torch.equal(lw.router, lb.router)
        assert lw.qkv_t.dtype == F4  # (the attention projections as before)
    assert not any(k.endswith("_s") or k.endswith("_t") for k in m.named_tensors())
    prompts = _cpu_prompts()
    sp = SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True)
    outs = eng.generate(prompts, sp)
    _assert_greedy_gap(m, prompts, outs, 0.15)
    # prefix-cached rerun (other step shapes, other summation order): held to the oracle like the first run, not to the
    # first run's tokens — these random-init logits have exact bf16 ties between the top two tokens at some positions.
    # A third run takes the second's path (same cached prefix, same step shapes) and must repeat it token for token.
    again = eng.generate(prompts, sp)
    _assert_greedy_gap(m, prompts, again, 0.15)
    assert eng.generate(prompts, sp) == again
    assert m.weight_bytes() < bf16.model.weight_bytes()
    # experts counted as e2m1 + exponents: 4.25 bits per weight against 16 (0.266)
    exp4 = sum(_nbytes(lw.w13_t, lw.w13_s, lw.w2_t, lw.w2_s) for lw in m.layers)
    exp16 = sum(_nbytes(lw.w13_t, lw.w2_t) for lw in bf16.model.layers)
    assert exp4 < 0.28 * exp16
    assert bf16.model.weight_bytes() - m.weight_bytes() >= exp16 - exp4
    assert m.stream_weight_bytes("mxfp4") < bf16.model.stream_weight_bytes() * 0.28
    # safetensors export, then build_model: the dequantised experts
    save_safetensors(m, tmp_path / "model.safetensors")
    back = build_model(m.cfg, "cpu", weights=str(tmp_path))
    for i, lw in enumerate(m.layers):
        assert torch.equal(back.layers[i].w13, ops.untile_experts_mxfp4(lw.w13_t, lw.w13_s, glu=True))
        assert torch.equal(back.layers[i].w2, ops.untile_experts_mxfp4(lw.w2_t, lw.w2_s))
        assert torch.equal(back.layers[i].router, lw.router)
    # tiled-only mode: the single row-major expert copy stays unquantised bf16
    only = LLMEngine(EngineConfig(**_cpu_cfg(weight_dtype="mxfp4", decode_gemm="stream_only")))
    for lw, lb in zip(only.model.layers, bf16.model.layers):
        assert only.model.tiled_only and lw.w13_t is None and lw.w2_t is None and lw.w13_s is None and lw.w2_s is None
        assert torch.equal(lw.w13, lb.w13) and torch.equal(lw.w2, lb.w2)
        assert lw.qkv_t.dtype == F4 and lw.qkv is None


def test_mxfp4_expert_tiles_of_ep_ranks_are_slices():
    """Every expert-parallel rank quantises its own whole experts: its tiles, scale images and row-major experts equal the
    matching slice of the EP = 1 model's (models built directly, no process group)."""
    from kafka_llm_service_amd.models.config import get_config
    from kafka_llm_service_amd.models.weights import build_model

    cfg = get_config("tiny-mixtral")
    full = build_model(cfg, "cpu")
    full.enable_stream_weights(weight_dtype="mxfp4")
    n = cfg.num_experts // 2
    for rank in (0, 1):
        part = build_model(cfg, "cpu", tp=2, tp_rank=rank)
        part.enable_stream_weights(weight_dtype="mxfp4")
        e0 = rank * n
        for lw, lf in zip(part.layers, full.layers):
            assert lw.w13_t.dtype == F4 and lw.w13_s.dtype == E8
            assert lw.w13_t.shape[0] == n and lw.w13_s.shape == (n, *lf.w13_s.shape[1:])
            for name in ("w13_t", "w13_s", "w2_t", "w2_s"):
                assert torch.equal(_u8(getattr(lw, name)), _u8(getattr(lf, name))[e0:e0 + n]), name
            for name in ("w13", "w2"):
                assert torch.equal(getattr(lw, name), getattr(lf, name)[e0:e0 + n]), name


# ---------------------------------------------------------------------------------------------------------------- GPU
@functools.lru_cache(maxsize=None)
def _gpu_experts(e_n, d, F):
    """(w13 tiles, scale images, dequantised w13 bf16 on the GPU, w2 tiles, scale images, dequantised w2), built once per
    shape."""
    dev = torch.device("cuda:0")
    w13 = _experts(e_n, 2 * F, d, seed=d + F, std=d ** -0.5, device=dev)
    w2 = _experts(e_n, d, F, seed=d + F + 7, std=F ** -0.5, device=dev)
    w13_4, w13_s = ops.tile_experts_mxfp4(w13, glu=True)
    w2_4, w2_s = ops.tile_experts_mxfp4(w2)
    d13, d2 = ops.untile_experts_mxfp4(w13_4, w13_s, glu=True), ops.untile_experts_mxfp4(w2_4, w2_s)
    _within(d13, w13)
    _within(d2, w2)
    assert not torch.equal(_u8(w13_s)[0], _u8(w13_s)[-1]) and not torch.equal(_u8(w2_s)[0], _u8(w2_s)[-1])
    return w13_4, w13_s, d13, w2_4, w2_s, d2


@functools.lru_cache(maxsize=None)
def _ref_experts(e_n, d, F):
    """The dequantised experts as CPU fp32, for the reference."""
    _, _, d13, _, _, d2 = _gpu_experts(e_n, d, F)
    return d13.float().cpu(), d2.float().cpu()


def _check_grouped_mxfp4(x, logits, d, F, E, e_lo, e_n, msg):
    """Both halves of the expert MLP on mxfp4 tiles vs the fp32 reference on the dequantised experts; the tolerances of
    ``_check_grouped_fp8``. Returns the routing (CPU)."""
    T = x.shape[0]
    w13_4, w13_s, _, w2_4, w2_s, _ = _gpu_experts(e_n, d, F)
    d13, d2 = _ref_experts(e_n, d, F)
    r = ops.moe_route(logits, 2)
    rc = _cpu_routing(r)
    a = ops.grouped_stream_glu(x, w13_4, r, e_lo=e_lo, scale=w13_s)
    h_ref = torch.zeros(T * 2, 2 * F)
    ref.grouped_gemm(x.cpu().float(), d13, rc.perm_tok, rc.perm_w, rc.expert_off, e_lo, True, h_ref, None)
    eo = rc.expert_off.tolist()
    lo, hi = eo[e_lo], eo[e_lo + e_n]
    _close(a[lo:hi], ref.silu_mul(h_ref[lo:hi]), atol=0.03, rtol=0.02, msg=f"grouped glu mxfp4 {msg}")
    out = torch.zeros(T, d, device=x.device)
    ops.grouped_stream_combine(a, w2_4, r, T, out, e_lo=e_lo, scale=w2_s)
    out_ref = torch.zeros(T, d)
    ref.grouped_gemm(a.cpu().float(), d2, rc.perm_tok, rc.perm_w, rc.expert_off, e_lo, False, None, out_ref)
    _close(out, out_ref, atol=0.02, rtol=0.01, msg=f"grouped combine mxfp4 {msg}")
    torch.cuda.synchronize()
    return rc


@pytest.mark.gpu
@pytest.mark.parametrize("T,d,F,E,e_lo,e_n,pin",
                         [s + (True,) for s in GROUPED_SHAPES] + [GROUPED_SHAPES[1] + (False,),
                                                                  GROUPED_SHAPES[4] + (False,)])
def test_wstream_grouped_mxfp4(cuda, monkeypatch, T, d, F, E, e_lo, e_n, pin):
    """W4 grouped streaming kernel (GLU-tiled w13 with fused SwiGLU, w2 with the fused weighted combine), the routing
    of ``ops.moe_route``: every row-tile size (MT = 1 / 2 / 4), 1..16 chunks with odd counts, a one-chunk w2,
    expert-parallel subsets (local-expert indexing of tiles and scale images), the real K = 4096, pinned and unpinned."""
    monkeypatch.setattr(ops, "GROUPED_PIN", pin)
    torch.manual_seed(9)
    x = torch.randn(T, d, device=cuda, dtype=torch.bfloat16)
    logits = torch.randn(T, E, device=cuda).to(torch.bfloat16)
    _check_grouped_mxfp4(x, logits, d, F, E, e_lo, e_n, f"T={T} d={d} F={F} e_lo={e_lo} pin={pin}")


@pytest.mark.gpu
@pytest.mark.parametrize("T,d,F,E,e_lo,e_n,mt",
                         [(24, 1024, 768, 8, 0, 8, 1), GROUPED_SHAPES[1] + (2,), GROUPED_SHAPES[3] + (2,),
                          GROUPED_SHAPES[4] + (4,)], ids=["mt1-24", "mt2-37", "mt2-128", "mt4-300"])
def test_wstream_grouped_mxfp4_glu_bit_equals_bf16_kernel(cuda, T, d, F, E, e_lo, e_n, mt):
    """The GLU half on mxfp4 tiles is bit for bit the bf16 grouped kernel on ``tile_experts(dequantised, glu=True)`` under
    the same routing: identical B fragments (e2m1 * 2^e is exact in bf16), shared MT / KC choice, the same MFMA sequence
    per accumulator. The launcher picks MT from max_rows = T (<= 32: 1, <= 192: 2, else 4), so (37, 1024, 768) and
    (128, 512, 1024) both run MT = 2 and (300, 1024, 512) MT = 4; the 24-token shape (the tiles of the 37-token one) is
    the MT = 1 case."""
    assert mt == (1 if T <= 32 else (2 if T <= 192 else 4))  # kafka_launch_wstream_grouped's rule, max_rows = T
    w13_4, w13_s, d13, _, _, _ = _gpu_experts(e_n, d, F)
    w13_t = ops.tile_experts(d13, glu=True)
    torch.manual_seed(9)
    x = torch.randn(T, d, device=cuda, dtype=torch.bfloat16)
    r = ops.moe_route(torch.randn(T, E, device=cuda).to(torch.bfloat16), 2)
    a4 = ops.grouped_stream_glu(x, w13_4, r, e_lo=e_lo, scale=w13_s)
    a16 = ops.grouped_stream_glu(x, w13_t, r, e_lo=e_lo)
    torch.cuda.synchronize()
    eo = r.expert_off.tolist()
    lo, hi = eo[e_lo], eo[e_lo + e_n]
    assert hi - lo >= T // 2 and a4[lo:hi].float().abs().max() > 0
    diff = (a4[lo:hi].float() - a16[lo:hi].float()).abs()
    print(f"glu mxfp4 vs bf16 kernel T={T} MT={mt}: rows {hi - lo}, differing elements {int((diff > 0).sum())}, "
          f"max |diff| {float(diff.max())}")
    assert torch.equal(a4[lo:hi], a16[lo:hi])


@pytest.mark.gpu
def test_wstream_grouped_mxfp4_thirty_row_expert(cuda):
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
    rc = _check_grouped_mxfp4(x, logits.to(torch.bfloat16).to(cuda), d, F, E, 0, E, "30-row expert")
    eo = rc.expert_off.tolist()
    assert eo[hot + 1] - eo[hot] == 30


# ---- the binding: fp8 and mxfp4 expert tiles are both uint8 [E, ., ., 64, 16]; the caller names the format ----------
SENTINEL = 7.0


@pytest.mark.gpu
def test_binding_grouped_mxfp4_matches_and_refusals(cuda):
    """Matching buffers run; fp8 tiles named mxfp4, mxfp4 tiles named fp8, mxfp4 tiles with fp8 row scales and a scale
    image of another K are refused on the host, before any launch (the output keeps its sentinel)."""
    from kafka_llm_service_amd.ops._ext import ext

    T, d, F, E = 8, 512, 256, 4
    fp8, mx = ops.weight_format("fp8").abi, ops.weight_format("mxfp4").abi
    w13 = _experts(E, 2 * F, d, seed=21, device=cuda)
    t4, s4 = ops.tile_experts_mxfp4(w13, glu=True)
    t8, s8 = ops.tile_experts_fp8(w13, glu=True)
    t4u, s4u = _u8(t4), _u8(s4)
    torch.manual_seed(12)
    x = torch.randn(T, d, device=cuda, dtype=torch.bfloat16)
    r = ops.moe_route(torch.randn(T, E, device=cuda).to(torch.bfloat16), 2)

    def call(wt, scale, fmt):
        y = torch.full((2 * T, F), SENTINEL, device=cuda, dtype=torch.bfloat16)
        ext().wstream_grouped(x, wt, scale, fmt, r.perm_tok, r.perm_w, r.expert_off, 0, T, True, y, None, True)
        torch.cuda.synchronize()
        return y

    def refused(wt, scale, fmt):
        y = torch.full((2 * T, F), SENTINEL, device=cuda, dtype=torch.bfloat16)
        with pytest.raises(RuntimeError):
            ext().wstream_grouped(x, wt, scale, fmt, r.perm_tok, r.perm_w, r.expert_off, 0, T, True, y, None, True)
        torch.cuda.synchronize()
        assert (y == SENTINEL).all(), "a refused call wrote its output"

    # control: the same buffers under their own names run and agree with ops
    y4 = call(t4u, s4u, mx)
    assert torch.equal(y4, ops.grouped_stream_glu(x, t4, r, scale=s4))
    deq = ops.untile_experts_mxfp4(t4, s4, glu=True).float().cpu()
    rc = _cpu_routing(r)
    h_ref = torch.zeros(2 * T, 2 * F)
    ref.grouped_gemm(x.cpu().float(), deq, rc.perm_tok, rc.perm_w, rc.expert_off, 0, True, h_ref, None)
    _close(y4, ref.silu_mul(h_ref), atol=0.03, rtol=0.02, msg="binding mxfp4")
    y8 = call(t8, s8, fp8)
    assert (y8 != SENTINEL).any()
    refused(t8, s8, mx)                       # fp8 tiles named mxfp4 (their own row scales)
    refused(t8, s4u, mx)                      # ... with an mxfp4 image: the tiles' K / 32 is not the image's K / 64
    refused(t4u, s4u, fp8)                    # mxfp4 tiles named fp8
    refused(t4u, s8, fp8)                     # ... even with the row scales an fp8 expert of this N would have
    refused(t4u, s8, mx)                      # mxfp4 tiles with fp8 row scales
    refused(t4u, s4u[:, :, :-1].contiguous(), mx)                    # a scale image of another K
    refused(t4u, torch.cat((s4u, s4u), 2).contiguous(), mx)
    refused(t4u, None, mx)                    # no scale


@pytest.mark.gpu
@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graphs"])
def test_mixtral_engine_mxfp4_experts_gpu(cuda, graphs, monkeypatch):
    """tiny-mixtral with mxfp4 experts vs the dense oracle (which reads the dequantised experts): prefill steps above
    MOE_STREAM_MAX_T run ops.grouped_gemm on them, decode steps the W4 grouped streaming kernel."""
    from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
    from kafka_llm_service_amd.engine.sequence import SamplingParams
    from kafka_llm_service_amd.models import moe

    monkeypatch.delenv("KAFKA_WEIGHT_DTYPE", raising=False)
    monkeypatch.setattr(moe, "MOE_STREAM_MAX_T", 32)
    calls = {"stream": 0, "gemm": 0}
    glu, gemm = ops.grouped_stream_glu, ops.grouped_gemm

    def counted_glu(x, wt, *a, **kw):
        assert wt.dtype == F4 and kw.get("scale") is not None and kw["scale"].dtype == E8
        calls["stream"] += 1
        return glu(x, wt, *a, **kw)

    def counted_gemm(*a, **kw):
        calls["gemm"] += 1
        return gemm(*a, **kw)

    monkeypatch.setattr(ops, "grouped_stream_glu", counted_glu)
    monkeypatch.setattr(ops, "grouped_gemm", counted_gemm)
    e = LLMEngine(EngineConfig(model="tiny-mixtral", device=str(cuda), num_kv_blocks=1024, max_model_len=4096,
                               weight_dtype="mxfp4", use_graphs=graphs))
    lw = e.model.layers[0]
    assert lw.w13_t.dtype == F4 and lw.w2_t.dtype == F4 and lw.w13_s.dtype == E8 and lw.w2_s.dtype == E8
    assert torch.equal(lw.w13, ops.untile_experts_mxfp4(lw.w13_t, lw.w13_s, glu=True))
    g = torch.Generator().manual_seed(3)  # prompts as tests/test_weight_fp8_moe.py test_mixtral_engine_fp8_experts_gpu
    prefix = torch.randint(0, e.model_cfg.vocab_size, (64,), generator=g).tolist()
    prompts = [prefix + torch.randint(0, e.model_cfg.vocab_size, (n,), generator=g).tolist() for n in (5, 40, 130)]
    outs = e.generate(prompts, SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True))
    assert calls["stream"] >= 1 and calls["gemm"] >= 1, calls
    if graphs:
        assert not e.runner.graphs.disabled and e.runner.graphs.stats["replays"] >= 1
    _assert_greedy_gap(e.model, prompts, outs, 0.25)
