"""MXFP8 activations on the MXFP4 expert tiles (csrc/grouped_tile_gemm_mx.hip): ``ops.grouped_tiles_glu`` /
``ops.grouped_tiles_combine`` with ``act="mxfp8"`` on the scaled fp8 x fp4 MFMA against the float64 product of the same
quantised operands, the quantising GLU epilogue (``quant_out``) against ``reference.mxfp8_quant`` bit for bit, bit-equality
with the dense scaled kernel, and the ``expert_tiles_only`` + ``act_dtype="mxfp8"`` engine mode.

Cases, routings and tolerances are tests/test_grouped_tiles.py's (GLU atol 0.03 / rtol 0.02, combine 0.02 / 0.01): both
sides use the exact quantised operands, so only accumulation order and bf16 rounding remain. Activations are
tests/test_tile_gemm_mx.py's ``_acts`` (a power of two per (row, block), the zero and binade-edge blocks) and the experts
differ per expert, so a wrong exponent, a wrong gathered row or a global-for-local expert index fails."""
import pytest
import torch
from test_grouped_tiles import CASES, EDGE_LENS, _routing, _tiles
from test_tile_gemm_mx import _acts
from test_weight_fp8_moe import _cpu_routing
from test_weight_mxfp4 import _assert_greedy_gap, _close, _cpu_cfg
from test_weight_mxfp4_moe import _experts

from kafka_llm_service_amd import ops
from kafka_llm_service_amd.ops import reference as ref


def _routed(cuda, kind):
    """(routing on the GPU, its CPU copy, T, e_lo, e_n, the local experts' entry range [lo, hi))"""
    logits, e_lo, e_n = _routing(kind)
    r = ops.moe_route(logits.to(cuda), 2)
    rc = _cpu_routing(r)
    eo = rc.expert_off.tolist()
    if kind == "edges":
        assert [eo[e_lo + i + 1] - eo[e_lo + i] for i in range(e_n)] == EDGE_LENS
    return r, rc, logits.shape[0], e_lo, e_n, eo[e_lo], eo[e_lo + e_n]


def _deq64(x):
    return ref.mxfp8_dequant(*ref.mxfp8_quant(x), dtype=torch.float64)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,Kg,F,Nc,Kc", CASES)
def test_grouped_tiles_mxfp8_vs_float64(cuda, kind, Kg, F, Nc, Kc):
    r, rc, T, e_lo, e_n, lo, hi = _routed(cuda, kind)
    x = _acts(T, Kg, seed=Kg)
    wt, st, deq = _tiles("mxfp4", e_n, 2 * F, Kg, True)
    y = ops.grouped_tiles_glu(x.to(cuda), wt, r, e_lo=e_lo, scale=st, act="mxfp8")
    h = torch.zeros(2 * T, 2 * F, dtype=torch.float64)
    ref.grouped_gemm(_deq64(x), deq.double(), rc.perm_tok, rc.perm_w, rc.expert_off, e_lo, True, h, None)
    assert y.dtype == torch.bfloat16 and y[lo:hi].float().abs().max() > 0
    _close(y[lo:hi], ref.silu_mul(h[lo:hi]), atol=0.03, rtol=0.02, msg=f"glu {kind} K={Kg} F={F}")
    a = _acts(2 * T, Kc, seed=Kc + 1)
    wt, st, deq = _tiles("mxfp4", e_n, Nc, Kc, False)
    out = torch.zeros(T, Nc, device=cuda)
    ops.grouped_tiles_combine(a.to(cuda), wt, r, T, out, e_lo=e_lo, scale=st, act="mxfp8")
    want = torch.zeros(T, Nc, dtype=torch.float64)
    ref.grouped_gemm(_deq64(a), deq.double(), rc.perm_tok, rc.perm_w, rc.expert_off, e_lo, False, None, want)
    assert out.abs().max() > 0
    _close(out, want, atol=0.02, rtol=0.01, msg=f"combine {kind} N={Nc} K={Kc}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind,Kg,F,Nc,Kc", CASES)
def test_grouped_tiles_quant_out_bit_for_bit(cuda, kind, Kg, F, Nc, Kc):
    r, rc, T, e_lo, e_n, lo, hi = _routed(cuda, kind)
    x = _acts(T, Kg, seed=Kg).to(cuda)
    wt, st, _ = _tiles("mxfp4", e_n, 2 * F, Kg, True)
    y = ops.grouped_tiles_glu(x, wt, r, e_lo=e_lo, scale=st, act="mxfp8")
    aq, ae = ops.grouped_tiles_glu(x, wt, r, e_lo=e_lo, scale=st, act="mxfp8", quant_out=True)
    assert aq.dtype == torch.uint8 and aq.shape == (2 * T, F) and ae.dtype == torch.float8_e8m0fnu
    wq, we = ref.mxfp8_quant(y[lo:hi].cpu())
    assert wq.any() and torch.equal(aq[lo:hi].cpu(), wq)
    assert ae.shape == (2 * T, F // 32) and torch.equal(ae.view(torch.uint8)[lo:hi].cpu(), we.view(torch.uint8))
    if F % 256 == 0:  # the pair feeds the down half as the bf16 tensor does
        wt, st, _ = _tiles("mxfp4", e_n, Nc, F, False)
        o_pair, o_bf16 = torch.zeros(T, Nc, device=cuda), torch.zeros(T, Nc, device=cuda)
        ops.grouped_tiles_combine((aq, ae), wt, r, T, o_pair, e_lo=e_lo, scale=st, act="mxfp8")
        y[:lo].zero_()  # (rows of the other ranks' experts are undefined: the combine does not read them)
        y[hi:].zero_()
        ops.grouped_tiles_combine(y, wt, r, T, o_bf16, e_lo=e_lo, scale=st, act="mxfp8")
        assert o_pair.abs().max() > 0 and torch.equal(o_pair, o_bf16)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [257, 515])
def test_grouped_tiles_mxfp8_bit_equals_dense_kernel(cuda, M):
    """One expert, identity routing: the same scaled MFMAs over ascending K per accumulator, the same GLU epilogue."""
    N, K = 320, 768
    wt, st = ops.tile_experts_as(_experts(1, N, K, seed=N + K, std=K ** -0.5, device=cuda), "mxfp4", True)
    x = _acts(M, K, seed=M).to(cuda)
    r = ops.moe_route(torch.zeros(M, 1, dtype=torch.bfloat16, device=cuda), 1)
    assert r.perm_tok.tolist() == list(range(M)) and r.expert_off.tolist()[:2] == [0, M]
    y = ops.grouped_tiles_glu(x, wt, r, scale=st, act="mxfp8")
    dense = ops.linear_tiles(x, wt[0], glu=True, scale=st[0], act="mxfp8")
    assert y.float().abs().max() > 0 and torch.equal(y, dense)


@pytest.mark.gpu
def test_grouped_tiles_mxfp8_refusals(cuda):
    e = ops._ext.load()
    T, E, K, N = 8, 2, 512, 128
    r = ops.moe_route(torch.randn(T, E).to(torch.bfloat16).to(cuda), 2)
    x = torch.zeros(T, K, device=cuda, dtype=torch.bfloat16)
    w = _experts(E, N, K, seed=3, device=cuda)
    for fmt in ("bf16", "fp8"):
        wt, st = ops.tile_experts_as(w, fmt, True)
        with pytest.raises(ValueError, match=fmt):
            ops.grouped_tiles_glu(x, wt, r, scale=st, act="mxfp8")
        with pytest.raises(ValueError, match=fmt):
            ops.grouped_tiles_combine(x, wt, r, T, torch.zeros(T, N, device=cuda), scale=st, act="mxfp8")
    w4, s4 = (t.view(torch.uint8) for t in ops.tile_experts_as(w, "mxfp4", True))
    u8 = dict(device=cuda, dtype=torch.uint8)
    xq, xe = torch.zeros(T, K, **u8), torch.full((T, K // 32), 127, **u8)
    y = torch.full((2 * T, N // 2), 7.0, device=cuda, dtype=torch.bfloat16)
    aq, ae = torch.full((2 * T, N // 2), 7, **u8), torch.full((2 * T, N // 64), 7, **u8)
    rt = (r.perm_tok, r.perm_w, r.expert_off, 0, True)
    for args in [(xq, xe[:, :8].contiguous(), w4, s4, *rt, y, None, None, None),            # a short xe
                 (xq[:, :384].contiguous(), xe[:, :12].contiguous(), w4[:, :, :6].contiguous(),
                  s4[:, :, :6].contiguous(), *rt, y, None, None, None),                      # K % 256 != 0
                 (torch.zeros(T, K + 8, **u8)[:, :K], xe, w4, s4, *rt, y, None, None, None),  # ldxq % 16 != 0
                 (xq, xe, w4, s4, *rt, y, aq, ae, None),                                     # quant_out and a bf16 y
                 (xq, xe, w4, s4, *rt, None, y, ae, None)]:                                  # a bf16 y as aq
        with pytest.raises(RuntimeError):
            e.grouped_tile_gemm_mx(*args)
    torch.cuda.synchronize()
    assert (y == 7.0).all() and (aq == 7).all() and (ae == 7).all(), "a refused call wrote its output"


def _engine_run(monkeypatch, device, **kw):
    """A prompt of MOE_STREAM_MAX_T + 60 tokens and 9 greedy tokens on tiny-mixtral in MXFP4 expert tiles alone with MXFP8
    activations; returns (engine, prompts, outputs, the (rows, act) of every grouped_tiles_glu call)."""
    from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
    from kafka_llm_service_amd.engine.sequence import SamplingParams
    from kafka_llm_service_amd.models import moe

    for env in ("KAFKA_WEIGHT_DTYPE", "KAFKA_DECODE_GEMM", "KAFKA_TILE_PREFILL", "KAFKA_ACT_DTYPE",
                "KAFKA_EXPERT_TILES_ONLY"):
        monkeypatch.delenv(env, raising=False)
    calls, glu = [], ops.grouped_tiles_glu
    monkeypatch.setattr(ops, "grouped_tiles_glu", lambda x, *a, **k: (calls.append((x.shape[0], k.get("act", "bf16"))),
                                                                      glu(x, *a, **k))[1])
    eng = LLMEngine(EngineConfig(model="tiny-mixtral", device=device, weight_dtype="mxfp4", expert_tiles_only=True,
                                 act_dtype="mxfp8", **kw))
    assert eng.model.act_dtype == "mxfp8" and all(lw.w13 is None for lw in eng.model.layers)
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(0, eng.model_cfg.vocab_size, (moe.MOE_STREAM_MAX_T + 60,), generator=g).tolist()]
    outs = eng.generate(prompts, SamplingParams(temperature=0.0, max_tokens=9, ignore_eos=True))
    return eng, prompts, outs, calls


def test_expert_act_mxfp8_engine_cpu(monkeypatch):
    from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
    from kafka_llm_service_amd.models import moe

    eng, prompts, outs, calls = _engine_run(monkeypatch, "cpu", num_kv_blocks=256, max_model_len=2048)
    # every layer's expert call of the prompt step, and none of the decode steps (they stream with bf16 activations)
    assert calls == [(moe.MOE_STREAM_MAX_T + 60, "mxfp8")] * len(eng.model.layers)
    _assert_greedy_gap(eng.model, prompts, outs, 0.25)
    for kw in (dict(weight_dtype="mxfp4"), dict(model="tiny-mixtral", weight_dtype="mxfp4"),
               dict(model="tiny-mixtral", weight_dtype="fp8", expert_tiles_only=True),
               dict(model="tiny-mixtral", weight_dtype="bf16", expert_tiles_only=True, decode_gemm="stream")):
        with pytest.raises(ValueError, match="act_dtype"):
            LLMEngine(EngineConfig(**_cpu_cfg(act_dtype="mxfp8", **kw)))
    with pytest.raises(ValueError):  # the two flags still exclude each other
        LLMEngine(EngineConfig(**_cpu_cfg(model="tiny-mixtral", weight_dtype="mxfp4", expert_tiles_only=True,
                                          tile_prefill=True, act_dtype="mxfp8")))


@pytest.mark.gpu
def test_expert_act_mxfp8_engine_gpu(cuda, monkeypatch):
    from kafka_llm_service_amd.models import moe

    mx, gemm = [], ops._ext.load().grouped_tile_gemm_mx
    monkeypatch.setattr(ops._ext.load(), "grouped_tile_gemm_mx", lambda xq, *a: (mx.append(xq.shape[0]), gemm(xq, *a))[1])
    eng, prompts, outs, calls = _engine_run(monkeypatch, str(cuda), num_kv_blocks=1024, max_model_len=4096)
    T, L = moe.MOE_STREAM_MAX_T + 60, len(eng.model.layers)
    # two launches per layer for the prompt step (token rows, then one row per routed entry), none afterwards
    assert calls == [(T, "mxfp8")] * L and mx == [T, 2 * T] * L
    _assert_greedy_gap(eng.model, prompts, outs, 0.25)
