"""fp8 activations on the fp8 expert tiles (csrc/grouped_tile_gemm_f8.hip): ``ops.grouped_tiles_glu`` /
``ops.grouped_tiles_combine`` with ``act="fp8"`` on the e4m3 x e4m3 MFMA against the float64 product of the same
quantised operands, bit-equality with the dense fp8 kernel, and the ``expert_tiles_only`` + ``act_dtype="fp8_experts"``
engine mode.

Cases, routings and tolerances are tests/test_grouped_tiles.py's (GLU atol 0.03 / rtol 0.02, combine 0.02 / 0.01): both
sides use the exact quantised operands, so only accumulation order and bf16 rounding remain. Activations are
tests/test_tile_gemm_f8.py's ``_acts`` (a power of two per row, the binade-edge rows and the zero row) and the experts
differ per expert, so a wrong gathered row, a wrong gathered exponent or a global-for-local expert index fails."""
import pytest
import torch
from test_grouped_tiles import CASES, EDGE_LENS, _routing, _tiles
from test_tile_gemm_f8 import _acts
from test_weight_fp8_moe import _cpu_routing
from test_weight_mxfp4 import _assert_greedy_gap, _close, _cpu_cfg
from test_weight_mxfp4_moe import _experts

from kafka_llm_service_amd import ops
from kafka_llm_service_amd.ops import reference as ref

ENVS = ("KAFKA_WEIGHT_DTYPE", "KAFKA_DECODE_GEMM", "KAFKA_TILE_PREFILL", "KAFKA_ACT_DTYPE", "KAFKA_EXPERT_TILES_ONLY")


def _deq64(x):
    xq, xe = ref.fp8_quant(x)
    return torch.ldexp(xq.view(torch.float8_e4m3fn).double(), xe[:, None])


# GLU K = 1280: twenty stages, the five-stage ring ends on its boundary (256 never wraps, 512 and 768 end mid-ring)
@pytest.mark.gpu
@pytest.mark.parametrize("kind,Kg,F,Nc,Kc", CASES + [("edges", 1280, 96, 64, 256)])
def test_grouped_tiles_fp8_vs_float64(cuda, kind, Kg, F, Nc, Kc):
    logits, e_lo, e_n = _routing(kind)
    T = logits.shape[0]
    r = ops.moe_route(logits.to(cuda), 2)
    rc = _cpu_routing(r)
    eo = rc.expert_off.tolist()
    lo, hi = eo[e_lo], eo[e_lo + e_n]
    if kind == "edges":
        assert [eo[e_lo + i + 1] - eo[e_lo + i] for i in range(e_n)] == EDGE_LENS
    x = _acts(T, Kg, seed=Kg)
    wt, st, deq = _tiles("fp8", e_n, 2 * F, Kg, True)
    y = ops.grouped_tiles_glu(x.to(cuda), wt, r, e_lo=e_lo, scale=st, act="fp8")
    h = torch.zeros(2 * T, 2 * F, dtype=torch.float64)
    ref.grouped_gemm(_deq64(x), deq.double(), rc.perm_tok, rc.perm_w, rc.expert_off, e_lo, True, h, None)
    assert y.dtype == torch.bfloat16 and y[lo:hi].float().abs().max() > 0
    _close(y[lo:hi], ref.silu_mul(h[lo:hi]), atol=0.03, rtol=0.02, msg=f"glu {kind} K={Kg} F={F}")
    a = _acts(2 * T, Kc, seed=Kc + 1)
    wt, st, deq = _tiles("fp8", e_n, Nc, Kc, False)
    out = torch.zeros(T, Nc, device=cuda)
    ops.grouped_tiles_combine(a.to(cuda), wt, r, T, out, e_lo=e_lo, scale=st, act="fp8")
    want = torch.zeros(T, Nc, dtype=torch.float64)
    ref.grouped_gemm(_deq64(a), deq.double(), rc.perm_tok, rc.perm_w, rc.expert_off, e_lo, False, None, want)
    assert out.abs().max() > 0
    _close(out, want, atol=0.02, rtol=0.01, msg=f"combine {kind} N={Nc} K={Kc}")
    out2 = torch.zeros(T, Nc, device=cuda)  # an (aq, ae) pair is the same call
    ops.grouped_tiles_combine(ops.fp8_act_quant(a.to(cuda)), wt, r, T, out2, e_lo=e_lo, scale=st, act="fp8")
    _close(out2, want, atol=0.02, rtol=0.01, msg=f"combine of a pair {kind} N={Nc} K={Kc}")


@pytest.mark.gpu
@pytest.mark.parametrize("M", [257, 515])
def test_grouped_tiles_fp8_bit_equals_dense_kernel(cuda, M):
    """One expert, identity routing: the same MFMAs over ascending K per accumulator, the same scaling and epilogue."""
    N, K = 320, 768
    wt, st = ops.tile_experts_as(_experts(1, N, K, seed=N + K, std=K ** -0.5, device=cuda), "fp8", True)
    x = _acts(M, K, seed=M).to(cuda)
    r = ops.moe_route(torch.zeros(M, 1, dtype=torch.bfloat16, device=cuda), 1)
    assert r.perm_tok.tolist() == list(range(M)) and r.expert_off.tolist()[:2] == [0, M]
    y = ops.grouped_tiles_glu(x, wt, r, scale=st, act="fp8")
    dense = ops.linear_tiles(x, wt[0], glu=True, scale=st[0], act="fp8")
    assert y.float().abs().max() > 0 and torch.equal(y, dense)


@pytest.mark.gpu
def test_grouped_tiles_fp8_refusals(cuda):
    e = ops._ext.load()
    T, E, K, N = 8, 2, 512, 128
    r = ops.moe_route(torch.randn(T, E).to(torch.bfloat16).to(cuda), 2)
    x = torch.zeros(T, K, device=cuda, dtype=torch.bfloat16)
    w = _experts(E, N, K, seed=3, device=cuda)
    for fmt in ("bf16", "mxfp4"):
        wt, st = ops.tile_experts_as(w, fmt, True)
        with pytest.raises(ValueError, match=fmt):
            ops.grouped_tiles_glu(x, wt, r, scale=st, act="fp8")
        with pytest.raises(ValueError, match=fmt):
            ops.grouped_tiles_combine(x, wt, r, T, torch.zeros(T, N, device=cuda), scale=st, act="fp8")
    w8, s8 = ops.tile_experts_as(w, "fp8", True)
    with pytest.raises(ValueError, match="quant_out"):
        ops.grouped_tiles_glu(x, w8, r, scale=s8, act="fp8", quant_out=True)
    u8 = dict(device=cuda, dtype=torch.uint8)
    xq, xe = torch.zeros(T, K, **u8), torch.zeros(T, device=cuda, dtype=torch.int32)
    y = torch.full((2 * T, N // 2), 7.0, device=cuda, dtype=torch.bfloat16)
    out = torch.full((T, N), 7.0, device=cuda)
    rt = (r.perm_tok, r.perm_w, r.expert_off, 0)
    for args in [(xq, xe[:T - 1], w8, s8, *rt, True, y, None),                                   # a short xe
                 (xq[:, :384].contiguous(), xe, w8[:, :, :12].contiguous(), s8, *rt, True, y, None),  # K % 256 != 0
                 (torch.zeros(T, K + 8, **u8)[:, :K], xe, w8, s8, *rt, True, y, None),           # ldxq % 16 != 0
                 (torch.zeros(2 * T, K + 8, **u8)[:, :K], xe.repeat(2), w8, s8, *rt, False, None, out)]:
        with pytest.raises(RuntimeError):
            e.grouped_tile_gemm_f8(*args)
    torch.cuda.synchronize()
    assert (y == 7.0).all() and (out == 7.0).all(), "a refused call wrote its output"


def _engine_run(monkeypatch, device, **kw):
    """A prompt of MOE_STREAM_MAX_T + 60 tokens and 9 greedy tokens on tiny-mixtral in fp8 expert tiles alone with fp8
    expert activations; returns (engine, prompts, outputs, the (rows, act) of every grouped_tiles_glu call)."""
    from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
    from kafka_llm_service_amd.engine.sequence import SamplingParams
    from kafka_llm_service_amd.models import moe

    for env in ENVS:
        monkeypatch.delenv(env, raising=False)
    calls, glu = [], ops.grouped_tiles_glu
    monkeypatch.setattr(ops, "grouped_tiles_glu", lambda x, *a, **k: (calls.append((x.shape[0], k.get("act", "bf16"))),
                                                                      glu(x, *a, **k))[1])
    eng = LLMEngine(EngineConfig(model="tiny-mixtral", device=device, weight_dtype="fp8", expert_tiles_only=True,
                                 act_dtype="fp8_experts", **kw))
    assert eng.model.act_dtype == "fp8_experts" and all(lw.w13 is None for lw in eng.model.layers)
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(0, eng.model_cfg.vocab_size, (moe.MOE_STREAM_MAX_T + 60,), generator=g).tolist()]
    outs = eng.generate(prompts, SamplingParams(temperature=0.0, max_tokens=9, ignore_eos=True))
    return eng, prompts, outs, calls


def test_expert_act_fp8_engine_cpu(monkeypatch):
    """The CPU path contains no kernel: the greedy gap it keeps is the format's (prompt rows see fp8 expert activations,
    decode rows bf16 ones). Measured on the reference path: 0.000 at each of the 9 tokens (the same model with bf16
    activations: at most 0.008); the bound is the sibling test's 0.25."""
    from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
    from kafka_llm_service_amd.models import moe

    eng, prompts, outs, calls = _engine_run(monkeypatch, "cpu", num_kv_blocks=256, max_model_len=2048)
    # every layer's expert call of the prompt step, and none of the decode steps (they stream with bf16 activations)
    assert calls == [(moe.MOE_STREAM_MAX_T + 60, "fp8")] * len(eng.model.layers)
    _assert_greedy_gap(eng.model, prompts, outs, 0.25)
    for kw in (dict(weight_dtype="fp8"), dict(model="tiny-mixtral", weight_dtype="fp8", tile_prefill=True),
               dict(model="tiny-mixtral", weight_dtype="fp8"),
               dict(model="tiny-mixtral", weight_dtype="bf16", expert_tiles_only=True, decode_gemm="stream"),
               dict(model="tiny-mixtral", weight_dtype="mxfp4", expert_tiles_only=True)):
        with pytest.raises(ValueError, match="act_dtype"):
            LLMEngine(EngineConfig(**_cpu_cfg(act_dtype="fp8_experts", **kw)))
    with pytest.raises(ValueError, match="fp8_experts"):  # the kernel-level tuple does not grow
        ops.linear_tiles(torch.zeros(1, 256), torch.zeros(2, 8, 64, 16, dtype=torch.uint8), act="fp8_experts")


@pytest.mark.gpu
def test_expert_act_fp8_engine_gpu(cuda, monkeypatch):
    from kafka_llm_service_amd.models import moe

    f8, gemm = [], ops._ext.load().grouped_tile_gemm_f8
    monkeypatch.setattr(ops._ext.load(), "grouped_tile_gemm_f8", lambda xq, *a: (f8.append(xq.shape[0]), gemm(xq, *a))[1])
    eng, prompts, outs, calls = _engine_run(monkeypatch, str(cuda), num_kv_blocks=1024, max_model_len=4096)
    T, L = moe.MOE_STREAM_MAX_T + 60, len(eng.model.layers)
    # two launches per layer for the prompt step (token rows, then one row per routed entry), none afterwards
    assert calls == [(T, "fp8")] * L and f8 == [T, 2 * T] * L
    _assert_greedy_gap(eng.model, prompts, outs, 0.25)
