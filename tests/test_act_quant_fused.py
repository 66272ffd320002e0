"""Quantised activations produced where they are made: the quantising RMSNorm (csrc/norm_act.hip rmsnorm_quant_kernel),
the MXFP8-emitting GLU epilogue of the dense scaled GEMM (tile_epilogue.h EPI_GLU_MX), ``linear_tiles(x_scale=,
quant_out=)`` and the engine path behind ``models.llama.FUSE_ACT_QUANT``. The fused kernels must give the bytes of the
unfused chain (bf16 tensor, then ``ops.mxfp8_quant`` / ``ops.fp8_act_quant``) bit for bit."""
import functools

import pytest
import torch
from test_tile_gemm_mx import _acts
from test_weight_mxfp4 import _cpu_cfg, _weight

from kafka_llm_service_amd import ops
from kafka_llm_service_amd.models import llama
from kafka_llm_service_amd.ops import reference as ref

QUANT = {"mxfp8": ops.mxfp8_quant, "fp8": ops.fp8_act_quant}
TILES = ops.ACT_TILES
# (T, d): the 256-thread one-vector path, the 512-thread path, NV = 4 with a dead last vector group, NV = 4 full
NORM_CASES = pytest.mark.parametrize("q,T,d,kind", [(q, T, d, kind) for q in ("mxfp8", "fp8") for kind in ("plain", "bf16", "slab")
                                                    for T, d in [(1, 256), (37, 4096), (5, 6144), (3, 8192)]])
ENVS = ("KAFKA_WEIGHT_DTYPE", "KAFKA_DECODE_GEMM", "KAFKA_TILE_PREFILL", "KAFKA_ACT_DTYPE", "KAFKA_EXPERT_TILES_ONLY")


@functools.lru_cache(maxsize=None)
def _norm_case(q, T, d, kind):
    """Both chains on the GPU, results on the CPU: (fused xq, xe, residual), (unfused xq, xe, residual), the float64
    norm of the float64 sum, all with eps = 0. The rows are ``_acts`` ones (a power of two per 32-column block); row 0 is
    built so that its mean square is exactly 64: the scale is 2^-3 and its blocks 0..3 reach the quantiser as an
    all-zero block and amax = 7 = 448 * 2^-6 exactly, the next bf16 above it and the next below it (w is 1 there)."""
    dev = torch.device("cuda:0")
    total = _acts(T, d, seed=d + T).float()
    part = total * 0.25  # (delta and residual of one sign: the fp32 add loses nothing to cancellation)
    row = torch.full((d,), 8.0)
    row[:32], row[37], row[73], row[98] = 0, 56.0, -56.25, 55.75
    row[128:131] = torch.tensor([7.75, 1.5, 1.25])
    row[131:131 + 148 - 38] = 0  # 64 d = 9408.125 (the three edges) + 63.875 + 64 (d - 148)
    total[0], part[0] = row, 0
    w = torch.cat([torch.ones(128), torch.randn(d - 128, generator=torch.Generator().manual_seed(d)) + 1]).bfloat16()
    if kind == "plain":
        delta, resid = total.bfloat16(), None
    elif kind == "bf16":
        delta, resid = torch.zeros(T, d + 8, dtype=torch.bfloat16)[:, :d].copy_(part), (total - part).bfloat16()
    else:  # two fp32 slabs
        delta, resid = torch.stack([part * 0.75, part * 0.25]), (total - part).bfloat16()
    s64 = delta.double() if resid is None else (delta.sum(0) if kind == "slab" else delta).double() + resid.double()
    want = s64 * torch.rsqrt(s64.pow(2).mean(-1, keepdim=True)) * w.double()
    dg = torch.zeros(delta.shape[:-1] + (d + 8,), dtype=delta.dtype, device=dev)[..., :d].copy_(delta) \
        if kind == "bf16" else delta.to(dev)
    wg = w.to(dev)
    if resid is None:
        fused = ops.rmsnorm(dg, wg, 0.0, quant=q) + (None,)
        plain = QUANT[q](ops.rmsnorm(dg, wg, 0.0)) + (None,)
    else:
        r1, r2 = resid.to(dev), resid.to(dev)
        fused = ops.fused_add_rmsnorm(dg, r1, wg, 0.0, quant=q) + (r1,)
        plain = QUANT[q](ops.fused_add_rmsnorm(dg, r2, wg, 0.0)) + (r2,)
    cpu = lambda ts: tuple(None if t is None else t.cpu() for t in ts)
    return cpu(fused), cpu(plain), want


@pytest.mark.gpu
@NORM_CASES
def test_quant_norm_equals_unfused_chain(cuda, q, T, d, kind):
    fused, plain, _ = _norm_case(q, T, d, kind)
    assert fused[1].dtype == plain[1].dtype and fused[0].shape == (T, d)
    if q == "mxfp8":  # the edges of row 0 survived the norm
        assert fused[1].view(torch.uint8)[0, :4].tolist() == [127, 122, 122, 121]
    for a, b, what in zip(fused, plain, ("xq", "xe", "residual")):
        if a is not None:
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"{what} differs from the unfused chain"


@pytest.mark.gpu
@NORM_CASES
def test_quant_norm_vs_float64(cuda, q, T, d, kind):
    """|err| <= (2^-4 + 2^-8) |ref| + 2^(e - 10): e4m3's half-ulp relative rounding, the two bf16 roundings (sum and
    output), and half a subnormal step of the grid scaled by the stored exponent e of the block (mxfp8) or row (fp8)."""
    (xq, xe, _), _, want = _norm_case(q, T, d, kind)
    if q == "mxfp8":
        got = ref.mxfp8_dequant(xq, xe, torch.float64)
        e = (xe.view(torch.uint8).double() - 127).repeat_interleave(32, dim=1)
    else:
        e = xe.double()[:, None]
        got = torch.ldexp(ref.fp8_act_order(xq).view(torch.float8_e4m3fn).double(), e)
    excess = (got - want).abs() - ((2.0 ** -4 + 2.0 ** -8) * want.abs() + torch.exp2(e - 10))
    assert excess.max() <= 0, f"{int((excess > 0).sum())} elements past the bound, worst by {excess.max():.3e}"


@functools.lru_cache(maxsize=None)
def _tiles(act, N, K, glu):
    return ops.tile_weight_as(_weight(N, K, seed=N + K, device="cuda:0"), TILES[act], glu)


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,glu,ms", [(257, 320, 768, False, 1), (515, 512, 2048, False, 8), (255, 320, 768, True, 1)])
@pytest.mark.parametrize("act", ["mxfp8", "fp8"])
def test_linear_tiles_x_scale(cuda, act, M, N, K, glu, ms):
    wt, s = _tiles(act, N, K, glu)
    x = _acts(M, K, seed=M).to(cuda)
    xq, xe = QUANT[act](x)
    y = ops.linear_tiles(xq, wt, max_splits=ms, glu=glu, scale=s, act=act, x_scale=xe)
    assert ops.is_slab(y) == (ms > 1) and torch.equal(y, ops.linear_tiles(x, wt, max_splits=ms, glu=glu, scale=s, act=act))


@pytest.mark.gpu
def test_fused_quant_refusals(cuda):
    e = ops._ext.load()
    x = _acts(40, 512).to(cuda)
    (w4, s4), (w8, s8) = _tiles("mxfp8", 128, 512, True), _tiles("fp8", 128, 512, True)
    xq, xe = ops.mxfp8_quant(x)
    for kw in (dict(x=xq, act="mxfp8", x_scale=xe[:, :8]), dict(x=xq, act="bf16", x_scale=xe),
               dict(x=x, act="mxfp8", quant_out=True), dict(x=x, wt=w8, scale=s8, act="fp8", glu=True, quant_out=True),
               dict(x=x, act="mxfp8", x_scale=xe)):  # (bf16 x with exponents)
        with pytest.raises(ValueError, match="x_scale|quant_out"):
            ops.linear_tiles(**{"wt": w4, "scale": s4, **kw})
    with pytest.raises(ValueError, match="out"):
        ops.rmsnorm(x, x[0], 1e-5, out=torch.empty_like(x), quant="fp8")
    u8 = dict(device=cuda, dtype=torch.uint8)
    aq, ae, y = torch.full((40, 64), 7, **u8), torch.full((40, 2), 7, **u8), torch.full((40, 64), 7.0, device=cuda).bfloat16()
    nq, ne, ni = torch.full((40, 512), 7, **u8), torch.full((40, 16), 7, **u8), torch.full((40,), 7, device=cuda).int()
    mx = (xq, xe.view(torch.uint8), w4.view(torch.uint8), s4.view(torch.uint8))
    for args in [mx + (None, None, 1, False, aq, ae),       # the quantised output without glu
                 mx + (y, None, 1, True, aq, ae),            # both outputs
                 mx + (None, None, 1, True, aq, None),       # half a pair
                 mx + (None, None, 1, True, aq, ae[:, :1].contiguous())]:
        with pytest.raises(RuntimeError):
            e.tile_gemm_mx(*args)
    for args in [(x[:, :384], None, x[0, :384].contiguous(), 1e-5, nq[:, :384].contiguous(), ne[:, :12].contiguous(), 1),
                 (x, None, x[0], 1e-5, nq, ni, 1), (x, None, x[0], 1e-5, nq, ne, 2), (x, None, x[0], 1e-5, nq, ne, 3),
                 (torch.zeros(2, 40, 512, device=cuda), None, x[0], 1e-5, nq, ne, 1)]:  # a slab without a residual
        with pytest.raises(RuntimeError):
            e.rmsnorm_quant(*args)
    torch.cuda.synchronize()
    assert all((t == 7).all() for t in (aq, ae, y, nq, ne, ni)), "a refused call wrote its output"


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(1, 64, 256), (255, 320, 768), (515, 512, 768)])
def test_quant_out_equals_quantised_glu(cuda, M, N, K):
    wt, s = _tiles("mxfp8", N, K, True)
    x, F = _acts(M, K, seed=N).to(cuda), N // 2
    y = ops.linear_tiles(x, wt, glu=True, scale=s, act="mxfp8")
    wq, we = ref.mxfp8_quant(y.cpu())
    aq, ae = ops.linear_tiles(x, wt, glu=True, scale=s, act="mxfp8", quant_out=True)
    assert ae.dtype == torch.float8_e8m0fnu and y.float().abs().max() > 0
    assert torch.equal(aq.cpu(), wq) and torch.equal(ae.view(torch.uint8).cpu(), we.view(torch.uint8))
    # rows past M: the outputs are the heads of sentinel-filled buffers whose tails the kernel must leave alone
    bq, be = (torch.full(((M + 3) * n,), 7, device=cuda, dtype=torch.uint8) for n in (F, F // 32))
    xq, xe = ops.mxfp8_quant(x)
    ops._ext.load().tile_gemm_mx(xq, xe.view(torch.uint8), wt.view(torch.uint8), s.view(torch.uint8), None, None, 1, True,
                                 bq[:M * F].view(M, F), be[:M * F // 32].view(M, F // 32))
    assert torch.equal(bq[:M * F].view(M, F), aq) and (bq[M * F:] == 7).all() and (be[M * F // 32:] == 7).all()
    if F % 256 == 0:  # the pair feeds down as it lies
        wd, sd = _tiles("mxfp8", 320, F, False)
        assert torch.equal(ops.linear_tiles(aq, wd, scale=sd, act="mxfp8", x_scale=ae),
                           ops.linear_tiles(y, wd, scale=sd, act="mxfp8"))


def _generate(monkeypatch, fuse, count, **kw):
    """(tokens, the first step's logits, what ``count`` recorded) of a 333-token prompt and a few greedy steps."""
    from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
    from kafka_llm_service_amd.engine.sequence import SamplingParams

    for env in ENVS:
        monkeypatch.delenv(env, raising=False)
    monkeypatch.setattr(llama, "FUSE_ACT_QUANT", fuse)
    eng = LLMEngine(EngineConfig(**kw))
    seen, sample = [], eng.runner.sample_device
    eng.runner.sample_device = lambda logits, sp: (seen.append(logits.float().cpu()), sample(logits, sp))[1]
    rec = count()
    prompts = [torch.randint(0, 5000, (333,), generator=torch.Generator().manual_seed(3)).tolist()]
    outs = eng.generate(prompts, SamplingParams(temperature=0.0, max_tokens=4, ignore_eos=True))
    return outs, seen[0], rec, len(eng.model.layers)


@pytest.mark.parametrize("act", ["mxfp8", "fp8"])
def test_fused_quant_engine_cpu(monkeypatch, act):
    """Routing through the reference paths: which ``linear_tiles`` calls take quantised rows / emit them."""
    monkeypatch.setattr(ops, "STREAM_MAX_M", 128)

    def count():
        calls, tiles = [], ops.linear_tiles
        monkeypatch.setattr(ops, "linear_tiles", lambda x, *a, **k: (calls.append(
            (x.shape[0], k.get("act"), "x_scale" in k, bool(k.get("quant_out")))), tiles(x, *a, **k))[1])
        return calls

    cfg = _cpu_cfg(weight_dtype=TILES[act], tile_prefill=True, act_dtype=act)
    on, logits_on, calls, L = _generate(monkeypatch, True, count, **cfg)
    mx = act == "mxfp8"
    layer = [(333, act, True, False), (333, act, False, False), (333, act, True, mx), (333, act, mx, False)]
    assert [c for c in calls if c[1] == act] == layer * L
    monkeypatch.undo()
    monkeypatch.setattr(ops, "STREAM_MAX_M", 128)
    off, logits_off, calls, L = _generate(monkeypatch, False, count, **cfg)
    assert [c for c in calls if c[1] == act] == [(333, act, False, False)] * (4 * L)
    assert on == off and torch.equal(logits_on, logits_off)


@pytest.mark.gpu
@pytest.mark.parametrize("act", ["mxfp8", "fp8"])
def test_fused_quant_engine_gpu(cuda, monkeypatch, act):
    """The stand-alone quantiser runs for o alone (and for down under fp8); tokens and logits do not move."""
    e = ops._ext.load()

    def count():
        n, quant = [], getattr(e, "act_quant_" + act)
        monkeypatch.setattr(e, "act_quant_" + act, lambda *a: (n.append(a[0].shape[0]), quant(*a))[1])
        return n

    cfg = dict(model="small-llama", device=str(cuda), num_kv_blocks=1024, max_model_len=4096, weight_dtype=TILES[act],
               tile_prefill=True, act_dtype=act)
    on, logits_on, n, L = _generate(monkeypatch, True, count, **cfg)
    assert n == [333] * ((1 if act == "mxfp8" else 2) * L)
    monkeypatch.undo()
    off, logits_off, n, L = _generate(monkeypatch, False, count, **cfg)
    assert n == [333] * (4 * L)
    assert on == off and torch.equal(logits_on, logits_off)
