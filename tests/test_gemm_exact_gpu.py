"""Exact integer probes of the GEMM family: inputs whose fp32 result is the same in ANY summation order, compared with
``torch.equal`` instead of a tolerance, so one dropped, doubled or misplaced (n, k) term fails the test.

Premise (asserted on the CPU by every builder before anything runs on the GPU): ``x`` holds small integers, the weights
sit on a grid their tile format stores bit for bit (``untile_weight_as(*tile_weight_as(w, fmt)) == w``), every term of
an output element y[m, n] is an integer multiple of that weight row's unit, and sum_k |x[m, k]| |w[n, k]| — which bounds
every partial sum in every order — stays below 2^22 units. fp32 then adds without rounding, the fp32 product equals the
fp64 one, and bf16 outputs are the RNE rounding of that exact sum. ``x`` carries census rows (all ones:
y[m, n] = sum_k w[n, k], every term of a weight row counted once) and needle rows (one-hot: y[m, n] = w[n, k_m]) at
k = 0, K - 1, K/S - 1, K/S and on each side of 16-, 32-, 64-, 128- and 256-column boundaries.

Per kernel path: what a failure means, the unit and the bit budget of the sums.

* Streaming GEMM (``linear_stream``, ``ext.wstream_gemm_cfg``; bf16, fp8, MXFP4). Split s covers K[s K/S, (s+1) K/S)
  (``k0 = blockIdx.y * ks``), so every fp32 slab is compared on its own: a wave skipping the last k-step of its chunk, a
  split starting a tile early or late, a lane reading its neighbour's 8 columns, a row tile reading row M (census in the
  last row; rows >= M of an over-allocated NaN output must stay NaN), a row or block scale taken from the neighbour
  (adjacent rows / blocks differ in scale at least half the time), gate | up slab order of GLU tiles. Units: bf16
  weights are integers in [-8, 8] (unit 1, sums <= 2048 * 3 * 8 < 2^16); fp8 the same times 2^-3..2^3 per row (unit
  2^r of the row, same 16 bits); MXFP4 e2m1 values times 2^-2..2^2 per block and 2^-3..2^3 per row (unit 2^(r - 3) of
  the row, sums <= 2048 * 3 * 6 * 2^2 / 2^-1 units < 2^19). ``slab_reduce`` of the slabs is the bf16 rounding of the
  exact sum: a slab added twice with another omitted shows.
* ``linear_res`` (FIN_RES). x, w in {-1, 0, 1}, residual integers in [-8, 8], ``nw`` a power of two per column: the new
  residual is an integer of magnitude <= 256 (asserted), exact in bf16, ``xn`` an exact power-of-two multiple, and
  ``ss_out`` an integer sum of squares <= 128 * 256^2 = 2^23. Every case runs twice on the same scratch and tickets
  with other inputs: a stale ticket or slab of the first run shows in the second.
* ``linear_qkv_rope`` (FIN_ROPE) and ``rope_kv_write``. A cos/sin table of quarter turns ((1, 0), (0, 1), (-1, 0),
  (0, -1), varying per position and per rotation pair) makes RoPE a signed permutation; values are integers of magnitude
  <= 256. q, every written cache entry and every unwritten cache element (sentinel) are compared. The fp8 KV writer
  gets integers in [-15, 15] times a power of two per token, which stay on the e4m3 grid: data and exponent bytes equal
  ``ref.rope_kv_write`` with no differing byte.
* Skinny GEMM. Split s is the contiguous range K[s K/S, (s+1) K/S) (``k0 = blockIdx.y * ks`` in skinny_gemm.hip), so its
  slabs are compared slab by slab as the streaming kernel's, the GLU gate | up order included. Units as bf16 above.
* Grouped kernels. Hand-built routing (E = 8, k = 2; 0, 1, 63, 64, 65 and 129 entries per expert), routing weights in
  {1/4, 1/2, 1}: w * y is exact and a token's two contributions add exactly in either order of the atomics. Detects a
  row tile reading the neighbouring expert's rows, weights or scales of the global instead of the local expert, rows of
  tokens without a local expert written, gather rows outside the local range written. Units as the streaming GEMM's.
* The one tolerance left: the fused SwiGLU outputs (``linear_glu``, ``linear_glu_rs``, ``grouped_stream_glu``, the
  one-split GLU of ``linear_skinny``). silu is not exact, so these run needle rows only, gate weights integers in
  [1, 4], up weights in +-[1, 3], under the existing atol 0.03 + rtol 0.02 * max|ref|: the largest reference value is
  4 silu(4) / 4 * 3 = 11.8, so at most 0.27 is allowed, while any single wrong g or u moves an output by at least 0.7
  (the smallest step, |silu(2) - silu(1)| * 1 = 1.03 or silu(1) * 1 = 0.73).

Exactness of ``v_mfma_f32_32x32x16_bf16`` accumulation under this premise follows from fp32 arithmetic, and was
measured on the MI355X when this file was added: every equality below held at the full ranges above (no range had to
shrink), in all three formats.

The mutation check at the end (CPU only) perturbs the REFERENCE of every streaming case five ways — one (n, k) term
dropped, two adjacent 8-column lane groups swapped, a split boundary moved by 16, an MXFP4 block read with its
neighbour's exponent, slab 0 added twice with slab 1 omitted — and asserts that the comparison reports each."""
import functools
import zlib

import pytest
import torch

from kafka_llm_service_amd import ops
from kafka_llm_service_amd.ops import reference as ref
from kafka_llm_service_amd.ops._ext import ext

gpu = pytest.mark.gpu
BF16 = torch.bfloat16
FMTS = ("bf16", "fp8", "mxfp4")
NAN = float("nan")
E2M1 = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


# ------------------------------------------------------------------------------------------------------ input builders
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _randint(g, lo, hi, shape):
    """Integers in [lo, hi] as fp32."""
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _pow2(g, lo, hi, shape):
    """2^e, e uniform in [lo, hi], differing between neighbours along the last dim at least half the time."""
    e = _randint(g, lo, hi, shape)
    if e.shape[-1] > 1:
        assert (e[..., 1:] != e[..., :-1]).float().mean() >= 0.5
    return torch.exp2(e)


def _needle_cols(K, S):
    """Columns of the one-hot rows: both ends, both sides of the first split boundary and of a first and an interior
    16-, 32-, 64-, 128- and 256-column boundary."""
    ks = K // S
    cols = [0, K - 1, ks - 1, ks % K]
    for b in (256, 128, 64, 32, 16):
        j = max(1, K // b // 2)
        cols += [b - 1, b, j * b - 1, j * b]
    out = []
    for c in cols:
        if 0 <= c < K and c not in out:
            out.append(c)
    return out


def _x(M, K, S, amp=3, seed=0):
    """bf16 [M, K] of integers in [-amp, amp]: census rows (all ones) first and last, needle rows (one-hot) on the odd
    rows, random integers elsewhere. Returns (x, {needle row: column})."""
    x = _randint(_gen("x", M, K, seed), -amp, amp, (M, K))
    if M >= 2:
        x[M - 1] = 1.0
    if M >= 3:
        x[0] = 1.0
    needles = {}
    for i, c in enumerate(_needle_cols(K, S)):
        m = 2 * i + 1
        if m >= M - 1:
            break
        x[m] = 0.0
        x[m, c] = 1.0
        needles[m] = c
    assert torch.equal(x.to(BF16).float(), x)
    return x.to(BF16), needles


def _needle_x(M, K, S):
    """bf16 [M, K], every row one-hot (the fused-SwiGLU cases)."""
    cols = _needle_cols(K, S)
    x = torch.zeros(M, K)
    for m in range(M):
        x[m, cols[m % len(cols)]] = 1.0
    return x.to(BF16)


@functools.lru_cache(maxsize=None)
def _weight(fmt, N, K, kind="full", seed=0):
    """(w bf16 [N, K], unit fp32 [N]) on the grid of ``fmt``; every w[n, k] is an integer multiple of unit[n].
    kind "full": the ranges of the module docstring; "tern": {-1, 0, 1}; "glu": rows [0, N/2) integers in [1, 4] (gate),
    rows [N/2, N) in +-[1, 3] (up)."""
    g = _gen("w", fmt, N, K, kind, seed)
    unit = torch.ones(N)
    if kind == "tern":
        w = _randint(g, -1, 1, (N, K))
    elif kind == "glu":
        up = _randint(g, 1, 3, (N // 2, K)) * (2 * _randint(g, 0, 1, (N // 2, K)) - 1)
        w = torch.cat([_randint(g, 1, 4, (N // 2, K)), up])
    elif fmt == "mxfp4":
        v = E2M1[torch.randint(0, 8, (N, K // 32, 32), generator=g)] * (2 * _randint(g, 0, 1, (N, K // 32, 32)) - 1)
        # element 0 of every block +-4 or +-6: the OCP rule floor(log2(amax)) - 2 then picks e = 0 for the block
        v[..., 0] = (4 + 2 * _randint(g, 0, 1, (N, K // 32))) * (2 * _randint(g, 0, 1, (N, K // 32)) - 1)
        rows = _pow2(g, -3, 3, (1, N)).reshape(N, 1, 1)
        w = (v * _pow2(g, -2, 2, (N, K // 32))[..., None] * rows).reshape(N, K) + 0.0  # (no -0: the codes hold +0)
        unit = rows.reshape(N) * 2.0 ** -3  # e2m1 step 1/2 times the smallest block scale 2^-2
    else:
        w = _randint(g, -8, 8, (N, K))
        if fmt == "fp8":
            unit = _pow2(g, -3, 3, (1, N)).reshape(N)
            w = w * unit[:, None]
    assert torch.equal(w.to(BF16).float(), w)
    assert torch.equal(torch.round(w / unit[:, None]) * unit[:, None], w)
    return w.to(BF16), unit


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.uint8)


def _to(t, dev):
    """Move a tensor of any tile dtype (through its bytes: the packed dtypes have no copy kernels of their own)."""
    if t is None or t.dtype in (BF16, torch.float32, torch.uint8):
        return None if t is None else t.to(dev)
    return t.view(torch.uint8).to(dev).view(t.dtype)


@functools.lru_cache(maxsize=None)
def _tiles(fmt, N, K, kind, glu, dev, seed=0):
    """(tiles, scale or None) of ``_weight`` on ``dev``; the round trip through the format is asserted bit for bit."""
    w, _ = _weight(fmt, N, K, kind, seed)
    wt, sc = ops.tile_weight_as(w, fmt, glu)
    assert torch.equal(_bits(ops.untile_weight_as(wt, sc, glu)), _bits(w)), f"{fmt} tiles do not hold this grid"
    return _to(wt, dev), _to(sc, dev)


def _exact_slabs(x, w, unit, S):
    """(fp32 slabs [S, M, N] of x @ w^T over K[s K/S, (s+1) K/S), their fp32 sum), both exact: every term is a
    multiple of unit[n], sum |x| |w| (a bound on every partial sum in every order) is below 2^22 units, and the fp32
    product equals the fp64 one."""
    K = x.shape[1]
    ks = K // S
    xd, wd = x.double(), w.double()
    bound = ((xd.abs() @ wd.abs().t()) / unit.double()).max().item()
    assert bound < 2 ** 22, f"partial sums reach {bound} units"
    p64 = torch.stack([xd[:, s * ks:(s + 1) * ks] @ wd[:, s * ks:(s + 1) * ks].t() for s in range(S)])
    xf, wf = x.float(), w.float()
    p32 = torch.stack([xf[:, s * ks:(s + 1) * ks] @ wf[:, s * ks:(s + 1) * ks].t() for s in range(S)])
    assert torch.equal(p32.double(), p64)
    tot = p64.sum(0)
    assert torch.equal(tot.float().double(), tot) and torch.equal((xf @ wf.t()).double(), tot)
    return p32, tot.float()


def _diff(got, want):
    """None if the tensors are equal element for element, else where they differ."""
    got, want = got.detach().cpu(), want.detach().cpu()
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"{got.dtype} {tuple(got.shape)} against {want.dtype} {tuple(want.shape)}"
    if torch.equal(got, want):
        return None
    bad = (got != want).nonzero()
    i = tuple(bad[0].tolist())
    rows = sorted(set(bad[:, -2].tolist()))[:12] if got.dim() >= 2 else []
    return (f"{bad.shape[0]} of {got.numel()} elements differ, first at {i}: {got[i].item()} against {want[i].item()}; "
            f"rows {rows}")


def _same(got, want, msg):
    d = _diff(got, want)
    assert d is None, f"{msg}: {d}"


def _close(a, b, msg, atol=0.03, rtol=0.02):
    """The fused-SwiGLU paths' existing tolerance (module docstring)."""
    a, b = a.float().cpu(), b.float().cpu()
    err, tol = (a - b).abs().max().item(), atol + rtol * b.abs().max().item()
    assert b.abs().max().item() <= 11.8 and tol <= 0.27
    assert err <= tol, f"{msg}: max err {err} > {tol}"


def _quarter_table(max_pos, D):
    """cos | sin table [max_pos, D] of quarter turns only, varying per position and per rotation pair."""
    p, i = torch.arange(max_pos)[:, None], torch.arange(D // 2)[None, :]
    q = (7 * p + 5 * i + p * i // 3) % 4
    cs = torch.cat([torch.tensor([1.0, 0.0, -1.0, 0.0])[q], torch.tensor([0.0, 1.0, 0.0, -1.0])[q]], dim=-1)
    assert (q[1:] != q[:-1]).any(1).all() and (q[:, 1:] != q[:, :-1]).any(0).all()
    assert all((q == v).any() for v in range(4))
    return cs.contiguous()


def _slots(T, g, nb):
    """A permutation of the nb pages' slots for T tokens, every fifth token unwritten (-1)."""
    s = torch.randperm(nb * 16, generator=g)[:T]
    s[::5] = -1
    if T == 1:
        s[0] = 5
    return s


# ------------------------------------------------------------------------------------- 1. streaming GEMM, three formats
STREAM_SHAPES = [(128, 256), (128, 1024), (256, 2048), (384, 1024), (160, 1024)]
STREAM_M = [1, 32, 33, 64, 65, 96, 97, 128, 129, 192, 193, 256]
# (MXFP4 runs the same K: each is already the smallest at which the case's plan is reached, and leaves every split of the
# widest plan K / 8 >= 128 columns, two 64-column tiles; only (128, 256) has S <= 2, also 128 columns)


def _want_splits(M, N, K, max_splits):
    """The plan each case is meant to hit; None where the case does not depend on it."""
    if max_splits == 1:
        return 1
    if (N, K) == (128, 1024) or (N, K) == (384, 1024):
        return 4 if M <= 96 else 8
    if (N, K) == (256, 2048):
        return 8
    return None


def _stream_guarded(x, wt, scale, max_splits, glu, S):
    """``linear_stream``'s launch into an over-allocated NaN output: (result, the rows beyond M)."""
    M, N = x.shape[0], wt.shape[0] * 32
    f = ops.WEIGHT_FORMATS[wt.dtype]
    if S == 1:
        buf = torch.full((M + 40, N), NAN, dtype=BF16, device=x.device)
        y, p, tail = buf[:M], None, buf[M:]
    else:
        buf = torch.full((S * M * N + 40 * N,), NAN, device=x.device)
        y, p, tail = None, buf[:S * M * N].view(S, M, N), buf[S * M * N:]
    if f.raw:
        wt, scale = wt.view(torch.uint8), scale.view(torch.uint8)
    ext().wstream_gemm(x, wt, y, p, int(max_splits), True, bool(glu), scale, f.abi)
    return (y if S == 1 else p), tail


@gpu
@pytest.mark.parametrize("max_splits", [1, 8])
@pytest.mark.parametrize("M", STREAM_M)
@pytest.mark.parametrize("N,K", STREAM_SHAPES)
@pytest.mark.parametrize("fmt", FMTS)
def test_stream_exact(cuda, fmt, N, K, M, max_splits):
    """Every slab of ``linear_stream`` (the bf16 output for one split) equals the exact product; rows beyond M stay
    NaN; GLU tiles give the same slabs in gate | up order; ``slab_reduce`` gives the bf16 rounding of the exact sum."""
    plan = ops.stream_plan(M, N, K, max_splits)
    assert plan is not None
    S = plan[2]
    want = _want_splits(M, N, K, max_splits)
    if (N, K) == (128, 256) and max_splits > 1:
        assert S in (1, 2)
    elif want is not None:
        assert S == want, f"plan S={S}, the case is meant to run S={want}"
    assert plan[0] == (1 if M <= 32 else 2 if M <= 64 else 3 if M <= 96 else 4 if M <= 128 or M > 192 else 6)
    assert (M + 32 * plan[0] - 1) // (32 * plan[0]) == (2 if M > 192 else 1)
    w, unit = _weight(fmt, N, K)
    x, _ = _x(M, K, S)
    slabs, total = _exact_slabs(x, w, unit, S)
    expect = total.to(BF16) if S == 1 else slabs
    xg = x.to(cuda)
    for glu in ((False, True) if S > 1 and N % 64 == 0 else (False,)):
        wt, sc = _tiles(fmt, N, K, "full", glu, str(cuda))
        msg = f"{fmt} M={M} N={N} K={K} S={S} glu={glu}"
        out = ops.linear_stream(xg, wt, max_splits, glu=glu, scale=sc)
        _same(out, expect, msg)
        out2, tail = _stream_guarded(xg, wt, sc, max_splits, glu, S)
        _same(out2, expect, msg + " (guarded)")
        assert bool(torch.isnan(tail).all()), msg + ": rows at and beyond M were written"
        if S > 1:
            _same(ops.slab_reduce(out), total.to(BF16), msg + " slab_reduce")


def _kw_pin(mt, kc, chunks):
    """kw / pin the engine's launcher picks (bindings.cpp wstream_kw_pin)."""
    return (2 if mt == 2 and kc == 256 and chunks >= 6 else 1), (1 if mt != 3 and chunks >= 3 else 0)


# (M, N, K, S) -> the launcher's own (mt, kc, kw, pin): every (kw, pin) pair it can produce — (1, 0), (1, 1), (2, 1) —
# on every row-tile count
CFG_CASES = [(32, 128, 1024, 4), (32, 128, 1024, 1), (64, 256, 2048, 1), (64, 256, 2048, 2), (33, 384, 1024, 4),
             (96, 128, 1024, 2), (128, 384, 1024, 8), (128, 128, 1024, 2), (129, 256, 2048, 8), (192, 128, 256, 1),
             (193, 128, 1024, 4), (256, 160, 1024, 1)]


def test_cfg_cases_cover_the_launcher():
    seen = set()
    for M, N, K, S in CFG_CASES:
        mt, kc, _ = ops.stream_plan(M, N, K, 8)
        assert K % (kc * S) == 0
        seen.add(_kw_pin(mt, kc, K // S // kc))
    assert seen == {(1, 0), (1, 1), (2, 1)}


@gpu
@pytest.mark.parametrize("M,N,K,S", CFG_CASES)
def test_stream_cfg_exact(cuda, M, N, K, S):
    """bf16 tiles through ``ext.wstream_gemm_cfg`` with the (mt, kc, kw, pin) the engine's launcher picks for the
    shape, at a split count of the test's choosing."""
    mt, kc, _ = ops.stream_plan(M, N, K, 8)
    kw, pin = _kw_pin(mt, kc, K // S // kc)
    w, unit = _weight("bf16", N, K)
    x, _ = _x(M, K, S)
    slabs, total = _exact_slabs(x, w, unit, S)
    wt, _ = _tiles("bf16", N, K, "full", False, str(cuda))
    if S == 1:
        buf = torch.full((M + 40, N), NAN, dtype=BF16, device=cuda)
        y, p, tail, expect = buf[:M], None, buf[M:], total.to(BF16)
    else:
        buf = torch.full((S * M * N + 40 * N,), NAN, device=cuda)
        y, p, tail, expect = None, buf[:S * M * N].view(S, M, N), buf[S * M * N:], slabs
    ext().wstream_gemm_cfg(x.to(cuda), wt, y, p, mt, kc, S, True, kw, pin)
    msg = f"cfg M={M} N={N} K={K} mt={mt} kc={kc} S={S} kw={kw} pin={pin}"
    _same(y if S == 1 else p, expect, msg)
    assert bool(torch.isnan(tail).all()), msg + ": rows at and beyond M were written"


# ---------------------------------------------------------------------------------------------- 2. fused SwiGLU outputs
def _glu_ref(x, w):
    return ref.silu_mul(x.float() @ w.float().t())


@gpu
@pytest.mark.parametrize("M", [1, 33, 64, 100, 128])
@pytest.mark.parametrize("fmt", FMTS)
def test_glu_needles(cuda, fmt, M):
    """``linear_glu`` (fused epilogue at one split, slabs + silu_mul otherwise) and, on bf16 tiles, ``linear_glu_rs``
    without row partials: one-hot rows, so out[m, n] = silu(gate[n, k_m]) * up[n, k_m]. Tolerance 0.03 + 0.02 * 11.8 <=
    0.27 against a smallest single-fault step of 0.7 (module docstring)."""
    N, K = 256, 1024
    w, _ = _weight(fmt, N, K, "glu")
    wt, sc = _tiles(fmt, N, K, "glu", True, str(cuda))
    for max_splits in (1, 8):
        S = ops.stream_plan(M, N, K, max_splits)[2]
        assert (S == 1) == (max_splits == 1)
        x = _needle_x(M, K, S)
        y_ref = _glu_ref(x, w)
        _close(ops.linear_glu(x.to(cuda), wt, max_splits, scale=sc), y_ref, f"linear_glu {fmt} M={M} S={S}")
        if fmt == "bf16" and max_splits == 1:
            _close(ops.linear_glu_rs(x.to(cuda), wt, None, 1e-5), y_ref, f"linear_glu_rs M={M}")


# ----------------------------------------------------------------------------------------------------- 3. linear_res
@gpu
@pytest.mark.parametrize("M", [1, 33, 64, 100, 128])
@pytest.mark.parametrize("N,K,max_splits", [(512, 1024, 8), (256, 256, 1)])
def test_linear_res_exact(cuda, M, N, K, max_splits):
    """FIN_RES: new residual, xn and the sums of squares, exactly; twice on the same scratch and ticket pool."""
    S = ops.stream_plan(M, N, K, max_splits)[2]
    assert (S == 1) == (max_splits == 1)
    wt, _ = _tiles("bf16", N, K, "tern", False, str(cuda))
    w, unit = _weight("bf16", N, K, "tern")
    for run in (0, 1):
        g = _gen("res", M, N, K, run)
        x, _ = _x(M, K, S, amp=1, seed=run)
        resid = _randint(g, -8, 8, (M, N))
        nw = _pow2(g, -2, 2, (N,))
        _, y = _exact_slabs(x, w, unit, S)
        s = resid + y
        assert s.abs().max().item() <= 256  # integers bf16 holds exactly
        ss = s.pow(2).view(M, N // 128, 128).sum(-1).t().contiguous()
        assert ss.max().item() <= 2 ** 23 and torch.equal(ss.double(), s.double().pow(2).view(M, N // 128, 128).sum(-1).t())
        r_g = resid.to(BF16).to(cuda)
        xn_g = torch.full((M, N), NAN, dtype=BF16, device=cuda)
        ss_g = torch.full((N // 128, M + 3), NAN, device=cuda)
        ops.linear_res(x.to(cuda), wt, r_g, nw.to(BF16).to(cuda), xn_g, ss_g, max_splits)
        msg = f"linear_res M={M} N={N} K={K} S={S} run {run}"
        _same(r_g, s.to(BF16), msg + " resid")
        _same(xn_g, (s * nw).to(BF16), msg + " xn")
        _same(ss_g[:, :M], ss, msg + " ss_out")
        assert bool(torch.isnan(ss_g[:, M:]).all()), msg + ": ss_out columns beyond M were written"
    assert ops.fin_errors(cuda) == 0


# ------------------------------------------------------------------------------------- 4. linear_qkv_rope, rope_kv_write
def _caches(nb, Hkv, D, kv_dtype, dev):
    """Sentinel-filled (k, v) caches: a value no case produces, so unwritten entries compare like written ones."""
    ks, vs, dt = ops.kv_cache_shapes(nb, Hkv, D, kv_dtype)
    fill = 0xA5 if kv_dtype == "fp8" else -777.0
    return torch.full(ks, fill, dtype=dt, device=dev), torch.full(vs, fill, dtype=dt, device=dev)


@gpu
@pytest.mark.parametrize("M", [1, 33, 64, 100, 128])
@pytest.mark.parametrize("Hq,Hkv,d", [(4, 1, 512), (8, 2, 1024)])
def test_linear_qkv_rope_exact(cuda, M, Hq, Hkv, d):
    """FIN_ROPE without row partials on a quarter-turn table: q, the written cache entries and every unwritten cache
    element, exactly."""
    N = (Hq + 2 * Hkv) * 128
    S = ops.stream_plan(M, N, d)[2]
    w, unit = _weight("bf16", N, d, "tern")
    wt, _ = _tiles("bf16", N, d, "tern", False, str(cuda))
    x, _ = _x(M, d, S, amp=1)
    _, y = _exact_slabs(x, w, unit, S)
    assert y.abs().max().item() <= 256
    g = _gen("qkv", M, Hq, d)
    cs = _quarter_table(64, 128)
    pos = torch.randint(0, 64, (M,), generator=g)
    nb = (M + 15) // 16 + 2
    slots = _slots(M, g, nb)
    q_ref = torch.empty(M, Hq, 128, dtype=BF16)
    k_ref, v_ref = _caches(nb, Hkv, 128, "bf16", "cpu")
    ops.linear_qkv_rope(x, ops.tile_weight(w), None, 1e-5, pos, cs, q_ref, k_ref, v_ref, slots, Hq, Hkv)
    written = int((slots >= 0).sum()) * Hkv * 128
    assert int((k_ref != -777.0).sum()) == written == int((v_ref != -777.0).sum())
    q = torch.full((M, Hq, 128), NAN, dtype=BF16, device=cuda)
    k, v = _caches(nb, Hkv, 128, "bf16", cuda)
    ops.linear_qkv_rope(x.to(cuda), wt, None, 1e-5, pos.to(cuda), cs.to(cuda), q, k, v, slots.to(cuda), Hq, Hkv)
    msg = f"linear_qkv_rope M={M} Hq={Hq} d={d} S={S}"
    _same(q, q_ref, msg + " q")
    _same(k, k_ref, msg + " k cache")
    _same(v, v_ref, msg + " v cache")
    assert ops.fin_errors(cuda) == 0


def _rope_input(T, W, S, g, fp8):
    """qkv [T, W] of exact values, as bf16 (S = 0) or as S fp32 slabs summing to it (integer parts)."""
    if fp8:  # integers in [-15, 15] (some tokens' largest 14, 7 or 3) times a power of two per token: on the e4m3 grid
        cap = torch.tensor([15, 14, 7, 15, 3])[torch.arange(T) % 5].float()[:, None]
        scale = torch.exp2(_randint(g, -3, 3, (T, 1)))
        v = torch.minimum(torch.maximum(_randint(g, -15, 15, (T, W)), -cap), cap)
        v[:, ::64] = cap  # every head's amax is the token's cap
    else:
        v, scale = _randint(g, -100, 100, (T, W)), torch.ones(T, 1)
    if S == 0:
        return (v * scale + 0.0).to(BF16)
    parts = _randint(g, -50, 50, (S, T, W))
    parts[S - 1] = v - parts[:S - 1].sum(0)
    p = parts * scale + 0.0
    assert torch.equal(p.sum(0), v * scale)
    return p


def _q_out(T, Hq, D, aligned, dev):
    """q_out [T, Hq, D] with 16-B aligned rows, or rows 8 B off (the launcher's two D = 128 variants)."""
    if aligned:
        return torch.full((T, Hq, D), NAN, dtype=BF16, device=dev)
    return torch.full((T, Hq * D + 4), NAN, dtype=BF16, device=dev)[:, :Hq * D].view(T, Hq, D)


@gpu
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("S", [0, 2, 4])
@pytest.mark.parametrize("Hq,Hkv", [(4, 1), (8, 2)])
@pytest.mark.parametrize("D", [128, 64])
def test_rope_kv_write_exact(cuda, D, Hq, Hkv, S, aligned):
    """Stand-alone RoPE + paged KV write on a quarter-turn table, bf16 caches: bf16 input or fp32 slabs, q rows 16-B
    aligned or not; q, written and unwritten cache elements, exactly."""
    T, W = 37, (Hq + 2 * Hkv) * D
    g = _gen("rope", D, Hq, S, aligned)
    qkv = _rope_input(T, W, S, g, fp8=False)
    cs = _quarter_table(64, D)
    pos = torch.randint(0, 64, (T,), generator=g)
    nb = 5
    slots = _slots(T, g, nb)
    q_ref = _q_out(T, Hq, D, aligned, "cpu")
    k_ref, v_ref = _caches(nb, Hkv, D, "bf16", "cpu")
    ops.rope_kv_write(qkv, pos, cs, q_ref, k_ref, v_ref, slots, Hq, Hkv)
    q = _q_out(T, Hq, D, aligned, cuda)
    assert (q.stride(0) % 8 == 0) == aligned
    k, v = _caches(nb, Hkv, D, "bf16", cuda)
    ops.rope_kv_write(qkv.to(cuda), pos.to(cuda), cs.to(cuda), q, k, v, slots.to(cuda), Hq, Hkv)
    msg = f"rope_kv_write D={D} Hq={Hq} S={S} aligned={aligned}"
    _same(q, q_ref, msg + " q")
    _same(k, k_ref, msg + " k cache")
    _same(v, v_ref, msg + " v cache")


@gpu
@pytest.mark.parametrize("S", [0, 2])
@pytest.mark.parametrize("Hq,Hkv", [(4, 1), (8, 2)])
def test_rope_kv_write_fp8_bytes(cuda, Hq, Hkv, S):
    """The fp8 KV writer on values that stay on the e4m3 grid: every data and exponent byte of both caches, written or
    not, equals ``ref.rope_kv_write``'s."""
    T, D = 37, 128
    W = (Hq + 2 * Hkv) * D
    g = _gen("rope8", Hq, S)
    qkv = _rope_input(T, W, S, g, fp8=True)
    cs = _quarter_table(64, D)
    pos = torch.randint(0, 64, (T,), generator=g)
    nb = 5
    slots = _slots(T, g, nb)
    q_ref = torch.empty(T, Hq, D, dtype=BF16)
    k_ref, v_ref = _caches(nb, Hkv, D, "fp8", "cpu")
    ops.rope_kv_write(qkv, pos, cs, q_ref, k_ref, v_ref, slots, Hq, Hkv)
    kd, vd = ref.fp8_dequant_pages(k_ref, v_ref)  # the premise: the stored values are the inputs, no rounding
    flat = (qkv.sum(0) if S else qkv).float().view(T, Hq + 2 * Hkv, D)
    for t in range(T):
        if slots[t] >= 0:
            blk, off = divmod(int(slots[t]), 16)
            assert torch.equal(vd[blk, :, :, off], flat[t, Hq + Hkv:])
            assert torch.equal(kd[blk, :, off].abs().sort(-1).values, flat[t, Hq:Hq + Hkv].abs().sort(-1).values)
    q = torch.full((T, Hq, D), NAN, dtype=BF16, device=cuda)
    k, v = _caches(nb, Hkv, D, "fp8", cuda)
    ops.rope_kv_write(qkv.to(cuda), pos.to(cuda), cs.to(cuda), q, k, v, slots.to(cuda), Hq, Hkv)
    msg = f"fp8 rope_kv_write Hq={Hq} S={S}"
    _same(q, q_ref, msg + " q")
    _same(k, k_ref, msg + " k pages")
    _same(v, v_ref, msg + " v pages")


# ---------------------------------------------------------------------------------------------------- 5. skinny GEMM
@gpu
@pytest.mark.parametrize("M", [129, 130, 192, 193, 255, 256])
@pytest.mark.parametrize("N,K,S", [(128, 256, 1), (128, 1024, 4), (256, 2048, 8)])
def test_skinny_exact(cuda, M, N, K, S):
    """``linear_skinny``: split s is the contiguous K[s K/S, (s+1) K/S) (skinny_gemm.hip ``k0 = blockIdx.y * ks``), so
    the slabs are compared one by one, in plain and in GLU gate | up order; one split: the bf16 output, and the
    activated GLU output on needle rows under the fused-SwiGLU tolerance."""
    assert ops.skinny_plan(M, N, K) == S
    w, unit = _weight("bf16", N, K)
    x, _ = _x(M, K, S)
    slabs, total = _exact_slabs(x, w, unit, S)
    xg = x.to(cuda)
    for glu in (False, True):
        if S == 1 and glu:
            wg, _ = _weight("bf16", N, K, "glu")
            xn = _needle_x(M, K, S)
            y = ops.linear_skinny(xn.to(cuda), _tiles("bf16", N, K, "glu", True, str(cuda))[0], glu=True)
            _close(y, _glu_ref(xn, wg), f"skinny glu M={M}")
            continue
        out = ops.linear_skinny(xg, _tiles("bf16", N, K, "full", glu, str(cuda))[0], glu=glu)
        _same(out, total.to(BF16) if S == 1 else slabs, f"skinny M={M} N={N} K={K} S={S} glu={glu}")


# -------------------------------------------------------------------------------------------------- 6. grouped kernels
E, TOPK = 8, 2
# entries per expert: an empty expert, one row, both sides of the 64-row tile, a multi-tile segment, and two that fill
# the rest; T = 192 runs the streaming kernel's 64-row tiles, T = 256 its 128-row ones
COUNTS = {192: (30, 1, 0, 63, 129, 65, 64, 32), 256: (95, 1, 0, 63, 129, 65, 64, 95)}


@functools.lru_cache(maxsize=None)
def _routing(T):
    """Hand-built CPU ``MoERouting``: expert e gets COUNTS[T][e] entries, every token two different experts, routing
    weights in {1/4, 1/2, 1}; sorted as ``moe_route`` sorts (by expert, token order inside)."""
    counts = COUNTS[T]
    assert sum(counts) == TOPK * T and max(counts) <= T and set((0, 1, 63, 64, 65, 129)) <= set(counts)
    order = [0, 1, 2, 3, 5, 6, 7, 4]  # runs laid end to end; entry i belongs to token i % T
    seq = torch.tensor([e for e in order for _ in range(counts[e])], dtype=torch.int32)
    te = seq.view(TOPK, T).t().contiguous()
    assert bool((te[:, 0] != te[:, 1]).all())
    tw = torch.tensor([1.0, 0.5, 0.25])[(torch.arange(T)[:, None] + 2 * torch.arange(TOPK)[None, :]) % 3]
    flat = te.reshape(-1).long()
    perm = torch.argsort(flat, stable=True)
    cnt = torch.bincount(flat, minlength=E)
    assert cnt.tolist() == list(counts)
    eo, to = torch.zeros(E + 1, dtype=torch.int32), torch.zeros(E + 1, dtype=torch.int32)
    eo[1:] = torch.cumsum(cnt, 0)
    to[1:] = torch.cumsum((cnt + ops.GG_BM - 1) // ops.GG_BM, 0)
    return ops.MoERouting(tw.contiguous(), te, (perm // TOPK).to(torch.int32), tw.reshape(-1)[perm].contiguous(), eo,
                          to, E)


def _routing_on(r, dev):
    return ops.MoERouting(*(t.to(dev) for t in (r.topk_w, r.topk_e, r.perm_tok, r.perm_w, r.expert_off, r.tile_off)),
                          r.num_experts)


@functools.lru_cache(maxsize=None)
def _experts(fmt, N, K, kind="full"):
    """(w bf16 [E, N, K], unit [E, N]): ``_weight`` per expert under its own seed; neighbours differ in sign pattern."""
    ws, us = zip(*(_weight(fmt, N, K, kind, seed=1 + e) for e in range(E)))
    w = torch.stack(ws)
    assert all(not torch.equal(torch.sign(w[e].float()), torch.sign(w[e + 1].float())) for e in range(E - 1))
    return w, torch.stack(us)


@functools.lru_cache(maxsize=None)
def _expert_tiles(fmt, N, K, kind, glu, dev, e_lo, e_n):
    w, _ = _experts(fmt, N, K, kind)
    wt, sc = ops.tile_experts_as(w[e_lo:e_lo + e_n], fmt, glu)
    assert torch.equal(_bits(ops.untile_experts_as(wt, sc, glu)), _bits(w[e_lo:e_lo + e_n]))
    return _to(wt, dev), _to(sc, dev)


def _combine_ref(a, w, unit, r, e_lo, e_n, T):
    """Exact fp32 [T, N] of the weighted combine over the local experts; guards as ``_exact_slabs``."""
    out = torch.zeros(T, w.shape[1], dtype=torch.float64)
    eo = r.expert_off.tolist()
    for e in range(e_lo, e_lo + e_n):
        lo, hi = eo[e], eo[e + 1]
        if lo == hi:
            continue
        _, y = _exact_slabs(a[lo:hi], w[e], unit[e], 1)
        out.index_add_(0, r.perm_tok[lo:hi].long(), y.double() * r.perm_w[lo:hi, None].double())
    # two routing weights >= 1/4 on sums below 2^22 units: within fp32 in either order
    assert torch.equal(out.float().double(), out)
    return out.float()


def _combine_input(r, F, e_lo, e_n):
    """a bf16 [n_ent, F]: integers in [-3, 3] with census and needle rows; rows of other ranks' experts hold 999 (the
    combine must not read them)."""
    n_ent = r.perm_tok.numel()
    a = _x(n_ent, F, 1, seed=5)[0].float()
    eo = r.expert_off.tolist()
    a[:eo[e_lo]] = 999.0
    a[eo[e_lo + e_n]:] = 999.0
    return a.to(BF16)


def _check_untouched_tokens(out, r, e_lo, e_n, msg):
    local = ((r.topk_e >= e_lo) & (r.topk_e < e_lo + e_n)).any(1)
    if e_n < E:
        assert bool((~local).any())
    assert bool((out.cpu()[~local] == 0).all()), msg + ": rows of tokens without a local expert were written"


@gpu
@pytest.mark.parametrize("e_lo,e_n", [(0, 8), (2, 4)])
@pytest.mark.parametrize("T", [192, 256])
def test_grouped_gemm_exact(cuda, T, e_lo, e_n):
    """``grouped_gemm`` (csrc/moe.hip): the gather half's bf16 rows (RNE of the exact sums; entries outside the local
    experts' range keep their sentinel) and the combine half's fp32 [T, d], exactly."""
    d, F = 256, 128
    r = _routing(T)
    rg = _routing_on(r, cuda)
    eo = r.expert_off.tolist()
    lo, hi = eo[e_lo], eo[e_lo + e_n]
    n_ent = TOPK * T
    # gather: h = x[perm_tok] @ w13_e^T, N = 2 F
    w13, u13 = _experts("bf16", 2 * F, d)
    x, _ = _x(T, d, 1, seed=3)
    h_ref = torch.full((n_ent, 2 * F), -777.0, dtype=BF16)
    for e in range(e_lo, e_lo + e_n):
        if eo[e] < eo[e + 1]:
            _, y = _exact_slabs(x[r.perm_tok[eo[e]:eo[e + 1]].long()], w13[e], u13[e], 1)
            h_ref[eo[e]:eo[e + 1]] = y.to(BF16)
    h = torch.full((n_ent, 2 * F), -777.0, dtype=BF16, device=cuda)
    ops.grouped_gemm(x.to(cuda), w13[e_lo:e_lo + e_n].to(cuda).contiguous(), rg, gather=True, e_lo=e_lo, y=h)
    msg = f"grouped_gemm T={T} e_lo={e_lo} e_n={e_n}"
    _same(h, h_ref, msg + " gather")
    assert bool((h_ref[:lo] == -777.0).all()) and bool((h_ref[hi:] == -777.0).all())
    # combine: out[tok] += w * (a[entry] @ w2_e^T), N = d
    w2, u2 = _experts("bf16", d, F)
    a = _combine_input(r, F, e_lo, e_n)
    out = torch.zeros(T, d, device=cuda)
    ops.grouped_gemm(a.to(cuda), w2[e_lo:e_lo + e_n].to(cuda).contiguous(), rg, gather=False, e_lo=e_lo,
                     combine_out=out)
    _same(out, _combine_ref(a, w2, u2, r, e_lo, e_n, T), msg + " combine")
    _check_untouched_tokens(out, r, e_lo, e_n, msg)


@gpu
@pytest.mark.parametrize("e_lo,e_n", [(0, 8), (2, 4)])
@pytest.mark.parametrize("T", [192, 256])
@pytest.mark.parametrize("fmt", FMTS)
def test_grouped_stream_exact(cuda, fmt, T, e_lo, e_n):
    """The grouped streaming kernel in three formats: the weighted combine's fp32 [T, d] exactly, and the fused-SwiGLU
    half on needle rows under its tolerance (0.27 allowed at most, 0.7 the smallest single-fault step)."""
    # d = 256 with F = 128 for the GLU half (N = 2 F, K = d); the combine streams K = F, and the kernel takes whole
    # 256-column chunks only (stream_moe_supported), so its F is 256 — the smallest every tile format takes
    d, F, F2 = 256, 128, 256
    assert ops.stream_moe_supported(2 * F, d) and ops.stream_moe_supported(d, F2) and not ops.stream_moe_supported(d, F)
    r = _routing(T)
    rg = _routing_on(r, cuda)
    eo = r.expert_off.tolist()
    lo, hi = eo[e_lo], eo[e_lo + e_n]
    msg = f"grouped stream {fmt} T={T} e_lo={e_lo} e_n={e_n}"
    w2, u2 = _experts(fmt, d, F2)
    w2t, w2s = _expert_tiles(fmt, d, F2, "full", False, str(cuda), e_lo, e_n)
    a = _combine_input(r, F2, e_lo, e_n)
    out = torch.zeros(T, d, device=cuda)
    ops.grouped_stream_combine(a.to(cuda), w2t, rg, T, out, e_lo=e_lo, scale=w2s)
    _same(out, _combine_ref(a, w2, u2, r, e_lo, e_n, T), msg + " combine")
    _check_untouched_tokens(out, r, e_lo, e_n, msg)
    w13, _ = _experts(fmt, 2 * F, d, "glu")
    w13t, w13s = _expert_tiles(fmt, 2 * F, d, "glu", True, str(cuda), e_lo, e_n)
    x = _needle_x(T, d, 1)
    y = ops.grouped_stream_glu(x.to(cuda), w13t, rg, e_lo=e_lo, scale=w13s)
    y_ref = torch.zeros(TOPK * T, F)
    for e in range(e_lo, e_lo + e_n):
        y_ref[eo[e]:eo[e + 1]] = _glu_ref(x[r.perm_tok[eo[e]:eo[e + 1]].long()], w13[e]).float()
    _close(y[lo:hi], y_ref[lo:hi], msg + " glu")


# ------------------------------------------------------------------------------------------ mutation check (CPU only)
def _mutation_cases():
    for fmt in FMTS:
        for N, K in STREAM_SHAPES:
            for M in (64, 256):
                S = ops.stream_plan(M, N, K)[2]
                if S > 1:
                    yield fmt, N, K, M, S


def _pick_term(x, w, ks):
    """(n, k) past the first split boundary with w[n, k] != 0 that a census row counts."""
    n = w.shape[0] // 2
    k = next(k for k in range(ks + 3, w.shape[1]) if w[n, k] != 0)
    return n, k


@pytest.mark.parametrize("fmt,N,K,M,S", list(_mutation_cases()))
def test_probes_notice_reference_mutations(fmt, N, K, M, S):
    """The exact comparison reports each of five single faults put into the REFERENCE of a streaming case (nothing
    here runs a kernel): the probes would have failed."""
    w, unit = _weight(fmt, N, K)
    x, _ = _x(M, K, S)
    slabs, total = _exact_slabs(x, w, unit, S)
    xf, wf, ks = x.float(), w.float(), K // S

    def split(wm, bounds=None):
        b = bounds or [s * ks for s in range(S + 1)]
        return torch.stack([xf[:, b[s]:b[s + 1]] @ wm[:, b[s]:b[s + 1]].t() for s in range(S)])

    assert _diff(split(wf), slabs) is None
    # one (n, k) term dropped
    n, k = _pick_term(x, w, ks)
    wm = wf.clone()
    wm[n, k] = 0.0
    assert _diff(split(wm), slabs) is not None
    # two adjacent 8-column lane groups swapped in one row
    k8 = next(c for c in range(0, K, 16) if not torch.equal(wf[n, c:c + 8], wf[n, c + 8:c + 16]))
    wm = wf.clone()
    wm[n, k8:k8 + 8], wm[n, k8 + 8:k8 + 16] = wf[n, k8 + 8:k8 + 16], wf[n, k8:k8 + 8]
    assert _diff(split(wm), slabs) is not None
    # the first split boundary moved by 16 columns
    bounds = [s * ks for s in range(S + 1)]
    bounds[1] += 16
    assert _diff(split(wf, bounds), slabs) is not None
    # an MXFP4 block dequantised with its neighbour's exponent
    if fmt == "mxfp4":
        # element 0 of a block is +-4 or +-6 times the block's scale 2^e: e = floor(log2 |w0|) - 2, the OCP rule
        e = torch.floor(torch.log2(wf.view(N, K // 32, 32)[..., 0].abs())) - 2
        b = next(b for b in range(K // 32 - 1) if e[n, b] != e[n, b + 1])
        wm = wf.clone()
        wm[n, 32 * b:32 * b + 32] *= torch.exp2(e[n, b + 1] - e[n, b])
        assert _diff(split(wm), slabs) is not None
    # slab 0 added twice, slab 1 omitted
    wrong = (2 * slabs[0] + slabs[2:].sum(0)).to(BF16)
    assert _diff(wrong, total.to(BF16)) is not None
