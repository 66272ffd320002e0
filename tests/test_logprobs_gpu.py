"""Per-token logprobs on the MI355X: the HIP kernel (ops/csrc/logprobs.hip) against the fp32 reference on the same
tensors, its ticket re-arm and graph capture, and the engine path from the sampler to ``StepOutput.logprobs``.

Bounds: ids exactly equal; values within 1e-3 absolute — fp32 accumulation over at most 131k terms of magnitude at
most 1 after the max shift and ``__expf`` / ``__logf`` at a few ulp put the error of the lse at ~1e-5, the bound leaves
100x over that (the reference itself stays within 1e-4 of float64, tests/test_logprobs_cpu.py)."""
import functools
import itertools
import math

import pytest
import torch

from kafka_llm_service_amd import ops
from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
from kafka_llm_service_amd.engine.sequence import SamplingParams
from kafka_llm_service_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

TOL = 1e-3
_RUNS = itertools.count()
KS = (0, 1, 5, 20)
B = 5


def _strided(x: torch.Tensor, stride: int, dev) -> torch.Tensor:
    """``x`` [B, V] on ``dev`` as a view of a [B, stride] buffer whose padding is NaN (a read past V would show)."""
    buf = torch.full((x.shape[0], stride), float("nan"), dtype=x.dtype, device=dev)
    buf[:, :x.shape[1]] = x.to(dev)
    return buf[:, :x.shape[1]]


@functools.lru_cache(maxsize=None)
def _case(V: int, bf16: bool):
    """Seeded normal logits scaled by 4 (bf16 ties over a long row), the sampled ids, and the reference's answer for
    every row at k = 20 (shared by the cases; never written to)."""
    g = torch.Generator().manual_seed(1000 + V)
    x = torch.randn(B, V, generator=g) * 4
    if bf16:
        x = x.to(torch.bfloat16)
    toks = torch.randint(0, V, (B,), generator=g)
    return x, toks, ref.token_logprobs(x, toks, None, 20)


def _check(got, want, k, msg=""):
    tl, pl, pi = (t.cpu() for t in got)
    wl, wp, wi = want
    wp, wi = wp[:, :k], wi[:, :k]
    assert torch.equal(pi.reshape(wi.shape), wi), f"{msg}: ids differ\n{pi}\n{wi}"
    assert pi.numel() == 0 or (int(pi.min()) >= -1 and int(pi.max()) < 1 << 31)
    for a, b, what in ((tl, wl, "token logprob"), (pl.reshape(wp.shape), wp, "top logprobs")):
        fin = torch.isfinite(b)
        assert torch.equal(torch.isfinite(a), fin), f"{msg}: {what} finiteness"
        assert torch.equal(a[~fin], b[~fin]), f"{msg}: {what} infinities"
        err = (a[fin] - b[fin]).abs().max().item() if fin.any() else 0.0
        assert err <= TOL, f"{msg}: {what} max err {err}"


@pytest.mark.parametrize("rows", [None, [3, 0, 4]], ids=["allrows", "rows304"])
@pytest.mark.parametrize("pad", [24, 0], ids=["strideV+24", "stride8"])
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", [128256, 32003, 16384 + 5, 1003, 8])
def test_kernel_matches_reference(cuda, V, bf16, pad, rows):
    """Split path without / with a tail, the smallest split size plus a tail, one workgroup with a tail, fewer entries
    than K; row stride V + 24 (rows that are not 16-byte aligned for most V: element loads) and the next multiple of
    8 above V (16-byte loads)."""
    x, toks, want = _case(V, bf16)
    stride = V + 24 if pad else (V + 7) // 8 * 8 + 8
    xd = _strided(x, stride, cuda)
    td = toks.to(cuda)
    if rows is not None:
        want = tuple(t[rows] for t in want)
    for k in KS:
        got = ops.token_logprobs(xd, td, rows, k)
        assert got[0].shape == (len(rows) if rows else B,) and got[1].shape == got[2].shape == (got[0].shape[0], k)
        _check(got, want, k, f"V={V} k={k}")
    if V < 20:
        assert (got[2][:, V:] == -1).all() and torch.isinf(got[1][:, V:]).all()


def _constructed(V: int, nsplit: int):
    """Rows built to hit the merge's corners at 8 splits of a V-entry row (slice = ceil(V/8 / nsplit) vectors)."""
    g = torch.Generator().manual_seed(7)
    per = -(-(V // 8) // nsplit) * 8
    base = torch.randn(7, V, generator=g)
    rows = []
    rows.append(torch.full((V,), 1.25))                                      # all equal: ids 0..K-1, -log V
    r = base[0].clone(); r[V - 1] = 50.0; rows.append(r)                     # maximum at the last index (the tail)
    r = base[1].clone(); r[(nsplit - 1) * per + 3] = 50.0; rows.append(r)    # maximum in the last split's first vector
    r = base[2].clone(); r[per + 100:per + 120] = torch.arange(20, 0, -1.0) + 30; rows.append(r)  # K largest, one split
    r = base[3].clone()
    for s in range(nsplit):                                                  # K largest spread one per split (ties too)
        r[min(V - 1, s * per + 17 * s)] = 40.0 - (s // 2)
    rows.append(r)
    r = base[4].clone(); rows.append(r)                                      # sampled token outside the top-K
    r = base[5].clone(); r[[0, 777, V - 1]] = float("nan"); r[5] = float("nan"); rows.append(r)  # a few NaN entries
    rows.append(base[6].clone())
    x = torch.stack(rows)
    toks = torch.randint(0, V, (x.shape[0],), generator=g)
    toks[5] = int(torch.argmin(x[5]))
    return x, toks


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", [128256, 32003])
def test_kernel_constructed_rows(cuda, V, bf16):
    x, toks = _constructed(V, ops.logprobs_split(V))
    if bf16:
        x = x.to(torch.bfloat16)
    want = ref.token_logprobs(x, toks, None, 20)
    xd = _strided(x, (V + 7) // 8 * 8 + 8, cuda)
    nan_row = 6
    for k in KS:
        got = ops.token_logprobs(xd, toks.to(cuda), None, k)
        ids = got[2].cpu()
        assert k == 0 or (int(ids.min()) >= 0 and int(ids.max()) < V)  # the NaN row included
        _check(got, want, k, f"V={V} k={k}")  # the reference treats NaN as -inf too: every row compares
        if k:
            assert ids[0].tolist() == list(range(k))
            assert abs(got[0][0].item() + math.log(V)) <= TOL
            assert not set(ids[nan_row].tolist()) & {0, 5, 777, V - 1}
    # the sampled token of row 5 is its smallest entry: outside the top 20, still scored
    assert int(toks[5]) not in got[2][5].tolist() and math.isfinite(got[0][5].item())


def test_rearm_and_reuse(cuda):
    """Three calls on the same outputs and workspace (B = 64, V = 128256, K = 20): the ticket re-arm and the partials'
    agent-scope round trip leave nothing behind, so every call gives the identical record."""
    V, n, k = 128256, 64, 20
    g = torch.Generator(device=cuda).manual_seed(11)
    x = (torch.randn(n, V, device=cuda, generator=g) * 4).to(torch.bfloat16)
    toks = torch.randint(0, V, (n,), device=cuda, generator=g)
    buf = ops.logprob_records(n, k, cuda)
    out = ops.unpack_logprob_records(buf, k)
    snaps = []
    for _ in range(3):
        buf.fill_(float("nan"))
        ops.token_logprobs(x, toks, None, k, out=out)
        snaps.append(buf.clone())
    assert torch.equal(snaps[0].view(torch.int32), snaps[1].view(torch.int32))
    assert torch.equal(snaps[0].view(torch.int32), snaps[2].view(torch.int32))
    _check(out, ref.token_logprobs(x.cpu(), toks.cpu(), None, k), k, "reuse")


def test_graph_capture(cuda):
    """One call captured in a hipGraph and replayed twice on new inputs equals the eager call: the op allocates
    nothing and never synchronises once its buffers exist."""
    V, n, k = 128256, 8, 5
    g = torch.Generator(device=cuda).manual_seed(12)
    x = (torch.randn(n, V, device=cuda, generator=g) * 4).to(torch.bfloat16)
    toks = torch.randint(0, V, (n,), device=cuda, generator=g)
    rows = torch.tensor([5, 1, 6], dtype=torch.int32, device=cuda)
    buf = ops.logprob_records(3, k, cuda)
    out = ops.unpack_logprob_records(buf, k)
    ops.token_logprobs(x, toks, rows, k, out=out)  # warm: workspace allocated before the capture
    eager = buf.clone()
    torch.cuda.synchronize()
    buf.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.token_logprobs(x, toks, rows, k, out=out)
    for _ in range(2):
        buf.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(buf.view(torch.int32), eager.view(torch.int32))
    x.copy_(x.flip(0))  # replay reads the static inputs as they are now
    graph.replay()
    again = ops.token_logprobs(x, toks, rows, k)
    torch.cuda.synchronize()
    for a, b in zip(out, again):
        assert torch.equal(a, b)


# ---- engine ---------------------------------------------------------------------------------------------------------
CFG = dict(model="small-llama", device="cuda:0", num_kv_blocks=4096, max_model_len=8192, cascade_min_prefix=64,
           prefill_kv_chunk=256)


@pytest.fixture(scope="module")
def eng(cuda):
    return LLMEngine(EngineConfig(**CFG, max_prefill_chunk=128))


def _fresh(eng, **kw):
    """A cold engine on the module's model: runs that are compared start from the same (empty) prefix cache, so they
    take the same kernels for the same rows (a prefix hit moves rows from the prefill tiles to the decode path, and
    the random-init model's flat logits turn that rounding difference into other tokens)."""
    return LLMEngine(EngineConfig(**CFG, max_prefill_chunk=128, **kw), model=eng.model)


def _prompts(seed, shared, tails, vocab=50000):
    g = torch.Generator().manual_seed(seed)
    prefix = torch.randint(0, vocab, (shared,), generator=g).tolist()
    return [prefix + torch.randint(0, vocab, (n,), generator=g).tolist() for n in tails]


def _params(ask: bool, short: bool = False):
    """Six requests: 0 / 2 / 4 ask when ``ask`` (top_logprobs 5, 0, 20); 2 and 3 sample with a seeded temperature."""
    out = []
    for i in range(6):
        kw = dict(temperature=0.8 if i in (2, 3) else 0.0, top_p=0.9 if i == 3 else 1.0, seed=50 + i,
                  max_tokens=4 if short and i % 2 == 0 else 10, ignore_eos=True)
        if ask and i % 2 == 0:
            kw.update(logprobs=True, top_logprobs=(5, 0, 20)[i // 2])
        out.append(SamplingParams(**kw))
    return out


def _serve(e, prompts, sps):
    """Run to completion (the last two requests join after two steps, so their chunked prefill meets decode rows):
    per-request StepOutputs, and for every step with logprob rows what the reference says about ITS logits."""
    launches, want, kinds = [], {}, set()
    r = e.runner
    o_launch, o_lp = r.launch, r.logprobs_device

    def launch(host, sample_seqs, prev=None):
        launches.append([s.request_id for s in sample_seqs])
        kinds.add(("decode" if host.B else "") + ("prefill" if host.T > host.B else ""))
        return o_launch(host, sample_seqs, prev)

    def lp_dev(logits, toks, sp):
        if sp.lp_rows is not None:
            tl, pl, pi = ref.token_logprobs(logits.float().cpu(), toks.cpu(), sp.lp_rows.tolist(), sp.lp_k)
            for j, row in enumerate(sp.lp_rows.tolist()):
                want.setdefault(launches[-1][row], []).append((int(toks[row]), tl[j].item(), pi[j].tolist()))
        return o_lp(logits, toks, sp)

    r.launch, r.logprobs_device = launch, lp_dev
    outs: dict = {}
    run = next(_RUNS)
    try:
        seqs = [e.add_request(f"q{run}-{i}", prompts[i], sps[i]) for i in range(4)]
        steps = 0
        while e.has_unfinished() or len(seqs) < len(prompts):
            if steps == 2:
                seqs += [e.add_request(f"q{run}-{i}", prompts[i], sps[i]) for i in (4, 5)]
            for o in e.step():
                outs.setdefault(o.request_id, []).append(o)
            steps += 1
    finally:
        r.launch, r.logprobs_device = o_launch, o_lp
    return seqs, outs, want, kinds


def _check_engine_run(seqs, outs, want, sps):
    for s, sp in zip(seqs, sps):
        os_ = outs[s.request_id]
        if not sp.logprobs:
            assert all(o.logprobs is None for o in os_)
            continue
        recs = [r for o in os_ for r in o.logprobs]
        assert all(len(o.logprobs) == len(o.new_token_ids) for o in os_)  # every token has its record
        assert [r[0] for r in recs] == s.output_ids and len(recs) == sp.max_tokens
        exp = want[s.request_id]
        assert len(exp) >= len(recs)
        for (t, lp, ids, lps), (wt, wlp, wids) in zip(recs, exp):
            assert t == wt and abs(lp - wlp) <= TOL, (lp, wlp)
            assert len(ids) == len(lps) == sp.top_logprobs and ids == wids[:sp.top_logprobs]
            assert all(a >= b for a, b in zip(lps, lps[1:])) and lp <= 0
            if sp.temperature == 0 and ids:
                assert ids[0] == t


def test_engine_logprobs(eng):
    prompts = _prompts(21, 100, (3, 50, 200, 9, 300, 150))
    e0 = _fresh(eng)
    plain = _serve(e0, prompts, _params(False))
    assert not plain[2] and e0.runner._lp_host is None  # nobody asked: nothing computed, nothing allocated
    sps = _params(True)
    seqs, outs, want, kinds = _serve(_fresh(eng), prompts, sps)
    assert "decodeprefill" in kinds or {"decode", "prefill"} <= kinds
    assert any(len(p) > 128 for p in prompts)  # chunked prefill (max_prefill_chunk = 128)
    _check_engine_run(seqs, outs, want, sps)
    # the sampler path is untouched: every request emits the ids it emits when nobody asks
    assert [s.output_ids for s in seqs] == [s.output_ids for s in plain[0]]


def test_engine_logprobs_with_graphs(eng):
    """TP = 1 with hipGraph decode: steps with asking rows run eagerly (the logits are internal to a captured graph),
    later steps replay graphs; the results equal the eager engine's."""
    prompts = _prompts(22, 100, (3, 50, 77, 9, 30, 15))
    sps = _params(True, short=True)
    eager = _fresh(eng)
    eager.runner.fixed_decode_items = True  # the graph engine's decode split, so both sum in the same order
    e_seqs, e_outs, _, _ = _serve(eager, prompts, sps)
    g = _fresh(eng, use_graphs=True)
    replays_at_lp = []
    o_lp = g.runner.logprobs_device

    def lp_dev(logits, toks, sp):
        if sp.lp_rows is not None:
            replays_at_lp.append(g.runner.graphs.stats["replays"])
        return o_lp(logits, toks, sp)

    g.runner.logprobs_device = lp_dev
    seqs, outs, want, _ = _serve(g, prompts, sps)
    st = g.runner.graphs.stats
    assert not g.runner.graphs.disabled, "hipGraph capture failed (see log)"
    assert replays_at_lp and st["replays"] > replays_at_lp[-1] and st["replays"] >= 1
    _check_engine_run(seqs, outs, want, sps)
    assert [s.output_ids for s in seqs] == [s.output_ids for s in e_seqs]
    for a, b in zip(seqs, e_seqs):
        ra = [r for o in outs[a.request_id] for r in (o.logprobs or [])]
        rb = [r for o in e_outs[b.request_id] for r in (o.logprobs or [])]
        assert len(ra) == len(rb)
        for x, y in zip(ra, rb):
            assert x[0] == y[0] and x[2] == y[2] and abs(x[1] - y[1]) <= TOL
