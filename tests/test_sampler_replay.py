"""The token sampler (ops/csrc/sampling.hip) against a per-draw oracle. The kernel's noise is a pure integer function
of (seed, step, round, index), so ``ops.reference.sample_replay`` reproduces its stream bit for bit and replays every
decision in float64. The CPU tests prove that the replayed algorithm samples the intended distribution (chi-square
against softmax(x / T) and its top-k / top-p renormalisation, the kept set against the sort-based definition); the GPU
tests pin the kernel to the replay: every row the replay does not flag ``ambiguous`` (a decision within an fp32 band,
see SAMPLE_SCORE_BAND / SAMPLE_MASS_BAND in ops/reference.py) has exactly one right token."""
import itertools

import numpy as np
import pytest
import torch

from kafka_llm_service_amd import ops
from kafka_llm_service_amd.ops import reference as ref

AMBIGUOUS_CAP = 0.02  # of a test's rows; asserted on the replay's flags before the kernel runs


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the replayed algorithm
# ---------------------------------------------------------------------------------------------------------------------

M64 = (1 << 64) - 1


def _py_mix64(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _py_lowbias32(x: int) -> int:
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    return x ^ (x >> 16)


def test_integer_stream_is_bit_exact():
    """The wrapping numpy integers against plain Python integers masked by hand, and splitmix64's published first two
    outputs for seed 0; the clamp of u is the fp32 value 1 - 2^-24."""
    assert _py_mix64(0) == 0xE220A8397B1DCDAF and _py_mix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    rng = np.random.default_rng(0)
    z = rng.integers(0, 1 << 64, 256, dtype=np.uint64)
    z[:4] = [0, M64, 1 << 63, 0x9E3779B97F4A7C15]
    with np.errstate(all="ignore"):
        got = ref._mix64(z)
        low = ref._lowbias32(z.astype(np.uint32))
    assert [int(v) for v in got] == [_py_mix64(int(v)) for v in z]
    assert [int(v) for v in low] == [_py_lowbias32(int(v) & 0xFFFFFFFF) for v in z]
    assert ref._U_CLAMP == 1.0 - 2.0 ** -24 == float(np.float32(0.99999994))
    # one whole plain draw and one filtered round by hand: V = 9 (a tail of one), a negative seed, a step above 2^32
    seed, step, V = -5, (1 << 40) + 3, 9
    x = torch.tensor([[0.5, -1.0, 2.0, 0.0, 1.5, -0.5, 1.0, 0.25, 1.75]])
    inv_t = float(np.float32(1.0) / np.float32(0.7))
    xv = [float(np.float32(v) * np.float32(inv_t)) for v in x[0].tolist()]
    gum = lambda h: -np.log(-np.log(min((h + 1) * 2.0 ** -24, 1.0 - 2.0 ** -24)))
    stream = (step << 8) & M64
    key = _py_mix64((seed & M64) ^ _py_mix64((stream * 0x632BE59BD9B4E019) & M64))
    score = [xv[i] + gum(_py_lowbias32(_py_lowbias32((i + key) & 0xFFFFFFFF) ^ (key >> 32)) >> 8) for i in range(V)]
    args = dict(temperature=torch.tensor([0.7]), seeds=torch.tensor([seed]), step=torch.tensor([step]))
    assert int(ref.sample_replay(x, **args).tokens[0]) == int(np.argmax(score))
    score = [xv[i] + gum(_py_mix64((seed & M64) ^ _py_mix64((stream * 0x632BE59BD9B4E019 + i) & M64)) >> 40)
             for i in range(V)]
    r = ref.sample_replay(x, top_k=torch.tensor([V - 1], dtype=torch.int32), **args)  # accepts all but the smallest
    assert int(np.argmax(score)) != 1  # (index 1 is the smallest: the one token top_k = V - 1 rejects)
    assert int(r.tokens[0]) == int(np.argmax(score)) and int(r.rounds[0]) == 1 and not bool(r.plain[0])


GOF_V, GOF_N, GOF_T = 64, 200_000, 0.8
GOF_CONFIGS = {"temperature": (0, 1.0), "top_k=5": (5, 1.0), "top_p=0.5": (0, 0.5), "top_k=8,top_p=0.7": (8, 0.7)}


def _gof_logits():
    return torch.randn(1, GOF_V, generator=torch.Generator().manual_seed(1234)) * 2


def _kept(x64: np.ndarray, k: int, p: float):
    """float64 softmax of the scaled logits x64 and the set {c : #(x > x_c) < k and mass(x > x_c) < p}."""
    q = np.exp(x64 - x64.max())
    q /= q.sum()
    above = x64[None, :] > x64[:, None]  # [c, j]: j strictly above c
    cnt = above.sum(1)
    mass = (above * q[None, :]).sum(1)
    return q, ((cnt < k) if k > 0 else np.ones_like(cnt, dtype=bool)) & (mass < p)


def _chi2_sf(chi2: float, df: int) -> float:
    return float(torch.special.gammaincc(torch.tensor(df / 2.0, dtype=torch.float64),
                                         torch.tensor(chi2 / 2.0, dtype=torch.float64)))


@pytest.mark.parametrize("name", list(GOF_CONFIGS))
def test_replay_goodness_of_fit(name):
    """200 000 fixed (seed, step) pairs over one row of 64 fp32 logits: the replayed draws fit softmax(x / T)
    renormalised over the kept set (Pearson chi-square, bins with expected count below 5 merged, p > 1e-4), and no
    token outside the kept set is ever drawn."""
    k, p = GOF_CONFIGS[name]
    x = _gof_logits()
    i = torch.arange(GOF_N, dtype=torch.long)
    seeds = (i // 4) * 2654435761 + 17
    steps = i % 4
    r = ref.sample_replay(x.expand(GOF_N, GOF_V), torch.full((GOF_N,), GOF_T), torch.full((GOF_N,), p),
                          torch.full((GOF_N,), k, dtype=torch.int32), seeds, steps)
    assert not bool(r.fell_back.any()), f"fallback rows {int(r.fell_back.sum())}, max rounds {int(r.rounds.max())}"
    assert bool(r.plain.all()) == (name == "temperature")
    q, keep = _kept(x[0].double().numpy() / GOF_T, k, p)
    assert 0 < keep.sum() < GOF_V or name == "temperature"
    obs = np.bincount(r.tokens.numpy(), minlength=GOF_V).astype(np.float64)
    assert obs[~keep].sum() == 0, f"drawn outside the kept set: {np.nonzero((obs > 0) & ~keep)[0]}"
    exp = np.where(keep, q, 0.0) / q[keep].sum() * GOF_N
    order = np.argsort(exp[keep])
    e, o = exp[keep][order], obs[keep][order]
    small = int((e < 5).sum())
    if small:  # pool the small bins; if the pool is still below 5, the smallest remaining bin joins it
        while small < e.size and e[:small].sum() < 5:
            small += 1
        e = np.concatenate([[e[:small].sum()], e[small:]])
        o = np.concatenate([[o[:small].sum()], o[small:]])
    chi2 = float(((o - e) ** 2 / e).sum())
    pv = _chi2_sf(chi2, e.size - 1) if e.size > 1 else 1.0
    assert pv > 1e-4, f"{name}: chi2 {chi2:.1f} over {e.size} bins, p = {pv:.3g}"


def test_kept_set_is_the_sorted_prefix():
    """On tie-free rows the kernel's acceptance set {c : cnt_above(c) < k and mass_above(c) < p} is the keep mask of
    ref.sample's sort (first k of the descending order, and every token whose preceding mass is below p), and the
    replay draws inside it."""
    g = torch.Generator().manual_seed(5)
    for V, k, p, T in [(257, 0, 0.9, 1.0), (257, 10, 1.0, 0.7), (257, 10, 0.5, 1.3), (40, 3, 0.8, 1.0),
                       (1031, 50, 0.999, 2.5), (9, 8, 0.1, 0.5)]:
        x = torch.randn(1, V, generator=g) * 2
        assert x.unique().numel() == V
        x64 = x[0].double().numpy() / T
        q, keep = _kept(x64, k, p)
        order = np.argsort(-q, kind="stable")  # ref.sample: argsort(p, descending), keep[tk:] = False, above < tp
        ps = q[order]
        skeep = np.ones(V, dtype=bool)
        if k > 0:
            skeep[k:] = False
        skeep &= (np.cumsum(ps) - ps) < p
        want = np.zeros(V, dtype=bool)
        want[order[skeep]] = True
        assert (keep == want).all(), (V, k, p)
        n = 512
        r = ref.sample_replay(x.expand(n, V), torch.full((n,), T), torch.full((n,), p),
                              torch.full((n,), k, dtype=torch.int32), torch.arange(n) * 31 + 1)
        assert not bool(r.fell_back.any()) and bool(keep[r.tokens.numpy()].all()), (V, k, p)
        assert len(set(r.tokens.tolist())) > 1 or keep.sum() == 1


def _mixed_params(B, seed0=3):
    temp = torch.tensor([0.0, 0.7, 1.0, 1.5] * ((B + 3) // 4))[:B]
    seeds = torch.arange(B, dtype=torch.long) * 7919 + seed0
    return temp, seeds


@pytest.mark.parametrize("V", [1, 7, 8, 9, 40, 1031, 16389])
def test_replay_split_invariance(V):
    """``nsplit`` (1, a split count that leaves splits without a vector, the sampler's 8, the maximum 64) does not
    change the token: the noise of an index does not depend on the split that owns it."""
    B = 8
    x = (torch.randn(B, V, generator=torch.Generator().manual_seed(V)) * 3).to(torch.bfloat16)
    temp, seeds = _mixed_params(B)
    step = torch.tensor([11])
    one = ref.sample_replay(x, temp, seeds=seeds, step=step, nsplit=1)
    assert torch.equal(one.tokens[0::4], x[0::4].float().argmax(-1))
    for ns in (2, 3, 8, 64):
        r = ref.sample_replay(x, temp, seeds=seeds, step=step, nsplit=ns)
        assert torch.equal(r.tokens, one.tokens) and torch.equal(r.ambiguous, one.ambiguous), ns


def test_replay_step_and_seed_select_the_stream():
    """Equal (seed, step) give equal draws; another step or another seed gives another stream, on the plain path and
    on the filtered one."""
    B, V = 64, 1031
    x = torch.randn(B, V, generator=torch.Generator().manual_seed(2))
    temp = torch.ones(B)
    seeds = torch.arange(B, dtype=torch.long) * 13 - 40
    for topp in (None, torch.full((B,), 0.95)):
        draw = lambda sd, st: ref.sample_replay(x, temp, topp, None, sd, torch.tensor([st])).tokens
        a = draw(seeds, 4)
        assert torch.equal(a, draw(seeds.clone(), 4))
        for other in (draw(seeds, 5), draw(seeds, 4 + (1 << 40)), draw(seeds + 1, 4), draw(seeds + (1 << 41), 4)):
            assert (other != a).float().mean() > 0.8
    # a per-row step (replay only) is the same stream as that step given alone
    steps = torch.arange(B, dtype=torch.long) % 3
    per_row = ref.sample_replay(x, temp, seeds=seeds, step=steps).tokens
    for s in range(3):
        alone = ref.sample_replay(x, temp, seeds=seeds, step=torch.tensor([s])).tokens
        assert torch.equal(per_row[steps == s], alone[steps == s])


def test_replay_tie_rules():
    """Strict inequalities: tokens tied with the candidate count toward neither k nor the mass, so top_k = 1 over a
    row of equal logits accepts the first draw whatever it is, and over a row whose maximum occurs twice returns one
    of the two; a row with nothing above the pivot falls back to the argmax (all masked: token 0)."""
    V, n = 40, 64
    seeds = torch.arange(n, dtype=torch.long)
    one = torch.ones(n, dtype=torch.int32)
    flat = ref.sample_replay(torch.zeros(n, V), torch.ones(n), None, one, seeds)
    assert int(flat.rounds.max()) == 1 and len(set(flat.tokens.tolist())) > 8 and not bool(flat.fell_back.any())
    x = torch.randn(1, V, generator=torch.Generator().manual_seed(9))
    x[0, 5] = x[0, 33] = 4.0
    twice = ref.sample_replay(x.expand(n, V), torch.ones(n), None, one, seeds)
    assert set(twice.tokens.tolist()) == {5, 33} and not bool(twice.fell_back.any())
    dead = ref.sample_replay(torch.full((2, V), float("-inf")), torch.ones(2), torch.full((2,), 0.5))
    assert dead.tokens.tolist() == [0, 0] and bool(dead.fell_back.all()) and dead.rounds.tolist() == [0, 0]


# ---------------------------------------------------------------------------------------------------------------------
# GPU: every non-ambiguous row's token equals the replay's
# ---------------------------------------------------------------------------------------------------------------------

def _capped(rep, what):
    """Assert the ambiguity cap on the replay alone (before the kernel is looked at); returns the report line."""
    B = rep.tokens.numel()
    msg = (f"{what}: rows {B}, ambiguous {int(rep.ambiguous.sum())}, max rounds {int(rep.rounds.max())}, "
           f"fallback rows {int(rep.fell_back.sum())}")
    assert int(rep.ambiguous.sum()) <= AMBIGUOUS_CAP * B, msg
    return msg


def _same(tok, rep, msg):
    tok = tok.cpu()
    bad = torch.nonzero((tok != rep.tokens) & ~rep.ambiguous).flatten().tolist()
    assert not bad, f"{msg}; rows {bad[:8]} differ: kernel {tok[bad[:8]].tolist()} replay {rep.tokens[bad[:8]].tolist()}"
    print(msg)


def _ws(cuda, B, nsplit):
    return torch.zeros(65536 + 2 * B * nsplit, dtype=torch.int32, device=cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_sample_plain_full_vocab_matches_replay(cuda, dtype):
    """Greedy and plain-temperature rows over the full vocabulary, through ops.sample (8 splits, launched three times:
    the tickets re-arm) and through one workgroup per row, at steps 0, 5 and 2^40 and seeds that include 0, a negative
    value and values above 2^40."""
    from kafka_llm_service_amd.ops._ext import ext

    B, V = 64, 128256
    x = (torch.randn(B, V, generator=torch.Generator().manual_seed(31)) * 3).to(dtype)
    temp = torch.tensor([0.0, 0.25, 0.7, 1.0, 1.3, 4.0] * 11)[:B]
    seeds = torch.arange(B, dtype=torch.long) * 1000003 - 17
    seeds[:4] = torch.tensor([0, -1, (1 << 40) + 12345, -(1 << 62)])
    xg, tg, sg = x.to(cuda), temp.to(cuda), seeds.to(cuda)
    for stepv in (0, 5, 1 << 40):
        step = torch.tensor([stepv], dtype=torch.long)
        rep = ref.sample_replay(x, temp, seeds=seeds, step=step, nsplit=8)
        msg = _capped(rep, f"plain {dtype} step {stepv}")
        assert bool(rep.plain[temp > 0].all()) and not bool(rep.plain[temp == 0].any())
        for it in range(3):
            _same(ops.sample(xg, tg, seeds=sg, step=step.to(cuda)), rep, f"{msg}, 8 splits launch {it}")
        one = torch.empty(B, dtype=torch.long, device=cuda)
        ext().sample(xg, tg, None, None, sg, step.to(cuda), one, None, 1)
        _same(one, rep, f"{msg}, one workgroup")


@pytest.mark.gpu
@pytest.mark.parametrize("V", [1, 7, 8, 9, 40, 1031, 16389])
def test_sample_ragged_vocab_matches_replay(cuda, V):
    """Vocabularies that are no multiple of 8 in rows with a padded stride whose padding holds the dtype's largest
    finite value (a read past V would win the argmax): the scalar tail, splits that own no vector (V = 40: three of
    eight) and the filtered path (top_k = 3 with top_p = 0.8) all see stochastic draws."""
    from kafka_llm_service_amd.ops._ext import ext

    B = 16
    temp, seeds = _mixed_params(B, seed0=V)
    step = torch.tensor([3], dtype=torch.long)
    topk = torch.full((B,), 3, dtype=torch.int32)
    topp = torch.full((B,), 0.8)
    for dtype in (torch.bfloat16, torch.float32):
        x = torch.randn(B, V, generator=torch.Generator().manual_seed(100 + V)) * 3
        x[0::3, V - 1] = x[0::3].max(1).values + 1  # every third row (greedy rows 0 and 12) peaks at the tail's end
        x = x.to(dtype)
        buf =torch.full((B, (V + 7) // 8 * 8 + 8), torch.finfo(dtype).max, dtype=dtype, device=cuda)
        buf[:, :V] = x.to(cuda)
        xg = buf[:, :V]
        for what, tp, tk in (("plain", None, None), ("top_k 3 top_p 0.8", topp, topk)):
            rep = ref.sample_replay(x, temp, tp, tk, seeds, step, nsplit=8)
            msg = _capped(rep, f"V {V} {dtype} {what}")
            assert torch.equal(rep.tokens[0::4], x[0::4].float().argmax(-1))
            assert V % 8 == 0 or int((rep.tokens >= V // 8 * 8).sum()) >= 2, msg  # the tail wins in some rows
            for nsplit in (1, 8):
                out = torch.full((B,), -1, dtype=torch.long, device=cuda)
                ext().sample(xg, temp.to(cuda), None if tp is None else tp.to(cuda), None if tk is None else tk.to(cuda),
                             seeds.to(cuda), step.to(cuda), out, _ws(cuda, B, nsplit), nsplit)
                _same(out, rep, f"{msg}, nsplit {nsplit}")


def _padded(cuda, x):
    """x on the device in rows of a padded stride whose padding holds the dtype's largest finite value."""
    B, V = x.shape
    buf = torch.full((B, (V + 7) // 8 * 8 + 8), torch.finfo(x.dtype).max, dtype=x.dtype, device=cuda)
    buf[:, :V] = x.to(cuda)
    return buf[:, :V]


@pytest.mark.gpu
def test_sample_fallback_argmax_matches_replay(cuda):
    """A top_p that no mass is below accepts no candidate, so the pivot climbs until nothing lies above it and every row
    ends in the fallback: the fp32 argmax of the row itself, over its vectors and its scalar tail, not past V. The
    value is -1, not 0: the mass above the row's maximum is exactly 0, which the replay's band around ``mass < top_p``
    (SAMPLE_MASS_BAND) has to call ambiguous in every row; against -1 no mass is anywhere near."""
    from kafka_llm_service_amd.ops._ext import ext

    B, V = 8, 1031
    x = torch.randn(B, V, generator=torch.Generator().manual_seed(77)) * 3
    x[0::3, V - 1] = x[0::3].max(1).values + 1  # rows 0, 3 and 6 peak at the tail's end
    temp = torch.tensor([0.5, 0.7, 1.0, 1.5] * 2)
    seeds = torch.arange(B, dtype=torch.long) * 7919 + 5
    step = torch.tensor([4], dtype=torch.long)
    topp = torch.full((B,), -1.0)
    rep = ref.sample_replay(x, temp, topp, None, seeds, step)
    msg = _capped(rep, "fallback V 1031")
    assert bool(rep.fell_back.all()), msg
    assert torch.equal(rep.tokens, x.argmax(-1)) and int((rep.tokens >= V // 8 * 8).sum()) >= 3, msg
    xg = _padded(cuda, x)
    for nsplit in (1, 8):
        out = torch.full((B,), -1, dtype=torch.long, device=cuda)
        ext().sample(xg, temp.to(cuda), topp.to(cuda), None, seeds.to(cuda), step.to(cuda), out, _ws(cuda, B, nsplit),
                     nsplit)
        _same(out, rep, f"{msg}, nsplit {nsplit}")
        assert torch.equal(out.cpu(), x.argmax(-1))


@pytest.mark.gpu
@pytest.mark.parametrize("V,owning", [(1031, 64), (1039, 43)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_sample_64_splits_short_ragged_row_matches_replay(cuda, dtype, V, owning):
    """A short ragged row over 64 splits. V = 1031: 128 vectors, two in every slice, the last slice also owns the tail
    of 7. V = 1039: 129 vectors, three per slice, so slices 0..42 own vectors and 43..63 own none — a greedy or plain
    split with nothing to offer, a min_p split that publishes (-inf, no winner) — and the empty last slice still owns
    the tail of 7. Greedy, plain-temperature and min_p rows (proc[7]), three launches on one workspace (the tickets
    re-arm): the tokens are the replay's at 64 splits and those of the one-workgroup launch."""
    from test_min_p import min_p_proc

    from kafka_llm_service_amd.ops._ext import ext

    B, NS = 16, 64
    nvec = V // 8
    per = -(-nvec // NS)  # the kernel's partition (row_slice): slice k holds the vectors [k * per, min(nvec, k * per + per))
    assert sum(k * per < nvec for k in range(NS)) == owning and V - nvec * 8 == 7
    x = torch.randn(B, V, generator=torch.Generator().manual_seed(64)) * 3
    x[0::3, V - 1] = x[0::3].max(1).values + 1
    x = x.to(dtype)
    temp, seeds = _mixed_params(B, seed0=V)  # rows 0, 4, 8, 12 greedy
    step = torch.tensor([6], dtype=torch.long)
    proc = min_p_proc(B, [0.1 if i % 2 else 0.0 for i in range(B)])  # odd rows: min_p under temperature
    assert bool((proc[1::2, 7] != 0).all()) and not bool(proc[0::2, 7].any())
    rep = ref.sample_replay(x, temp, seeds=seeds, step=step, proc=proc, nsplit=NS)
    msg = _capped(rep, f"64 splits V {V} {dtype}")
    assert torch.equal(rep.tokens, ref.sample_replay(x, temp, seeds=seeds, step=step, proc=proc, nsplit=1).tokens)
    assert torch.equal(rep.tokens[0::4], x[0::4].float().argmax(-1))
    xg, pg = _padded(cuda, x), proc.to(cuda)
    mt = torch.zeros(1, (V + 31) // 32, dtype=torch.int32, device=cuda)
    one = torch.full((B,), -1, dtype=torch.long, device=cuda)
    ext().sample(xg, temp.to(cuda), None, None, seeds.to(cuda), step.to(cuda), one, None, 1, pg, mt, None, None)
    _same(one, rep, f"{msg}, one workgroup")
    ws = _ws(cuda, B, NS)
    for launch in range(3):
        out = torch.full((B,), -1, dtype=torch.long, device=cuda)
        ext().sample(xg, temp.to(cuda), None, None, seeds.to(cuda), step.to(cuda), out, ws, NS, pg, mt, None, None)
        _same(out, rep, f"{msg}, launch {launch}")
        assert torch.equal(out, one), f"{msg}, launch {launch}: 64 splits differ from one workgroup"
    assert not bool(ws[:65536].any())  # every ticket re-armed


def _filtered_case(V, dtype):
    """Rows walk the product top_k x top_p x T (64 rows over two steps, stride 7 through its 90 entries); row 0 takes
    top_k = V with top_p = 1 (the plain stream), row 1 is a row of equal logits and row 2 a row whose maximum occurs
    twice, both under top_k = 1."""
    B = 32
    combos = list(itertools.product([0, 1, 2, 50, V - 1, V], [1.0, 0.999, 0.9, 0.5, 0.1], [0.5, 1.0, 2.5]))
    x = (torch.randn(B, V, generator=torch.Generator().manual_seed(V)) * 3).to(dtype)
    x[1] = 1.25
    x[2, 77] = x[2, V - 3] = x[2].float().max() + 1
    seeds = torch.arange(B, dtype=torch.long) * 104729 - 5
    cases = []
    for s, stepv in enumerate((2, 7)):
        rows = [combos[(7 * (s * B + i)) % len(combos)] for i in range(B)]
        rows[0], rows[1], rows[2] = (V, 1.0, 1.0), (1, 1.0, 1.0), (1, 1.0, 1.0)
        tk = torch.tensor([r[0] for r in rows], dtype=torch.int32)
        tp = torch.tensor([r[1] for r in rows], dtype=torch.float32)
        temp = torch.tensor([r[2] for r in rows], dtype=torch.float32)
        cases.append((temp, tp, tk, torch.tensor([stepv], dtype=torch.long)))
    return x, seeds, cases


@pytest.mark.gpu
@pytest.mark.parametrize("V,dtype", [(128256, torch.bfloat16), (32000, torch.float32)])
def test_sample_filtered_matches_replay(cuda, V, dtype):
    """The rejection loop draw by draw: pivot raise, strict comparisons on ties (bf16 rows of 128k entries are full of
    exact ties), mass < p, cnt < k, every round's own stream. Rows without an effective filter take the plain stream,
    and the replay says so."""
    x, seeds, cases = _filtered_case(V, dtype)
    xg, sg = x.to(cuda), seeds.to(cuda)
    for temp, tp, tk, step in cases:
        rep = ref.sample_replay(x, temp, tp, tk, seeds, step, nsplit=8)
        msg = _capped(rep, f"filtered V {V} {dtype} step {int(step)}")
        unfiltered = (tp >= 1) & ((tk <= 0) | (tk >= V))
        assert torch.equal(rep.plain, unfiltered) and bool(rep.plain[0]) and int(rep.rounds[0]) == 0
        assert int(rep.rounds[1]) == 1 and int(rep.tokens[2]) in (77, V - 3), msg
        assert bool((rep.rounds[~unfiltered] >= 1).all())
        tok = ops.sample(xg, temp.to(cuda), tp.to(cuda), tk.to(cuda), sg, step.to(cuda))
        _same(tok, rep, msg)


@pytest.mark.gpu
def test_sample_proc_with_temperature_matches_replay(cuda):
    """Device-side logits processing under temperature: bitmask, forced and penalty rows at T = 0.9, plain and with
    top_p = 0.9, four successive steps each with the count table carried along — tokens and counts equal the replay's
    after every step. Penalties are multiples of 1/8 and the bf16 logits stay below 16 in magnitude, so the fp32
    penalty arithmetic is exact with or without an fma."""
    from kafka_llm_service_amd.engine.logits_proc import LogitsProcessor
    from kafka_llm_service_amd.engine.sequence import SamplingParams, Sequence

    B, V = 24, 128256
    x = (torch.randn(B, V, generator=torch.Generator().manual_seed(21)) * 3).clamp(-15.5, 15.5).to(torch.bfloat16)
    lp_g = LogitsProcessor(cuda, V, max_slots=32, mask_rows=16)
    lp_c = LogitsProcessor("cpu", V, max_slots=32, mask_rows=16)
    seqs = [Sequence(f"r{i}", [1], SamplingParams(temperature=0.9, presence_penalty=0.5 * (i % 3 == 2),
                                                  frequency_penalty=1.5 * (i % 3 == 2))) for i in range(B)]
    g = torch.Generator().manual_seed(3)
    rows = []
    for i in range(B):
        if i % 4 == 0:
            rows.append((i, seqs[i], torch.randint(0, V, (int(torch.randint(2, 3000, (1,), generator=g)),),
                                                   generator=g).tolist()))
        elif i % 4 == 1:
            rows.append((i, seqs[i], [int(torch.randint(0, V, (1,), generator=g))]))
        elif i % 3 == 2:
            rows.append((i, seqs[i], None))
    proc, upd = lp_g.build(rows, B)
    proc_c, upd_c = lp_c.build(rows, B)
    assert (proc == proc_c).all()
    lp_g.apply(upd, lambda a: torch.from_numpy(a).to(cuda))
    lp_c.apply(upd_c, torch.from_numpy)
    mt_g, cnt_g = lp_g.tables()
    mt_c, cnt_c = lp_c.tables()
    pd_c = torch.from_numpy(proc)
    pd_g = pd_c.to(cuda)
    xg = x.to(cuda)
    temp = torch.full((B,), 0.9)
    seeds = torch.arange(B, dtype=torch.long) * 13 + 1
    stepv = 0
    for topp in (1.0, 0.9):
        tp = torch.full((B,), topp)
        for _ in range(4):
            step = torch.tensor([stepv], dtype=torch.long)
            stepv += 1
            rep = ref.sample_replay(x, temp, tp, None, seeds, step, proc=pd_c, mask_tab=mt_c, counts=cnt_c, nsplit=8)
            msg = _capped(rep, f"proc top_p {topp} step {int(step)}")
            tok = ops.sample(xg, temp.to(cuda), tp.to(cuda), None, seeds.to(cuda), step.to(cuda), proc=pd_g,
                             mask_tab=mt_g, counts=cnt_g)
            _same(tok, rep, msg)
            assert not bool(rep.ambiguous.any()), msg  # the count tables can only be compared when no row may differ
            assert torch.equal(cnt_g.cpu(), cnt_c), f"counts after {msg}"
    assert int(cnt_c.max()) >= 2  # a penalised row drew a token again: the penalties were in play
