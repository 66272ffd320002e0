"""``logit_bias`` inside the sampler kernel (ops/csrc/sampling.hip: bias pairs staged in LDS, a binary search per
16-byte logit load) against ``ops.reference.sample_replay``, token for token: every row the replay does not flag
``ambiguous`` has exactly one right token. The tables are built by ``LogitsProcessor`` on both devices, as the engine
builds them. Biases are multiples of 1/8 and the logits stay within +-14, so ``|x + b| / T`` stays below 128 (the
replay's score band is then above ten fp32 ulps) and the bf16 rows' penalty and bias arithmetic is exact."""
import numpy as np
import pytest
import torch

from kafka_llm_service_amd import ops
from kafka_llm_service_amd.engine.logits_proc import LogitsProcessor
from kafka_llm_service_amd.engine.sequence import SamplingParams, Sequence
from kafka_llm_service_amd.engine.step_plan import LOGIT_BIAS_MAX
from kafka_llm_service_amd.ops import reference as ref

AMBIGUOUS_CAP = 0.02  # of a test's rows (the sampler suite's cap); asserted on the replay before the kernel runs
COUNTS = (1, 7, 300)
# (name, temperature, top_p, top_k)
MODES = (("greedy", 0.0, 1.0, 0), ("T 0.9", 0.9, 1.0, 0), ("top_p 0.9", 0.9, 0.9, 0), ("top_k 40 T 1.3", 1.3, 1.0, 40))


def _capped(rep, what):
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


def _ws(dev, B, nsplit):
    return torch.zeros(65536 + 2 * B * nsplit, dtype=torch.int32, device=dev)


def _bias(V: int, n: int, i: int, rng: np.random.Generator) -> dict:
    """Row i's logit_bias of min(n, V) entries. The ids start from the places where the kernel's indexing can go wrong
    — 0, V - 1, the last index of the vector part, the first tail index, two ids in one 8-vector — rotated by the row
    when n is too small for all of them, then random ids. A third of the rows stay within +-4 (the draw is not
    decided), another third carries one +100 and the last one -100."""
    n = min(n, V)
    v8 = V // 8 * 8
    a = (8 * (i % max(1, V // 8)) + 2) % max(1, v8 - 1) if v8 else 0
    must = [0, V - 1, max(v8 - 1, 0), min(v8, V - 1), a, min(a + 1, V - 1)]
    must = list(dict.fromkeys(must))
    must = must[i % len(must):] + must[:i % len(must)]
    ids = must[:n]
    if len(ids) < n:
        rest = np.setdiff1d(np.arange(V), ids)
        ids += rng.permutation(rest)[:n - len(ids)].tolist()
    lim = 32 if i % 3 == 0 else 400
    b = rng.integers(-lim, lim + 1, size=n) / 8.0
    b[b == 0] = 0.125
    if i % 3:  # the bounds themselves: -100 in one third of the rows, +100 in another (the other entries stay
        b[int(rng.integers(0, n))] = 100.0 if i % 3 == 2 else -100.0  # within +-50: a +100 decides its row)
    return {int(t): float(v) for t, v in zip(ids, b)}


def _logits(B, V, seed, dtype):
    return (torch.randn(B, V, generator=torch.Generator().manual_seed(seed)) * 3).clamp(-14, 14).to(dtype)


def _tables(dev, V, rows, B, **kw):
    lp = LogitsProcessor(dev, V, **kw)
    proc, upd = lp.build(rows, B)
    up = torch.from_numpy if str(dev) == "cpu" else (lambda a: torch.from_numpy(a).to(dev))
    lp.apply(upd, up)
    return lp, torch.from_numpy(proc).to(dev)


def _mode_args(B, mode, seed0):
    _, t, p, k = mode
    return (torch.full((B,), t), torch.full((B,), p) if p < 1 else None,
            torch.full((B,), k, dtype=torch.int32) if k else None, torch.arange(B, dtype=torch.long) * 13 + seed0)


# ---- ragged and small vocabularies ------------------------------------------------------------------------------------
def ragged_case(V, dtype):
    B = 20 * len(COUNTS)
    rng = np.random.default_rng(5 + V)
    biases = [_bias(V, COUNTS[i % 3], i // 3, rng) for i in range(B)]
    rows = [(i, Sequence(f"r{i}", [1], SamplingParams(logit_bias=b)), None) for i, b in enumerate(biases)]
    x = _logits(B, V, 31 + V, dtype)
    lp, proc = _tables("cpu", V, rows, B, max_slots=8, mask_rows=2, bias_rows=B)
    step = torch.tensor([3], dtype=torch.long)
    reps = []
    for mode in MODES:
        temp, tp, tk, seeds = _mode_args(B, mode, 1)
        rep = ref.sample_replay(x, temp, tp, tk, seeds, step, proc=proc, mask_tab=lp.tables()[0], nsplit=8,
                                bias_tab=lp.bias_table())
        reps.append((mode, rep, _capped(rep, f"V {V} {dtype} {mode[0]}")))
    return x, rows, biases, step, reps


@pytest.mark.gpu
@pytest.mark.parametrize("V", [9, 40, 1031, 16389])
def test_bias_ragged_vocab_matches_replay(cuda, V):
    """Entry counts 1, 7 and 300 (capped at V) in one batch, bf16 and fp32 rows with a padded stride whose padding
    holds the largest finite value, one workgroup and 8 splits, greedy / plain / top_p / top_k."""
    from kafka_llm_service_amd.ops._ext import ext

    for dtype in (torch.bfloat16, torch.float32):
        x, rows, biases, step, reps = ragged_case(V, dtype)
        B = x.shape[0]
        lp, proc = _tables(cuda, V, rows, B, max_slots=8, mask_rows=2, bias_rows=B)
        buf = torch.full((B, (V + 7) // 8 * 8 + 8), torch.finfo(dtype).max, dtype=dtype, device=cuda)
        buf[:, :V] = x.to(cuda)
        xg = buf[:, :V]
        forced = [(i, max(b, key=b.get)) for i, b in enumerate(biases) if max(b.values()) == 100.0]
        assert len(forced) >= B // 4
        for mode, rep, msg in reps:
            # a +100 entry decides its row (the logits span +-14) whatever the mode
            assert all(int(rep.tokens[i]) == t for i, t in forced), msg
            assert mode[0] != "greedy" or len(set(rep.tokens.tolist())) > 4
            temp, tp, tk, seeds = _mode_args(B, mode, 1)
            for nsplit in (1, 8):
                out = torch.full((B,), -1, dtype=torch.long, device=cuda)
                ext().sample(xg, temp.to(cuda), None if tp is None else tp.to(cuda), None if tk is None else tk.to(cuda),
                             seeds.to(cuda), step.to(cuda), out, _ws(cuda, B, nsplit), nsplit, proc, lp.tables()[0],
                             None, lp.bias_table())
                _same(out, rep, f"{msg}, nsplit {nsplit}")


# ---- combined processing at the full vocabulary -----------------------------------------------------------------------
def combined_case():
    """64 rows of 128,256 bf16 logits; the kind of a row is i % 8, its sampling mode (i // 8) % 4:
    0 bias only (1 entry), 1 bias + penalties, 2 bias + bitmask with a +100 id OUTSIDE the mask, 3 forced + bias,
    4 penalties only (no bias, between biased rows), 5 the object of row i - 5 again (two rows share a table row),
    6 bias + penalties + bitmask, 7 bias only (300 entries)."""
    B, V = 64, 128256
    x = _logits(B, V, 31, torch.bfloat16)
    rng = np.random.default_rng(5)
    temp = torch.tensor([MODES[(i // 8) % 4][1] for i in range(B)])
    topp = torch.tensor([MODES[(i // 8) % 4][2] for i in range(B)])
    topk = torch.tensor([MODES[(i // 8) % 4][3] for i in range(B)], dtype=torch.int32)
    seeds = torch.arange(B, dtype=torch.long) * 13 + 1
    rows, biases, banned = [], {}, {}
    g = torch.Generator().manual_seed(3)
    for i in range(B):
        kind = i % 8
        pen = dict(presence_penalty=0.5, frequency_penalty=1.5) if kind in (1, 4, 6) else {}
        bias = None
        if kind != 4:
            bias = biases[i - 5] if kind == 5 else _bias(V, (1, 7, 20, 7, 0, 0, 20, 300)[kind], i, rng)
        spec = None
        if kind in (2, 6):
            allowed = torch.randint(0, V, (int(torch.randint(50, 3000, (1,), generator=g)),), generator=g).tolist()
            if kind == 2:  # a +100 on a token the grammar does not allow: it must never be drawn
                out = next(t for t in range(1000 + i, V) if t not in set(allowed))
                bias = {**bias, out: 100.0}
                banned[i] = out
            spec = allowed
        elif kind == 3:
            spec = [int(torch.randint(0, V, (1,), generator=g))]
        biases[i] = bias
        rows.append((i, Sequence(f"c{i}", [1], SamplingParams(temperature=float(temp[i]) or 1.0, logit_bias=bias,
                                                              **pen)), spec))
    return x, rows, banned, (temp, topp, topk, seeds)


@pytest.mark.gpu
def test_bias_combined_processing_matches_replay(cuda):
    """Four successive steps with the count table carried along: tokens and counts equal the replay's after each."""
    x, rows, banned, (temp, topp, topk, seeds) = combined_case()
    B, V = x.shape
    lp_c, pd_c = _tables("cpu", V, rows, B, max_slots=64, mask_rows=32, bias_rows=64)
    lp_g, pd_g = _tables(cuda, V, rows, B, max_slots=64, mask_rows=32, bias_rows=64)
    assert torch.equal(pd_c, pd_g.cpu())
    p = pd_c.numpy()
    assert all(p[i, 5] == p[i - 5, 5] and p[i, 6] == p[i - 5, 6] > 0 for i in range(5, B, 8))  # a shared table row
    assert (p[4::8, 5:8] == 0).all() and (p[4::8, 2] >= 0).all() and (p[3::8, 0] == 2).all() and (p[3::8, 6] > 0).all()
    st = lp_c.stats  # (7 of 8 rows carry a bias; equal objects, the kind-5 rows' at least, cost one upload)
    assert st["bias_rows_used"] == 7 * (B // 8) and st["bias_uploads"] <= 6 * (B // 8)
    (mt_c, cnt_c), (mt_g, cnt_g) = lp_c.tables(), lp_g.tables()
    xg = x.to(cuda)
    dev = [t.to(cuda) for t in (temp, topp, topk, seeds)]
    for stepv in range(4):
        step = torch.tensor([stepv], dtype=torch.long)
        rep = ref.sample_replay(x, temp, topp, topk, seeds, step, proc=pd_c, mask_tab=mt_c, counts=cnt_c, nsplit=8,
                                bias_tab=lp_c.bias_table())
        msg = _capped(rep, f"combined step {stepv}")
        assert not bool(rep.ambiguous.any()), msg  # the count tables can only be compared when no row may differ
        assert torch.equal(rep.tokens[3::8], pd_c[3::8, 1].long())
        tok = ops.sample(xg, *dev, step.to(cuda), proc=pd_g, mask_tab=mt_g, counts=cnt_g, bias_tab=lp_g.bias_table())
        _same(tok, rep, msg)
        assert torch.equal(cnt_g.cpu(), cnt_c), f"counts after {msg}"
        assert all(int(tok[i]) != t for i, t in banned.items()), msg
    assert int(cnt_c.max()) >= 1 and int(cnt_c.sum()) == 4 * 3 * (B // 8)


# ---- one workgroup and 8 splits ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_bias_split_equality(cuda):
    """Greedy and plain-temperature rows with 1 / 7 / 300 entries: every split stages the same pairs, so 8 splits give
    the one-workgroup tokens (and the replay's)."""
    from kafka_llm_service_amd.ops._ext import ext

    B, V = 24, 128256
    rng = np.random.default_rng(7)
    rows = [(i, Sequence(f"s{i}", [1], SamplingParams(logit_bias=_bias(V, COUNTS[i % 3], i // 3 * 3, rng))), None)
            for i in range(B)]
    x = _logits(B, V, 33, torch.bfloat16)
    temp = torch.tensor([0.0, 0.0, 0.0, 0.9, 0.9, 0.9] * 4)
    seeds = torch.arange(B, dtype=torch.long) * 13 + 1
    step = torch.tensor([1], dtype=torch.long)
    lp_c, pd_c = _tables("cpu", V, rows, B, max_slots=8, mask_rows=2, bias_rows=B)
    rep = ref.sample_replay(x, temp, seeds=seeds, step=step, proc=pd_c, mask_tab=lp_c.tables()[0], nsplit=8,
                            bias_tab=lp_c.bias_table())
    msg = _capped(rep, "split equality")
    lp, proc = _tables(cuda, V, rows, B, max_slots=8, mask_rows=2, bias_rows=B)
    outs = []
    for nsplit in (1, 8):
        out = torch.full((B,), -1, dtype=torch.long, device=cuda)
        ext().sample(x.to(cuda), temp.to(cuda), None, None, seeds.to(cuda), step.to(cuda), out, _ws(cuda, B, nsplit),
                     nsplit, proc, lp.tables()[0], None, bias_tab=lp.bias_table())
        _same(out, rep, f"{msg}, nsplit {nsplit}")
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1])
    assert len(set(rep.tokens.tolist())) > B // 2


# ---- a table row overwritten between two launches ---------------------------------------------------------------------
@pytest.mark.gpu
def test_bias_table_row_update_between_launches(cuda):
    """A two-row table: the second step's new objects evict the first step's, ``apply`` rewrites the rows on the
    stream between the two launches, and the second launch samples with the new pairs."""
    B, V = 2, 16389
    x = _logits(B, V, 35, torch.bfloat16)
    buf = torch.zeros(B, (V + 7) // 8 * 8, dtype=x.dtype, device=cuda)  # (the kernel wants a row stride of 8 k)
    buf[:, :V] = x.to(cuda)
    xg = buf[:, :V]
    lp_c = LogitsProcessor("cpu", V, max_slots=8, mask_rows=2, bias_rows=2)
    lp_g = LogitsProcessor(cuda, V, max_slots=8, mask_rows=2, bias_rows=2)
    toks, reps, procs = [], [], []
    for stepv, sets in enumerate(([{5: 100.0, 9: 3.0}, {V - 1: 100.0}], [{16388 - 7: 100.0}, {12: 100.0, 5: -100.0}])):
        rows = [(i, Sequence(f"u{stepv}{i}", [1], SamplingParams(logit_bias=b)), None) for i, b in enumerate(sets)]
        proc, upd = lp_g.build(rows, B)
        proc_c, upd_c = lp_c.build(rows, B)
        assert upd.bias_rows.size == 2 and (proc == proc_c).all()
        lp_g.apply(upd, lambda a: torch.from_numpy(a).to(cuda))  # (stream-ordered: no synchronisation in between)
        lp_c.apply(upd_c, torch.from_numpy)
        pd_c = torch.from_numpy(proc)
        reps.append(ref.sample_replay(x, None, proc=pd_c, mask_tab=lp_c.tables()[0], nsplit=8,
                                      bias_tab=lp_c.bias_table()))
        toks.append(ops.sample(xg, proc=pd_c.to(cuda), mask_tab=lp_g.tables()[0], bias_tab=lp_g.bias_table()))
        procs.append(proc)
    assert sorted(procs[0][:, 5].tolist()) == sorted(procs[1][:, 5].tolist()) == [0, 1]  # the same two rows, rewritten
    assert reps[0].tokens.tolist() == [5, V - 1] and reps[1].tokens.tolist() == [16388 - 7, 12]
    assert toks[0].tolist() == [5, V - 1] and toks[1].tolist() == [16388 - 7, 12]


# ---- the launcher's checks --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_bias_table_checks(cuda):
    from kafka_llm_service_amd.ops._ext import ext

    B, V = 2, 64
    x = torch.zeros(B, V, device=cuda)
    proc = torch.zeros(B, 8, dtype=torch.int32, device=cuda)
    proc[:, 2] = -1
    mt = torch.zeros(1, 2, dtype=torch.int32, device=cuda)
    out = torch.empty(B, dtype=torch.long, device=cuda)
    with pytest.raises(RuntimeError):  # a leading dimension below 2 * LOGIT_BIAS_MAX
        ext().sample(x, None, None, None, None, None, out, None, 1, proc, mt, None,
                     torch.zeros(4, 2 * LOGIT_BIAS_MAX - 4, dtype=torch.int32, device=cuda))
    proc[1, 6] = 1
    with pytest.raises(ValueError):  # entries without a table: refused on the host
        ops.sample(x, proc=proc, mask_tab=mt)
    # all-zero ints 5..7 and no table: the processing path as every earlier caller builds it
    proc[1, 6] = 0
    assert ops.sample(x, proc=proc, mask_tab=mt).tolist() == [0, 0]
