"""Sampler reference self-checks (no GPU): the float64 survivor-set reference of sampler_ref.py
against oracle.sample, the 2 % undecided cap for the exact inputs test_sampler_gpu.py launches, the
distribution of the Philox/Gumbel scheme, the oracle at the edges the kernel has to match, and a
float32 model of sample_topkp_kernel showing which wrong kernels the GPU cases catch."""

import numpy as np
import pytest
import torch

import sampler_ref as sr
from llm_consensus_amd import ops
from llm_consensus_amd.ops import oracle

ALL_CASES = sr.all_cases()
CASES = {c.name: c for c in ALL_CASES}


def test_case_names_unique():
    assert len(CASES) == len(ALL_CASES)


# -- survivor sets --------------------------------------------------------------------------------
def test_nucleus_survivor_counts():
    """0.05 / 0.35 / 0.55 / 0.95 of ten ~0.1 masses leave exactly 1, 4, 6, 10 tokens, with no band
    between must and may; inside top_k = 3 the mass is renormalised (2 survivors, not 3)."""
    row, live = sr.support_row(0.01)
    for it in (1.0, 0.5, 2.0):
        for p, n in zip(sr.NUCLEUS_PS, sr.NUCLEUS_SURVIVORS):
            must, may = sr.survivor_sets(row, it, 0, p)
            assert np.array_equal(must, may) and int(must.sum()) == n, (it, p, int(must.sum()), int(may.sum()))
            want = live[:n]  # live[j] holds 2.0 - 0.01 * j
            assert set(np.flatnonzero(must)) == set(want)
    must, may = sr.survivor_sets(row, 1.0, 3, 0.55)
    assert np.array_equal(must, may) and set(np.flatnonzero(must)) == set(live[:2])


def test_survivor_sets_rules():
    row = torch.tensor([0.5, 2.0, 1.0, 2.0, 1.0, -1.0, 1.0])
    # top-k keeps every tie at the k-th value
    must, may = sr.survivor_sets(row, 1.0, 3, 1.0)
    assert must.tolist() == may.tolist() == [False, True, True, True, True, False, True]
    # top_p <= 0: exactly the top-1 tie group
    for p in (0.0, -0.5):
        must, may = sr.survivor_sets(row, 1.0, 0, p)
        assert must.tolist() == may.tolist() == [False, True, False, True, False, False, False]
    # greedy rows and top_p >= 1 skip the top-p rule; k outside (0, V) is no filter
    for it, k, p in ((0.0, 0, 0.1), (1.0, 0, 1.0), (1.0, 7, 1.0), (1.0, 12, 1.0), (1.0, -3, 1.0)):
        must, may = sr.survivor_sets(row, it, k, p)
        assert must.all() and may.all()
    # the band: a bound placed exactly on a cumulative mass splits must from may
    r = np.array([0.0, -1.0, -2.0])
    w = np.exp(r)
    p_edge = w[0] / w.sum()  # mass strictly above element 1 == p * z
    must, may = sr.survivor_sets(r, 1.0, 0, p_edge)
    assert must.tolist() == [True, False, False] and may.tolist() == [True, True, False]


def test_expected_tokens_greedy_and_gap():
    row = torch.tensor([1.0, 3.0, 3.0, 2.0])
    assert sr.expected_tokens(row, 0.0, 0, 1.0, 5, 0) == (1, 1, float("inf"))
    t_must, t_may, gap = sr.expected_tokens(row, 1.0, 0, 1.0, 5, 9)
    s = row.double().numpy() + sr.gumbel64(5, np.arange(4), 9)
    top = np.sort(s)
    assert t_must == t_may == int(np.argmax(s)) and gap == pytest.approx(top[-1] - top[-2])


# -- the undecided cap, for the exact GPU inputs --------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_undecided_cap_and_oracle_agreement(name):
    """At most 2 % of a case's rows are undecided, and oracle.sample returns the expected token on
    every decided row."""
    case = CASES[name]
    ex = sr.expectation(case)
    und = sum(not e.decided for e in ex)
    print(f"{name}: {und} of {case.B} rows undecided")
    # a launch of fewer than 50 rows has no room for an undecided row under the cap
    assert und <= sr.UNDECIDED_CAP * case.B, (name, und, case.B)
    it, tk, tp, seeds, pos = sr.case_tensors(case)
    ref = oracle.sample(case.row.unsqueeze(0).expand(case.B, case.V), it, tk, tp, seeds, pos)
    bad = [(b, int(ref[b]), e.tok) for b, e in enumerate(ex) if e.decided and int(ref[b]) != e.tok]
    assert not bad, bad[:5]
    sr.check_tokens(case, ref.tolist())


def test_radix_cases_hold_boundary_rows():
    """Every radix case has rows whose winner is the k-th element and rows where the (k+1)-th would
    win if it were kept: the rows that tell k from k - 1 and k + 1."""
    for neg in (True, False):
        for k in sr.RADIX_KS:
            at_k, past_k = sr.radix_boundary_rows(neg, k)
            assert at_k >= 2 and past_k >= 2, (neg, k, at_k, past_k)


def test_tie_and_zero_cases_draw_every_tie():
    row, ties = sr.tie_row()
    drawn = {e.tok for e in sr.expectation(sr.tie_case())}
    assert set(ties) <= drawn and all(float(row[t]) >= 1.0 for t in drawn)
    row, zeros = sr.zero_row()
    drawn = {e.tok for e in sr.expectation(sr.zero_case())}
    assert set(zeros) <= drawn and all(float(row[t]) >= 0.0 for t in drawn)


def test_advance_rows_are_decided():
    for topkp in (False, True):
        assert all(sr.advance_rows_decided(topkp))


# -- the Philox / Gumbel scheme -------------------------------------------------------------------
def test_philox_np_matches_oracle():
    idx = np.arange(0, 3000, 7)
    for seed, pos in ((0, 0), (77, 15), (-1, 3), (-(1 << 63), (1 << 31) - 1), ((1 << 63) - 1, 1 << 24)):
        a = oracle.philox_draw(seed, torch.from_numpy(idx), pos).numpy().astype(np.uint64)
        b = sr.philox_np(np.array([seed]), idx, np.array([pos]))
        assert np.array_equal(a, b)
    # a negative seed is its two's complement: both words of the key are used
    i8 = torch.arange(8)
    assert torch.equal(oracle.philox_draw(-1, i8, 0), oracle.philox_draw((1 << 64) - 1, i8, 0))
    assert not torch.equal(oracle.philox_draw(5, i8, 0), oracle.philox_draw(5 + (1 << 32), i8, 0))
    assert not torch.equal(oracle.philox_draw(5, i8, 0), oracle.philox_draw(5, i8, 1 << 31))


def test_saturated_draw_gives_infinite_gumbel():
    """A Philox word with its top 24 bits set gives 0xFFFFFF + 0.5, which float32 rounds to 2^24:
    u = 1, the Gumbel is +inf and that index wins whatever its logit. This is what kernel and oracle
    do today (sampler_ref.SATURATED_DRAWS), stated here so that a change of the mapping shows."""
    case = sr.saturated_case()
    for b, (seed, pos, idx) in enumerate(sr.SATURATED_DRAWS):
        assert int(oracle.philox_draw(seed, torch.tensor([idx]), pos)) >> 8 == 0xFFFFFF
        assert float(oracle.gumbel(seed, torch.tensor([idx]), pos)) == float("inf")
        assert float(case.row[idx]) == -30.0 and sr.expectation(case)[b].tok == idx


def test_gumbel_max_distribution_chi_square():
    """4096 draws (256 seeds x 16 positions) over a 10-token support inside V = 1500: Pearson
    chi-square against the softmax, 9 degrees of freedom, below the 0.1 % point 27.88; nothing
    lands outside the support."""
    V = 1500
    live = np.random.RandomState(31).permutation(V)[:10]
    row = torch.full((V,), -30.0)
    row[torch.from_numpy(live)] = 2.0 - 0.25 * torch.arange(10, dtype=torch.float32)
    seeds = torch.tensor([77 + s for s in range(256) for _ in range(16)], dtype=torch.int64)
    pos = torch.tensor([t for _ in range(256) for t in range(16)], dtype=torch.int32)
    n = seeds.numel()
    tok = oracle.sample(row.unsqueeze(0).expand(n, V), torch.ones(n), torch.zeros(n, dtype=torch.int32), torch.ones(n),
                        seeds, pos).numpy()
    assert np.isin(tok, live).all()
    prob = torch.softmax(row.double(), 0).numpy()[live]
    prob = prob / prob.sum()  # the other 1490 tokens carry 2e-11 of the mass
    obs = np.array([(tok == t).sum() for t in live])
    chi2 = float(((obs - n * prob) ** 2 / (n * prob)).sum())
    print("chi-square", chi2)
    assert chi2 < 27.88


# -- the oracle at the edges ------------------------------------------------------------------------
def _oracle1(row, it, k, p, seed=3, pos=4):
    return int(oracle.sample(row.unsqueeze(0), torch.tensor([it]), torch.tensor([k], dtype=torch.int32),
                             torch.tensor([p]), torch.tensor([seed], dtype=torch.int64),
                             torch.tensor([pos], dtype=torch.int32))[0])


def test_oracle_top_p_at_or_below_zero_is_top1():
    row = sr.random_row(5000, 2.0, 24)
    top = int(row.argmax())
    for p in (0.0, -0.5):
        for k in (0, 40):
            for seed in range(8):
                assert _oracle1(row, 1.0, k, p, seed=seed) == top


def test_oracle_top_k_edges():
    row = sr.random_row(300, 2.0, 32)
    V = row.numel()
    order = torch.argsort(row, descending=True)
    smallest = int(order[-1])
    row2 = row.clone()
    row2[smallest] = row[order[0]] + 40.0  # would win every draw if it survived ...
    for seed in range(16):
        assert _oracle1(row, 1.0, 1, 1.0, seed=seed) == int(order[0])
        free = _oracle1(row, 1.0, 0, 1.0, seed=seed)
        for k in (V, V + 5, -3):
            assert _oracle1(row, 1.0, k, 1.0, seed=seed) == free
    # ... and V - 1 drops exactly the smallest element
    low = row.clone()
    low[smallest] = row[order[-2]] - 1e-3
    for seed in range(16):
        must, _ = sr.survivor_sets(low, 1.0, V - 1, 1.0)
        assert int(must.sum()) == V - 1 and not must[smallest]
        assert _oracle1(low, 1.0, V - 1, 1.0, seed=seed) == sr.expected_tokens(low, 1.0, V - 1, 1.0, seed, 4)[1]
    assert _oracle1(row2, 1.0, V, 1.0) == smallest


def test_oracle_all_nan_row_returns_zero():
    row = torch.full((64,), float("nan"))
    for it, k, p in ((0.0, 0, 1.0), (1.0, 0, 1.0), (1.0, 5, 0.9), (1.0, 0, 0.0)):
        assert _oracle1(row, it, k, p) == 0
    # through ops.sample on CPU tensors, next to an ordinary row
    logits = torch.stack([sr.random_row(64, 2.0, 33), row])
    nxt = torch.full((2,), -1, dtype=torch.int32)
    ops.sample(logits, torch.ones(2), torch.zeros(2, dtype=torch.int32), torch.ones(2),
               torch.tensor([1, 2], dtype=torch.int64), torch.tensor([0, 0], dtype=torch.int32), nxt)
    assert 0 <= int(nxt[0]) < 64 and int(nxt[1]) == 0


# -- a float32 model of sample_topkp_kernel, and the wrong kernels the cases catch -------------------
def _fkey(r32: np.ndarray, bug=None) -> np.ndarray:
    u = r32.view(np.uint32).copy()
    if bug != "signed_zero":
        u[u == 0x80000000] = 0
    if bug == "no_negative_flip":
        return u | np.uint32(0x80000000)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _model_survivors(r32: np.ndarray, it: float, k: int, p: float, bug=None) -> np.ndarray:
    V = r32.size
    keys = _fkey(r32, bug)
    greedy = it <= 0
    it = np.float32(1.0 if greedy else it)
    thr = np.uint32(0)
    if 0 < k < V:
        desc = np.sort(keys)[::-1]
        kk = {"one_too_few": k - 1, "one_too_many": k + 1}.get(bug, k)
        thr = desc[max(kk, 1) - 1]
        if bug == "ties_dropped" and (keys >= thr).sum() > k:
            thr = thr + np.uint32(1)
    if p < 1.0 and not greedy and bug != "top_p_ignored":
        with np.errstate(invalid="ignore", over="ignore"):
            m = np.exp((r32 - r32.max()) * it).astype(np.float32)
        live = keys >= thr
        z = (m if bug == "not_renormalised" else m[live]).sum(dtype=np.float32)
        rem = np.float32(p) * z
        order = np.argsort(keys[live], kind="stable")[::-1]
        ks, ms = keys[live][order], m[live][order]
        starts = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
        gm = np.add.reduceat(ms, starts).astype(np.float32)
        thr2 = np.uint32(0)
        if bug == "top_p_le0_unfixed" and rem <= 0:
            thr2 = np.uint32(0xFFFFFFFF)
        else:
            for g in range(starts.size):
                if gm[g] >= rem and gm[g] > 0:
                    g = min(g + 1, starts.size - 1) if bug == "threshold_one_late" else g
                    thr2 = ks[starts[g]]
                    break
                rem = np.float32(rem - gm[g])
        thr = max(thr, thr2)
    return keys >= thr


def model_tokens(case, bug=None):
    """Tokens of a float32 model of the top-k/top-p launch (sorting stands in for the radix passes)."""
    r32 = case.row.numpy()
    idx = torch.arange(case.V)
    sets, out = {}, []
    for b in range(case.B):
        it, k, p = float(case.inv_temp[b]), int(case.top_k[b]), float(case.top_p[b])
        if (it, k, p) not in sets:
            sets[(it, k, p)] = _model_survivors(r32, it, k, p, bug)
        keep = sets[(it, k, p)]
        if it <= 0:
            v = r32.copy()
        else:
            step = 0 if bug == "step_ignored" else int(case.pos[b])
            v = r32 * np.float32(it) + oracle.gumbel(case.seeds[b], idx, step).numpy()
        v = np.where(keep, v, -np.inf).astype(np.float32)
        if not keep.any() or np.isnan(v.max()):
            out.append(0 if bug != "no_survivor_unfixed" else 0x7FFFFFFF)
            continue
        hits = np.flatnonzero(v == v.max())
        out.append(int(hits[-1] if bug == "tie_to_larger_index" else hits[0]))
    return out


MODEL_CASES = [c.name for c in ALL_CASES if c.V <= 5000 and "topkp" in c.launches]


@pytest.mark.parametrize("name", MODEL_CASES)
def test_float32_model_passes(name):
    """A correct float32 kernel satisfies the decided-row rule on every case."""
    sr.check_tokens(CASES[name], model_tokens(CASES[name]))


# wrong kernel -> a case that must reject it
SENSITIVITY = [
    ("threshold_one_late", "nucleus-p0.35-it1.0"),
    ("threshold_one_late", "nucleus-p0.05-it2.0"),
    ("top_p_ignored", "nucleus-p0.55-it0.5"),
    ("top_p_ignored", "random-V5000-k700-p0.97"),
    ("not_renormalised", "nucleus-k3-p0.55"),
    ("step_ignored", "nucleus-p0.95-it1.0"),
    ("no_negative_flip", "radix-neg-k255-gumbel"),
    ("no_negative_flip", "radix-neg-k2-greedy"),
    ("no_negative_flip", "mixed-k700"),
    ("one_too_few", "radix-neg-k256-gumbel"),
    ("one_too_many", "radix-neg-k256-gumbel"),
    ("one_too_few", "radix-pos-k257-gumbel"),
    ("one_too_many", "radix-pos-k1499-gumbel"),
    ("one_too_many", "radix-pos-k1-gumbel"),
    ("ties_dropped", "ties-at-k"),
    ("signed_zero", "signed-zero-at-k"),
    ("top_p_le0_unfixed", "degenerate-p0.0-k0"),
    ("top_p_le0_unfixed", "degenerate-p-0.5-k40"),
]


@pytest.mark.parametrize("bug,name", SENSITIVITY)
def test_wrong_kernels_are_caught(bug, name):
    case = CASES[name]
    toks = model_tokens(case, bug)
    with pytest.raises(AssertionError):
        sr.check_tokens(case, toks)
    ex = sr.expectation(case)
    wrong = sum(e.decided and t != e.tok for t, e in zip(toks, ex))
    print(f"{bug} on {name}: {wrong} of {case.B} decided rows wrong")


def test_out_of_range_id_is_caught():
    """What the kernel wrote for top_p <= 0 and all-NaN rows before it was fixed."""
    case = CASES["degenerate-p0.0-k0"]
    with pytest.raises(AssertionError, match="outside"):
        sr.check_tokens(case, [0x7FFFFFFF] * case.B)
