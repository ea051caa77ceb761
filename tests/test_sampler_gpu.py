"""Sampler kernels (csrc/kernels/sampler.hip) against the float64 reference of sampler_ref.py.

Every case is one ops.sample launch over B rows that share a logits row and differ in seed and
position, checked row by row with the decided-row rule (sampler_ref.check_tokens):
test_sampler_cpu.py shows on the CPU that each case keeps within the 2 % undecided cap and which
wrong kernels each group rejects. Every token read back must lie in [0, V)."""

import numpy as np
import pytest
import torch

import sampler_ref as sr
from llm_consensus_amd import ops

pytestmark = pytest.mark.gpu


def _bufs(B):
    P = ops.sample_parts()
    return (torch.empty(B, P, device="cuda"), torch.empty(B, P, dtype=torch.int32, device="cuda"),
            torch.full((B,), -1, dtype=torch.int32, device="cuda"))


def _read(nxt, V):
    toks = nxt.cpu().tolist()
    assert all(0 <= t < V for t in toks), f"token id outside [0, {V}): {[t for t in toks if not 0 <= t < V][:5]}"
    return toks


def _launch(case, launch, logits=None):
    """One bare ops.sample launch of a case ('fast' = the two-stage argmax, 'topkp' = the
    top-k/top-p kernel); the positions must come back unchanged."""
    it, tk, tp, seeds, pos = sr.case_tensors(case, "cuda")
    if logits is None:
        logits = case.row.cuda().unsqueeze(0).expand(case.B, case.V).contiguous()
    wv, wi, nxt = _bufs(case.B)
    ops.sample(logits, it, tk, tp, seeds, pos, nxt, wv, wi, use_topkp=launch == "topkp")
    toks = _read(nxt, case.V)
    assert pos.cpu().tolist() == case.pos.tolist(), "a bare call moved the position"
    return toks


def _run(case):
    out = {}
    for launch in case.launches:
        out[launch] = _launch(case, launch)
        sr.check_tokens(case, out[launch])
    return out


def _ids(cases):
    return [c.name for c in cases]


# -- nucleus exactness ------------------------------------------------------------------------------
NUCLEUS = sr.nucleus_cases()


@pytest.mark.parametrize("case", NUCLEUS, ids=_ids(NUCLEUS))
def test_nucleus_exact_survivors(cuda, case):
    """Ten ~0.1 masses: top_p of 0.05 / 0.35 / 0.55 / 0.95 leaves exactly 1 / 4 / 6 / 10 tokens
    (must == may, so every row is pinned up to its Gumbel gap); each survivor is drawn about B / n
    times, so a threshold one token early or late fails on dozens of rows."""
    toks = _run(case)["topkp"]
    must, may = sr.survivor_sets(case.row, float(case.inv_temp[0]), int(case.top_k[0]), float(case.top_p[0]))
    assert np.array_equal(must, may)
    assert set(toks) <= set(np.flatnonzero(must).tolist())
    if case.name != "nucleus-k3-p0.55":
        n = sr.NUCLEUS_SURVIVORS[sr.NUCLEUS_PS.index(round(float(case.top_p[0]), 2))]
        assert int(must.sum()) == n
        if n > 1 and float(case.inv_temp[0]) == 1.0:
            assert len(set(toks)) == n  # every survivor is drawn over the 256 rows


# -- radix-select edges -----------------------------------------------------------------------------
RADIX = sr.radix_cases()


@pytest.mark.parametrize("case", RADIX, ids=_ids(RADIX))
def test_radix_select_edges(cuda, case):
    """Consecutive floats that differ in the low two bytes (negative and positive), a row with
    negatives, positives and -inf, a +inf entry, and top_k at and beyond V, with top_p = 1 and
    greedy. The radix cases carry rows whose winner is the k-th element and rows whose winner would
    be the (k+1)-th."""
    out = _run(case)
    if case.name.startswith("inf-"):
        for toks in out.values():
            assert set(toks) == {sr.INF_INDEX}


def test_top_k_outside_range_is_no_filter(cuda):
    toks = [_launch(c, "topkp") for c in RADIX if c.name.startswith("nofilter-")]
    assert len(toks) == 4 and all(t == toks[0] for t in toks)


def test_top_k_keeps_all_ties(cuda):
    """The k-th value five times: each of the five is drawn, nothing below it is."""
    case = sr.tie_case()
    toks = _run(case)["topkp"]
    row, ties = sr.tie_row()
    assert set(ties.tolist()) <= set(toks)
    assert all(float(row[t]) >= 1.0 for t in toks)


def test_top_k_keeps_zeros_of_either_sign(cuda):
    """The k-th value is zero: -0.0 == +0.0, so `row >= kth` keeps the zeros of both signs."""
    case = sr.zero_case()
    toks = _run(case)["topkp"]
    row, zeros = sr.zero_row()
    assert set(zeros.tolist()) <= set(toks)
    assert all(float(row[t]) >= 0.0 for t in toks)


# -- random rows ------------------------------------------------------------------------------------
RANDOM = sr.random_cases()


@pytest.mark.parametrize("case", RANDOM, ids=_ids(RANDOM))
def test_random_rows(cuda, case):
    _run(case)


# -- path agreement ---------------------------------------------------------------------------------
def test_paths_agree_without_filters(cuda):
    """top_k = 0, top_p = 1 through the top-k/top-p kernel (what a mixed batch does in
    Engine._sample) yields the token of the two-stage launch."""
    case = sr.agreement_case()
    out = _run(case)
    ex = sr.expectation(case)
    diff = [b for b, e in enumerate(ex) if e.decided and out["fast"][b] != out["topkp"][b]]
    assert not diff, diff[:5]


def test_mixed_batch(cuda):
    _run(sr.mixed_batch_case())


# -- fast path --------------------------------------------------------------------------------------
FAST = sr.fast_shape_cases() + [sr.fast_large_case(), sr.edge_seed_case(), sr.saturated_case()]


@pytest.mark.parametrize("case", FAST, ids=_ids(FAST))
def test_fast_path(cuda, case):
    """V around the 64 stage-1 parts and the 256-thread stride, B of 1 / 3 / 32, V = 128256, seeds
    with bits above 2^31 and negative seeds, positions up to 2^31 - 1, and draws whose Philox word
    saturates the 24-bit uniform (u = 1, Gumbel +inf: that index wins, in kernel and oracle alike)."""
    _run(case)


def test_greedy_ties_lowest_index_wins(cuda):
    """The maximum duplicated across threads, waves and stage-1 parts: the lowest index wins on
    both launches."""
    V, B = 5000, 3
    P = ops.sample_parts()
    per = (V + P - 1) // P  # stage-1 part p covers [p * per, (p + 1) * per)
    mid = P // 2
    assert per > 70 and (P - 1) * per < V
    groups = [(0, mid * per, (P - 1) * per),  # first index of part 0, of a middle part, of the last
              (mid * per + 3, mid * per + 70, (P - 1) * per),  # two waves of one part, and a later part
              ((P - 1) * per, (P - 1) * per + 20, V - 1),  # inside the last part
              (7, 7 + 1024, 7 + 4096)]  # one thread of the 1024-thread kernel, three strides
    base = sr.random_row(V, 3.0, 28)
    for idx in groups:
        row = base.clone()
        row[list(idx)] = float(base.max()) + 1.0
        for launch in ("fast", "topkp"):
            case = sr.make_case(f"greedy-ties-{idx}", row, B, inv_temp=0.0, seed_base=140)
            assert _launch(case, launch) == [min(idx)] * B, (idx, launch)
        case = sr.make_case(f"greedy-ties-k2-{idx}", row, B, inv_temp=0.0, top_k=2, seed_base=140)
        assert _launch(case, "topkp") == [min(idx)] * B, idx


def test_strided_logits_skip_the_padding(cuda):
    """A [B, V] view of a [B, V + 37] buffer whose padding columns hold +inf."""
    case = sr.strided_case()
    buf = torch.full((case.B, case.V + 37), float("inf"), device="cuda")
    buf[:, :case.V] = case.row.cuda()
    view = buf[:, :case.V]
    assert view.stride(0) == case.V + 37
    for launch in case.launches:
        sr.check_tokens(case, _launch(case, launch, logits=view))


# -- state advance ----------------------------------------------------------------------------------
def _advance_run(device, topkp):
    logits, bt_full, it, tk, tp, seeds = [t.to(device) for t in sr.advance_inputs(topkp)]
    bt = bt_full[:, :5]
    assert bt.stride(0) == 8
    st = sr.advance_state(device)
    out_tokens = st["out_full"][:sr.ADV_B]
    ws = _bufs(sr.ADV_B) if device == "cuda" else (None, None, torch.empty(sr.ADV_B, dtype=torch.int32))
    snaps = []
    for _ in range(3):
        ops.sample(logits, it, tk, tp, seeds, st["positions"], ws[2], ws[0], ws[1], tokens_in=st["tokens_in"],
                   seq_lens=st["seq_lens"], slots=st["slots"], block_tables=bt, bs=sr.ADV_BS, out_tokens=out_tokens,
                   out_count=st["out_count"], use_topkp=topkp)
        snap = {k: v.cpu().clone() for k, v in st.items()}
        snap["next"] = ws[2].cpu().clone()
        snaps.append(snap)
    return snaps, bt_full


@pytest.mark.parametrize("topkp", [False, True], ids=["fast", "topkp"])
def test_state_advance_matches_cpu(cuda, topkp):
    """Three consecutive calls against ops.sample on CPU tensors (oracle.sample + _advance_cpu):
    a non-identity block table passed as a strided slice, block-boundary crossings at different
    calls, and cap = 2, so the third call only counts."""
    ref, bt_full = _advance_run("cpu", topkp)
    got, _ = _advance_run("cuda", topkp)
    for call, (g, r) in enumerate(zip(got, ref)):
        _read(g["next"], sr.ADV_V)
        for k in r:
            assert torch.equal(g[k], r[k]), (call, k, g[k].tolist(), r[k].tolist())
    last = got[-1]
    assert last["positions"].tolist() == [p + 3 for p in sr.ADV_START]
    assert last["seq_lens"].tolist() == [p + 4 for p in sr.ADV_START]
    assert last["slots"].tolist() == [int(bt_full[b, (p + 3) // sr.ADV_BS]) * sr.ADV_BS + (p + 3) % sr.ADV_BS
                                      for b, p in enumerate(sr.ADV_START)]
    # cap = 2: counted, not written; the next row's tokens and the guard row are untouched
    assert last["out_count"].tolist() == [3] * sr.ADV_B
    assert torch.equal(last["out_full"], got[1]["out_full"])
    assert last["out_full"][sr.ADV_B].tolist() == [sr.ADV_SENTINEL] * sr.ADV_CAP
    assert last["out_full"][:sr.ADV_B, 0].tolist() == got[0]["next"].tolist()
    assert last["out_full"][:sr.ADV_B, 1].tolist() == got[1]["next"].tolist()
    assert last["tokens_in"].tolist() == last["next"].tolist()


@pytest.mark.parametrize("topkp", [False, True], ids=["fast", "topkp"])
def test_bare_call_moves_nothing(cuda, topkp):
    """tokens_in=None: no state array changes, even when all the others are passed, and two calls
    return the same token."""
    logits, bt_full, it, tk, tp, seeds = [t.cuda() for t in sr.advance_inputs(topkp)]
    st = sr.advance_state("cuda")
    before = {k: v.cpu().clone() for k, v in st.items()}
    wv, wi, nxt = _bufs(sr.ADV_B)
    toks = []
    for _ in range(2):
        ops.sample(logits, it, tk, tp, seeds, st["positions"], nxt, wv, wi, tokens_in=None, seq_lens=st["seq_lens"],
                   slots=st["slots"], block_tables=bt_full[:, :5], bs=sr.ADV_BS, out_tokens=st["out_full"][:sr.ADV_B],
                   out_count=st["out_count"], use_topkp=topkp)
        toks.append(_read(nxt, sr.ADV_V))
        for k, v in before.items():
            assert torch.equal(st[k].cpu(), v), k
    assert toks[0] == toks[1]


# -- degenerate rows --------------------------------------------------------------------------------
DEGENERATE = sr.degenerate_cases()


@pytest.mark.parametrize("case", DEGENERATE, ids=_ids(DEGENERATE))
def test_top_p_at_or_below_zero_is_top1(cuda, case):
    """top_p <= 0 keeps the top-1 of the top-k set, as oracle.sample does (the kernel used to keep
    nothing and write 0x7fffffff)."""
    toks = _run(case)["topkp"]
    assert toks == [int(case.row.argmax())] * case.B


@pytest.mark.parametrize("launch,k,p", [("fast", 0, 1.0), ("topkp", 0, 1.0), ("topkp", 40, 0.9), ("topkp", 0, 0.0)])
@pytest.mark.parametrize("it", [0.0, 1.0])
def test_all_nan_row_returns_zero(cuda, launch, k, p, it):
    """An all-NaN row yields id 0 (never an id outside [0, V)) and leaves its neighbours alone."""
    V = 1000
    row = sr.random_row(V, 3.0, 29)
    case = sr.make_case(f"nan-{launch}-{k}-{p}-{it}", row, 3, inv_temp=it, top_k=k, top_p=p, seed_base=150)
    logits = row.cuda().unsqueeze(0).repeat(3, 1)
    logits[1] = float("nan")
    toks = _launch(case, launch, logits=logits)
    assert toks[1] == 0
    ex = sr.expectation(case)
    assert all(e.decided for e in ex)
    assert [toks[0], toks[2]] == [ex[0].tok, ex[2].tok]
