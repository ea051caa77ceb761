"""Float64 reference for the sampler kernels (csrc/kernels/sampler.hip) and the shared inputs of
test_sampler_cpu.py / test_sampler_gpu.py.

The reference states which tokens MUST and which MAY survive top-k / top-p (`survivor_sets`), and
which token Gumbel-max then picks (`expected_tokens`). A row is *decided* when the pick is the same
over both sets and the runner-up is at least GAP behind; a decided row pins the kernel's token
exactly. Every GPU case is a `Case`: one logits row shared by B rows of a single launch that differ
in seed and position, so the CPU file can prove the 2 % undecided cap for the very inputs the GPU
file launches.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from llm_consensus_amd.ops import oracle

# Relative slack on the top-p bound: covers the kernel's float32 __expf, atomic-order sums and the
# `rem -= mass[bin]` walk (<= 1020 subtractions of <= 0.5 ulp(rem) each is 6e-5 relative).
DELTA = 1e-4
# Score tolerance test_sample_greedy_and_gumbel already grants the kernel's fast-math __logf.
GAP = 1e-3
UNDECIDED_CAP = 0.02


# -- reference -----------------------------------------------------------------------------------
def _f64(row) -> np.ndarray:
    if isinstance(row, torch.Tensor):
        row = row.detach().cpu().numpy()
    return np.asarray(row, dtype=np.float64)


def survivor_sets(row, inv_temp: float, top_k: int, top_p: float, delta: float = DELTA):
    """Boolean masks (must, may) over the row, in float64.

    top-k keeps `row >= kth largest` (all ties at the k-th value); top-p keeps an element iff the
    mass exp((l - max) * inv_temp) of the strictly larger top-k survivors is below top_p * z, with
    the bound scaled by (1 - delta) for `must` and (1 + delta) for `may`. The top element always
    survives, so top_p <= 0 leaves exactly the top-1 tie group. Greedy rows and top_p >= 1 skip the
    top-p rule, as the kernel and the oracle do."""
    r = _f64(row)
    V = r.size
    keep = np.ones(V, dtype=bool)
    if 0 < top_k < V:
        kth = np.partition(r, V - top_k)[V - top_k]
        keep = r >= kth
    if not (inv_temp > 0 and top_p < 1.0):
        return keep, keep.copy()
    m = r.max()
    with np.errstate(invalid="ignore"):
        w = np.where(keep, np.exp((r - m) * inv_temp), 0.0)
    order = np.argsort(-r, kind="stable")
    rs = r[order]
    cum = np.concatenate([[0.0], np.cumsum(w[order])])
    z = cum[-1]
    first = np.searchsorted(-rs, -rs, side="left")  # start of each element's tie group
    larger = np.empty(V)
    larger[order] = cum[first]  # mass of the strictly larger survivors
    top = keep & (r == m)
    must = (keep & (larger < top_p * z * (1.0 - delta))) | top
    may = (keep & (larger < top_p * z * (1.0 + delta))) | top
    return must, may


def gumbel64(seed: int, idx: np.ndarray, pos: int) -> np.ndarray:
    return oracle.gumbel(int(seed), torch.from_numpy(np.asarray(idx, dtype=np.int64)), int(pos)).double().numpy()


def _scores(r: np.ndarray, idx: np.ndarray, inv_temp: float, seed: int, pos: int) -> np.ndarray:
    if inv_temp <= 0:
        return r[idx]
    return r[idx] * float(inv_temp) + gumbel64(seed, idx, pos)


def _best(s: np.ndarray) -> Tuple[int, float]:
    """(position of the max, lowest index on ties; gap to the runner-up)."""
    j = int(np.argmax(s))
    if s.size == 1:
        return j, float("inf")
    rest = np.delete(s, j)
    with np.errstate(invalid="ignore"):
        return j, float(s[j] - rest.max())


def expected_tokens(row, inv_temp: float, top_k: int, top_p: float, seed: int, pos: int, sets=None):
    """(token over `must`, token over `may`, gap between the best two scores in `may`) with scores
    l * inv_temp + gumbel(seed, idx, pos) in float64; greedy rows (inv_temp <= 0) score l alone,
    lowest index on ties, and their gap is reported as inf: no fast-math enters a greedy pick, so
    it is exact whatever the runner-up."""
    r = _f64(row)
    must, may = sets if sets is not None else survivor_sets(r, inv_temp, top_k, top_p)
    i_must, i_may = np.flatnonzero(must), np.flatnonzero(may)
    s_may = _scores(r, i_may, inv_temp, seed, pos)
    j, gap = _best(s_may)
    if i_must.size == i_may.size:
        t_must = int(i_may[j])
    else:
        t_must = int(i_must[_best(_scores(r, i_must, inv_temp, seed, pos))[0]])
    if inv_temp <= 0:
        gap = float("inf")
    return t_must, int(i_may[j]), gap


def is_decided(t_must: int, t_may: int, gap: float) -> bool:
    return t_must == t_may and gap >= GAP


# -- cases ---------------------------------------------------------------------------------------
def mix_seed(n: int) -> int:
    """Spread n over all 64 bits (high word set, about half of them negative as int64)."""
    u = ((n + 1) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    return u - (1 << 64) if u >> 63 else u


@dataclass
class Case:
    name: str
    row: torch.Tensor  # [V] float32
    inv_temp: np.ndarray  # [B] float32
    top_k: np.ndarray  # [B] int32
    top_p: np.ndarray  # [B] float32
    seeds: List[int]  # [B] signed 64-bit
    pos: np.ndarray  # [B] int32 (as int64 array)
    launches: Tuple[str, ...] = ("topkp",)  # which launches the GPU file sends it through

    @property
    def B(self) -> int:
        return len(self.seeds)

    @property
    def V(self) -> int:
        return self.row.numel()


def make_case(name, row, B, inv_temp=1.0, top_k=0, top_p=1.0, seed_base=0, seeds=None, pos=None,
              launches=("topkp",)) -> Case:
    def arr(x, dt):
        a = np.asarray(x, dtype=dt)
        return np.full(B, a, dtype=dt) if a.ndim == 0 else a

    if seeds is None:
        seeds = [mix_seed(seed_base * 1000 + b) for b in range(B)]
    if pos is None:
        pos = [(b * 7 + 3 + seed_base) % 4096 for b in range(B)]
    c = Case(name, row.float().contiguous(), arr(inv_temp, np.float32), arr(top_k, np.int32), arr(top_p, np.float32),
             [int(s) for s in seeds], arr(pos, np.int64), tuple(launches))
    assert len(c.inv_temp) == len(c.top_k) == len(c.top_p) == len(c.pos) == c.B
    return c


@dataclass
class RowExp:
    tok: int  # pick over `may`
    decided: bool
    may_idx: Optional[np.ndarray] = None  # kept for undecided rows only
    may_scores: Optional[np.ndarray] = None


_EXP: Dict[str, List[RowExp]] = {}


def expectation(case: Case) -> List[RowExp]:
    """Per-row expectation of a case, computed once per process and shared by every test."""
    if case.name in _EXP:
        return _EXP[case.name]
    r = _f64(case.row)
    sets: Dict[tuple, tuple] = {}
    out = []
    for b in range(case.B):
        it, k, p = float(case.inv_temp[b]), int(case.top_k[b]), float(case.top_p[b])
        if (it, k, p) not in sets:
            sets[(it, k, p)] = survivor_sets(r, it, k, p)
        st = sets[(it, k, p)]
        t_must, t_may, gap = expected_tokens(r, it, k, p, case.seeds[b], int(case.pos[b]), sets=st)
        e = RowExp(t_may, is_decided(t_must, t_may, gap))
        if not e.decided:
            e.may_idx = np.flatnonzero(st[1])
            e.may_scores = _scores(r, e.may_idx, it, case.seeds[b], int(case.pos[b]))
        out.append(e)
    _EXP[case.name] = out
    return out


def check_tokens(case: Case, toks: Sequence[int]) -> None:
    """The decided-row rule: exact token on a decided row; on an undecided one a token in `may`
    whose score is within GAP of the best. Every token must be a valid id."""
    ex = expectation(case)
    toks = [int(t) for t in toks]
    assert len(toks) == case.B
    bad = []
    for b, (t, e) in enumerate(zip(toks, ex)):
        if not 0 <= t < case.V:
            bad.append((b, t, e.tok, "id outside [0, V)"))
        elif e.decided:
            if t != e.tok:
                bad.append((b, t, e.tok, "decided row"))
        else:
            hit = np.flatnonzero(e.may_idx == t)
            if hit.size == 0:
                bad.append((b, t, e.tok, "not a possible survivor"))
            elif not e.may_scores[hit[0]] >= e.may_scores.max() - GAP:
                bad.append((b, t, e.tok, "score more than GAP below the best"))
    assert not bad, f"{case.name}: {len(bad)} of {case.B} rows wrong, first (row, got, want, why): {bad[:5]}"


def check_row(tok: int, row, inv_temp: float, top_k: int, top_p: float, seed: int, pos: int) -> bool:
    """The decided-row rule for one stand-alone row; returns whether the row was decided."""
    r = _f64(row)
    tok = int(tok)
    assert 0 <= tok < r.size, tok
    sets = survivor_sets(r, inv_temp, top_k, top_p)
    t_must, t_may, gap = expected_tokens(r, inv_temp, top_k, top_p, seed, pos, sets=sets)
    if is_decided(t_must, t_may, gap):
        assert tok == t_may, (tok, t_may, gap)
        return True
    assert sets[1][tok], f"token {tok} is not a possible survivor"
    idx = np.flatnonzero(sets[1])
    s = _scores(r, idx, inv_temp, seed, pos)
    assert s[np.flatnonzero(idx == tok)[0]] >= s.max() - GAP, (tok, t_may)
    return False


# -- inputs ---------------------------------------------------------------------------------------
V_SMALL = 1500


def _perm(n: int, seed: int) -> np.ndarray:
    return np.random.RandomState(seed).permutation(n)


def support_row(step: float, seed: int = 11) -> Tuple[torch.Tensor, np.ndarray]:
    """V = 1500 with 10 live tokens 2.0 - step * j at shuffled indices, everything else -30."""
    live = _perm(V_SMALL, seed)[:10]
    row = np.full(V_SMALL, -30.0, dtype=np.float32)
    row[live] = (2.0 - step * np.arange(10)).astype(np.float32)
    return torch.from_numpy(row), live


def consecutive_row(negative: bool) -> torch.Tensor:
    """1500 consecutive floats just inside (-1, 0) or (0, 1): bit patterns 0x?F7FFFFF - i, which
    differ in the low two bytes only, shuffled."""
    bits = (np.uint32(0xBF7FFFFF if negative else 0x3F7FFFFF) - np.arange(V_SMALL, dtype=np.uint32)).astype(np.uint32)
    return torch.from_numpy(bits.view(np.float32)[_perm(V_SMALL, 12)].copy())


def mixed_row() -> torch.Tensor:
    rs = np.random.RandomState(13)
    row = (rs.randn(V_SMALL) * 3).astype(np.float32)
    row[rs.permutation(V_SMALL)[:200]] = -np.inf
    return torch.from_numpy(row)


INF_INDEX = 777


def inf_row() -> torch.Tensor:
    row = (np.random.RandomState(14).randn(V_SMALL) * 3).astype(np.float32)
    row[INF_INDEX] = np.inf
    return torch.from_numpy(row)


TIE_K = 20


def tie_row() -> Tuple[torch.Tensor, np.ndarray]:
    """Ranks 0..18 hold 1.001 + 0.001 * j, ranks 19..23 all hold 1.0 (the k-th value for k = 20,
    five times), everything else lies in [0.5, 0.9]; returns (row, indices of the five ties)."""
    rs = np.random.RandomState(15)
    perm = rs.permutation(V_SMALL)
    row = (0.5 + 0.4 * rs.rand(V_SMALL)).astype(np.float32)
    row[perm[:19]] = (1.001 + 0.001 * np.arange(19)).astype(np.float32)
    row[perm[19:24]] = 1.0
    return torch.from_numpy(row), np.sort(perm[19:24])


ZERO_K = 12


def zero_row() -> Tuple[torch.Tensor, np.ndarray]:
    """Ten small positives, five +0.0 and five -0.0, everything else in [-2, -1]: for k = 12 the
    k-th value is zero and `row >= kth` keeps all ten zeros of either sign."""
    rs = np.random.RandomState(16)
    perm = rs.permutation(V_SMALL)
    row = (-1.0 - rs.rand(V_SMALL)).astype(np.float32)
    row[perm[:10]] = (0.001 * (1 + np.arange(10))).astype(np.float32)
    row[perm[10:15]] = 0.0
    row[perm[15:20]] = -0.0
    return torch.from_numpy(row), np.sort(perm[10:20])


def random_row(V: int, scale: float, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randn(V, generator=g) * scale


# vectorised Philox4x32-10 over (seed, index) grids: only used to FIND seeds whose Gumbel winner sits
# right at a top-k boundary; every expectation still comes from oracle.gumbel
def philox_np(seeds: np.ndarray, idx: np.ndarray, pos: np.ndarray) -> np.ndarray:
    M = np.uint64(0xFFFFFFFF)
    key = np.asarray(seeds).astype(np.int64).view(np.uint64)
    c0 = np.asarray(idx, dtype=np.uint64) & M
    c1 = np.asarray(pos).astype(np.int64).view(np.uint64) & M
    c0, c1 = np.broadcast_arrays(c0, c1)
    c2 = np.full(c0.shape, 0x5EED, dtype=np.uint64)
    c3 = np.zeros(c0.shape, dtype=np.uint64)
    k0, k1 = key & M, (key >> np.uint64(32)) & M
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> s32) ^ c1 ^ k0) & M, p1 & M, ((p0 >> s32) ^ c3 ^ k1) & M, p0 & M
        k0 = (k0 + np.uint64(0x9E3779B9)) & M
        k1 = (k1 + np.uint64(0xBB67AE85)) & M
    return c0


@functools.lru_cache(maxsize=None)
def _noise_winner_ranks(negative: bool, n: int = 8192):
    """For n candidate (seed, pos) pairs: rank (0 = largest logit) of the element that wins
    Gumbel-max over the WHOLE consecutive row at inv_temp = 1."""
    r = _f64(consecutive_row(negative))
    rank = np.empty(V_SMALL, dtype=np.int64)
    rank[np.argsort(-r, kind="stable")] = np.arange(V_SMALL)
    seeds = np.array([mix_seed(500000 + i) for i in range(n)], dtype=np.int64)
    pos = (np.arange(n) * 5 + 1) % 4096
    win = np.empty(n, dtype=np.int64)
    for lo in range(0, n, 1024):
        d = philox_np(seeds[lo:lo + 1024, None], np.arange(V_SMALL)[None, :], pos[lo:lo + 1024, None])
        u = np.minimum(((d >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0, 1.0 - 2.0 ** -24)
        win[lo:lo + 1024] = np.argmax(r[None, :] - np.log(-np.log(u)), axis=1)
    return seeds, pos, rank[win]


RADIX_KS = (1, 2, 255, 256, 257, 1499)


def radix_case(negative: bool, k: int, greedy: bool) -> Case:
    """B = 64 rows over the consecutive-float row with top_k = k. The logits are equal to 1e-4, so
    the Gumbel winner is set by the noise alone; the seeds are chosen so that for some rows the
    k-th largest element wins (a kernel keeping one too few fails there) and for others the
    (k+1)-th would win were it kept (a kernel keeping one too many fails there)."""
    seeds, pos, wr = _noise_winner_ranks(negative)
    at_k = np.flatnonzero(wr == k - 1)[:8]
    past_k = np.flatnonzero(wr == k)[:8]
    rest = np.setdiff1d(np.arange(64 + 16), np.concatenate([at_k, past_k]))[:64 - at_k.size - past_k.size]
    pick = np.concatenate([at_k, past_k, rest])
    name = f"radix-{'neg' if negative else 'pos'}-k{k}-{'greedy' if greedy else 'gumbel'}"
    return make_case(name, consecutive_row(negative), 64, inv_temp=0.0 if greedy else 1.0, top_k=k,
                     seeds=seeds[pick].tolist(), pos=pos[pick])


def radix_boundary_rows(negative: bool, k: int) -> Tuple[int, int]:
    _, _, wr = _noise_winner_ranks(negative)
    return int(min(8, (wr == k - 1).sum())), int(min(8, (wr == k).sum()))


NUCLEUS_PS = (0.05, 0.35, 0.55, 0.95)
NUCLEUS_SURVIVORS = (1, 4, 6, 10)


def nucleus_cases() -> List[Case]:
    row, _ = support_row(0.01)
    cs = []
    for it in (1.0, 0.5, 2.0):
        for p in NUCLEUS_PS:
            cs.append(make_case(f"nucleus-p{p}-it{it}", row, 256, inv_temp=it, top_p=p, seed_base=len(cs) + 1))
    cs.append(make_case("nucleus-k3-p0.55", row, 256, top_k=3, top_p=0.55, seed_base=20))
    return cs


def radix_cases() -> List[Case]:
    cs = [radix_case(neg, k, greedy) for neg in (True, False) for k in RADIX_KS for greedy in (False, True)]
    for k in (5, 700, 1400):  # 1400 > 1300 finite entries: the k-th value is -inf
        cs.append(make_case(f"mixed-k{k}", mixed_row(), 64, top_k=k, seed_base=30 + k))
        cs.append(make_case(f"mixed-k{k}-greedy", mixed_row(), 64, inv_temp=0.0, top_k=k, seed_base=31 + k))
    for k in (0, 10):
        cs.append(make_case(f"inf-k{k}", inf_row(), 64, top_k=k, seed_base=40 + k, launches=("topkp", "fast")))
    cs.append(make_case("inf-greedy", inf_row(), 64, inv_temp=0.0, seed_base=42, launches=("topkp", "fast")))
    for k in (V_SMALL, V_SMALL + 5, 0, -3):  # all mean "no filter"; same seeds, so the same tokens
        cs.append(make_case(f"nofilter-k{k}", random_row(V_SMALL, 2.0, 17), 64, top_k=k, seed_base=50))
    return cs


def tie_case() -> Case:
    return make_case("ties-at-k", tie_row()[0], 256, top_k=TIE_K, seed_base=60)


def zero_case() -> Case:
    return make_case("signed-zero-at-k", zero_row()[0], 256, top_k=ZERO_K, seed_base=61)


RANDOM_SPECS = ((32000, 2.0, 0, 0.9, 1.0), (32000, 2.0, 50, 0.9, 1.0), (5000, 2.0, 0, 0.999, 1.0),
                (5000, 2.0, 700, 0.97, 2.0), (300, 4.0, 0, 0.3, 1.3), (128256, 3.0, 0, 0.95, 1.25))


def random_cases() -> List[Case]:
    return [make_case(f"random-V{V}-k{k}-p{p}", random_row(V, sc, 100 + n), 256, inv_temp=it, top_k=k, top_p=p,
                      seed_base=70 + n) for n, (V, sc, k, p, it) in enumerate(RANDOM_SPECS)]


def agreement_case() -> Case:
    return make_case("paths-agree", random_row(5000, 2.0, 18), 256, inv_temp=1.1, seed_base=80,
                     launches=("topkp", "fast"))


def mixed_batch_case() -> Case:
    """One launch whose rows cycle through greedy, plain temperature, top-k only, top-p only, both."""
    B = 65
    kinds = [(0.0, 0, 1.0), (0.9, 0, 1.0), (1.0, 40, 1.0), (1.2, 0, 0.8), (0.8, 200, 0.9)]
    it, k, p = zip(*[kinds[b % 5] for b in range(B)])
    return make_case("mixed-batch", random_row(5000, 2.0, 19), B, inv_temp=it, top_k=k, top_p=p, seed_base=81)


FAST_VS = (1, 63, 65, 1000, 1023, 1025, 4097)
FAST_BS = (1, 3, 32)


def fast_shape_cases() -> List[Case]:
    cs = []
    for V in FAST_VS:
        for B in FAST_BS:
            row = random_row(V, 3.0, 200 + V)
            cs.append(make_case(f"fast-V{V}-B{B}", row, B, inv_temp=0.9, seed_base=90 + B, launches=("fast", "topkp")))
            cs.append(make_case(f"fast-V{V}-B{B}-greedy", row, B, inv_temp=0.0, seed_base=90 + B,
                                launches=("fast", "topkp")))
    return cs


def fast_large_case() -> Case:
    return make_case("fast-V128256", random_row(128256, 3.0, 21), 64, inv_temp=0.8, seed_base=95, launches=("fast",))


EDGE_SEEDS = ((1 << 31) + 5, (1 << 32) - 1, (1 << 63) - 1, 0x1234567800000000, -1, -(1 << 63), -(1 << 31) - 7, 0)
EDGE_POS = (0, 1, 65535, 65536, 1 << 24, (1 << 31) - 16, (1 << 31) - 1, 123456789)


def edge_seed_case() -> Case:
    """Seeds with bits above 2^31, negative seeds, and positions up to 2^31 - 1 (the uint32 step)."""
    seeds = [s for s in EDGE_SEEDS for _ in EDGE_POS]
    pos = [p for _ in EDGE_SEEDS for p in EDGE_POS]
    return make_case("edge-seeds", random_row(1000, 3.0, 22), len(seeds), inv_temp=0.9, seeds=seeds, pos=pos,
                     launches=("fast", "topkp"))


# (seed, position, vocabulary index) whose Philox word has its top 24 bits all set: 0xFFFFFF + 0.5
# rounds to 2^24 in float32, which gives u = 1 and a Gumbel of +inf, so that index wins whatever its
# logit (found by scanning seeds 1..200 x positions 0..63 over 1500 indices with
# oracle.philox_draw). One draw in 2^24 does this: about one token in 128 at V = 128k without
# filters. It is the rule of kernel and oracle alike and is pinned here as it is, not as it should
# be: capping u below 1 changes the tokens of every long sampled sequence.
SATURATED_DRAWS = ((10, 17, 685), (68, 59, 749), (102, 34, 894))


def saturated_case() -> Case:
    row, live = support_row(0.25, seed=23)
    assert not set(live) & {i for _, _, i in SATURATED_DRAWS}
    return make_case("saturated-uniform", row, 3, seeds=[s for s, _, _ in SATURATED_DRAWS],
                     pos=[p for _, p, _ in SATURATED_DRAWS], launches=("fast", "topkp"))


DEGENERATE_PS = (0.0, -0.5)
DEGENERATE_KS = (0, 40)


def degenerate_cases() -> List[Case]:
    row = random_row(5000, 2.0, 24)
    return [make_case(f"degenerate-p{p}-k{k}", row, 64, top_k=k, top_p=p, seed_base=110 + n)
            for n, (p, k) in enumerate((p, k) for p in DEGENERATE_PS for k in DEGENERATE_KS)]


def strided_case() -> Case:
    return make_case("strided", random_row(1000, 3.0, 25), 3, inv_temp=0.9, seed_base=120, launches=("fast", "topkp"))


def all_cases() -> List[Case]:
    """Every case the GPU file launches through check_tokens."""
    return (nucleus_cases() + radix_cases() + [tie_case(), zero_case()] + random_cases()
            + [agreement_case(), mixed_batch_case()] + fast_shape_cases()
            + [fast_large_case(), edge_seed_case(), saturated_case(), strided_case()] + degenerate_cases())


def case_tensors(case: Case, device="cpu"):
    """(inv_temp, top_k, top_p, seeds, positions) tensors of a case."""
    return (torch.from_numpy(case.inv_temp).to(device), torch.from_numpy(case.top_k).to(device),
            torch.from_numpy(case.top_p).to(device), torch.tensor(case.seeds, dtype=torch.int64, device=device),
            torch.from_numpy(case.pos.astype(np.int32)).to(device))


# -- state advance --------------------------------------------------------------------------------
ADV_B, ADV_BS, ADV_CAP, ADV_V = 3, 4, 2, 300
ADV_START = (2, 3, 7)
ADV_SENTINEL = -7


def advance_inputs(topkp: bool):
    """Inputs of the three-call state-advance run: per-row logits, a non-identity block table that
    is a [B, 5] slice of a [B, 8] buffer, and positions that cross a block boundary (bs = 4) at
    different calls."""
    g = torch.Generator().manual_seed(26)
    logits = torch.randn(ADV_B, ADV_V, generator=g) * 3
    bt_full = torch.from_numpy(np.stack([_perm(8, 27 + b) + 8 * b for b in range(ADV_B)]).astype(np.int32))
    it = torch.full((ADV_B,), 1.0)
    tk = torch.full((ADV_B,), 40 if topkp else 0, dtype=torch.int32)
    tp = torch.full((ADV_B,), 0.9 if topkp else 1.0)
    seeds = torch.tensor([mix_seed(130 + b) for b in range(ADV_B)], dtype=torch.int64)
    return logits, bt_full, it, tk, tp, seeds


def advance_state(device="cpu"):
    return dict(tokens_in=torch.full((ADV_B,), ADV_SENTINEL, dtype=torch.int32, device=device),
                positions=torch.tensor(ADV_START, dtype=torch.int32, device=device),
                seq_lens=torch.tensor([p + 1 for p in ADV_START], dtype=torch.int32, device=device),
                slots=torch.full((ADV_B,), ADV_SENTINEL, dtype=torch.int32, device=device),
                out_full=torch.full((ADV_B + 1, ADV_CAP), ADV_SENTINEL, dtype=torch.int32, device=device),
                out_count=torch.zeros(ADV_B, dtype=torch.int32, device=device))


def advance_rows_decided(topkp: bool) -> List[bool]:
    """Whether each (call, row) of the state-advance run is a decided row (positions as they are
    at that call), so that CPU oracle and kernel must agree on the token."""
    logits, _, it, tk, tp, seeds = advance_inputs(topkp)
    out = []
    for call in range(3):
        for b in range(ADV_B):
            e = expected_tokens(logits[b], float(it[b]), int(tk[b]), float(tp[b]), int(seeds[b]), ADV_START[b] + call)
            out.append(is_decided(*e))
    return out
