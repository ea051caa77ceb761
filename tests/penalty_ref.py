"""Float32 reference of the sampling penalties and min-p (csrc/kernels/sampler.hip:
penalize_logits_kernel, the min-p predicate of sample_topkp_kernel, the count in advance()) and the
shared inputs of test_penalties_cpu.py / test_penalties_gpu.py.

The transform is pinned to the bit, so the reference is exact: division and multiplication are
numpy float32 (IEEE, round to nearest), and the fused step fma(-f, c, l) is computed as a
`fractions.Fraction` and rounded ONCE to float32, half to even. After the transform a row goes
through sampler_ref unchanged: must / may = survivor_sets(penalised row) & min-p mask, then
expected_tokens / check_tokens with the project's GAP and UNDECIDED_CAP.

History word of a vocabulary id (uint16): bit 15 = the id occurs in the context the row was bound
with; bits 0-14 = c, how often the id was generated since, saturating at 32767.
"""

from __future__ import annotations

import math
from dataclasses import dataclass
from fractions import Fraction
from typing import Dict, List, Tuple

import numpy as np
import torch

import sampler_ref as sr
from llm_consensus_amd import ops

CTX, COUNT = 0x8000, 0x7FFF
F32 = np.float32


# -- exact float32 arithmetic ---------------------------------------------------------------------
def round_f32(x: Fraction) -> np.float32:
    """The float32 nearest to the rational x, ties to even (overflow to inf, subnormals included)."""
    if x == 0:
        return F32(0.0)
    sign = -1 if x < 0 else 1
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()  # 2^(e-1) < a < 2^(e+1)
    if a < Fraction(2) ** e:
        e -= 1  # now 2^e <= a < 2^(e+1)
    q = max(e, -126) - 23  # exponent of the last place (subnormals share -149)
    scaled = a / Fraction(2) ** q
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    if n * Fraction(2) ** q >= Fraction(2) ** 128:
        return F32(sign * np.inf)
    return F32(sign * math.ldexp(n, q))  # n < 2^25 and the result is representable: exact


def fma_f32(a: np.float32, b: np.float32, c: np.float32) -> np.float32:
    """a * b + c rounded once. Non-finite operands follow IEEE through float64 (no rounding matters)."""
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(invalid="ignore"):
            return F32(np.float64(a) * np.float64(b) + np.float64(c))
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if exact == 0:  # an exact cancellation is +0 in round to nearest, unless both terms are -0
        return F32(np.float64(a) * np.float64(b) + np.float64(c))
    return round_f32(exact)


# -- the transform --------------------------------------------------------------------------------
MODELS = ("right", "unfused", "rep-on-generated-only", "presence-on-context", "div-mul-swapped")


def penalise(row, words, r: float, f: float, p: float, model: str = "right") -> np.ndarray:
    """The penalised copy of a float32 row. ``model`` other than "right" is a wrong kernel the cases
    have to reject:
      unfused                 float32(f * c) rounded, then subtracted
      rep-on-generated-only   repetition penalty where c > 0 instead of where the word is non-zero
      presence-on-context     presence penalty on every seen id
      div-mul-swapped         l * r for positive logits, l / r for the others"""
    assert model in MODELS
    out = np.array(row, dtype=F32, copy=True)
    w = np.asarray(words).astype(np.int64) & 0xFFFF
    r, f, p = F32(r), F32(f), F32(p)
    if r == 1 and f == 0 and p == 0:
        return out
    with np.errstate(all="ignore"):
        for i in np.flatnonzero(w):
            l = out[i]
            c = int(w[i]) & COUNT
            if model != "rep-on-generated-only" or c > 0:
                if model == "div-mul-swapped":
                    l = F32(l * r) if l > 0 else F32(l / r)
                else:
                    l = F32(l / r) if l > 0 else F32(l * r)
            if c > 0:
                if model == "unfused":
                    l = F32(l - F32(f * F32(c)))
                else:
                    l = fma_f32(F32(-f), F32(c), l)
                l = F32(l - p)
            elif model == "presence-on-context":
                l = F32(l - p)
            out[i] = l
    return out


def advance_words(words: np.ndarray, tok: int) -> np.ndarray:
    """The words after ``tok`` was generated once more (a copy)."""
    out = np.array(words, dtype=np.uint16, copy=True)
    if int(out[tok]) & COUNT != COUNT:
        out[tok] += 1
    return out


def ln_min_p(min_p: float) -> np.float32:
    """What the host passes to the kernel: float32(log(min_p)); -inf = off."""
    return F32(math.log(min_p)) if min_p > 0 else F32(-np.inf)


def min_p_mask(row, inv_temp: float, min_p: float) -> np.ndarray:
    """Sampled rows keep l iff it is the row maximum or (l - max) * inv_temp >= ln(min_p), all in
    float32 (a subtraction followed by a multiplication cannot be contracted). Greedy rows and
    min_p = 0 keep everything."""
    r = np.asarray(row, dtype=F32)
    lmp = ln_min_p(min_p)
    if inv_temp <= 0 or not lmp > -np.inf:
        return np.ones(r.size, dtype=bool)
    with np.errstate(invalid="ignore"):
        mx = F32(np.nanmax(r)) if not np.isnan(r).all() else F32(-np.inf)
        return (r == mx) | (((r - mx).astype(F32) * F32(inv_temp)).astype(F32) >= lmp)


def sets_for(prow, inv_temp: float, top_k: int, top_p: float, min_p: float):
    must, may = sr.survivor_sets(prow, inv_temp, top_k, top_p)
    m = min_p_mask(prow, inv_temp, min_p)
    return must & m, may & m


# -- cases ----------------------------------------------------------------------------------------
@dataclass
class PenCase:
    name: str
    raw: torch.Tensor  # [V] float32, before the penalties
    words: np.ndarray  # [V] uint16
    r: float
    f: float
    p: float
    min_p: np.ndarray  # [B] float32
    case: sr.Case  # over the PENALISED row (what the sampler kernels see)

    @property
    def B(self) -> int:
        return self.case.B

    @property
    def V(self) -> int:
        return self.case.V


def make_words(V: int, seed: int, n_ctx: int = 300, n_gen: int = 70, must_gen=()) -> np.ndarray:
    """``n_ctx`` context ids (0 and V - 1 among them), ``n_gen`` generated ids with counts 1-5 (about
    a third of them context ids too), one count at 32767, and ``must_gen`` generated as well."""
    rs = np.random.RandomState(seed)
    n_ctx, n_gen = min(n_ctx, V), min(n_gen, V)
    w = np.zeros(V, dtype=np.uint16)
    ctx = rs.permutation(V)[:n_ctx]
    w[ctx] = CTX
    w[0] |= CTX
    w[V - 1] |= CTX
    gen = np.concatenate([ctx[: n_gen // 3], rs.permutation(V)[: n_gen - n_gen // 3], np.asarray(must_gen, dtype=np.int64)])
    gen = np.unique(gen)
    w[gen] = (w[gen] & CTX) | rs.randint(1, 6, size=gen.size).astype(np.uint16)
    w[gen[len(gen) // 2]] |= COUNT
    return w


def pen_case(name, raw, words, r, f, p, B, inv_temp=1.0, top_k=0, top_p=1.0, min_p=0.0, seed_base=0) -> PenCase:
    raw = raw.float().contiguous()
    prow = torch.from_numpy(penalise(raw.numpy(), words, r, f, p))
    c = sr.make_case(name, prow, B, inv_temp=inv_temp, top_k=top_k, top_p=top_p, seed_base=seed_base)
    mp = np.full(B, min_p, dtype=F32) if np.ndim(min_p) == 0 else np.asarray(min_p, dtype=F32)
    return PenCase(name, raw, np.asarray(words, dtype=np.uint16), float(r), float(f), float(p), mp, c)


R, F, P = 1.3, 0.2, 0.5
SHARED_VS = ((1500, 256), (5000, 256), (32000, 64))  # (V, rows per launch)
# (inv_temp, top_k, top_p, min_p); the last one keeps top-p and a wide min-p apart (MINP_ORDER_SET)
PARAM_SETS = ((1.0, 0, 1.0, 0.0), (0.0, 0, 1.0, 0.0), (1.0, 50, 0.9, 0.05), (0.7, 0, 1.0, 0.1), (1.0, 0, 1.0, 0.01),
              (1.4, 0, 0.95, 0.5), (1.0, 0, 1.0, 1.0), (1.0, 0, 0.9, 0.02))
MINP_ORDER_SET = 7


def shared_raw(V: int) -> Tuple[torch.Tensor, np.ndarray]:
    raw = sr.random_row(V, 2.0, 300 + V)
    top = torch.topk(raw, 3).indices.numpy()  # the penalties have to move the argmax
    return raw, make_words(V, 310 + V, must_gen=top)


_SHARED: List[PenCase] = []


def shared_cases() -> List[PenCase]:
    if not _SHARED:
        for V, B in SHARED_VS:
            raw, words = shared_raw(V)
            for n, (it, k, tp, mp) in enumerate(PARAM_SETS):
                _SHARED.append(pen_case(f"pen-V{V}-it{it}-k{k}-p{tp}-minp{mp}", raw, words, R, F, P, B, it, k, tp, mp,
                                        seed_base=400 + 10 * n + V % 7))
    return _SHARED


def large_count_case() -> PenCase:
    """f = 0.2 with counts in the thousands: f * c is inexact in float32, so a multiply rounded
    before the subtraction differs from the fused form."""
    V = 1500
    rs = np.random.RandomState(33)
    w = np.zeros(V, dtype=np.uint16)
    gen = rs.permutation(V)[:400]
    w[gen] = rs.randint(1000, COUNT + 1, size=gen.size).astype(np.uint16)
    w[gen[:50]] |= CTX
    return pen_case("pen-large-counts", sr.random_row(V, 2.0, 34), w, R, F, P, 64, seed_base=480)


def min_p_winner_cases() -> List[PenCase]:
    """Rows whose Gumbel winner WITHOUT the mask lies outside it: neutral penalties, min_p = 0.3 at
    inv_temp = 2 over a flat row, where the mask keeps a handful of ids."""
    V = 1500
    raw = sr.random_row(V, 1.0, 35)
    w = np.zeros(V, dtype=np.uint16)
    return [pen_case(f"minp-winner-{mp}", raw, w, 1.0, 0.0, 0.0, 64, inv_temp=2.0, min_p=mp, seed_base=490 + n)
            for n, mp in enumerate((0.3, 0.6))]


def all_sampled_cases() -> List[PenCase]:
    return shared_cases() + [large_count_case()] + min_p_winner_cases()


# -- expectations ---------------------------------------------------------------------------------
def expectation(pc: PenCase) -> List[sr.RowExp]:
    """sampler_ref.expectation with the min-p mask laid over the survivor sets; stored where
    sampler_ref.check_tokens looks it up, so the decided-row rule is the project's own."""
    c = pc.case
    if c.name in sr._EXP:
        return sr._EXP[c.name]
    r = sr._f64(c.row)
    sets: Dict[tuple, tuple] = {}
    out = []
    for b in range(c.B):
        it, k, p, mp = float(c.inv_temp[b]), int(c.top_k[b]), float(c.top_p[b]), float(pc.min_p[b])
        if (it, k, p, mp) not in sets:
            sets[(it, k, p, mp)] = sets_for(c.row.numpy(), it, k, p, mp)
        st = sets[(it, k, p, mp)]
        t_must, t_may, gap = sr.expected_tokens(r, it, k, p, c.seeds[b], int(c.pos[b]), sets=st)
        e = sr.RowExp(t_may, sr.is_decided(t_must, t_may, gap))
        if not e.decided:
            e.may_idx = np.flatnonzero(st[1])
            e.may_scores = sr._scores(r, e.may_idx, it, c.seeds[b], int(c.pos[b]))
        out.append(e)
    sr._EXP[c.name] = out
    return out


def check_tokens(pc: PenCase, toks) -> None:
    expectation(pc)
    sr.check_tokens(pc.case, toks)


def check_row(tok: int, prow, inv_temp, top_k, top_p, min_p, seed, pos) -> bool:
    """The decided-row rule for one stand-alone penalised row; returns whether it was decided."""
    r = sr._f64(prow)
    tok = int(tok)
    assert 0 <= tok < r.size, tok
    sets = sets_for(np.asarray(prow, dtype=F32), inv_temp, top_k, top_p, min_p)
    t_must, t_may, gap = sr.expected_tokens(r, inv_temp, top_k, top_p, seed, pos, sets=sets)
    if sr.is_decided(t_must, t_may, gap):
        assert tok == t_may, (tok, t_may, gap)
        return True
    assert sets[1][tok], f"token {tok} is not a possible survivor"
    idx = np.flatnonzero(sets[1])
    s = sr._scores(r, idx, inv_temp, seed, pos)
    assert s[np.flatnonzero(idx == tok)[0]] >= s.max() - sr.GAP, (tok, t_may)
    return False


def case_tensors(pc: PenCase, device="cpu"):
    """(inv_temp, top_k, top_p, seeds, positions, ln_min_p, words [B, V] int16, rep, freq, pres)."""
    it, tk, tp, seeds, pos = sr.case_tensors(pc.case, device)
    lmp = torch.tensor([float(ln_min_p(float(m))) for m in pc.min_p], dtype=torch.float32, device=device)
    words = words_tensor(pc.words, device).unsqueeze(0).repeat(pc.B, 1)
    full = lambda v: torch.full((pc.B,), v, dtype=torch.float32, device=device)  # noqa: E731
    return it, tk, tp, seeds, pos, lmp, words, full(pc.r), full(pc.f), full(pc.p)


def words_tensor(words: np.ndarray, device="cpu") -> torch.Tensor:
    return torch.from_numpy(np.asarray(words, dtype=np.uint16).view(np.int16).copy()).to(device)


def words_array(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().numpy().view(np.uint16)


# -- the kernel alone: bit equality ----------------------------------------------------------------
BIT_VS = (1, 63, 65, 1023, 1025, 4097)
BIT_BS = (1, 3)
SPECIALS = (0.0, -0.0, np.inf, -np.inf, np.nan)


def bit_inputs(V: int, B: int):
    """(logits [B, V] float32, words [B, V] uint16, rep, freq, pres [B]) of the bit-equality test:
    touched ids include 0 and V - 1, the seen ids hold 0.0, -0.0, +-inf and a NaN, one count is
    32767, and with B = 3 the middle row is neutral (its words are set all the same)."""
    rs = np.random.RandomState(1000 + 7 * V + B)
    logits = (rs.randn(B, V) * 3).astype(F32)
    words = np.zeros((B, V), dtype=np.uint16)
    for b in range(B):
        words[b] = make_words(V, 2000 + 13 * V + b, n_ctx=max(1, V // 5), n_gen=max(1, V // 20))
        seen = np.flatnonzero(words[b])
        for j, v in enumerate(SPECIALS):
            if j < seen.size:
                logits[b, seen[(j * 7) % seen.size]] = v
        if V > 8:  # a generated id (count > 0) holding a special value too, and an unseen NaN
            gen = np.flatnonzero(words[b] & COUNT)
            logits[b, gen[0]] = -np.inf
            logits[b, gen[-1]] = np.nan
    rep = np.array([R, 1.0, 0.8][:B], dtype=F32) if B == 3 else np.array([R], dtype=F32)
    freq = np.array([F, 0.0, -0.3][:B], dtype=F32) if B == 3 else np.array([F], dtype=F32)
    pres = np.array([P, 0.0, 1.5][:B], dtype=F32) if B == 3 else np.array([P], dtype=F32)
    return logits, words, rep, freq, pres


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=F32)).view(np.uint32)


def same_bits(got, want) -> np.ndarray:
    """Element-wise bit equality, any NaN equal to any NaN."""
    g, w = np.asarray(got, dtype=F32), np.asarray(want, dtype=F32)
    return (bits(g) == bits(w)) | (np.isnan(g) & np.isnan(w))


# -- chained calls --------------------------------------------------------------------------------
CH_V, CH_B = 300, 3
CH_SAT = 77  # row 2: a generated id at count 32767 that keeps winning


def chain_inputs():
    """Three rows for three chained calls with state advance: row 0 greedy, row 1 sampled with
    top-k / min-p, row 2 greedy with an id at count 32767 whose logit wins whatever the penalty."""
    g = torch.Generator().manual_seed(36)
    logits = torch.randn(CH_B, CH_V, generator=g) * 3
    logits[2, CH_SAT] = 1.0e5
    words = np.stack([make_words(CH_V, 3000 + b, n_ctx=40, n_gen=10) for b in range(CH_B)])
    words[2, CH_SAT] = CTX | COUNT
    it = torch.tensor([0.0, 1.0, 0.0])
    tk = torch.tensor([0, 40, 0], dtype=torch.int32)
    tp = torch.tensor([1.0, 0.9, 1.0])
    mp = np.array([0.0, 0.05, 0.0], dtype=F32)
    seeds = torch.tensor([sr.mix_seed(600 + b) for b in range(CH_B)], dtype=torch.int64)
    rep = torch.tensor([R, R, R])
    freq = torch.tensor([F, F, F])
    pres = torch.tensor([P, P, P])
    return logits, words, it, tk, tp, mp, seeds, rep, freq, pres


def chain_run(device, sample_fn=None):
    """Three ops.sample calls with state advance over the same raw logits; returns per call
    (tokens, words uint16 [B, V]). The reference words advance with the tokens the run produced."""
    logits0, words0, it, tk, tp, mp, seeds, rep, freq, pres = chain_inputs()
    B, V = CH_B, CH_V
    dev = lambda t: t.to(device)  # noqa: E731
    words = torch.stack([words_tensor(words0[b]) for b in range(B)]).to(device)
    lmp = dev(torch.tensor([float(ln_min_p(float(m))) for m in mp]))
    st = dict(tokens_in=torch.zeros(B, dtype=torch.int32, device=device),
              positions=torch.tensor([5, 9, 2], dtype=torch.int32, device=device),
              seq_lens=torch.zeros(B, dtype=torch.int32, device=device))
    nxt = torch.zeros(B, dtype=torch.int32, device=device)
    if device != "cpu":
        P_ = ops.sample_parts()
        wv, wi = torch.empty(B, P_, device=device), torch.empty(B, P_, dtype=torch.int32, device=device)
    else:
        wv = wi = None
    out = []
    for _ in range(3):
        logits = dev(logits0.clone())
        pos = st["positions"].cpu().tolist()
        ops.sample(logits, dev(it), dev(tk), dev(tp), dev(seeds), st["positions"], nxt, wv, wi,
                   tokens_in=st["tokens_in"], seq_lens=st["seq_lens"], use_topkp=True, words=words, rep=dev(rep),
                   freq=dev(freq), pres=dev(pres), ln_min_p=lmp)
        out.append((nxt.cpu().tolist(), words_array(words).copy(), logits.cpu().numpy(), pos))
    return out


def check_chain(out):
    logits0, words0, it, tk, tp, mp, seeds, rep, freq, pres = chain_inputs()
    ref = words0.copy()
    for call, (toks, words, plog, pos) in enumerate(out):
        for b in range(CH_B):
            prow = penalise(logits0[b].numpy(), ref[b], float(rep[b]), float(freq[b]), float(pres[b]))
            assert same_bits(plog[b], prow).all(), (call, b)
            check_row(toks[b], prow, float(it[b]), int(tk[b]), float(tp[b]), float(mp[b]), int(seeds[b]), pos[b])
            ref[b] = advance_words(ref[b], toks[b])
        assert np.array_equal(words, ref), call
    assert [o[0][2] for o in out] == [CH_SAT] * 3
    assert ref[2, CH_SAT] == CTX | COUNT  # 32767 stays 32767
    assert (ref != words0).any()


# -- engine runs ---------------------------------------------------------------------------------
def check_steps(toks, raw_rows, prompt, sp):
    V = raw_rows.shape[1]
    words = np.zeros(V, dtype=np.uint16)
    words[np.asarray(prompt)] = CTX
    decided = 0
    for i, t in enumerate(toks):
        prow = penalise(raw_rows[i], words, sp.repetition_penalty, sp.frequency_penalty, sp.presence_penalty)
        it = 0.0 if sp.temperature <= 0 else 1.0 / sp.temperature
        decided += check_row(t, prow, it, sp.top_k, sp.top_p, sp.min_p, sp.seed, len(prompt) - 1 + i)
        words = advance_words(words, t)
    assert decided >= len(toks) - 1


def batcher_requests(SP):
    return [([300 + i for i in range(12)], SP(max_tokens=6, temperature=0.0, stop_on_eos=False)),
            ([400 + i for i in range(7)], SP(max_tokens=22, temperature=0.0, stop_on_eos=False, repetition_penalty=1.3,
                                             frequency_penalty=0.2, presence_penalty=0.5)),
            ([500 + i for i in range(9)], SP(max_tokens=18, temperature=0.9, top_k=40, seed=7, stop_on_eos=False,
                                             min_p=0.05, presence_penalty=1.5))]


def run_staggered(eng, reqs, Batcher):
    bat = Batcher(eng)
    rows = []
    for prompt, sp in reqs:  # one admission per step: the rows join at different replays
        seq = eng.new_sequence()
        eng.prefill([seq], [prompt])
        rows.append(bat.admit(seq, sp))
        bat.step()
    bat.drain()
    for r in rows:
        assert r.error is None and r.seq.ids == reqs[rows.index(r)][0] + r.tokens
        eng.free_sequence(r.seq)
    return [r.tokens for r in rows]
