"""float64 reference of the token log-probabilities and the cases the CPU and GPU tests share.

Definition (README, "Sampling"): for a raw float32 logits row l[0..V), lp[j] = l[j] - lse,
lse = M + ln(sum exp(l - M)) over the non-NaN entries, M their maximum. The top-N are the non-NaN
entries ordered by (logit descending, id ascending); places past them hold id -1 and -inf.

The module also holds wrong models of the two-stage kernel (``MODELS``); ``rejected_by`` says which
shared cases tell a model from the right one, and a test asserts that every model is told.
"""

from dataclasses import dataclass
from typing import List, Optional

import numpy as np

PARTS = 64
MAX_TOP = 20
TOL = 1e-4  # nats, finite values, against the float64 reference (derivation: test_logprobs_gpu)


def _order(row: np.ndarray, larger_id_first: bool = False) -> np.ndarray:
    """Ids of the non-NaN entries by (logit descending, id ascending): a stable sort on -logit."""
    ids = np.nonzero(~np.isnan(row))[0]
    if larger_id_first:
        ids = ids[::-1]
    return ids[np.argsort(-row[ids].astype(np.float64), kind="stable")]


def _lse(vals: np.ndarray) -> float:
    vals = vals[~np.isnan(vals)].astype(np.float64)
    if vals.size == 0 or vals.max() == -np.inf:
        return -np.inf
    M = vals.max()
    return float(M + np.log(np.exp(vals - M).sum()))


def _fill(row, order, n, lse):
    top_i = np.full(n, -1, np.int64)
    top_v = np.full(n, -np.inf, np.float64)
    k = min(n, order.size)
    top_i[:k] = order[:k]
    with np.errstate(invalid="ignore"):
        top_v[:k] = row[order[:k]].astype(np.float64) - lse
    return top_v, top_i


def reference(logits: np.ndarray, tokens: np.ndarray, n: int, model: str = "right",
              penalised: Optional[np.ndarray] = None):
    """(lp_tok [B], top_v [B, n], top_i [B, n]) in float64 / int64 of float32 ``logits`` [B, V].
    ``model`` other than "right" is one of the wrong kernels of ``MODELS``; "penalised_row" takes
    its values from ``penalised`` (the row after the penalty launch) as a kernel would that read the
    logits buffer after ``penalize_logits`` rewrote it."""
    B, V = logits.shape
    per = -(-V // PARTS)
    lp_tok = np.empty(B, np.float64)
    top_v = np.empty((B, n), np.float64)
    top_i = np.empty((B, n), np.int64)
    for b in range(B):
        row = logits[b]
        if model == "penalised_row":
            row = penalised[b]
        lse = _lse(row)
        order = _order(row, larger_id_first=(model == "ties_larger_id"))
        if model == "half_candidates":  # per-part lists of ceil(n / 2), then the merge
            keep = -(-n // 2)
            parts = [_order(row[lo:lo + per])[:keep] + lo for lo in range(0, V, per)]
            cand = np.concatenate(parts) if parts else np.zeros(0, np.int64)
            order = cand[np.lexsort((cand, -row[cand].astype(np.float64)))]
        elif model == "no_rescale":  # sum_p s_p without exp(m_p - M)
            M, s = -np.inf, 0.0
            for lo in range(0, V, per):
                v = row[lo:lo + per]
                v = v[~np.isnan(v)].astype(np.float64)
                if v.size and v.max() > -np.inf:
                    M = max(M, v.max())
                    s += np.exp(v - v.max()).sum()
            lse = M + np.log(s) if s > 0 else -np.inf
        elif model == "lse_top_only":
            lse = _lse(row[order[:n]]) if n else -np.inf
        with np.errstate(invalid="ignore"):
            lp_tok[b] = np.float64(row[tokens[b]]) - lse
        top_v[b], top_i[b] = _fill(row, order, n, lse)
    return lp_tok, top_v, top_i


MODELS = ("ties_larger_id", "half_candidates", "no_rescale", "lse_top_only", "penalised_row")


@dataclass
class Case:
    name: str
    logits: np.ndarray            # float32 [B, V]: a view of ``buffer`` when the case is strided
    tokens: np.ndarray            # int32 [B], the "sampled" ids
    n: int
    buffer: Optional[np.ndarray] = None   # the wider float32 buffer whose padding must come back intact
    penalised: Optional[np.ndarray] = None  # the rows after a penalty, for the "penalised_row" model

    @property
    def B(self):
        return self.logits.shape[0]

    @property
    def V(self):
        return self.logits.shape[1]


def _gauss(rng, B, V, scale=6.0):
    return np.clip(rng.standard_normal((B, V)) * scale, -64, 64).astype(np.float32)


def _tokens(rng, logits):
    """One sampled id per row: the argmax, a middling id, then random non-NaN ids."""
    B, V = logits.shape
    out = np.empty(B, np.int32)
    for b in range(B):
        ok = np.nonzero(~np.isnan(logits[b]))[0]
        out[b] = _order(logits[b])[0] if b == 0 else ok[rng.integers(ok.size)]
    return out


_CASES: Optional[List[Case]] = None


def cases() -> List[Case]:
    """The shared cases, built once; tests must not write to their arrays."""
    global _CASES
    if _CASES is not None:
        return _CASES
    rng = np.random.default_rng(20261021)
    out: List[Case] = []
    # the grid: B x V x N, Gaussian logits with |l| <= 64
    for V in (1, 19, 63, 64, 65, 255, 257, 1025, 16385):
        for B in (1, 3):
            for n in (0, 1, 5, 20):
                lg = _gauss(rng, B, V, scale=4.0 if (V + n) % 2 else 16.0)
                out.append(Case(f"gauss-B{B}-V{V}-N{n}", lg, _tokens(rng, lg), n))

    def add(name, lg, n, tokens=None, **kw):
        lg = np.ascontiguousarray(lg, dtype=np.float32) if "buffer" not in kw else lg
        out.append(Case(name, lg, _tokens(rng, lg) if tokens is None else np.asarray(tokens, np.int32), n, **kw))

    # ties that straddle the N-th place and a part boundary: V = 1025 -> per = 17; ids 16 | 17 are the
    # last of part 0 and the first of part 1. Seven entries share the top value, N = 5 cuts through them.
    lg = _gauss(rng, 3, 1025)
    for b in range(3):
        lg[b, [3, 16, 17, 18, 500, 1000, 1024]] = lg[b].max() + 1.0
    add("ties-straddle-N-and-part", lg, 5, tokens=[17, 1000, 3])
    # the same with N = 20 and a second tie group at the cut (places 19..22)
    lg = _gauss(rng, 1, 1025)
    top = lg.max()
    lg[0, np.arange(0, 18) * 50] = top + 5.0 + np.arange(18, dtype=np.float32)
    lg[0, [33, 34, 67, 68, 1023]] = top + 2.0
    add("ties-at-place-20", lg, 20, tokens=[68])
    # the global top-N all inside one part (a merge that takes < N per part loses them)
    for n in (5, 20):
        lg = _gauss(rng, 3, 16385)  # per = 257
        for b in range(3):
            lo = 257 * (7 + b)
            lg[b, lo + 3:lo + 3 + n] = 70.0 - np.arange(n, dtype=np.float32) * 0.25
        add(f"top-in-one-part-N{n}", lg, n)
    # one whole part of -inf (a masked vocabulary range), and a row that is mostly masked
    lg = _gauss(rng, 3, 1025)
    lg[:, 17 * 5:17 * 6] = -np.inf
    lg[2, 100:] = -np.inf
    add("part-of-minus-inf", lg, 20)
    lg = _gauss(rng, 1, 257)  # per = 5
    lg[0, 10:] = -np.inf  # 10 finite entries, N = 20: -inf ids are ranked by id after them
    add("fewer-finite-than-N", lg, 20, tokens=[4])
    # scattered NaNs, also the row maximum's neighbours and whole parts
    lg = _gauss(rng, 3, 1025)
    lg[:, ::7] = np.nan
    lg[1, 17 * 3:17 * 4] = np.nan
    lg[2, 5:900] = np.nan
    add("scattered-nan", lg, 20)
    lg = _gauss(rng, 1, 19)
    lg[0, [0, 5, 18]] = np.nan
    add("nan-V-below-N", lg, 20)
    # ids 0 and V - 1 among the winners
    for V in (65, 16385):
        lg = _gauss(rng, 3, V)
        lg[:, 0] = 66.0
        lg[:, V - 1] = 66.0
        lg[1, V - 1] = 67.0
        add(f"edge-ids-V{V}", lg, 5, tokens=[0, V - 1, V - 1])
    # far-apart part maxima: a sum that forgets the exp(m_p - M) rescale is off by nats
    lg = (_gauss(rng, 3, 1025, scale=1.0) - 40.0).astype(np.float32)
    lg[:, 17 * 9:17 * 10] += 60.0
    add("part-maxima-far-apart", lg, 5)
    # a [B, V] view of a wider buffer: the padding must come back intact
    for V, W in ((257, 300), (1025, 1088)):
        buf = np.full((3, W), 1e30, np.float32)
        buf[:, :V] = _gauss(rng, 3, V)
        view = buf[:, :V]
        add(f"strided-V{V}", view, 20, buffer=buf)
    # a penalised decode row: repetition 1.3 + presence 0.7 on the 40 most likely ids. The reported
    # values must be the raw row's.
    lg = _gauss(rng, 3, 1025)
    pen = lg.copy()
    for b in range(3):
        hit = _order(lg[b])[:40]
        v = pen[b, hit]
        pen[b, hit] = np.where(v > 0, v / np.float32(1.3), v * np.float32(1.3)) - np.float32(0.7)
    add("penalised-row", lg, 20, penalised=pen)
    _CASES = out
    return out


def differs(a, b, tol: float = TOL) -> bool:
    """True when two (lp_tok, top_v, top_i) results disagree as the GPU test would notice: any id, any
    -inf / NaN pattern, or a finite value by more than ``tol``."""
    if not np.array_equal(a[2], b[2]):
        return True
    for x, y in ((a[0], b[0]), (a[1], b[1])):
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        fin = np.isfinite(x)
        if not np.array_equal(fin, np.isfinite(y)) or not np.array_equal(x[~fin], y[~fin], equal_nan=True):
            return True
        if fin.any() and np.abs(x[fin] - y[fin]).max() > tol:
            return True
    return False


def rejected_by(model: str) -> List[str]:
    """Names of the shared cases on which ``model`` disagrees with the reference."""
    names = []
    for c in cases():
        if model == "penalised_row" and c.penalised is None:
            continue
        right = reference(c.logits, c.tokens, c.n)
        wrong = reference(c.logits, c.tokens, c.n, model=model, penalised=c.penalised)
        if differs(right, wrong):
            names.append(c.name)
    return names


def check(case: Case, lp_tok, top_v, top_i, tol: float = TOL) -> None:
    """Assert a float32 result against the float64 reference: ids exact, -inf exact, finite values
    within ``tol``, and the sampled token's value the same bits as its entry in the top list."""
    lp_tok = np.asarray(lp_tok, np.float32)
    top_v = np.asarray(top_v, np.float32)
    top_i = np.asarray(top_i, np.int64)
    r_tok, r_v, r_i = reference(case.logits, case.tokens, case.n)
    assert top_i.shape == r_i.shape and top_v.shape == r_v.shape, case.name
    assert np.array_equal(top_i, r_i), f"{case.name}: ids {top_i.tolist()} != {r_i.tolist()}"
    assert ((top_i >= -1) & (top_i < case.V)).all(), case.name
    for got, ref, what in ((lp_tok, r_tok, "token"), (top_v, r_v, "top")):
        fin = np.isfinite(ref)
        assert np.array_equal(got[~fin].astype(np.float64), ref[~fin], equal_nan=True), f"{case.name}: {what} -inf"
        if fin.any():
            err = np.abs(got[fin].astype(np.float64) - ref[fin]).max()
            assert err <= tol, f"{case.name}: {what} off by {err:.3g} nats"
    for b in range(case.B):
        hit = np.nonzero(top_i[b] == case.tokens[b])[0]
        if hit.size:
            assert lp_tok[b].tobytes() == top_v[b, hit[0]].tobytes(), f"{case.name}: row {b} token vs top bits"
