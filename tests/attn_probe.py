"""Structured attention probes: inputs on which a missing, extra or misplaced key moves the output
by about 1, an fp64 reference that reads the paged cache through the block table, and mutants of
that reference (the mistakes attention kernels make). No GPU is used here: the GPU tests feed a
case's tensors to a kernel and pass its output to ``check``; tests/test_attn_probe_cpu.py proves
that ``check`` rejects every applicable mutant on every case list the GPU tests use.

Data.
  V is position-coded: V[row, kv head, logical position j, d] is +1 or -1 from a seeded generator,
  so a wrong page, kv head, row or position shows as errors of 1 or 2 in about half the dims.
  Poison fills every cache slot a row must not read (positions >= L up to the end of the row's
  pages, every page no row owns, and for windowed cases the positions below every row's window):
  its key scores far above every permitted key for every head and its V is 64. Every block-table
  entry is a valid page (unused entries name a shared poison page): nothing is ever out of bounds.

Kinds.
  needle  background keys are zero (score 0); query head g of a kv group is one-hot on dim
          ``needle_dim(g)`` and its needle key carries ln(L) + 8 (scaled) on that dim alone, so the
          heads of a group seek different positions. Needle positions walk the row's edge list
          (sub-tile, page, chunk, block and window boundaries), one launch after another.
  mix     two needles per head, in the first and the last block, with unequal scores: a difference
          of ln 3 (expected 0.75 V[a] + 0.25 V[b]) or of 30 (the weaker must vanish in the max
          rescale); the stronger one is first for even heads, last for odd ones.
  ramp    the scaled score of key j is about j (ascending) or 1024 - j (descending), coded exactly
          as (j div 256, j mod 256) on dims 0 / 1 against q = (256 t, t): the newest (oldest)
          permitted keys get 0.632, 0.233, 0.085, ... so every row's upper (lower) mask edge is
          pinned. Scores stay in [0, 1024]: ramps stop at 1024 keys.
  qkv_attn's q comes from its projection: there the needles are multiples of the oracle's q_h.
"""

import math

import torch

BF = torch.bfloat16
POISON_V = 64.0
SHAPES = [(8, 2, 128), (4, 2, 64), (32, 32, 96), (14, 2, 64)]  # (14, 2, 64): G = 7
RAMP_MAX = 1024
ONE_LEVEL, GROUP = 32, 16  # csrc/kernels/attn_core.h kAttnOneLevel / kAttnGroup


def needle_dim(g, D):
    """Dim of query head g (within its kv group): distinct for g < 8, never the ramp's dims 0 / 1."""
    return (17 * g + 5) % D


# -- the kernels' key partitions (Python ports) ----------------------------------------------------
def decode_nsplit(L, gc, min_chunk):
    """csrc/kernels/common.h decode_nsplit, balanced form (chunk_arg = -min_chunk)."""
    n = (L + min_chunk - 1) // min_chunk
    return 1 if n < 1 else min(n, gc)


def decode_range(L, n, c):
    """csrc/kernels/common.h decode_range, balanced form: block c of n over L keys in 32-key units."""
    units = (L + 31) // 32
    return 32 * (c * units // n), min(L, 32 * ((c + 1) * units // n))


def decode_blocks(L, form, window=0):
    """The key ranges [start, end) of a row's blocks, as csrc/kernels/attn_decode.hip cuts them;
    form = ("fused", chunk) or ("split", min_chunk, gc)."""
    lo = max(0, L - window) if window > 0 else 0
    if form[0] == "fused":
        chunk = form[1]
        return [(max(lo, c * chunk), min(L, (c + 1) * chunk)) for c in range(lo // chunk, (L + chunk - 1) // chunk)]
    lo32 = lo & ~31
    n = decode_nsplit(L - lo32, form[2], form[1])
    out = []
    for c in range(n):
        s, e = decode_range(L - lo32, n, c)
        out.append((max(lo, s + lo32), e + lo32))
    return out


# -- cases ---------------------------------------------------------------------------------------
class Case:
    """One launch: tensors (CPU, bf16 / int32) and what the mutants need to know about it."""

    def __init__(self, **kw):
        self.window = 0
        self.blocks = None   # per row: the decode blocks' key ranges (None: no cross-block merge)
        self.prev = None     # the launch before this one on the same workspace and cache
        self.needles = {}    # (row, query head) -> [key positions]
        self.edges = {}      # row -> needle positions of this launch (mutant (e) drops each)
        self.__dict__.update(kw)
        self._ref = None

    @property
    def B(self):
        return len(self.q_lens)

    @property
    def ref(self):
        if self._ref is None:
            self._ref = attention(self)
        return self._ref

    @property
    def rows(self):
        """Indices of the query rows that belong to a sequence (the others must stay untouched)."""
        return [r for q0, ql in zip(self.q_start, self.q_lens) for r in range(q0, q0 + ql)]

    def tensors(self, dev):
        """(q, kc, vc, bt, q_start, q_lens, ctx_lens) on ``dev``."""
        i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)  # noqa: E731
        return (self.q.to(dev), self.kc.to(dev), self.vc.to(dev), self.bt.to(dev), i32(self.q_start), i32(self.q_lens),
                i32(self.ctx_lens))


def _poison_key(kind, D, kmax):
    k = torch.zeros(D)
    if kind == "ramp":
        k[0] = 2.0 * RAMP_MAX / 256  # code 2048: twice the largest permitted score
    else:
        k[:] = 2.0 * kmax            # every head's one-hot q scores it at twice its needle
    return k.to(BF)


def _pool(ctx_lens, nkv, D, bs, gen, poison):
    """A paged pool filled with poison and a block table: each row owns ceil(L / bs) + 1 pages (so
    the key one past the end exists, as poison); unused entries name a shared poison page."""
    own = [(L + bs - 1) // bs + 1 for L in ctx_lens]
    nb = sum(own) + 3
    perm = torch.randperm(nb, generator=gen).to(torch.int32)
    bt = torch.full((len(ctx_lens), max(own)), int(perm[-1]), dtype=torch.int32)
    at = 0
    for b, n in enumerate(own):
        bt[b, :n] = perm[at:at + n]
        at += n
    kc = poison.view(1, 1, 1, D).expand(nb, nkv, bs, D).contiguous()
    vc = torch.full((nb, nkv, bs, D), POISON_V, dtype=BF)
    return kc, vc, bt


def _write(case, b, first, k, v):
    """Keys / values [nkv, n, D] into row b's logical positions first .. first + n - 1."""
    idx = torch.arange(first, first + k.shape[1])
    pages = case.bt[b, idx // case.bs].long()
    case.kc[pages, :, idx % case.bs] = k.transpose(0, 1).to(BF)
    case.vc[pages, :, idx % case.bs] = v.transpose(0, 1).to(BF)


def _ramp_code(pos, D):
    k = torch.zeros(len(pos), D)
    k[:, 0] = torch.div(pos, 256, rounding_mode="floor")
    k[:, 1] = pos % 256
    return k


def build(nh, nkv, D, kind, seqs, *, window=0, form=None, bs=64, seed=0, launch=0, edges=None, descending=False,
          pad=0, prev=None):
    """One case. seqs = [(q_len, ctx_len)] (decode: q_len 1). ``edges[b]``: row b's edge list, walked
    by the needles as ``launch`` advances; ``pad`` rows that belong to no sequence follow each
    sequence's queries. ``form``: the decode form, for the block ranges."""
    gen = torch.Generator().manual_seed(1000 * seed + launch)
    G = nh // nkv
    scale = 1 / math.sqrt(D)
    qv = float(torch.tensor(math.sqrt(D)).to(BF))
    ctxs = [c for _, c in seqs]
    if kind == "ramp":
        assert max(ctxs) <= RAMP_MAX
    kmax = math.log(max(ctxs)) + 8 + 30
    q_start, at = [], 0
    for ql, _ in seqs:
        q_start.append(at)
        at += ql + pad
    T = at
    kc, vc, bt = _pool(ctxs, nkv, D, bs, gen, _poison_key(kind, D, kmax))
    case = Case(nh=nh, nkv=nkv, D=D, bs=bs, scale=scale, window=window, kind=kind, kc=kc, vc=vc, bt=bt,
                q=torch.zeros(T, nh * D, dtype=BF), q_start=q_start, q_lens=[ql for ql, _ in seqs], ctx_lens=ctxs, T=T,
                prev=prev, form=form)
    if form is not None:
        case.blocks = [decode_blocks(L, form, window) for L in ctxs]
    for b, (ql, L) in enumerate(seqs):
        lo = max(0, L - ql + 1 - window) if window > 0 else 0  # below it no query of the row reads
        n = L - lo
        v = torch.randint(0, 2, (nkv, n, D), generator=gen).float() * 2 - 1
        k = torch.zeros(nkv, n, D)
        qrow = case.q[q_start[b]:q_start[b] + ql].view(ql, nh, D)
        if kind == "ramp":
            pos = torch.arange(lo, L)
            k[:] = _ramp_code(RAMP_MAX - pos if descending else pos, D)
            qrow[:, :, 0] = 256 * qv
            qrow[:, :, 1] = qv
        else:
            kval = math.log(L) + 8
            for hh in range(nh):
                kvh, g = divmod(hh, G)
                d = needle_dim(g, D)
                qrow[:, hh, d] = qv
                if kind == "needle":
                    e = edges[b]
                    spots = [(e[(launch * nh + hh) % len(e)], kval)]
                else:  # mix
                    span = L - lo
                    a = lo + min(5, max(0, span - 2) // 2)
                    z = L - 1 - min(3, max(0, span - 2) // 2)
                    gap = math.log(3) if (hh // 2) % 2 == 0 else 30.0
                    strong, weak = (a, z) if hh % 2 == 0 else (z, a)
                    spots = [(strong, kval + gap)] + ([(weak, kval)] if weak != strong else [])
                for p, val in spots:
                    k[kvh, p - lo, d] = val / (qv * scale)
                case.needles[(b, hh)] = [p for p, _ in spots]
            if kind == "needle":
                case.edges[b] = sorted({p for (bb, _), ps in case.needles.items() if bb == b for p in ps})
        _write(case, b, lo, k, v)
    return case


# -- the reference and its mutants ---------------------------------------------------------------
def attention(case, rows=None, kvhs=None, hi=0, lo=0, drop=None, page_shift=0, kv_shift=0, q_shift=0, pos_shift=0,
              merge=None):
    """fp64 softmax attention of the case, reading the cache through the block table: query at
    position p attends keys [max(0, p - W + 1), p] (W = 0: [0, p]). Mutations (all default off):
    hi / lo move the upper / lower mask edge by that many keys; drop = {row: [positions]} masks
    those keys; page_shift reads page i + s for page i; kv_shift reads kv head g + s; q_shift gives
    query head g head g + s's q within its group; pos_shift moves every query's position; merge =
    "norescale" adds the blocks' partials without the max rescale, "stale" takes one block's keys
    and values (the block holding the first needle of the kv head's first query head) from
    ``case.prev``. Rows not in ``rows`` / kv heads not in ``kvhs`` stay zero."""
    nh, nkv, D, bs = case.nh, case.nkv, case.D, case.bs
    G = nh // nkv
    out = torch.zeros(case.T, nh * D, dtype=torch.float64)
    for b in (range(case.B) if rows is None else rows):
        ql, ctx, q0 = case.q_lens[b], case.ctx_lens[b], case.q_start[b]
        n = min(ctx + 1, case.bt.shape[1] * bs)  # the key one past the end can be admitted
        idx = torch.arange(n)
        pages = case.bt[b, (idx // bs + page_shift).clamp(max=case.bt.shape[1] - 1)].long()
        qpos = torch.arange(ctx - ql, ctx) + pos_shift
        ok = idx.view(1, n) <= (qpos + hi).view(ql, 1)
        if case.window > 0:
            first = qpos - case.window + 1
            first = first.clamp(min=0) + lo if lo > 0 else first + lo  # drop the first key that exists
            ok &= idx.view(1, n) >= first.view(ql, 1)
        elif lo > 0:
            ok &= idx.view(1, n) >= lo
        if drop is not None:
            ok[:, drop.get(b, [])] = False
        qb = case.q[q0:q0 + ql].view(ql, nh, D)
        for kvh in (range(nkv) if kvhs is None else kvhs):
            src = (kvh + kv_shift) % nkv
            k = case.kc[pages, src, idx % bs].double()
            v = case.vc[pages, src, idx % bs].double()
            heads = [kvh * G + (g + q_shift) % G for g in range(G)]
            qh = qb[:, heads].double()  # [ql, G, D]
            if merge == "stale":
                s0, e0 = _block_of(case, b, case.needles[(b, kvh * G)][0])
                k, v = k.clone(), v.clone()
                old = case.prev  # the same logical positions of the row, through the earlier block table
                op = old.bt[b, (idx[s0:e0] // bs).clamp(max=old.bt.shape[1] - 1)].long()
                k[s0:e0] = old.kc[op, src, idx[s0:e0] % bs].double()
                v[s0:e0] = old.vc[op, src, idx[s0:e0] % bs].double()
            s = torch.einsum("qgd,kd->gqk", qh, k) * case.scale
            s = s.masked_fill(~ok.view(1, ql, n), float("-inf"))
            if merge == "norescale":
                num, den = 0.0, 0.0
                for s0, e0 in case.blocks[b]:
                    sb = s[..., s0:e0]
                    p = torch.exp(sb - sb.max(dim=-1, keepdim=True).values)
                    num = num + p @ v[s0:e0]
                    den = den + p.sum(-1, keepdim=True)
                o = num / den
            else:
                o = torch.softmax(s, dim=-1) @ v
            out[q0:q0 + ql].view(ql, nh, D)[:, kvh * G:(kvh + 1) * G] = o.transpose(0, 1)
    return out


def _block_of(case, b, pos):
    for s0, e0 in case.blocks[b]:
        if s0 <= pos < e0:
            return s0, e0
    raise AssertionError((b, pos))


def needle_weights(case):
    """Per (row, query head) of a needle / mix case: the total softmax weight of its needles in the
    fp64 reference, for the last query of the row (decode: the only one)."""
    G = case.nh // case.nkv
    out = {}
    for (b, hh), spots in case.needles.items():
        ctx = case.ctx_lens[b]
        lo = max(0, ctx - case.window) if case.window > 0 else 0
        idx = torch.arange(lo, ctx)
        pages = case.bt[b, idx // case.bs].long()
        k = case.kc[pages, hh // G, idx % case.bs].double()
        qh = case.q[case.q_start[b] + case.q_lens[b] - 1].view(case.nh, case.D)[hh].double()
        p = torch.softmax(k @ qh * case.scale, dim=-1)
        out[(b, hh)] = float(sum(p[s - lo] for s in spots))
    return out


def multi_block(case):
    return case.blocks is not None and any(len(r) > 1 for r in case.blocks)


# Mutants: name -> (what it is, applies(case), keyword arguments of ``attention``). (e) is the
# per-edge family, see ``drop_mutants``.
MUTANTS = {
    "a_drop_last_key": (lambda c: True, dict(hi=-1)),
    "b_admit_key_past_end": (lambda c: True, dict(hi=1)),
    "c_drop_first_key": (lambda c: True, dict(lo=1)),
    # without a window, or with every row inside it, there is no key before the first one
    "d_admit_key_before_window": (lambda c: 0 < c.window < max(c.ctx_lens), dict(lo=-1)),
    "f_next_page": (lambda c: True, dict(page_shift=1)),
    "g_next_kv_head": (lambda c: c.nkv > 1, dict(kv_shift=1)),
    # the ramps give every head of a group the same q; G = 1 has no other head in the group
    # ... and where every head seeks the same key (a row of one permitted key) every q gives its V
    "h_next_q_head": (lambda c: c.nh // c.nkv > 1 and c.kind != "ramp"
                      and len({(b, tuple(p)) for (b, _), p in c.needles.items()}) > c.B, dict(q_shift=1)),
    # (i) / (j): a launch whose rows all fit one block merges nothing across blocks
    "i_merge_without_rescale": (lambda c: multi_block(c), dict(merge="norescale")),
    "j_stale_granule": (lambda c: multi_block(c) and c.prev is not None and c.prev.B >= c.B and c.kind != "ramp",
                        dict(merge="stale")),
    # (k): decode has one query per row, at L - 1 by definition: its edges are (a) - (d)
    "k_row_position_plus_1": (lambda c: max(c.q_lens) > 1, dict(pos_shift=1)),
    "k_row_position_minus_1": (lambda c: max(c.q_lens) > 1, dict(pos_shift=-1)),
}


def mutant(case, name):
    """The named mutant's output for the case, or None where it does not apply."""
    applies, kw = MUTANTS[name]
    if not applies(case):
        return None
    if name == "j_stale_granule":  # only rows with more than one block have a granule to go stale
        rows = [b for b in range(case.B) if len(case.blocks[b]) > 1 and (b, 0) in case.needles]
        out = case.ref.clone()
        out[[case.q_start[b] for b in rows]] = attention(case, rows=rows, **kw)[[case.q_start[b] for b in rows]]
        return out
    return attention(case, **kw)


def drop_mutant(case, b, pos):
    """Mutant (e): row b loses key ``pos`` (recomputed for the kv heads with a needle there; the
    others barely notice one key of thousands)."""
    G = case.nh // case.nkv
    kvhs = sorted({hh // G for (bb, hh), ps in case.needles.items() if bb == b and pos in ps})
    out = case.ref.clone()
    q0, ql = case.q_start[b], case.q_lens[b]
    new = attention(case, rows=[b], kvhs=kvhs, drop={b: [pos]})[q0:q0 + ql].view(ql, case.nkv, -1)
    out[q0:q0 + ql].view(ql, case.nkv, -1)[:, kvhs] = new[:, kvhs]
    return out


# -- the criterion -------------------------------------------------------------------------------
def mismatches(out, case):
    """(count, max error) of the elements of ``out`` beyond the project's criterion |err| <= 0.02 +
    0.02 |ref| against the fp64 reference."""
    ref = case.ref[case.rows]
    err = (out.detach().cpu().double()[case.rows] - ref).abs()
    bad = ~(err <= 0.02 + 0.02 * ref.abs())  # a NaN is a mismatch
    return int(bad.sum()), float(err.nan_to_num(nan=float("inf")).max())


def check(out, case, what=""):
    bad, worst = mismatches(out, case)
    n = len(case.rows) * case.ref.shape[1]
    assert bad == 0, f"{what}: {bad}/{n} elements off the fp64 reference, max err {worst:.4g}"


# -- the case lists of the GPU tests -------------------------------------------------------------
FUSED_LENS = [[1, 2, 31, 32], [33, 63, 64, 65], [127, 128, 129, 255], [256, 257, 2049, 4096]]
BALANCED_ROUNDS = [[5000, 130, 1], [5000, 130, 1], [300, 4999, 2], [4097, 3000, 700], [5000, 130, 1]]
MAX_LAUNCHES = 6


def decode_edges(L, form, window=0):
    """A decode row's edge list: first / last key, sub-tile and page boundaries, the first key of
    the window, and the start / end - 1 of the row's blocks (the group boundary of a two-level
    merge first, then from both ends inwards)."""
    lo = max(0, L - window) if window > 0 else 0
    blocks = decode_blocks(L, form, window)
    e = [lo, L - 1, 31, 32, 63, 64]
    order = []
    if len(blocks) > GROUP:
        order += [GROUP - 1, GROUP]
    i, j = 0, len(blocks) - 1
    while i <= j:
        order += [i, j]
        i, j = i + 1, j - 1
    for c in order:
        e += [blocks[c][0], blocks[c][1] - 1]
    seen, out = set(), []
    for p in e:
        if lo <= p < L and p not in seen:
            seen.add(p)
            out.append(p)
    return out


def needle_launches(nh, nkv, D, seqs, edges, *, min_launches=1, prev=None, **kw):
    """Launches whose needles walk every row's edge list (cut to MAX_LAUNCHES * nh edges)."""
    n = max(min_launches, min(MAX_LAUNCHES, max(-(-len(e) // nh) for e in edges)))
    out = []
    for r in range(n):
        prev = build(nh, nkv, D, "needle", seqs, edges=edges, launch=r, prev=prev, **kw)
        out.append(prev)
    return out


def decode_list(nh, nkv, D, lens, form, *, window=0, seed=0, min_launches=1, prev=None,
                kinds=("needle", "mix", "ramp")):
    """The launches of one length set on one workspace, in order: needles over the edge lists, the
    mix case, and (<= 1024 keys) the ascending ramp, with a window also the descending one."""
    seqs = [(1, L) for L in lens]
    kw = dict(window=window, form=form, seed=seed)
    out = []
    if "needle" in kinds:
        edges = [decode_edges(L, form, window) for L in lens]
        out += needle_launches(nh, nkv, D, seqs, edges, min_launches=min_launches, prev=prev, **kw)
    if "mix" in kinds:
        out.append(build(nh, nkv, D, "mix", seqs, prev=out[-1] if out else prev, launch=50, **kw))
    if "ramp" in kinds and max(lens) <= RAMP_MAX:
        out.append(build(nh, nkv, D, "ramp", seqs, prev=out[-1] if out else prev, launch=60, **kw))
        if window > 0:
            out.append(build(nh, nkv, D, "ramp", seqs, prev=out[-1], launch=61, descending=True, **kw))
    return out


def fused_lists(nh, nkv, D, chunk):
    """attn_decode's fused form: one list per batch of FUSED_LENS, >= 3 needle rounds each."""
    return [decode_list(nh, nkv, D, lens, ("fused", chunk), seed=chunk + i, min_launches=3)
            for i, lens in enumerate(FUSED_LENS)]


def balanced_list(nh, nkv, D, gc):
    """attn_decode's balanced split: the rounds of test_attn_decode_balanced_split on one workspace."""
    out = []
    for i, lens in enumerate(BALANCED_ROUNDS):
        out += decode_list(nh, nkv, D, lens, ("split", 128, gc), seed=gc * 10 + i, prev=out[-1] if out else None,
                           kinds=("needle", "mix"))
    return out


# (nh, nkv, D, form, long length): gc = 256 / 300 balanced blocks, and the fixed-chunk form's 256 chunks
TWO_LEVEL = [(4, 1, 128, ("split", 128, 256), 33000), (16, 2, 128, ("split", 128, 300), 33000),
             (4, 1, 128, ("fused", 128), 32767)]


def two_level_list(nh, nkv, D, form, long=33000):
    """One long row (33 000 keys: fills a 256-block grid) and one short (130) on one workspace."""
    out = []
    for i, lens in enumerate([[long, 130], [130, long]]):
        out += decode_list(nh, nkv, D, lens, form, seed=77 + i, prev=out[-1] if out else None, kinds=("needle", "mix"))
    return out


WINDOWS = [1, 32, 100, 128, 1000]
WINDOW_LENS = [[1, 31, 32, 33], [99, 100, 101, 127], [128, 129, 300, 999], [1000, 1001, 1024, 257]]
WINDOW_LONG = [2049, 4096, 1000]


def window_lists(nh, nkv, D, form):
    """Windowed decode: every W against lengths below, at and above it (ramps both ways, needles
    with the first one at L - W), and longer rows with needles alone."""
    out = []
    for i, W in enumerate(WINDOWS):
        for j, lens in enumerate(WINDOW_LENS):
            out.append(decode_list(nh, nkv, D, lens, form, window=W, seed=300 + 10 * i + j))
        out.append(decode_list(nh, nkv, D, WINDOW_LONG, form, window=W, seed=390 + i, kinds=("needle", "mix")))
    return out


PREFILL_SEQS = {"full": [(300, 300)], "chunk": [(200, 1000), (64, 64)], "ragged": [(1, 1), (33, 97), (130, 700)],
                "tile": [(257, 513)]}
PREFILL_WINDOWS = [1, 64, 100]


def prefill_edges(ql, ctx):
    """Needle positions of a prefill row: key 0, the diagonals of its first and last query and of
    the queries either side of the 64- / 128- / 256-row tile boundaries, the 64-key tile boundary."""
    first = ctx - ql
    e = [0, first, ctx - 1, 63, 64] + [first + r for r in (63, 64, 127, 128, 255, 256)]
    seen, out = set(), []
    for p in e:
        if 0 <= p < ctx and p not in seen:
            seen.add(p)
            out.append(p)
    return out


def prefill_list(nh, nkv, D, name, *, window=0, bs=64, seqs=None):
    """Prefill launches: the ascending ramp (every row's causal edge), with a window the descending
    one (every row's lower edge), without one the needles on the diagonals. Three rows that belong
    to no sequence follow each sequence's queries."""
    seqs = PREFILL_SEQS[name] if seqs is None else seqs
    kw = dict(window=window, bs=bs, seed=500 + len(name), pad=3)
    out = [build(nh, nkv, D, "ramp", seqs, launch=60, **kw)]
    if window > 0:
        out.append(build(nh, nkv, D, "ramp", seqs, launch=61, descending=True, **kw))
    else:
        out += needle_launches(nh, nkv, D, seqs, [prefill_edges(ql, ctx) for ql, ctx in seqs], **kw)
    return out


SMALL_PAGE_SEQS = [(130, 700), (40, 40)]  # test_attn_prefill_window_small_pages: 16-key pages


OPROJ_SHAPE = (8, 2, 128, 1024)  # nh, nkv, D, H
OPROJ_LENS = [1, 33, 1000]
OPROJ_CHUNK = 32  # ops.attn_oproj_chunk(1024, ops.attn_oproj_grid(1024, 8, 2, 128)): 128 blocks per kv head


def oproj_list(nh, nkv, D, L, chunk):
    """attn_oproj's attention (one row, fixed ``chunk``-key blocks): needles and the mix case."""
    return decode_list(nh, nkv, D, [L], ("fused", chunk), seed=900 + L, min_launches=2, kinds=("needle", "mix"))


# -- qkv_attn: q comes from the projection ---------------------------------------------------------
QKV_SHAPE = (4, 1, 128, 4096)  # nh, nkv, D, K: SHAPES[0] of tests/test_qkv_attn_gpu.py
QKV_CHUNK, QKV_GC = 128, 8     # the 1024-key bucket
QKV_LENS = [1, 2, 33, 128, 129, 257, 700]  # 129 / 257: the last block holds the new key alone
_QKV_INPUTS = {}


def _qkv_inputs():
    """x, norm weight and W of the projection (shared by every case) and the unrotated bf16 qkv row."""
    from llm_consensus_amd.ops import oracle

    if not _QKV_INPUTS:
        nh, nkv, D, K = QKV_SHAPE
        gen = torch.Generator().manual_seed(4242)
        x = torch.randn(1, K, generator=gen).to(BF)
        nw = (1 + 0.1 * torch.randn(K, generator=gen)).to(BF)
        W = (torch.randn((nh + 2 * nkv) * D, K, generator=gen) / math.sqrt(K)).to(BF)
        _QKV_INPUTS.update(x=x, nw=nw, W=W, qkv=oracle.linear(x, W, 0, None, nw, 1e-5))
    return _QKV_INPUTS


def qkv_case(L, kind, launch=0, prev=None, bs=64):
    """A qkv_attn case: the launch projects the token at position L - 1, writes its K / V and attends
    the L - 1 cached keys and the new one. q is the oracle's rotated projection output, so a cached
    needle for head h is alpha q_h with alpha |q_h|^2 scale = ln(L) + 10 (two more than the one-hot
    needles: the heads' q are not orthogonal, so a head also scores the other heads' needles; kind "needle": the needles
    walk the fused form's edge list over the cached keys; nothing to place at L = 1, where the
    output is the new token's V) or, kind "repel", every cached key is -alpha sum_g q_g: the new key
    must dominate. ``kc`` / ``vc`` are the cache AFTER the launch (the oracle's new K / V at L - 1),
    ``kc_pre`` / ``vc_pre`` the one before it, where that slot still holds poison."""
    from llm_consensus_amd.ops import oracle

    nh, nkv, D, K = QKV_SHAPE
    G = nh // nkv
    inp = _qkv_inputs()
    gen = torch.Generator().manual_seed(7000 + 10 * L + launch)
    scale = 1 / math.sqrt(D)
    form = ("fused", QKV_CHUNK)
    kc, vc, bt = _pool([L], nkv, D, bs, gen, torch.zeros(D, dtype=BF))
    theta = 500000.0
    inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    cos, sin = oracle.rope_tables(inv.tolist(), bt.shape[1] * bs + 8)
    pos = torch.tensor([L - 1], dtype=torch.int32)
    slots = torch.tensor([int(bt[0, (L - 1) // bs]) * bs + (L - 1) % bs], dtype=torch.int32)
    q = torch.zeros(1, nh * D, dtype=BF)
    k_new, v_new = torch.zeros_like(kc), torch.zeros_like(vc)
    oracle.rope_kv_write(inp["qkv"], pos, cos, sin, k_new, v_new, slots, nh, nkv, D, bs, q)
    qh = q.view(nh, D).double()
    case = Case(nh=nh, nkv=nkv, D=D, bs=bs, scale=scale, kind=kind, bt=bt, q=q, q_start=[0], q_lens=[1], ctx_lens=[L],
                T=1, prev=prev, form=form, blocks=[decode_blocks(L, form)], cos=cos, sin=sin, pos=pos, slots=slots,
                **inp)
    target = math.log(L) + 10
    # poison: 2.5 x the strongest needle for the head it attracts least
    for kvh in range(nkv):
        grp = qh[kvh * G:(kvh + 1) * G]
        tot = grp.sum(0)
        least = float((grp @ tot).min()) * scale
        assert least > 0
        kc[:, kvh] = (tot * 2.5 * (target + 30) / least).to(BF)
    case.kc, case.vc = kc, vc
    n = L - 1
    if n > 0:
        v = torch.randint(0, 2, (nkv, n, D), generator=gen).float() * 2 - 1
        k = torch.zeros(nkv, n, D)
        edges = [p for p in decode_edges(L, form) if p < n] or [0]
        for hh in range(nh):
            kvh = hh // G
            if kind == "needle":
                p = edges[(launch * nh + hh) % len(edges)]
                k[kvh, p] += (qh[hh] * target / (float(qh[hh] @ qh[hh]) * scale)).float()
                case.needles[(0, hh)] = [p]
            else:
                grp = qh[kvh * G:(kvh + 1) * G]
                tot = grp.sum(0)
                k[kvh, :] = -(tot * target / (float((grp @ tot).min()) * scale)).float()
                case.needles[(0, hh)] = [L - 1]
        _write(case, 0, 0, k, v)
    else:
        case.needles = {(0, hh): [0] for hh in range(nh)}
    case.edges[0] = sorted({p for ps in case.needles.values() for p in ps})
    case.kc_pre, case.vc_pre = case.kc.clone(), case.vc.clone()
    page, off = int(slots[0]) // bs, int(slots[0]) % bs
    case.kc[page, :, off] = k_new[page, :, off]
    case.vc[page, :, off] = v_new[page, :, off]
    return case


def qkv_list(L):
    """Two needle launches (none at L = 1) and the repelling cache, on one workspace."""
    out = []
    for r in range(2 if L > 1 else 1):
        out.append(qkv_case(L, "needle", r, out[-1] if out else None))
    if L > 1:
        out.append(qkv_case(L, "repel", 5, out[-1]))
    return out


# -- scale-aware bounds of the long-context random tests -----------------------------------------
def dense_decode(q, kc, vc, bt, lens, nh, nkv, D, bs, scale, window=0):
    """Unrounded fp64 decode attention on the tensors' own device: [B, nh * D]."""
    G = nh // nkv
    out = torch.zeros(len(lens), nh * D, dtype=torch.float64, device=q.device)
    for b, L in enumerate(lens):
        idx = torch.arange(max(0, L - window) if window > 0 else 0, L, device=q.device)
        pages = bt[b].to(q.device).long()[idx // bs]
        for kvh in range(nkv):
            k = kc[pages, kvh, idx % bs].double()
            v = vc[pages, kvh, idx % bs].double()
            qg = q[b].view(nh, D)[kvh * G:(kvh + 1) * G].double()
            out[b].view(nh, D)[kvh * G:(kvh + 1) * G] = torch.softmax(qg @ k.t() * scale, dim=-1) @ v
    return out


def dense_prefill(q, kc, vc, bt, q_start, q_lens, ctx_lens, nh, nkv, D, bs, scale):
    """Unrounded fp64 causal prefill attention on the tensors' own device: [T, nh * D]."""
    G = nh // nkv
    out = torch.zeros(q.shape[0], nh * D, dtype=torch.float64, device=q.device)
    for b, (q0, ql, ctx) in enumerate(zip(q_start, q_lens, ctx_lens)):
        idx = torch.arange(ctx, device=q.device)
        pages = bt[b].to(q.device).long()[idx // bs]
        dead = idx.view(1, 1, ctx) > torch.arange(ctx - ql, ctx, device=q.device).view(1, ql, 1)
        for kvh in range(nkv):
            k = kc[pages, kvh, idx % bs].double()
            v = vc[pages, kvh, idx % bs].double()
            qg = q[q0:q0 + ql].view(ql, nh, D)[:, kvh * G:(kvh + 1) * G].double()
            s = (torch.einsum("qgd,kd->gqk", qg, k) * scale).masked_fill(dead, float("-inf"))
            out[q0:q0 + ql].view(ql, nh, D)[:, kvh * G:(kvh + 1) * G] = (torch.softmax(s, dim=-1) @ v).transpose(0, 1)
    return out


def rms_ratio(a, ref):
    return float((a.double() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())


# name -> (bound on rms(out - ref) / rms(ref), smallest length of the test, nh, nkv, D). The bound
# is twice the largest ratio the kernel gave over the test's cases and launches on an MI355X; the
# floor is rms(bf16(ref) - ref) / rms(ref), rounding the output alone (largest over the same runs).
RMS_BOUNDS = {
    "decode_wide_split": (0.0063, 130, 4, 1, 128),                 # kernel 0.003149, floor 0.001705
    "decode_fused_long_context": (0.0061, 130, 4, 1, 128),         # kernel 0.003061, floor 0.001744
    "decode_fused_window_long_context": (0.0061, 130, 4, 1, 128),  # kernel 0.003056, floor 0.001726
    "decode_split_window_two_level": (0.0063, 9000, 4, 1, 128),    # kernel 0.003162, floor 0.001670
    "prefill_long_context": (0.0040, 300, 8, 2, 128),              # kernel 0.001978, floor 0.001590
}


def assert_rms(out, ref, name):
    """The scale-aware bound of a random-data test: the close() criterion's 0.02 absolute term is as
    large as the whole signal at long contexts; this one is relative to the signal."""
    ratio, floor = rms_ratio(out, ref), rms_ratio(ref.to(BF), ref)
    print(f"RMS {name}: kernel {ratio:.6f} output-rounding floor {floor:.6f}")
    assert ratio <= RMS_BOUNDS[name][0], (name, ratio, floor, RMS_BOUNDS[name][0])
