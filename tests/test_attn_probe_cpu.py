"""The attention probes discriminate (no GPU): for every case list tests/test_attn_probe_gpu.py feeds
to a kernel, the fp64 reference rounded to bf16 passes ``attn_probe.check``, every needle holds its
head's softmax weight, and every mutant of the reference that applies to the list (a dropped or
admitted key at either mask edge, a dropped edge key, a wrong page / kv head / q head, a merge
without the max rescale, a stale granule, a row position off by one) is rejected by ``check`` on at
least one case of the list. Plus: the scale-aware bounds of the long-context random tests lie
below half of what the mildest structural mutant produces."""

import math

import pytest
import torch

import attn_probe as ap

BF = torch.bfloat16

# Mutants that apply to no case of a list, with the reason (anything else must be caught).
NOT_APPLICABLE = {
    "d_admit_key_before_window": "no window, or every row inside it: there is no key before the first one",
    "g_next_kv_head": "one kv head",
    "h_next_q_head": "G = 1, ramps only (every head of a group has the same q), or one key per row",
    "i_merge_without_rescale": "every row fits one block: nothing is merged across blocks",
    "j_stale_granule": "every row fits one block, or no earlier launch on the workspace",
    "k_row_position_plus_1": "decode: one query per row, at L - 1 by definition; (a) - (d) are its edges",
    "k_row_position_minus_1": "decode: one query per row, at L - 1 by definition; (a) - (d) are its edges",
}


def _rejected(out, case):
    return ap.mismatches(out, case)[0] > 0


def verify(cases, expect_na=()):
    """The acceptance gate for one case list."""
    for i, c in enumerate(cases):
        ap.check(c.ref.to(BF), c, f"case {i}: the reference itself")
        # rows of no sequence are zero in the reference (the GPU tests check them separately)
        for (b, hh), w in ap.needle_weights(c).items():
            assert w >= 0.999, (i, b, hh, w)
    na = []
    for name in ap.MUTANTS:
        outs = (ap.mutant(c, name) for c in cases)
        applicable = False
        for c, out in zip(cases, outs):
            if out is None:
                continue
            applicable = True
            if _rejected(out, c):
                break
        else:
            assert not applicable, f"mutant {name} passes check on every case of the list"
            assert name in NOT_APPLICABLE, name
            na.append(name)
    assert set(na) <= set(expect_na), (na, expect_na)
    # (e): every edge of every row, in the launch that has a needle there
    for i, c in enumerate(cases):
        for b, edges in c.edges.items():
            for p in edges:
                assert _rejected(ap.drop_mutant(c, b, p), c), f"case {i}: row {b} may lose key {p} unnoticed"
    return na


DECODE_NA = ("d_admit_key_before_window", "k_row_position_plus_1", "k_row_position_minus_1")
G1 = ("h_next_q_head",)
MERGE = ("i_merge_without_rescale", "j_stale_granule")


def _shape_na(nh, nkv):
    return (G1 if nh == nkv else ()) + (("g_next_kv_head",) if nkv == 1 else ())


@pytest.mark.parametrize("nh,nkv,D", ap.SHAPES)
@pytest.mark.parametrize("chunk", [128, 256])
def test_fused_lists(nh, nkv, D, chunk):
    for lens, cases in zip(ap.FUSED_LENS, ap.fused_lists(nh, nkv, D, chunk)):
        single = max(lens) <= chunk
        verify(cases, DECODE_NA + _shape_na(nh, nkv) + (MERGE if single else ()))


@pytest.mark.parametrize("nh,nkv,D", ap.SHAPES[:3])
@pytest.mark.parametrize("gc", [1, 3, 7, 64])
def test_balanced_lists(nh, nkv, D, gc):
    na = verify(ap.balanced_list(nh, nkv, D, gc),
                DECODE_NA + _shape_na(nh, nkv) + (("i_merge_without_rescale", "j_stale_granule") if gc == 1 else ()))
    assert ("i_merge_without_rescale" in na) == (gc == 1)


def test_ported_decode_range_covers_every_key():
    """The Python port of decode_nsplit / decode_range: contiguous 32-key-aligned blocks over [0, L),
    each at least half the minimum chunk where the row is split at all (ceil(L / 128) blocks)."""
    for L in (1, 2, 130, 300, 700, 3000, 4097, 4999, 5000, 33000, 40000):
        for gc in (1, 3, 7, 64, 256, 300):
            blocks = ap.decode_blocks(L, ("split", 128, gc))
            assert blocks[0][0] == 0 and blocks[-1][1] == L and len(blocks) <= gc
            assert all(a[1] == b[0] and b[0] % 32 == 0 for a, b in zip(blocks, blocks[1:]))
            assert len(blocks) == 1 or min(e - s for s, e in blocks) >= 64


@pytest.mark.parametrize("nh,nkv,D,form,long", ap.TWO_LEVEL)
def test_two_level_lists(nh, nkv, D, form, long):
    cases = ap.two_level_list(nh, nkv, D, form, long)
    assert max(len(r) for c in cases for r in c.blocks) > ap.ONE_LEVEL  # the merge has two levels
    verify(cases, DECODE_NA + _shape_na(nh, nkv))


@pytest.mark.parametrize("nh,nkv,D", ap.SHAPES[:3])
@pytest.mark.parametrize("form", [("fused", 128), ("fused", 256), ("split", 128, 3)], ids=str)
def test_window_lists(nh, nkv, D, form):
    na_w = tuple(n for n in DECODE_NA if n != "d_admit_key_before_window") + _shape_na(nh, nkv)
    for cases in ap.window_lists(nh, nkv, D, form):
        # the merge mutants apply only where a windowed row still spans two blocks
        verify(cases, na_w + ("i_merge_without_rescale", "j_stale_granule", "d_admit_key_before_window",
                              "h_next_q_head"))


@pytest.mark.parametrize("nh,nkv,D", ap.SHAPES)
@pytest.mark.parametrize("name", list(ap.PREFILL_SEQS))
def test_prefill_lists(nh, nkv, D, name):
    pre_na = ("d_admit_key_before_window", "i_merge_without_rescale", "j_stale_granule") + _shape_na(nh, nkv)
    verify(ap.prefill_list(nh, nkv, D, name), pre_na)
    for W in ap.PREFILL_WINDOWS:
        verify(ap.prefill_list(nh, nkv, D, name, window=W),
               ("i_merge_without_rescale", "j_stale_granule", "h_next_q_head") + _shape_na(nh, nkv))


def test_prefill_small_page_lists():
    for W in (33, 100):
        verify(ap.prefill_list(8, 2, 128, "small", window=W, bs=16, seqs=ap.SMALL_PAGE_SEQS),
               ("i_merge_without_rescale", "j_stale_granule", "h_next_q_head"))


@pytest.mark.parametrize("L", ap.OPROJ_LENS)
def test_oproj_lists(L):
    nh, nkv, D, _ = ap.OPROJ_SHAPE
    verify(ap.oproj_list(nh, nkv, D, L, ap.OPROJ_CHUNK),
           DECODE_NA + (("i_merge_without_rescale", "j_stale_granule") if L <= ap.OPROJ_CHUNK else ())
           + (("h_next_q_head",) if L == 1 else ()))


@pytest.mark.parametrize("L", ap.QKV_LENS)
def test_qkv_lists(L):
    """q from the projection (the oracle's): needles alpha q_h, and the cache that repels every head
    so that the launch's own new key must carry the output."""
    cases = ap.qkv_list(L)
    one_block = L <= ap.QKV_CHUNK
    verify(cases, DECODE_NA + ("g_next_kv_head",) + (MERGE if one_block else ())
           + (("h_next_q_head",) if L <= 2 else ()))  # one cached key: every head's needle


# -- the scale-aware bounds of the long-context random tests ----------------------------------------
def _random_decode(L, nh, nkv, D, seed):
    """The long-context tests' data (N(0, 1) q, K, V rounded to bf16) and its fp64 attention."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(nh, D, generator=g).to(BF).double()
    k = torch.randn(L, nkv, D, generator=g).to(BF).double().repeat_interleave(nh // nkv, dim=1)
    v = torch.randn(L, nkv, D, generator=g).to(BF).double().repeat_interleave(nh // nkv, dim=1)
    return q, k, v


def _attend(q, k, v, scale):
    return torch.einsum("hl,lhd->hd", torch.softmax(torch.einsum("hd,lhd->hl", q, k) * scale, dim=-1), v)


def _ratio(a, ref):
    return float((a - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())


@pytest.mark.parametrize("name", list(ap.RMS_BOUNDS))
def test_rms_bounds_sit_below_the_mildest_mutant(name):
    """Each bound (twice the kernel's measured rms(out - ref) / rms(ref), recorded beside it) is at
    most half the ratio of the mildest of: drop one 64-key page, swap two pages' V, scale x 1.05 —
    on the test's own kind of data at its smallest length — and above the bf16 output-rounding
    floor."""
    bound, L, nh, nkv, D = ap.RMS_BOUNDS[name]
    q, k, v = _random_decode(L, nh, nkv, D, 1)
    scale = 1 / math.sqrt(D)
    ref = _attend(q, k, v, scale)
    keep = torch.ones(L, dtype=torch.bool)
    keep[L - 64 - L % 64:L - L % 64] = False  # the last whole page
    vs = v.clone()
    vs[0:64], vs[64:128] = v[64:128], v[0:64]
    mutants = {"drop_page": _attend(q, k[keep], v[keep], scale), "swap_pages": _attend(q, k, vs, scale),
               "scale_1.05": _attend(q, k, v, 1.05 * scale)}
    mild = min(_ratio(m, ref) for m in mutants.values())
    floor = _ratio(ref.to(BF).double(), ref)
    assert floor < bound <= mild / 2, (name, floor, bound, mild, {n: _ratio(m, ref) for n, m in mutants.items()})
