"""The attention kernels on a real MI355X against the structured probes of tests/attn_probe.py
(position-coded V, poison in every slot a row must not read, needles on the mask / page / chunk /
block / window edges, unequal needles across blocks, score ramps): a missing, extra or misplaced key
moves the output by about 1, far beyond ``check``'s |err| <= 0.02 + 0.02 |ref| against the fp64
reference. tests/test_attn_probe_cpu.py proves, without a GPU, that every case list used here rejects
every applicable mutant of the reference."""

import pytest
import torch

import attn_probe as ap
from llm_consensus_amd import ops

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
UNTOUCHED = 7.0


class _Decode:
    """One attn_decode workspace and the launches that ran on it."""

    def __init__(self, B, nh, nkv, D, gc, fused):
        self.B, self.gc, self.fused = B, gc, fused
        self.part, self.ctr = ops.decode_attn_workspace(B, nh, nkv, D, gc, "cuda", fused=fused)
        self.fault = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.merges = torch.zeros(B, dtype=torch.int32)  # launches in which the row merged

    def run(self, case, what):
        q, kc, vc, bt, _, _, sl = case.tensors("cuda")
        out = torch.full((case.B, case.nh * case.D), UNTOUCHED, dtype=BF, device="cuda")
        ops.attn_decode(q, kc, vc, bt, sl, out, self.part, self.ctr, case.nh, case.nkv, case.D, case.bs, case.form[1],
                        case.scale, grid_chunks=self.gc, fused=self.fused, fault=self.fault, window=case.window)
        torch.cuda.synchronize()
        assert int(self.fault.item()) == 0, what
        ap.check(out, case, what)
        for b, blocks in enumerate(case.blocks):
            self.merges[b] += len(blocks) > 1

    def tickets_rearmed(self, epochs=False):
        """Every ticket is 0 again; fused one-level workspaces: the epoch of every (row, kv head)
        advanced once per launch that merged, and nothing else on the counter lines was written."""
        ctr = self.ctr.cpu()
        tickets = torch.cat([ctr[..., :1, 0], ctr[..., 2:, 0]], dim=-1)
        assert int(tickets.abs().sum()) == 0, ctr
        if epochs:
            assert torch.equal(ctr[..., 1, 0], self.merges.view(-1, 1).expand(self.B, ctr.shape[1])), ctr
            assert int(ctr[..., 1:].abs().sum()) == 0  # one word per 128-B counter line


@pytest.mark.parametrize("nh,nkv,D", ap.SHAPES)
@pytest.mark.parametrize("chunk", [128, 256])
def test_attn_decode_fused_probes(cuda, nh, nkv, D, chunk):
    """Fixed-chunk form, lengths 1 .. 4096 in batches of four on ONE workspace: per batch at least
    three needle rounds (the needles move along the edge list: sub-tile, page and chunk boundaries,
    first and last key), the unequal needles of the mix case, and the ramp up to 1024 keys."""
    ws = _Decode(4, nh, nkv, D, 4096 // chunk, True)
    for lens, cases in zip(ap.FUSED_LENS, ap.fused_lists(nh, nkv, D, chunk)):
        for i, case in enumerate(cases):
            ws.run(case, f"lens {lens} launch {i} ({case.kind})")
    ws.tickets_rearmed(epochs=True)


@pytest.mark.parametrize("nh,nkv,D", ap.SHAPES[:3])
@pytest.mark.parametrize("gc", [1, 3, 7, 64])
def test_attn_decode_balanced_split_probes(cuda, nh, nkv, D, gc):
    """Balanced split: needles on the start / end - 1 of the blocks that the ported decode_range
    gives each round's lengths; the lengths change between rounds on one workspace."""
    ws = _Decode(3, nh, nkv, D, gc, False)
    for i, case in enumerate(ap.balanced_list(nh, nkv, D, gc)):
        ws.run(case, f"launch {i} lens {case.ctx_lens} ({case.kind})")
    ws.tickets_rearmed()


@pytest.mark.parametrize("nh,nkv,D,form,long", ap.TWO_LEVEL)
def test_attn_decode_two_level_probes(cuda, nh, nkv, D, form, long):
    """More than 32 blocks per row: groups of 16 merge first, then the group results. A long row
    and a short one swap places on one workspace; needles on the group boundary and the outermost
    blocks, the mix case across the first and the last group."""
    fused = form[0] == "fused"
    ws = _Decode(2, nh, nkv, D, 256 if fused else form[2], fused)
    for i, case in enumerate(ap.two_level_list(nh, nkv, D, form, long)):
        ws.run(case, f"launch {i} lens {case.ctx_lens} ({case.kind})")
    ws.tickets_rearmed()


@pytest.mark.parametrize("nh,nkv,D", ap.SHAPES[:3])
@pytest.mark.parametrize("form", [("fused", 128), ("fused", 256), ("split", 128, 3)], ids=str)
def test_attn_decode_window_probes(cuda, nh, nkv, D, form):
    """Sliding window W in {1, 32, 100, 128, 1000} against lengths below, at and above W, all on
    one workspace: the first needle at L - W with poison at L - W - 1, the descending ramp on the
    lower edge, the ascending one on the upper."""
    fused = form[0] == "fused"
    ws = _Decode(4, nh, nkv, D, 4096 // form[1] if fused else form[2], fused)
    for cases in ap.window_lists(nh, nkv, D, form):
        for i, case in enumerate(cases):
            ws.run(case, f"W {case.window} lens {case.ctx_lens} launch {i} ({case.kind})")
    ws.tickets_rearmed(epochs=fused)


def _prefill(case, what, **kw):
    q, kc, vc, bt, qs, ql, cl = case.tensors("cuda")
    out = torch.full((case.T, case.nh * case.D), UNTOUCHED, dtype=BF, device="cuda")
    ops.attn_prefill(q, kc, vc, bt, qs, ql, cl, out, max(case.q_lens), case.nh, case.nkv, case.D, case.bs, case.scale,
                     max_ctx=max(case.ctx_lens), window=case.window, **kw)
    torch.cuda.synchronize()
    ap.check(out, case, f"{what} {kw}")
    foreign = sorted(set(range(case.T)) - set(case.rows))
    assert bool((out[foreign] == UNTOUCHED).all()), f"{what} {kw}: a row of no sequence was written"


def _window_forms(nh, nkv, D, bs):
    """The block forms that implement the window (tests/test_sliding_window_gpu.py): not the paired
    row tiles (G <= 4 dividing 8) nor the key halves (D = 128 on 64-key pages)."""
    G = nh // nkv
    refused = ([1] if G <= 4 and 8 % G == 0 else []) + ([3] if D == 128 and bs == 64 else [])
    return [f for f in (None, 0, 1, 2, 3) if f not in refused]


@pytest.mark.parametrize("nh,nkv,D", ap.SHAPES)
@pytest.mark.parametrize("name", list(ap.PREFILL_SEQS))
def test_attn_prefill_probes(cuda, nh, nkv, D, name):
    """Every block form and KV split: the ascending ramp pins every row's causal edge (the
    chunked-prefill offset ctx - qlen included), needles sit on the diagonals of the first / last
    query and of the row-tile boundaries; windowed, the descending ramp pins every row's lower
    edge. Rows of no sequence stay untouched."""
    for i, case in enumerate(ap.prefill_list(nh, nkv, D, name)):
        for form in (0, 1, 2, 3):
            _prefill(case, f"launch {i} ({case.kind})", ksplit=1, form=form)
        for ksplit in (1, 2, 4):
            _prefill(case, f"launch {i} ({case.kind})", ksplit=ksplit, kmin=1)
    for W in ap.PREFILL_WINDOWS:
        for i, case in enumerate(ap.prefill_list(nh, nkv, D, name, window=W)):
            for form in _window_forms(nh, nkv, D, 64):
                _prefill(case, f"W {W} launch {i}", ksplit=1, form=form)


def test_attn_prefill_small_page_probes(cuda):
    """16-key pages: the per-key page lookup of the register-staged forms, windowed."""
    for W in (33, 100):
        for i, case in enumerate(ap.prefill_list(8, 2, 128, "small", window=W, bs=16, seqs=ap.SMALL_PAGE_SEQS)):
            for form in (0, 2):
                _prefill(case, f"W {W} launch {i}", ksplit=1, form=form)


@pytest.mark.parametrize("L", ap.OPROJ_LENS)
def test_attn_oproj_probes(cuda, L):
    """The attention of the fused attention + o_proj launch (its ``attn_out``) on the needle and mix
    cases, one workspace through all launches, in both weight-request modes."""
    nh, nkv, D, H = ap.OPROJ_SHAPE
    nc = ops.attn_oproj_grid(H, nh, nkv, D)
    chunk = ops.attn_oproj_chunk(1024, nc)
    assert nc > 0 and chunk == ap.OPROJ_CHUNK, (nc, chunk)  # the edge lists were cut for this chunk
    torch.manual_seed(L)
    w_o = (torch.randn(H, nh * D, device="cuda") / (nh * D) ** 0.5).to(BF)
    ws = ops.attn_oproj_workspace(H, nh, nkv, D, nc, "cuda")
    fault = torch.zeros(1, dtype=torch.int32, device="cuda")
    for i, case in enumerate(ap.oproj_list(nh, nkv, D, L, chunk)):
        q, kc, vc, bt, _, _, sl = case.tensors("cuda")
        for mode in (-1, 1):
            h = torch.zeros(1, H, dtype=BF, device="cuda")
            attn = torch.full((1, nh * D), UNTOUCHED, dtype=BF, device="cuda")
            ops.attn_oproj(q, kc, vc, bt, sl, w_o, h, attn, ws, nh, nkv, D, case.bs, chunk, nc, case.scale, fault=fault,
                           mode=mode)
            torch.cuda.synchronize()
            assert int(fault.item()) == 0
            ap.check(attn, case, f"launch {i} ({case.kind}) mode {mode}")


@pytest.mark.parametrize("L", ap.QKV_LENS)
def test_qkv_attn_probes(cuda, L):
    """The one-launch qkv projection + attention: q comes from the projection, so the cached needles
    are multiples of the oracle's rotated q_h; the self-key that wave 0 folds in is pinned by L = 1
    (the output is the new token's V) and by a cache that repels every head (the new key must
    dominate). The cache slot of the new key holds poison before the launch."""
    nh, nkv, D, K = ap.QKV_SHAPE
    assert ops.qkv_attn_supported(nh, nkv, D, K)
    part, ctr = ops.decode_attn_workspace(1, nh, nkv, D, ap.QKV_GC, "cuda", fused=True)
    ws = ops.qkv_attn_workspace(nh, nkv, D, "cuda")
    fault = torch.zeros(1, dtype=torch.int32, device="cuda")
    for i, case in enumerate(ap.qkv_list(L)):
        _, _, _, bt, _, _, sl = case.tensors("cuda")
        kc, vc = case.kc_pre.cuda(), case.vc_pre.cuda()
        q = torch.zeros(1, nh * D, dtype=BF, device="cuda")
        out = torch.full((1, nh * D), UNTOUCHED, dtype=BF, device="cuda")
        ops.qkv_attn(case.x.cuda(), case.W.cuda(), case.nw.cuda(), 1e-5, q, kc, vc, case.pos.cuda(), case.slots.cuda(),
                     case.cos.cuda(), case.sin.cuda(), bt, sl, out, part, ctr, ws, nh, nkv, D, case.bs, ap.QKV_CHUNK,
                     ap.QKV_GC, case.scale, fault=fault)
        torch.cuda.synchronize()
        assert int(fault.item()) == 0
        # the projection against the oracle's (the bound of test_gemv_qkv_rope), the rest of the cache untouched
        for got, want in ((q, case.q), (kc, case.kc), (vc, case.vc)):
            err = (got.float().cpu() - want.float()).abs()
            assert bool((err <= 3e-2 + 0.02 * want.float().abs()).all()), (i, float(err.max()))
        ap.check(out, case, f"launch {i} ({case.kind})")
