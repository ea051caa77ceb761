"""Sliding-window attention on a real MI355X: the windowed decode (fused and split forms) and
prefill kernels against the fp32 oracle, and windowed engines (``mistral-tiny``, a windowed
``phi3-tiny``) against the CPU-oracle engine. Window W: position p attends keys (p - W, p]."""

import copy
import math

import pytest
import torch

import attn_probe
from llm_consensus_amd import ops
from llm_consensus_amd.engine import Engine, EngineConfig
from llm_consensus_amd.models.config import FAMILIES
from llm_consensus_amd.models.transformer import TransformerWeights
from llm_consensus_amd.ops import oracle
from llm_consensus_amd.parallel.comm import TPGroup

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SHAPES = [(32, 8, 128), (32, 32, 96), (4, 2, 64)]

FAMILIES.setdefault("phi3-tiny-swa", FAMILIES["phi3-tiny"].with_(name="phi3-tiny-swa", sliding_window=33))


def rnd(*shape, scale=1.0, dev="cuda"):
    return (torch.randn(*shape, device=dev) * scale).to(BF)


def close(a, b, atol, rtol=0.02):
    a = a.float().cpu()
    b = b.float().cpu()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol).sum().item()
    assert bad == 0, f"{bad}/{a.numel()} mismatches, max err {err.max().item():.4g}"


def _paged_kv(B, L_max, nkv, D, bs):
    nblk_per = (L_max + bs - 1) // bs
    nb = B * nblk_per + 3
    kc = rnd(nb, nkv, bs, D)
    vc = rnd(nb, nkv, bs, D)
    perm = torch.randperm(nb)[: B * nblk_per].view(B, nblk_per).to(torch.int32)
    return kc, vc, perm


# -- decode, fused form ---------------------------------------------------------------------------
def _live_chunks(L, W, chunk):
    lo = max(0, L - W) if W > 0 else 0
    return (L + chunk - 1) // chunk - lo // chunk


@pytest.mark.parametrize("nh,nkv,D", SHAPES)
@pytest.mark.parametrize("lens", [[1, 7, 100, 101], [128, 129, 257, 300], [1000, 2049, 4095, 4096]])
@pytest.mark.parametrize("chunk", [128, 256])
def test_attn_decode_fused_window(cuda, nh, nkv, D, lens, chunk):
    """Fixed-chunk form: the blocks of chunks below the window exit, the others merge as the live
    chunks. One workspace through six launches whose windows make a row's live chunk count shrink
    and grow (W = 1 at L = 300: chunk 128 leaves the only live chunk's first wave wholly below the
    window, chunk 256 a dead 32-key sub-tile inside a live 64-key wave; W = 33 at L = 300: one live
    chunk, stored directly although L > chunk; L = W and L = W + 1 at 100 / 101 and 128 / 129).
    Afterwards every ticket is 0 and a row's epoch advanced once per launch that merged."""
    torch.manual_seed(3)
    B, bs = len(lens), 64
    kc, vc, bt = _paged_kv(B, max(lens), nkv, D, bs)
    q = rnd(B, nh * D)
    sl = torch.tensor(lens, dtype=torch.int32)
    gc = 4096 // chunk
    part, ctr = ops.decode_attn_workspace(B, nh, nkv, D, gc, "cuda", fused=True)
    out = torch.empty(B, nh * D, dtype=BF, device="cuda")
    scale = 1 / math.sqrt(D)
    qc, kcc, vcc = q.cpu(), kc.cpu(), vc.cpu()
    windows = [5000, 1, 1000, 33, 128, 100]
    for W in windows:
        ref = oracle.attn_decode(qc, kcc, vcc, bt, sl, nh, nkv, D, bs, scale, W)
        out.zero_()
        ops.attn_decode(q, kc, vc, bt.cuda(), sl.cuda(), out, part, ctr, nh, nkv, D, bs, chunk, scale, grid_chunks=gc,
                        fused=True, window=W)
        close(out, ref, 2e-2)
    merges = [sum(_live_chunks(L, W, chunk) > 1 for W in windows) for L in lens]
    epochs = torch.tensor(merges, dtype=torch.int32).view(-1, 1).expand(B, nkv)
    assert int(ctr[..., 0, 0].abs().sum()) == 0 and torch.equal(ctr[..., 1, 0].cpu(), epochs), ctr
    assert int(ctr[..., 1:].abs().sum()) == 0  # one word per 128-B counter line


@pytest.mark.parametrize("nh,nkv,chunk,cap", [(4, 1, 128, 32768), (16, 2, 256, 32768)])
def test_attn_decode_fused_window_long_context(cuda, nh, nkv, chunk, cap):
    """The fixed-chunk form on TP ranks at judge lengths (up to 256 chunk blocks per kv head, merged
    in two levels of 16): the live chunks of a windowed row fill one group, several, or (W past
    kAttnOneLevel * chunk keys) both levels; windows and lengths change on one workspace."""
    torch.manual_seed(8)
    D, bs, B = 128, 64, 3
    kc, vc, bt = _paged_kv(B, cap, nkv, D, bs)
    q = rnd(B, nh * D)
    gc = cap // chunk
    part, ctr = ops.decode_attn_workspace(B, nh, nkv, D, gc, "cuda", fused=True)
    out = torch.empty(B, nh * D, dtype=BF, device="cuda")
    scale = 1 / math.sqrt(D)
    qc, kcc, vcc = q.cpu(), kc.cpu(), vc.cpu()
    for lens, W in (([cap, 9000, 130], 4096), ([2100, cap - 1, 17000], 20000), ([cap, 9000, 130], 1),
                    ([cap, 9000, 130], 2100)):
        sl = torch.tensor(lens, dtype=torch.int32)
        ref = oracle.attn_decode(qc, kcc, vcc, bt, sl, nh, nkv, D, bs, scale, W)
        out.zero_()
        ops.attn_decode(q, kc, vc, bt.cuda(), sl.cuda(), out, part, ctr, nh, nkv, D, bs, chunk, scale,
                        grid_chunks=gc, fused=True, window=W)
        close(out, ref, 2e-2)
        attn_probe.assert_rms(out, attn_probe.dense_decode(q, kc, vc, bt, lens, nh, nkv, D, bs, scale, W),
                              "decode_fused_window_long_context")
    tickets = torch.cat([ctr[..., :1, 0], ctr[..., 2:, 0]], dim=-1)
    assert int(tickets.abs().sum()) == 0, ctr


# -- decode, split form ---------------------------------------------------------------------------
@pytest.mark.parametrize("nh,nkv,D", SHAPES)
@pytest.mark.parametrize("gc", [1, 3, 64])
def test_attn_decode_split_window(cuda, nh, nkv, D, gc):
    """Balanced split over [lo & ~31, L): lengths and windows change between launches on one
    workspace (a row's block count shrinks and grows back)."""
    torch.manual_seed(5)
    bs, B = 64, 3
    kc, vc, bt = _paged_kv(B, 5000, nkv, D, bs)
    q = rnd(B, nh * D)
    part, ctr = ops.decode_attn_workspace(B, nh, nkv, D, gc, "cuda")
    out = torch.empty(B, nh * D, dtype=BF, device="cuda")
    scale = 1 / math.sqrt(D)
    qc, kcc, vcc = q.cpu(), kc.cpu(), vc.cpu()
    for lens in ([5000, 130, 1], [300, 4999, 2], [4097, 3000, 700]):
        sl = torch.tensor(lens, dtype=torch.int32)
        for W in (1, 100, 1000, 4096, 6000):
            ref = oracle.attn_decode(qc, kcc, vcc, bt, sl, nh, nkv, D, bs, scale, W)
            out.zero_()
            ops.attn_decode(q, kc, vc, bt.cuda(), sl.cuda(), out, part, ctr, nh, nkv, D, bs, 128, scale,
                            grid_chunks=gc, window=W)
            close(out, ref, 2e-2)
    assert int(ctr[..., 0, 0].abs().sum()) == 0, ctr


def test_attn_decode_split_window_two_level(cuda):
    """A windowed row over 300 blocks (a TP=8 rank's one kv head): the partials merge in two
    levels; the second row's window covers all of it."""
    torch.manual_seed(6)
    nh, nkv, D, bs, gc = 4, 1, 128, 64, 300
    lens = [40000, 9000]
    kc, vc, bt = _paged_kv(2, 40000, nkv, D, bs)
    q = rnd(2, nh * D)
    part, ctr = ops.decode_attn_workspace(2, nh, nkv, D, gc, "cuda")
    out = torch.zeros(2, nh * D, dtype=BF, device="cuda")
    scale = 1 / math.sqrt(D)
    sl = torch.tensor(lens, dtype=torch.int32)
    ref = oracle.attn_decode(q.cpu(), kc.cpu(), vc.cpu(), bt, sl, nh, nkv, D, bs, scale, 39000)
    ops.attn_decode(q, kc, vc, bt.cuda(), sl.cuda(), out, part, ctr, nh, nkv, D, bs, 128, scale, grid_chunks=gc,
                    window=39000)
    close(out, ref, 2e-2)
    attn_probe.assert_rms(out, attn_probe.dense_decode(q, kc, vc, bt, lens, nh, nkv, D, bs, scale, 39000),
                          "decode_split_window_two_level")
    tickets = torch.cat([ctr[..., :1, 0], ctr[..., 2:, 0]], dim=-1)
    assert int(tickets.abs().sum()) == 0, ctr


@pytest.mark.parametrize("nh,nkv,D", SHAPES)
@pytest.mark.parametrize("fused", [True, False])
def test_attn_decode_window_covering_everything_is_bit_identical(cuda, nh, nkv, D, fused):
    """W >= max(L) is the unwindowed arithmetic: the same bits as W = 0."""
    torch.manual_seed(7)
    bs = 64
    lens = [1, 300, 2049, 4096] if fused else [5000, 130, 1, 3000]
    B = len(lens)
    kc, vc, bt = _paged_kv(B, max(lens), nkv, D, bs)
    q = rnd(B, nh * D)
    sl = torch.tensor(lens, dtype=torch.int32).cuda()
    chunk, gc = (128, 32) if fused else (128, 7)
    part, ctr = ops.decode_attn_workspace(B, nh, nkv, D, gc, "cuda", fused=fused)
    scale = 1 / math.sqrt(D)
    outs = []
    for W in (0, max(lens), max(lens) + 1, 1 << 30):
        out = torch.zeros(B, nh * D, dtype=BF, device="cuda")
        ops.attn_decode(q, kc, vc, bt.cuda(), sl, out, part, ctr, nh, nkv, D, bs, chunk, scale, grid_chunks=gc,
                        fused=fused, window=W)
        outs.append(out)
    torch.cuda.synchronize()
    for o in outs[1:]:
        assert torch.equal(o, outs[0])


# -- prefill --------------------------------------------------------------------------------------
PREFILL_CASES = {
    "full": ([300], [300], (1, 33, 64, 100, 1000)),
    "chunk": ([200, 64], [1000, 64], (1, 33, 64, 100, 1000)),
    "ragged": ([1, 33, 130], [1, 97, 700], (1, 33, 64, 100, 1000)),
    "unaligned": ([96], [1037], (1, 33, 64, 100, 1000)),  # first position not tile-aligned
    "phi3-4k": ([2500], [2500], (2047,)),
}


def _prefill(q, kc, vc, bt, qs, ql, cl, qlens, ctx, nh, nkv, D, bs, **kw):
    out = torch.zeros(q.shape[0], nh * D, dtype=BF, device="cuda")
    ops.attn_prefill(q, kc, vc, bt, qs, ql, cl, out, max(qlens), nh, nkv, D, bs, 1 / math.sqrt(D), max_ctx=max(ctx),
                     **kw)
    return out


def _unimplemented_forms(nh, nkv, D, bs):
    """Forced block forms the windowed launcher refuses: paired row tiles (where the shape has them:
    G <= 4 divides 8; else form 1 is the 8-wave form) and key halves (D = 128 on 64-key pages; else
    form 3 is the 4-wave form)."""
    G = nh // nkv
    return ([1] if G <= 4 and 8 % G == 0 else []) + ([3] if D == 128 and bs == 64 else [])


@pytest.mark.parametrize("nh,nkv,D", SHAPES)
@pytest.mark.parametrize("case", list(PREFILL_CASES))
def test_attn_prefill_window(cuda, nh, nkv, D, case):
    """Every implemented form of the windowed prefill (8 waves: LDS-DMA staging at D = 128,
    register staging at D = 96 / 64; 4 waves; the library's own choice) against the fp32 oracle
    computed on the GPU; the forms and the KV split that do not implement the window raise; a
    window that covers every context gives the bits of W = 0."""
    torch.manual_seed(4)
    bs = 64
    qlens, ctx, windows = PREFILL_CASES[case]
    B = len(qlens)
    kc, vc, bt = _paged_kv(B, max(ctx), nkv, D, bs)
    qs = torch.tensor([sum(qlens[:i]) for i in range(B)], dtype=torch.int32)
    T = sum(qlens)
    q = rnd(T, nh * D)
    ql, cl = torch.tensor(qlens, dtype=torch.int32), torch.tensor(ctx, dtype=torch.int32)
    scale = 1 / math.sqrt(D)
    args = (q, kc, vc, bt.cuda(), qs.cuda(), ql.cuda(), cl.cuda(), qlens, ctx, nh, nkv, D, bs)
    refused = _unimplemented_forms(nh, nkv, D, bs)
    forms = [f for f in (None, 0, 1, 2, 3) if f not in refused]
    base = {f: _prefill(*args, ksplit=1, form=f) for f in forms}
    for W in windows:
        ref = torch.zeros(T, nh * D, dtype=BF, device="cuda")
        oracle.attn_prefill(q, kc, vc, bt.cuda(), qs, ql, cl, nh, nkv, D, bs, scale, ref, W)  # fp32 math, on the GPU
        ref = ref.float().cpu()
        for f in forms:
            out = _prefill(*args, ksplit=1, form=f, window=W)
            close(out, ref, 2e-2)
            if W >= max(ctx) and f is not None:  # (None: the library may choose another form with a window)
                assert torch.equal(out, base[f]), (W, f)
                # without max_ctx the windowed kernel itself runs: still the bits of W = 0
                out = torch.zeros_like(out)
                ops.attn_prefill(*args[:7], out, max(qlens), nh, nkv, D, bs, scale, ksplit=1, form=f, window=W)
                assert torch.equal(out, base[f]), (W, f, "kernel")
        out = _prefill(*args, window=W)  # the plan never splits a windowed launch
        close(out, ref, 2e-2)
    W = windows[0]
    for f in refused:
        with pytest.raises(RuntimeError):
            _prefill(*args, ksplit=1, form=f, window=W)
    for k in (2, 4):
        with pytest.raises(RuntimeError):
            _prefill(*args, ksplit=k, kmin=1, window=W)
    assert ops.attn_prefill_plan(B, max(qlens), max(ctx), nh, nkv, D=D, bs=bs, window=W)[0] == 1


def test_attn_prefill_window_small_pages(cuda):
    """16-key pages: the per-key page lookup of the register-staged form."""
    torch.manual_seed(14)
    nh, nkv, D, bs = 8, 2, 128, 16
    qlens, ctx = [130, 40], [700, 40]
    kc, vc, bt = _paged_kv(2, max(ctx), nkv, D, bs)
    qs = torch.tensor([0, 130], dtype=torch.int32)
    T = sum(qlens)
    q = rnd(T, nh * D)
    ql, cl = torch.tensor(qlens, dtype=torch.int32), torch.tensor(ctx, dtype=torch.int32)
    args = (q, kc, vc, bt.cuda(), qs.cuda(), ql.cuda(), cl.cuda(), qlens, ctx, nh, nkv, D, bs)
    for W in (33, 100):
        ref = torch.zeros(T, nh * D, dtype=BF, device="cuda")
        oracle.attn_prefill(q, kc, vc, bt.cuda(), qs, ql, cl, nh, nkv, D, bs, 1 / math.sqrt(D), ref, W)
        for f in (0, 2):
            close(_prefill(*args, ksplit=1, form=f, window=W), ref.float().cpu(), 2e-2)


# -- engine ---------------------------------------------------------------------------------------
WINDOWED = ["mistral-tiny", "phi3-tiny-swa"]


def _pair(name, ctx=512, **kw):
    cfg = FAMILIES[name]
    wc = TransformerWeights(cfg, TPGroup.single(), torch.device("cpu"), seed=3)
    wg = copy.deepcopy(wc)
    ecpu = Engine(cfg, EngineConfig(device="cpu", max_context=ctx), weights=wc)
    egpu = Engine(cfg, EngineConfig(device="cuda:0", max_context=ctx, **kw), weights=wg)
    return cfg, ecpu, egpu


def _logits_match(lc, lg, frac, what):
    """The thresholds of the unwindowed engine tests: max error below ``frac`` of the logit range;
    returns whether the oracle's argmax is decided (top-2 gap beyond twice the error)."""
    err = (lc - lg).abs().max().item()
    assert err < frac * max(1.0, lc.abs().max().item()), (what, err)
    top2 = torch.topk(lc, 2).values
    return (top2[0] - top2[1]).item() > 2 * err


@pytest.mark.parametrize("name", WINDOWED)
def test_windowed_engine_bypasses_the_fused_launches(cuda, name):
    cfg, _, egpu = _pair(name)
    assert egpu.window == cfg.sliding_window > 0
    assert not any(egpu.ao_chunks) and not any(egpu.qa_plan)


@pytest.mark.parametrize("name", WINDOWED)
def test_windowed_prefill_logits_match_oracle(cuda, name):
    cfg, ecpu, egpu = _pair(name)
    prompt = [(i * 37) % (cfg.vocab - 300) + 256 for i in range(150)]
    s1 = ecpu.new_sequence()
    ecpu.prefill([s1], [prompt])
    s2 = egpu.new_sequence()
    egpu.prefill([s2], [prompt])
    torch.cuda.synchronize()
    lc, lg = s1.logits.float(), s2.logits.float().cpu()
    if _logits_match(lc, lg, 0.05, name):
        assert int(lc.argmax()) == int(lg.argmax())
    # the window matters at this length: the unwindowed model's logits differ
    full = FAMILIES[name].with_(name=name + "-full", sliding_window=0)
    ef = Engine(full, EngineConfig(device="cpu", max_context=512), weights=ecpu.w)
    s3 = ef.new_sequence()
    ef.prefill([s3], [prompt])
    assert (s3.logits.float() - lc).abs().max().item() > 1e-3


@pytest.mark.parametrize("name", WINDOWED)
def test_windowed_decode_logits_match_oracle(cuda, name):
    """Teacher-forced at every step, lengths 41..52: across L = W = 48 (mistral-tiny), past W = 33
    throughout (phi3-tiny-swa)."""
    cfg, ecpu, egpu = _pair(name)
    prompt = [(i * 53) % (cfg.vocab - 300) + 256 for i in range(40)]
    n = 12
    toks, lg = egpu.debug_decode_logits(prompt, n)
    assert len(toks) == n and lg.shape == (n, cfg.vocab)
    for i in range(n):
        s = ecpu.new_sequence()
        ecpu.prefill([s], [prompt + toks[:i]])
        lc = s.logits.float()
        ecpu.free_sequence(s)
        if _logits_match(lc, lg[i], 0.03, (name, i)):
            assert int(lc.argmax()) == toks[i], i


@pytest.mark.parametrize("name", WINDOWED)
def test_windowed_graph_equals_eager(cuda, name):
    """A 40-token prompt and 40 tokens: the length crosses W = 48 inside one graph replay."""
    cfg = FAMILIES[name]
    w = TransformerWeights(cfg, TPGroup.single(), torch.device("cuda:0"), seed=9)
    eg = Engine(cfg, EngineConfig(device="cuda:0", max_context=1024, use_graphs=True), weights=w)
    ee = Engine(cfg, EngineConfig(device="cuda:0", max_context=1024, use_graphs=False), weights=w)
    prompt = list(range(500, 540))
    a = eg.generate_ids(prompt, 40, temperature=0.9, seed=42, stop_on_eos=False)
    b = ee.generate_ids(prompt, 40, temperature=0.9, seed=42, stop_on_eos=False)
    assert a == b
    assert eg.generate_ids(prompt, 40, temperature=0.9, seed=42, stop_on_eos=False) == a


def test_windowed_batched_rows_equal_single(cuda):
    """Five rows of different lengths on both sides of W = 48 decoded in one batch against their
    single-row runs. Five rows take the MFMA decode GEMV and one row the VALU one, which round
    differently, so the comparison is the teacher-forced one of the oracle tests (greedy, logits at
    every step to 3 % of the logit range, equal tokens while the argmax is decided) and a row is
    compared up to its first undecided step."""
    cfg = FAMILIES["mistral-tiny"]
    w = TransformerWeights(cfg, TPGroup.single(), torch.device("cuda:0"), seed=11)
    e = Engine(cfg, EngineConfig(device="cuda:0", max_context=512, max_batch=5), weights=w)
    prompts = [[(i * (53 + 2 * r)) % (cfg.vocab - 300) + 256 for i in range(L)] for r, L in enumerate((10, 40, 47, 60, 100))]
    n = 12
    toks, lg = e.debug_decode_logits_batch(prompts, n)
    for r, p in enumerate(prompts):
        t1, l1 = e.debug_decode_logits(p, n)
        for i in range(n):
            decided = _logits_match(l1[i].float().cpu(), lg[r, i].float().cpu(), 0.03, (r, i))
            if not decided:
                break
            assert toks[r][i] == t1[i], (r, i)


@pytest.mark.parametrize("name", WINDOWED)
def test_windowed_chunked_prefill_matches_oracle(cuda, name):
    """A 150-token prompt prefilled in chunks of 64 (ctx > qlen from the second chunk on, the
    window reaching back into earlier chunks) against the CPU oracle's one-shot prefill."""
    cfg, ecpu, egpu = _pair(name, prefill_chunk=64)
    prompt = [(i * 37) % (cfg.vocab - 300) + 256 for i in range(150)]
    s1 = ecpu.new_sequence()
    ecpu.prefill([s1], [prompt])
    s2 = egpu.new_sequence()
    egpu.prefill([s2], [prompt])
    torch.cuda.synchronize()
    lc, lg = s1.logits.float(), s2.logits.float().cpu()
    if _logits_match(lc, lg, 0.05, name):
        assert int(lc.argmax()) == int(lg.argmax())
