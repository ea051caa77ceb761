"""Qwen2 / Qwen2.5 on a real MI355X: the q/k/v bias in the RoPE kernels (prefill ``rope_kv_write``,
the decode qkv GEMV's RoPE epilogue in its bf16, 13-bit-plane and MFMA forms), decode and prefill
attention at GQA groups of 5, 6 and 7, and the ``qwen2-tiny`` engine (group 7, biased) against the
CPU-oracle engine and against ``transformers``. Tolerances are the sibling tests' (test_kernels_gpu.py,
test_packed_gemv_gpu.py, test_engine_gpu.py, test_checkpoint.py)."""

import copy
import math

import pytest
import torch

from llm_consensus_amd import ops
from llm_consensus_amd.engine import Engine, EngineConfig, SamplingParams
from llm_consensus_amd.models.config import FAMILIES, LLAMA3_8B, rope_inv_freq
from llm_consensus_amd.models.transformer import TransformerWeights
from llm_consensus_amd.ops import oracle, wpack
from llm_consensus_amd.parallel.comm import TPGroup

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def rnd(*shape, scale=1.0, dev="cuda"):
    return (torch.randn(*shape, device=dev) * scale).to(BF)


def close(a, b, atol, rtol=0.02):
    a = a.float().cpu()
    b = b.float().cpu()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol).sum().item()
    assert bad == 0, f"{bad}/{a.numel()} mismatches, max err {err.max().item():.4g}"


def no_worse_than_oracle(got, ref, exact, slack=1e-2):
    """test_kernels_gpu.py's: the kernel is no further from the exact fp32 math than the oracle."""
    e_k = (got.float().cpu() - exact.float()).abs().max().item()
    e_o = (ref.float().cpu() - exact.float()).abs().max().item()
    assert e_k <= 1.5 * e_o + slack, (e_k, e_o)


def equal_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8),
                                                                    b.contiguous().view(torch.uint8))


def _normed_exact(x, nw, eps=1e-5):
    xf = x.cpu().float()
    return xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * nw.cpu().float()


def _rope_setup(nh, nkv, D, T, bs=64, nblocks=8):
    cos_t, sin_t = oracle.rope_tables(rope_inv_freq(LLAMA3_8B.with_(head_dim=D)), 4096)
    qkv = rnd(T, (nh + 2 * nkv) * D)
    pos = torch.randint(0, 4000, (T,), dtype=torch.int32)
    slots = torch.randperm(nblocks * bs)[:T].to(torch.int32)
    kc = torch.zeros(nblocks, nkv, bs, D, dtype=BF)
    return cos_t, sin_t, qkv, pos, slots, kc, torch.zeros_like(kc)


def _paged_kv(B, L_max, nkv, D, bs):
    nblk_per = (L_max + bs - 1) // bs
    nb = B * nblk_per + 3
    kc = rnd(nb, nkv, bs, D)
    vc = rnd(nb, nkv, bs, D)
    perm = torch.randperm(nb)[: B * nblk_per].view(B, nblk_per).to(torch.int32)
    return kc, vc, perm


# -- prefill RoPE with a bias ---------------------------------------------------------------------
@pytest.mark.parametrize("nh,nkv,D", [(28, 4, 128), (14, 2, 64), (32, 32, 96)])
def test_rope_kv_write_bias(cuda, nh, nkv, D):
    torch.manual_seed(2)
    T = 11
    cos_t, sin_t, qkv, pos, slots, kc, vc = _rope_setup(nh, nkv, D, T)
    bias = rnd((nh + 2 * nkv) * D)  # std 1.0, the size of real Qwen2 biases
    kc_ref, vc_ref = kc.clone(), vc.clone()
    q_ref = torch.zeros(T, nh * D, dtype=BF)
    oracle.rope_kv_write(qkv.cpu(), pos, cos_t, sin_t, kc_ref, vc_ref, slots, nh, nkv, D, 64, q_ref, bias=bias.cpu())

    def run(b):
        kd, vd = kc.cuda(), vc.cuda()
        qd = torch.zeros(T, nh * D, dtype=BF, device="cuda")
        ops.rope_kv_write(qkv, pos.cuda(), cos_t.cuda(), sin_t.cuda(), kd, vd, slots.cuda(), nh, nkv, D, 64, qd, bias=b)
        torch.cuda.synchronize()
        return qd, kd, vd

    qd, kd, vd = run(bias)
    close(qd, q_ref, 1e-2)
    close(kd, kc_ref, 1e-2)
    assert torch.equal(vd.cpu(), vc_ref)
    # the bias moved the result: the same launch without it is far off
    q0, k0, v0 = run(None)
    assert (q0.float() - qd.float()).abs().max().item() > 0.5 and not torch.equal(v0, vd)
    # a zero bias is the biasless launch, bit for bit
    for z, w in zip(run(torch.zeros_like(bias)), (q0, k0, v0)):
        assert equal_bits(z, w)


# -- decode qkv GEMV with a bias ------------------------------------------------------------------
QKV_SHAPES = [(28, 4, 128, 3584), (14, 2, 64, 896), (4, 2, 64, 256), (32, 8, 128, 256), (1, 1, 4, 128)]


def _qkv_case(M, nh, nkv, D, H, seed=12):
    torch.manual_seed(seed)
    cos_t, sin_t, _, pos, slots, kc, vc = _rope_setup(nh, nkv, D, M)
    N = (nh + 2 * nkv) * D
    x, W, nw, bias = rnd(M, H), rnd(N, H, scale=0.05), rnd(H), rnd(N)
    dev = dict(pos=pos.cuda(), slots=slots.cuda(), cos=cos_t.cuda(), sin=sin_t.cuda())

    def run(b, Wp=None):
        kd, vd = kc.cuda(), vc.cuda()
        qd = torch.zeros(M, nh * D, dtype=BF, device="cuda")
        ops.qkv_rope(x, W, nw, 1e-5, qd, kd, vd, dev["pos"], dev["slots"], dev["cos"], dev["sin"], nh, nkv, D, 64,
                     Wp=Wp, bias=b)
        torch.cuda.synchronize()
        return qd, kd, vd

    def ref(proj):  # the two-step oracle on a given projection
        kc_r, vc_r = kc.clone(), vc.clone()
        q_r = torch.zeros(M, nh * D, dtype=BF)
        oracle.rope_kv_write(proj, pos, cos_t, sin_t, kc_r, vc_r, slots, nh, nkv, D, 64, q_r, bias=bias.cpu())
        return q_r, kc_r, vc_r

    return x, W, nw, bias, run, ref


@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 16, 19, 32])
@pytest.mark.parametrize("nh,nkv,D,H", QKV_SHAPES)
def test_qkv_rope_bias(cuda, M, nh, nkv, D, H):
    """Fused decode qkv GEMV with the bias against the two-step oracle (``oracle.linear`` then
    ``oracle.rope_kv_write(bias=...)``). Forms taken (``launch_gemv`` in gemv.hip, M <= 2; the MFMA
    form of gemv_mfma.hip from 3 rows): (28, 4, 128, 3584) -> 4608 rows = 12-wave blocks, one row
    per wave, the pair meeting through LDS (RPW == 1); (14, 2, 64, 896) -> 1152 rows and
    (4, 2, 64, 256) -> 512 rows = 4-wave blocks, RPW == 1. None of the issue's shapes reaches
    RPW == 2, so two more: (32, 8, 128, 256) -> 6144 rows = 768 threads x 2 rows per wave (the
    Llama-3-8B geometry at a small K), and (1, 1, 4, 128) -> 12 rows, which tile by no block size:
    256 threads x 2 rows per wave (the fallback; waves past N load a clamped bias pair)."""
    x, W, nw, bias, run, ref = _qkv_case(M, nh, nkv, D, H)
    got = run(bias)
    want = ref(oracle.linear(x.cpu(), W.cpu(), 0, None, nw.cpu(), 1e-5))
    if M <= 2:
        for g, w in zip(got, want):
            close(g, w, 3e-2)
    else:  # MFMA form, factorised norm: against the exact fp32 math, next to the oracle
        exact = ref(_normed_exact(x, nw) @ W.cpu().float().t())
        for g, w, e in zip(got, want, exact):
            no_worse_than_oracle(g, w, e)
    # the bias is not a no-op at this tolerance
    assert max((a.float() - b.float()).abs().max().item() for a, b in zip(run(None), got)) > 0.5


@pytest.mark.parametrize("M", [1, 2, 5])
@pytest.mark.parametrize("nh,nkv,D,H", QKV_SHAPES)
def test_qkv_rope_zero_bias_is_bit_identical(cuda, M, nh, nkv, D, H):
    x, W, nw, bias, run, _ = _qkv_case(M, nh, nkv, D, H)
    want = run(None)
    assert bool(want[0].float().abs().sum() > 0)
    for g, w in zip(run(torch.zeros_like(bias)), want):
        assert equal_bits(g, w)


@pytest.mark.parametrize("M", [1, 2])
def test_qkv_rope_bias_packed_weights(cuda, M):
    """The biased launch from the 13-bit planes equals the biased bf16 launch bit for bit (as
    test_packed_gemv_gpu.py asserts for the unbiased pair): 2560 rows = 10-wave blocks."""
    nh, nkv, D, H = 16, 2, 128, 2048
    torch.manual_seed(21)
    cos_t, sin_t, _, pos, slots, kc, vc = _rope_setup(nh, nkv, D, M)
    N = (nh + 2 * nkv) * D
    x, nw, bias = rnd(M, H), rnd(H), rnd(N)
    W = (torch.randn(N, H, device="cuda") * H ** -0.5).to(BF)
    pw = wpack.pack(W)
    assert pw.raw_rows <= N // 100

    def run(Wp, b):
        kd, vd = kc.cuda(), vc.cuda()
        qd = torch.zeros(M, nh * D, dtype=BF, device="cuda")
        ops.qkv_rope(x, W, nw, 1e-5, qd, kd, vd, pos.cuda(), slots.cuda(), cos_t.cuda(), sin_t.cuda(), nh, nkv, D, 64,
                     Wp=Wp, bias=b)
        torch.cuda.synchronize()
        return qd, kd, vd

    want = run(None, bias)
    assert (want[0].float() - run(None, None)[0].float()).abs().max().item() > 0.5
    for g, w in zip(run(pw, bias), want):
        assert equal_bits(g, w)


# -- decode attention at groups of 5, 6, 7 ---------------------------------------------------------
ODD_SHAPES = [(28, 4, 128), (40, 8, 128), (12, 2, 128), (14, 2, 64)]


@pytest.mark.parametrize("nh,nkv,D", ODD_SHAPES)
@pytest.mark.parametrize("lens", [[1, 7], [100, 1000], [4096, 128, 129, 2049]])
@pytest.mark.parametrize("chunk", [128, 256])
def test_attn_decode_fused_odd_groups(cuda, nh, nkv, D, lens, chunk):
    """test_attn_decode_fused at G = 7, 5, 6, 7: same oracle, tolerance and ticket / epoch checks."""
    torch.manual_seed(3)
    B, bs = len(lens), 64
    kc, vc, bt = _paged_kv(B, max(lens), nkv, D, bs)
    q = rnd(B, nh * D)
    sl = torch.tensor(lens, dtype=torch.int32)
    gc = 4096 // chunk
    part, ctr = ops.decode_attn_workspace(B, nh, nkv, D, gc, "cuda", fused=True)
    out = torch.empty(B, nh * D, dtype=BF, device="cuda")
    scale = 1 / math.sqrt(D)
    ref = oracle.attn_decode(q.cpu(), kc.cpu(), vc.cpu(), bt, sl, nh, nkv, D, bs, scale)
    for _ in range(3):
        out.zero_()
        ops.attn_decode(q, kc, vc, bt.cuda(), sl.cuda(), out, part, ctr, nh, nkv, D, bs, chunk, scale, grid_chunks=gc,
                        fused=True)
        close(out, ref, 2e-2)
    # tickets re-armed, epochs advanced once per launch where a merge ran
    epochs = torch.tensor([3 if n > chunk else 0 for n in lens], dtype=torch.int32).view(-1, 1).expand(B, nkv)
    assert int(ctr[..., 0, 0].abs().sum()) == 0 and torch.equal(ctr[..., 1, 0].cpu(), epochs), ctr
    assert int(ctr[..., 1:].abs().sum()) == 0  # one word per 128-B counter line


@pytest.mark.parametrize("nh,nkv,D", ODD_SHAPES)
@pytest.mark.parametrize("gc", [1, 7, 64])
def test_attn_decode_split_odd_groups(cuda, nh, nkv, D, gc):
    """test_attn_decode_balanced_split at the odd groups: one block (gc = 1), a one-level merge
    (7 blocks) and a two-level merge (5000 keys over 39 blocks > 32: groups of 16), the lengths
    changing between launches on one workspace."""
    torch.manual_seed(5)
    bs, B = 64, 3
    kc, vc, bt = _paged_kv(B, 5000, nkv, D, bs)
    q = rnd(B, nh * D)
    part, ctr = ops.decode_attn_workspace(B, nh, nkv, D, gc, "cuda")
    out = torch.empty(B, nh * D, dtype=BF, device="cuda")
    scale = 1 / math.sqrt(D)
    qc, kcc, vcc = q.cpu(), kc.cpu(), vc.cpu()
    for lens in ([5000, 130, 1], [300, 4999, 2], [5000, 130, 1]):
        sl = torch.tensor(lens, dtype=torch.int32)
        ref = oracle.attn_decode(qc, kcc, vcc, bt, sl, nh, nkv, D, bs, scale)
        out.zero_()
        ops.attn_decode(q, kc, vc, bt.cuda(), sl.cuda(), out, part, ctr, nh, nkv, D, bs, 128, scale, grid_chunks=gc)
        close(out, ref, 2e-2)
    tickets = torch.cat([ctr[..., :1, 0], ctr[..., 2:, 0]], dim=-1)
    assert int(tickets.abs().sum()) == 0, ctr


@pytest.mark.parametrize("fused", [True, False])
def test_attn_decode_window_group_of_7(cuda, fused):
    """One windowed case per form at (28, 4, 128), W = 48 (test_sliding_window_gpu.py's oracle and
    tolerance): lengths below, at and past the window, past one chunk and past several."""
    torch.manual_seed(7)
    nh, nkv, D, bs, W = 28, 4, 128, 64, 48
    lens = [7, 48, 49, 300, 2049] if fused else [5000, 130, 1, 48, 3000]
    B = len(lens)
    kc, vc, bt = _paged_kv(B, max(lens), nkv, D, bs)
    q = rnd(B, nh * D)
    sl = torch.tensor(lens, dtype=torch.int32)
    chunk, gc = (128, 32) if fused else (128, 7)
    part, ctr = ops.decode_attn_workspace(B, nh, nkv, D, gc, "cuda", fused=fused)
    out = torch.zeros(B, nh * D, dtype=BF, device="cuda")
    scale = 1 / math.sqrt(D)
    ref = oracle.attn_decode(q.cpu(), kc.cpu(), vc.cpu(), bt, sl, nh, nkv, D, bs, scale, W)
    for _ in range(2):
        out.zero_()
        ops.attn_decode(q, kc, vc, bt.cuda(), sl.cuda(), out, part, ctr, nh, nkv, D, bs, chunk, scale, grid_chunks=gc,
                        fused=fused, window=W)
        close(out, ref, 2e-2)
    assert int(ctr[..., 0, 0].abs().sum()) == 0, ctr


# -- prefill attention at a group of 7 ------------------------------------------------------------
@pytest.mark.parametrize("nh,nkv,D", [(28, 4, 128), (14, 2, 64)])
@pytest.mark.parametrize("form", [None, 0, 2])
def test_attn_prefill_group_of_7(cuda, nh, nkv, D, form):
    """150 query rows over 150 keys beside 40 rows over 300 keys (a chunk of a longer prefill), the
    8-wave and 4-wave forms forced and the library's own choice; a block of 8 (4) waves spans two
    32-row tiles of the 7 heads. test_attn_prefill's oracle and tolerance."""
    torch.manual_seed(4)
    bs = 64
    qlens, ctx = [150, 40], [150, 300]
    kc, vc, bt = _paged_kv(2, max(ctx), nkv, D, bs)
    qs = torch.tensor([0, 150], dtype=torch.int32)
    T = sum(qlens)
    q = rnd(T, nh * D)
    out = torch.zeros(T, nh * D, dtype=BF, device="cuda")
    ql, cl = torch.tensor(qlens, dtype=torch.int32), torch.tensor(ctx, dtype=torch.int32)
    scale = 1 / math.sqrt(D)
    ops.attn_prefill(q, kc, vc, bt.cuda(), qs.cuda(), ql.cuda(), cl.cuda(), out, max(qlens), nh, nkv, D, bs, scale,
                     max_ctx=max(ctx), ksplit=1, form=form)
    ref = torch.zeros(T, nh * D, dtype=BF)
    oracle.attn_prefill(q.cpu(), kc.cpu(), vc.cpu(), bt, qs, ql, cl, nh, nkv, D, bs, scale, ref)
    close(out, ref, 2e-2)


# -- the engine on qwen2-tiny ----------------------------------------------------------------------
def _pair(name, ctx=512, **kw):
    cfg = FAMILIES[name]
    wc = TransformerWeights(cfg, TPGroup.single(), torch.device("cpu"), seed=3)
    wg = copy.deepcopy(wc)
    ecpu = Engine(cfg, EngineConfig(device="cpu", max_context=ctx), weights=wc)
    egpu = Engine(cfg, EngineConfig(device="cuda:0", max_context=ctx, **kw), weights=wg)
    return cfg, ecpu, egpu


def _teacher_forced(ecpu, prompt, toks, lg, tag):
    for i in range(len(toks)):
        s = ecpu.new_sequence()
        ecpu.prefill([s], [prompt + toks[:i]])
        lc = s.logits.float()
        ecpu.free_sequence(s)
        err = (lc - lg[i]).abs().max().item()
        assert err < 0.03 * max(1.0, lc.abs().max().item()), (tag, i, err)
        top2 = torch.topk(lc, 2).values
        if (top2[0] - top2[1]).item() > 2 * err:
            assert int(lc.argmax()) == toks[i], (tag, i)


def test_engine_prefill_and_decode_match_oracle(cuda):
    """test_engine_gpu.py's prefill (150 tokens) and teacher-forced decode (40-token prompt, 12
    steps) checks on ``qwen2-tiny``; the engine keeps the two-launch decode path."""
    cfg, ecpu, egpu = _pair("qwen2-tiny")
    assert cfg.qkv_bias and egpu.w.layers[0].b_qkv.is_cuda
    assert not any(egpu.qa_plan) and not any(egpu.qa_buckets)  # no qkv_attn bucket for a biased model
    prompt = [(i * 37) % (cfg.vocab - 300) + 256 for i in range(150)]
    s1, s2 = ecpu.new_sequence(), egpu.new_sequence()
    ecpu.prefill([s1], [prompt])
    egpu.prefill([s2], [prompt])
    torch.cuda.synchronize()
    lc, lg = s1.logits.float(), s2.logits.float().cpu()
    err = (lc - lg).abs().max().item()
    assert err < 0.05 * max(1.0, lc.abs().max().item()), err
    top2 = torch.topk(lc, 2).values
    if (top2[0] - top2[1]).item() > 2 * err:
        assert int(lc.argmax()) == int(lg.argmax())
    ecpu.free_sequence(s1)
    egpu.free_sequence(s2)
    prompt = [(i * 53) % (cfg.vocab - 300) + 256 for i in range(40)]
    toks, lgd = egpu.debug_decode_logits(prompt, 12)
    assert len(toks) == 12 and lgd.shape == (12, cfg.vocab)
    _teacher_forced(ecpu, prompt, toks, lgd, "decode")


def test_engine_never_selects_qkv_attn_for_a_biased_model(cuda):
    """A G = 8 Qwen shape passes ``qkv_attn``'s own shape check; the bias still keeps it out, in
    every mode. The same shape without the bias takes it (so the condition is the bias)."""
    biased = FAMILIES["llama-tiny"].with_(name="qwen2-g8", n_heads=16, n_kv_heads=2, hidden=1024, qkv_bias=True)
    assert ops.qkv_attn_supported(16, 2, 64, 1024)
    for mode in ("1", "all"):
        e = Engine(biased, EngineConfig(device="cuda:0", max_context=512, qkv_attn=mode))
        assert not any(e.qa_plan), (mode, e.qa_plan)
        assert len(e.generate_ids(list(range(300, 320)), 4, temperature=0.0, stop_on_eos=False)) == 4
    plain = Engine(biased.with_(name="llama-g8", qkv_bias=False),
                   EngineConfig(device="cuda:0", max_context=512, qkv_attn="all"))
    assert any(plain.qa_plan)


@pytest.mark.parametrize("B", [5, 19])
def test_engine_batched_decode_rows_match_oracle(cuda, B):
    """The MFMA decode form's biased RoPE epilogue in the engine, one (5) and two (19) token groups."""
    cfg, ecpu, egpu = _pair("qwen2-tiny", max_batch=max(16, B))
    prompts = [[(i * (53 + 2 * r)) % (cfg.vocab - 300) + 256 for i in range(20 + 3 * r)] for r in range(B)]
    n = 3
    toks, lg = egpu.debug_decode_logits_batch(prompts, n)
    assert lg.shape == (B, n, cfg.vocab)
    for r in range(B):
        _teacher_forced(ecpu, prompts[r], toks[r], lg[r], r)


def test_engine_graph_equals_eager_and_two_rows_equal_single(cuda):
    cfg = FAMILIES["qwen2-tiny"]
    w = TransformerWeights(cfg, TPGroup.single(), torch.device("cuda:0"), seed=9)
    eg = Engine(cfg, EngineConfig(device="cuda:0", max_context=1024, use_graphs=True), weights=w)
    ee = Engine(cfg, EngineConfig(device="cuda:0", max_context=1024, use_graphs=False), weights=w)
    prompt = list(range(500, 600))
    a = eg.generate_ids(prompt, 24, temperature=0.9, seed=42, stop_on_eos=False)
    assert a == ee.generate_ids(prompt, 24, temperature=0.9, seed=42, stop_on_eos=False)
    assert a == eg.generate_ids(prompt, 24, temperature=0.9, seed=42, stop_on_eos=False)  # replay again
    # M = 2 GEMV rows accumulate per row as M = 1 does; attention per row is independent
    e2 = Engine(cfg, EngineConfig(device="cuda:0", max_context=1024, max_batch=2), weights=w)
    p1, p2 = list(range(300, 350)), list(range(700, 790))
    sp = [SamplingParams(16, 0.7, 1.0, 0, 5, False), SamplingParams(16, 0.7, 1.0, 0, 6, False)]
    both = e2.generate_batch([p1, p2], sp)
    assert both[0] == e2.generate_ids(p1, 16, 0.7, seed=5, stop_on_eos=False)
    assert both[1] == e2.generate_ids(p2, 16, 0.7, seed=6, stop_on_eos=False)


def test_qwen2_checkpoint_matches_transformers_gpu(cuda, tmp_path):
    """test_qwen2_cpu.py's parity (non-zero biases) through the HIP path, then 16 greedy tokens
    through the HIP-graph decode: teacher-forced argmax agreement, at most one disagreement."""
    pytest.importorskip("transformers")
    from test_qwen2_cpu import PROMPTS, compare, qwen2_checkpoint
    from llm_consensus_amd.models.checkpoint import config_from_hf

    hf = qwen2_checkpoint(str(tmp_path))
    cfg = config_from_hf(str(tmp_path), name="ck-gpu-qwen2")
    eng = Engine(cfg, EngineConfig(device="cuda:0", max_context=512))
    assert not any(eng.qa_plan)
    compare(eng, hf, PROMPTS)
    prompt = [3, 14, 15, 92, 65]
    ours = eng.generate_ids(prompt, 16, temperature=0.0, stop_on_eos=False)
    with torch.no_grad():
        logits = hf.float()(torch.tensor([prompt + ours])).logits[0]
    agree = sum(int(t == logits[len(prompt) - 1 + i].argmax().item()) for i, t in enumerate(ours))
    assert agree >= len(ours) - 1, (agree, len(ours))
