"""Qwen3 on a real MI355X: the per-head q/k RMSNorm + RoPE + KV-write kernel
(csrc/kernels/qk_norm_rope.hip) against ``oracle.rope_kv_write`` with norms, its row independence,
``ops.qkv_rope`` with norms (GEMV or MFMA projection, then the kernel) with and without a packed
twin, and the ``qwen3-tiny`` engine (heads of 128 over a hidden of 256) against the CPU-oracle engine
and against ``transformers``. Helpers and tolerances are test_qwen2_gpu.py's."""

import pytest
import torch

from test_qwen2_gpu import (BF, _normed_exact, _pair, _rope_setup, _teacher_forced, close, equal_bits,
                            no_worse_than_oracle, rnd)

from llm_consensus_amd import ops
from llm_consensus_amd.engine import Engine, EngineConfig, SamplingParams
from llm_consensus_amd.models.config import FAMILIES
from llm_consensus_amd.models.transformer import TransformerWeights
from llm_consensus_amd.ops import oracle, wpack
from llm_consensus_amd.parallel.comm import TPGroup

pytestmark = pytest.mark.gpu

EPS = 1e-6
# (32, 8, 128): Qwen3-8B, 42 waves in 11 blocks; (5, 1, 128): 6 heads + 1 V wave do not fill the second
# 4-wave block; (14, 2, 64): half-wave heads
SHAPES = [(32, 8, 128), (5, 1, 128), (14, 2, 64)]


def gamma(D, dev="cuda"):
    """Norm weights 1 + 0.3 randn: far enough from ones that a dropped or misplaced weight shows."""
    return (1.0 + 0.3 * torch.randn(D, device=dev)).to(BF)


def _case(nh, nkv, D, T, seed=2):
    """Inputs on the CPU (test_qwen2_gpu.py's ``_rope_setup``) with one slot = -1 row, the norm
    weights, and a runner of the kernel on fresh copies of the caches."""
    torch.manual_seed(seed)
    cos_t, sin_t, qkv, pos, slots, kc, vc = _rope_setup(nh, nkv, D, T)
    slots[T // 2] = -1
    kc, vc = rnd(*kc.shape, dev="cpu"), rnd(*vc.shape, dev="cpu")  # non-zero, so an untouched row shows
    gq, gk = gamma(D), gamma(D)
    cos_d, sin_d = cos_t.cuda(), sin_t.cuda()

    def run(gq_, gk_, rows=slice(None)):
        kd, vd = kc.cuda(), vc.cuda()
        n = qkv[rows].shape[0]
        qd = torch.zeros(n, nh * D, dtype=BF, device="cuda")
        ops.rope_kv_write(qkv[rows].contiguous(), pos[rows].cuda(), cos_d, sin_d, kd, vd, slots[rows].cuda(), nh, nkv,
                          D, 64, qd, q_norm=gq_, k_norm=gk_, qk_eps=EPS)
        torch.cuda.synchronize()
        return qd, kd, vd

    return cos_t, sin_t, qkv, pos, slots, kc, vc, gq, gk, run


# -- the kernel -----------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 11])
@pytest.mark.parametrize("nh,nkv,D", SHAPES)
def test_qk_norm_rope_kv_write(cuda, nh, nkv, D, T):
    cos_t, sin_t, qkv, pos, slots, kc, vc, gq, gk, run = _case(nh, nkv, D, T)
    kc_ref, vc_ref = kc.clone(), vc.clone()
    q_ref = torch.zeros(T, nh * D, dtype=BF)
    oracle.rope_kv_write(qkv.cpu(), pos, cos_t, sin_t, kc_ref, vc_ref, slots, nh, nkv, D, 64, q_ref,
                         q_norm=gq.cpu(), k_norm=gk.cpu(), qk_eps=EPS)
    qd, kd, vd = run(gq, gk)
    close(qd, q_ref, 1e-2)
    close(kd, kc_ref, 1e-2)
    assert torch.equal(vd.cpu(), vc_ref)  # v copied bit for bit, and nothing else in the cache touched
    written = [int(s) for s in slots if int(s) >= 0]
    assert len(written) == T - 1
    for s in written:
        assert torch.equal(vd[s // 64, :, s % 64].cpu(), qkv[slots.tolist().index(s), (nh + nkv) * D:].view(nkv, D).cpu())
    mask = torch.ones(kc.shape[0] * 64, dtype=torch.bool)
    mask[written] = False
    untouched = mask.view(kc.shape[0], 1, 64, 1).expand_as(kc)
    assert torch.equal(kd.cpu()[untouched], kc[untouched]) and torch.equal(vd.cpu()[untouched], vc[untouched])


def test_qk_norm_rope_kv_write_refuses_other_head_dims(cuda):
    nh, nkv, D, T = 4, 2, 96, 2
    cos_t, sin_t, qkv, pos, slots, kc, vc, gq, gk, run = _case(nh, nkv, D, T)
    with pytest.raises(ValueError):
        run(gq, gk)
    with pytest.raises(RuntimeError):  # the kernel library itself
        from llm_consensus_amd.utils.native import kernels
        qd = torch.zeros(T, nh * D, dtype=BF, device="cuda")
        kd, vd = kc.cuda(), vc.cuda()
        kernels().qk_norm_rope_kv_write(qkv.data_ptr(), qkv.stride(0), qd.data_ptr(), qd.stride(0), pos.cuda().data_ptr(),
                                        cos_t.cuda().data_ptr(), sin_t.cuda().data_ptr(), kd.data_ptr(), vd.data_ptr(),
                                        0, T, nh, nkv, D, 64, gq.data_ptr(), gk.data_ptr(), EPS,
                                        torch.cuda.current_stream().cuda_stream)
    nh, nkv, D = 4, 2, 128
    _, _, _, _, _, _, _, gq, gk, run = _case(nh, nkv, D, T)
    with pytest.raises(ValueError):
        run(gq, None)
    with pytest.raises(ValueError):
        run(gq[:64].contiguous(), gk)


@pytest.mark.parametrize("nh,nkv,D", SHAPES)
def test_rows_are_independent_and_launches_repeat(cuda, nh, nkv, D):
    T = 11
    _, _, qkv, pos, slots, kc, vc, gq, gk, run = _case(nh, nkv, D, T, seed=4)
    qd, kd, vd = run(gq, gk)
    for g, w in zip(run(gq, gk), (qd, kd, vd)):  # two identical launches
        assert equal_bits(g, w)
    for t in (0, 3, 10):  # row t alone (none of them the slot = -1 row)
        q1, k1, v1 = run(gq, gk, slice(t, t + 1))
        assert equal_bits(q1[0], qd[t])
        s = int(slots[t])
        assert equal_bits(k1[s // 64, :, s % 64], kd[s // 64, :, s % 64])
        assert equal_bits(v1[s // 64, :, s % 64], vd[s // 64, :, s % 64])


@pytest.mark.parametrize("nh,nkv,D", SHAPES)
def test_norm_weights_matter(cuda, nh, nkv, D):
    _, _, _, _, _, _, _, gq, gk, run = _case(nh, nkv, D, 11, seed=6)
    qd, kd, _ = run(gq, gk)
    ones = torch.ones_like(gq)
    for other in (run(ones, ones), run(gk, gq)):
        err = (other[0].float() - qd.float()).abs()
        assert (err > 1e-2 + 0.02 * qd.float().abs()).any() and err.max().item() > 0.1
        assert (other[1].float() - kd.float()).abs().max().item() > 0.1


# -- ops.qkv_rope with norms ------------------------------------------------------------------------
QKV_SHAPES = [(4, 2, 128, 256), (32, 8, 128, 2048)]


def _qkv_case(M, nh, nkv, D, H, seed=12):
    torch.manual_seed(seed)
    cos_t, sin_t, _, pos, slots, kc, vc = _rope_setup(nh, nkv, D, M)
    N = (nh + 2 * nkv) * D
    x, nw = rnd(M, H), rnd(H)
    W = (torch.randn(N, H, device="cuda") * H ** -0.5).to(BF)
    gq, gk = gamma(D), gamma(D)
    dev = dict(pos=pos.cuda(), slots=slots.cuda(), cos=cos_t.cuda(), sin=sin_t.cuda())
    buf = torch.zeros(M + 1, N, dtype=BF, device="cuda")

    def run(normed=True, Wp=None, **kw):
        kd, vd = kc.cuda(), vc.cuda()
        qd = torch.zeros(M, nh * D, dtype=BF, device="cuda")
        if normed:
            kw = dict(q_norm=gq, k_norm=gk, qk_eps=EPS, qkv_buf=buf)
        ops.qkv_rope(x, W, nw, 1e-5, qd, kd, vd, dev["pos"], dev["slots"], dev["cos"], dev["sin"], nh, nkv, D, 64,
                     Wp=Wp, **kw)
        torch.cuda.synchronize()
        return qd, kd, vd

    def ref(proj):  # the two-step oracle on a given projection
        kc_r, vc_r = kc.clone(), vc.clone()
        q_r = torch.zeros(M, nh * D, dtype=BF)
        oracle.rope_kv_write(proj, pos, cos_t, sin_t, kc_r, vc_r, slots, nh, nkv, D, 64, q_r,
                             q_norm=gq.cpu(), k_norm=gk.cpu(), qk_eps=EPS)
        return q_r, kc_r, vc_r

    return x, W, nw, run, ref


@pytest.mark.parametrize("M", [1, 2, 5])
@pytest.mark.parametrize("nh,nkv,D,H", QKV_SHAPES)
def test_qkv_rope_with_norms(cuda, M, nh, nkv, D, H):
    """The decode projection of a Qwen3 layer (GEMV for 1-2 rows, the MFMA form for 5, then the norm
    kernel) against the oracle composite; test_qwen2_gpu.py's ``test_qkv_rope_bias`` checks."""
    x, W, nw, run, ref = _qkv_case(M, nh, nkv, D, H)
    got = run()
    want = ref(oracle.linear(x.cpu(), W.cpu(), 0, None, nw.cpu(), 1e-5))
    if M <= 2:
        for g, w in zip(got, want):
            close(g, w, 3e-2)
    else:
        exact = ref(_normed_exact(x, nw) @ W.cpu().float().t())
        for g, w, e in zip(got, want, exact):
            no_worse_than_oracle(g, w, e)
    # the norm is not a no-op at this tolerance
    assert (run(normed=False)[0].float() - got[0].float()).abs().max().item() > 0.1


@pytest.mark.parametrize("M", [1, 2])
def test_qkv_rope_with_norms_packed_twin_is_bit_identical(cuda, M):
    nh, nkv, D, H = QKV_SHAPES[1]
    x, W, nw, run, _ = _qkv_case(M, nh, nkv, D, H, seed=21)
    pw = wpack.pack_best(W)
    assert pw is not None and pw.raw_rows <= W.shape[0] // 100
    for g, w in zip(run(Wp=pw), run()):
        assert equal_bits(g, w)


@pytest.mark.parametrize("M", [1, 2, 5])
@pytest.mark.parametrize("nh,nkv,D,H", QKV_SHAPES)
def test_qkv_rope_without_norms_is_the_fused_launch(cuda, M, nh, nkv, D, H):
    x, W, nw, run, _ = _qkv_case(M, nh, nkv, D, H)
    want = run(normed=False)
    assert bool(want[0].float().abs().sum() > 0)
    buf = torch.full((M, W.shape[0]), 7.0, dtype=BF, device="cuda")
    for g, w in zip(run(normed=False, q_norm=None, k_norm=None, qkv_buf=buf), want):
        assert equal_bits(g, w)
    assert bool((buf == 7.0).all())  # one launch, as ever: the buffer is not used


def test_qkv_rope_norms_need_a_buffer_and_no_bias(cuda):
    nh, nkv, D, H = QKV_SHAPES[0]
    x, W, nw, run, _ = _qkv_case(1, nh, nkv, D, H)
    g = gamma(D)
    with pytest.raises(ValueError):
        run(normed=False, q_norm=g, k_norm=g)
    with pytest.raises(ValueError):
        run(normed=False, q_norm=g, k_norm=g, bias=rnd(W.shape[0]),
            qkv_buf=torch.zeros(1, W.shape[0], dtype=BF, device="cuda"))


# -- the engine on qwen3-tiny -----------------------------------------------------------------------
def test_engine_prefill_and_decode_match_oracle(cuda):
    """test_qwen2_gpu.py's prefill (150 tokens) and teacher-forced decode (40-token prompt, 12
    steps) checks on ``qwen3-tiny``; the engine keeps qkv_rope + the norm launch in every bucket."""
    cfg, ecpu, egpu = _pair("qwen3-tiny")
    L0 = egpu.w.layers[0]
    assert cfg.qk_norm and L0.q_norm.is_cuda and L0.k_norm.is_cuda and L0.b_qkv is None
    assert all(p is None for p in egpu.qa_plan) and not any(egpu.qa_buckets)
    assert egpu.qkv_buf.shape == (1, egpu.w.qkv_size)
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


def test_engine_never_selects_qkv_attn_for_a_normed_model(cuda):
    """A G = 8 shape passes ``qkv_attn``'s own shape check; the q/k norm still keeps it out, in
    every mode. The same shape without the norm takes it (so the condition is the norm)."""
    normed = FAMILIES["llama-tiny"].with_(name="qwen3-g8", n_heads=16, n_kv_heads=2, hidden=1024, qk_norm=True)
    assert ops.qkv_attn_supported(16, 2, 64, 1024)
    for mode in ("1", "all"):
        e = Engine(normed, EngineConfig(device="cuda:0", max_context=512, qkv_attn=mode))
        assert all(p is None for p in e.qa_plan), (mode, e.qa_plan)
        assert len(e.generate_ids(list(range(300, 320)), 4, temperature=0.0, stop_on_eos=False)) == 4
    plain = Engine(normed.with_(name="llama-g8", qk_norm=False),
                   EngineConfig(device="cuda:0", max_context=512, qkv_attn="all"))
    assert any(plain.qa_plan)


def test_engine_batched_decode_rows_match_oracle(cuda):
    """The MFMA decode form (5 rows) into the norm kernel in the engine."""
    B = 5
    cfg, ecpu, egpu = _pair("qwen3-tiny", max_batch=16)
    prompts = [[(i * (53 + 2 * r)) % (cfg.vocab - 300) + 256 for i in range(20 + 3 * r)] for r in range(B)]
    n = 3
    toks, lg = egpu.debug_decode_logits_batch(prompts, n)
    assert lg.shape == (B, n, cfg.vocab)
    for r in range(B):
        _teacher_forced(ecpu, prompts[r], toks[r], lg[r], r)


def test_engine_graph_equals_eager_and_two_rows_equal_single(cuda):
    cfg = FAMILIES["qwen3-tiny"]
    w = TransformerWeights(cfg, TPGroup.single(), torch.device("cuda:0"), seed=9)
    eg = Engine(cfg, EngineConfig(device="cuda:0", max_context=1024, use_graphs=True), weights=w)
    ee = Engine(cfg, EngineConfig(device="cuda:0", max_context=1024, use_graphs=False), weights=w)
    prompt = list(range(500, 600))
    a = eg.generate_ids(prompt, 24, temperature=0.9, seed=42, stop_on_eos=False)
    assert a == ee.generate_ids(prompt, 24, temperature=0.9, seed=42, stop_on_eos=False)
    assert a == eg.generate_ids(prompt, 24, temperature=0.9, seed=42, stop_on_eos=False)  # replay again
    e2 = Engine(cfg, EngineConfig(device="cuda:0", max_context=1024, max_batch=2), weights=w)
    p1, p2 = list(range(300, 350)), list(range(700, 790))
    sp = [SamplingParams(16, 0.7, 1.0, 0, 5, False), SamplingParams(16, 0.7, 1.0, 0, 6, False)]
    both = e2.generate_batch([p1, p2], sp)
    assert both[0] == e2.generate_ids(p1, 16, 0.7, seed=5, stop_on_eos=False)
    assert both[1] == e2.generate_ids(p2, 16, 0.7, seed=6, stop_on_eos=False)


def test_qwen3_checkpoint_matches_transformers_gpu(cuda, tmp_path):
    """test_qwen3_cpu.py's parity (norm weights 1 + 0.3 randn) through the HIP path, then 16 greedy
    tokens through the HIP-graph decode: teacher-forced argmax agreement, at most one disagreement."""
    pytest.importorskip("transformers")
    from test_qwen2_cpu import compare
    from test_qwen3_cpu import PROMPTS, qwen3_checkpoint
    from llm_consensus_amd.models.checkpoint import config_from_hf

    hf = qwen3_checkpoint(str(tmp_path))
    cfg = config_from_hf(str(tmp_path), name="ck-gpu-qwen3")
    eng = Engine(cfg, EngineConfig(device="cuda:0", max_context=512))
    assert cfg.qk_norm and all(p is None for p in eng.qa_plan)
    compare(eng, hf, PROMPTS)
    prompt = [3, 14, 15, 92, 65]
    ours = eng.generate_ids(prompt, 16, temperature=0.0, stop_on_eos=False)
    with torch.no_grad():
        logits = hf.float()(torch.tensor([prompt + ours])).logits[0]
    agree = sum(int(t == logits[len(prompt) - 1 + i].argmax().item()) for i, t in enumerate(ours))
    assert agree >= len(ours) - 1, (agree, len(ours))
