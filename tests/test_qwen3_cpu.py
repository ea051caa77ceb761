"""Qwen3 (dense) without a GPU: the loader and the per-head q/k RMSNorm against ``transformers`` (a
tiny random Qwen3 checkpoint whose ``q_norm`` / ``k_norm`` weights are 1 + 0.3 randn:
``Qwen3ForCausalLM`` initialises them to ones, and with ones a dropped, swapped or wrongly ordered
weight would pass), the hub Qwen3-8B config, the refused variants, the CPU engine's decode against
its prefill on ``qwen3-tiny`` (heads of 128 over a hidden of 256), TP = 2 over gloo against TP = 1,
and the catalog record. ``compare`` and the TP harness are test_qwen2_cpu.py's."""

import io
import json

import pytest
import torch
import torch.multiprocessing as mp

from test_qwen2_cpu import PROMPTS as QWEN2_PROMPTS, _free_port, compare

from llm_consensus_amd import cli
from llm_consensus_amd.engine import Engine, EngineConfig
from llm_consensus_amd.models.checkpoint import CheckpointError, config_from_hf
from llm_consensus_amd.models.config import FAMILIES
from llm_consensus_amd.models.transformer import pair_interleave_heads

# prompts of 5, 39 and 97 tokens inside the 512-token vocabulary
PROMPTS = [QWEN2_PROMPTS[1], [(i * 29) % 500 + 3 for i in range(39)], [(i * 53) % 490 + 7 for i in range(97)]]


def qwen3_checkpoint(tmp):
    """Tiny random Qwen3 (4 / 2 heads of 128 over a hidden of 256) with q/k norm weights 1 + 0.3 randn,
    saved to ``tmp``."""
    from transformers import Qwen3Config, Qwen3ForCausalLM

    c = Qwen3Config(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                    num_attention_heads=4, num_key_value_heads=2, head_dim=128, max_position_embeddings=2048,
                    rms_norm_eps=1e-6, rope_theta=1e6, tie_word_embeddings=False, bos_token_id=510, eos_token_id=511)
    torch.manual_seed(3)
    m = Qwen3ForCausalLM(c)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for layer in m.model.layers:
            for norm in (layer.self_attn.q_norm, layer.self_attn.k_norm):
                norm.weight.copy_(1.0 + 0.3 * torch.randn(norm.weight.shape, generator=g))
    m = m.to(torch.bfloat16)
    m.save_pretrained(tmp, safe_serialization=True)
    return m


def _engine(tmp_path, name):
    cfg = config_from_hf(str(tmp_path), name=name)
    return cfg, Engine(cfg, EngineConfig(device="cpu", max_context=512, use_graphs=False))


def test_qwen3_checkpoint_matches_transformers(tmp_path):
    pytest.importorskip("transformers")
    hf = qwen3_checkpoint(str(tmp_path))
    cfg, eng = _engine(tmp_path, "ck-qwen3")
    assert cfg.arch == "llama" and cfg.qk_norm and not cfg.qkv_bias
    assert (cfg.n_heads, cfg.n_kv_heads, cfg.head_dim, cfg.hidden, cfg.q_size) == (4, 2, 128, 256, 512)
    assert cfg.sliding_window == 0 and cfg.bos_id == 510 and cfg.eos == (511,) and cfg.rms_eps == 1e-6
    for i, L in enumerate(eng.w.layers):
        a = hf.model.layers[i].self_attn
        assert L.b_qkv is None and L.q_norm.shape == (128,) and L.q_norm.dtype == torch.bfloat16
        assert torch.equal(L.q_norm, a.q_norm.weight.detach().to(torch.bfloat16))  # canonical order, as stored
        assert torch.equal(L.k_norm, a.k_norm.weight.detach().to(torch.bfloat16))
        assert (L.q_norm.float() - 1).abs().max() > 0.3
    compare(eng, hf, PROMPTS)


@pytest.mark.parametrize("variant", ["ones", "swapped", "pair_interleaved"])
def test_qwen3_parity_fails_with_wrong_norm_weights(tmp_path, variant):
    """The same comparison is outside ``compare``'s bounds once the engine's norm weights are ones,
    q and k exchanged, or applied in the pair-interleaved order of the qkv rows."""
    pytest.importorskip("transformers")
    hf = qwen3_checkpoint(str(tmp_path))
    _, eng = _engine(tmp_path, "ck-qwen3-" + variant)
    for L in eng.w.layers:
        if variant == "ones":
            L.q_norm, L.k_norm = torch.ones_like(L.q_norm), torch.ones_like(L.k_norm)
        elif variant == "swapped":
            L.q_norm, L.k_norm = L.k_norm, L.q_norm
        else:
            L.q_norm = pair_interleave_heads(L.q_norm.view(-1, 1), 128).reshape(-1).contiguous()
            L.k_norm = pair_interleave_heads(L.k_norm.view(-1, 1), 128).reshape(-1).contiguous()
    with pytest.raises(AssertionError):
        compare(eng, hf, PROMPTS)
    # ... and each of the longer prompts on its own (without the rotation q.k is the same with the
    # weights exchanged, so the 5-token prompt sits near compare's bounds in that variant)
    for ids in PROMPTS[1:]:
        with pytest.raises(AssertionError):
            compare(eng, hf, [ids])


def test_qwen3_decode_matches_transformers_greedy(tmp_path):
    pytest.importorskip("transformers")
    hf = qwen3_checkpoint(str(tmp_path))
    _, eng = _engine(tmp_path, "ck-qwen3-g")
    prompt = [3, 14, 15, 92, 65]
    ours = eng.generate_ids(prompt, 12, temperature=0.0, stop_on_eos=False)
    with torch.no_grad():
        logits = hf.float()(torch.tensor([prompt + ours])).logits[0]
    for i, t in enumerate(ours):
        row = logits[len(prompt) - 1 + i]
        top2 = torch.topk(row, 2).values
        if (top2[0] - top2[1]).item() > 1e-2:  # skip numerical near-ties
            assert t == row.argmax().item(), i


QWEN3_8B_HUB = {  # the public Qwen3-8B config.json
    "architectures": ["Qwen3ForCausalLM"], "model_type": "qwen3", "hidden_size": 4096, "intermediate_size": 12288,
    "num_hidden_layers": 36, "num_attention_heads": 32, "num_key_value_heads": 8, "head_dim": 128,
    "vocab_size": 151936, "rope_theta": 1000000, "rope_scaling": None, "rms_norm_eps": 1e-06,
    "max_position_embeddings": 40960, "attention_bias": False, "sliding_window": None, "use_sliding_window": False,
    "max_window_layers": 36, "bos_token_id": 151643, "eos_token_id": 151645, "tie_word_embeddings": False,
    "hidden_act": "silu", "attention_dropout": 0.0, "torch_dtype": "bfloat16",
}


def test_config_from_hf_qwen3_8b(tmp_path):
    (tmp_path / "config.json").write_text(json.dumps(QWEN3_8B_HUB))
    cfg = config_from_hf(str(tmp_path))
    fam = FAMILIES["qwen3-8b"]
    assert cfg.qk_norm and not cfg.qkv_bias and cfg.sliding_window == 0 and cfg.arch == "llama"
    for f in ("arch", "n_layers", "hidden", "n_heads", "n_kv_heads", "head_dim", "intermediate", "vocab", "rope_theta",
              "rms_eps", "max_position", "n_experts", "top_k_experts", "rope_scaling", "qkv_bias", "qk_norm",
              "sliding_window", "tie_embeddings", "q_size", "qkv_size"):
        assert getattr(cfg, f) == getattr(fam, f), f
    assert cfg.bos_id == 151643 and cfg.eos == (151645,)
    assert cfg.num_params() == fam.num_params()
    assert fam.num_params() - fam.with_(qk_norm=False).num_params() == fam.n_layers * 2 * fam.head_dim
    assert 8.1e9 < fam.num_params() < 8.3e9


def test_config_from_hf_keeps_a_decoupled_head_dim(tmp_path):
    """Qwen3-4B: hidden 2560 over 32 heads of 128 (hidden / heads would be 80)."""
    (tmp_path / "config.json").write_text(json.dumps(dict(QWEN3_8B_HUB, hidden_size=2560, intermediate_size=9728,
                                                          tie_word_embeddings=True)))
    cfg = config_from_hf(str(tmp_path))
    assert (cfg.head_dim, cfg.q_size, cfg.hidden) == (128, 4096, 2560) and cfg.qk_norm and cfg.tie_embeddings


def test_config_written_by_transformers_loads(tmp_path):
    """The config.json transformers writes for Qwen3 (``layer_types`` all full_attention,
    ``sliding_window`` null, ``max_window_layers``, ``rope_parameters`` of type default)."""
    pytest.importorskip("transformers")
    qwen3_checkpoint(str(tmp_path))
    hc = json.loads((tmp_path / "config.json").read_text())
    assert hc["model_type"] == "qwen3" and hc["head_dim"] == 128
    cfg = config_from_hf(str(tmp_path))
    assert cfg.qk_norm and cfg.sliding_window == 0 and cfg.rope_theta == 1e6 and cfg.rope_scaling is None
    # the same fields spelled out, whatever the installed transformers wrote
    (tmp_path / "config.json").write_text(json.dumps(dict(
        {k: v for k, v in QWEN3_8B_HUB.items() if k not in ("rope_theta", "rope_scaling")},
        num_hidden_layers=2, layer_types=["full_attention"] * 2, sliding_window=None, max_window_layers=28,
        rope_parameters={"rope_type": "default", "rope_theta": 1000000.0})))
    cfg = config_from_hf(str(tmp_path))
    assert cfg.qk_norm and cfg.sliding_window == 0 and cfg.rope_theta == 1e6 and cfg.rope_scaling is None


def test_refused_qwen3_configs_raise(tmp_path):
    def refused(d, word=None):
        (tmp_path / "config.json").write_text(json.dumps(d))
        with pytest.raises(CheckpointError) as e:
            config_from_hf(str(tmp_path))
        if word:
            assert word in str(e.value)

    refused(dict(QWEN3_8B_HUB, model_type="qwen3_moe"), "qwen3")  # the message lists the supported types
    refused(dict(QWEN3_8B_HUB, attention_bias=True))
    refused(dict(QWEN3_8B_HUB, rope_scaling={"rope_type": "yarn", "factor": 4.0,
                                             "original_max_position_embeddings": 32768}))
    no_theta = {k: v for k, v in QWEN3_8B_HUB.items() if k not in ("rope_theta", "rope_scaling")}
    refused(dict(no_theta, rope_parameters={"rope_type": "yarn", "rope_theta": 1e6, "factor": 4.0,
                                            "original_max_position_embeddings": 32768}))
    refused(dict(QWEN3_8B_HUB, num_hidden_layers=2, sliding_window=16,
                 layer_types=["full_attention", "sliding_attention"]))


def test_cpu_engine_decode_equals_prefill():
    """``qwen3-tiny``: greedy decode from a 40-token prompt; the logits each token was sampled from
    equal the prefill logits of the same prefix (test_qwen2_cpu.py's check and bounds)."""
    cfg = FAMILIES["qwen3-tiny"]
    assert cfg.qk_norm and cfg.head_dim == 128 and cfg.q_size == 2 * cfg.hidden
    eng = Engine(cfg, EngineConfig(device="cpu", max_context=256, use_graphs=False, seed=5))
    prompt = [(i * 53) % (cfg.vocab - 300) + 256 for i in range(40)]
    n = 8
    toks, lg = eng.debug_decode_logits(prompt, n)
    for i in range(n):
        s = eng.new_sequence()
        eng.prefill([s], [prompt + toks[:i]])
        lc = s.logits.float()
        eng.free_sequence(s)
        err = (lc - lg[i]).abs().max().item()
        assert err < 0.03 * max(1.0, lc.abs().max().item()), (i, err)
        top2 = torch.topk(lc, 2).values
        if (top2[0] - top2[1]).item() > 2 * err:
            assert int(lc.argmax()) == toks[i], i


def test_random_init_norms_are_wide_and_other_families_have_none():
    eng = Engine(FAMILIES["qwen3-tiny"], EngineConfig(device="cpu", max_context=64, use_graphs=False, seed=5))
    D = eng.cfg.head_dim
    for L in eng.w.layers:
        for g in (L.q_norm, L.k_norm):
            assert g.shape == (D,) and g.dtype == torch.bfloat16 and g.is_contiguous()
            assert 0.9 < g.float().mean().item() < 1.1 and 0.2 < g.float().std().item() < 0.4
        assert not torch.equal(L.q_norm, L.k_norm) and L.b_qkv is None
    assert not torch.equal(eng.w.layers[0].q_norm, eng.w.layers[1].q_norm)
    for name, cfg in FAMILIES.items():
        if cfg.qk_norm or cfg.checkpoint or cfg.n_layers > 4:
            continue
        plain = Engine(cfg, EngineConfig(device="cpu", max_context=64, use_graphs=False, seed=5))
        assert all(L.q_norm is None and L.k_norm is None for L in plain.w.layers), name
    assert [n for n, c in FAMILIES.items() if c.qk_norm and not c.checkpoint] == ["qwen3-8b", "qwen3-tiny"]


def test_oracle_rope_kv_write_norm_arguments():
    """The oracle's numerics spelled out on one head, and the argument checks of the op."""
    from llm_consensus_amd import ops
    from llm_consensus_amd.models.config import rope_inv_freq
    from llm_consensus_amd.ops import oracle

    torch.manual_seed(0)
    nh, nkv, D, T, bs = 2, 1, 64, 3, 16
    half = D // 2
    cos_t, sin_t = oracle.rope_tables(rope_inv_freq(FAMILIES["qwen3-tiny"].with_(head_dim=D)), 64)
    qkv = torch.randn(T, (nh + 2 * nkv) * D).to(torch.bfloat16)
    gq, gk = (1 + 0.3 * torch.randn(D)).to(torch.bfloat16), (1 + 0.3 * torch.randn(D)).to(torch.bfloat16)
    pos = torch.tensor([5, 0, 33], dtype=torch.int32)
    slots = torch.tensor([17, -1, 2], dtype=torch.int32)
    kc = torch.zeros(4, nkv, bs, D, dtype=torch.bfloat16)
    vc = torch.zeros_like(kc)
    q = torch.zeros(T, nh * D, dtype=torch.bfloat16)
    ops.rope_kv_write(qkv, pos, cos_t, sin_t, kc, vc, slots, nh, nkv, D, bs, q, q_norm=gq, k_norm=gk, qk_eps=1e-6)
    for t, head, g in ((0, 1, gq), (2, 2, gk)):
        x = qkv[t, head * D:(head + 1) * D].float().view(half, 2)
        x = torch.cat([x[:, 0], x[:, 1]])  # canonical order
        y = x * torch.rsqrt(x.pow(2).sum() / D + 1e-6) * g.float()
        c, s = cos_t[int(pos[t])], sin_t[int(pos[t])]
        want = torch.cat([y[:half] * c - y[half:] * s, y[half:] * c + y[:half] * s]).to(torch.bfloat16)
        sl = int(slots[t])
        got = q[t, head * D:(head + 1) * D] if head < nh else kc[sl // bs, head - nh, sl % bs]
        assert (got.float() - want.float()).abs().max().item() <= 2 ** -6, (t, head)
    assert torch.equal(vc[1, 0, 1], qkv[0, (nh + nkv) * D:]) and int(kc[:, :, :, :].abs().sum(-1).ne(0).sum()) == 2
    with pytest.raises(ValueError):
        ops.rope_kv_write(qkv, pos, cos_t, sin_t, kc, vc, slots, nh, nkv, D, bs, q, bias=qkv[0], q_norm=gq, k_norm=gk)
    with pytest.raises(ValueError):
        ops.rope_kv_write(qkv, pos, cos_t, sin_t, kc, vc, slots, nh, nkv, D, bs, q, q_norm=gq)


def _tp_worker(rank, world, port, name, q):
    import os

    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.set_num_threads(1)
        from llm_consensus_amd.parallel.comm import TPGroup

        cfg = FAMILIES[name]
        e = Engine(cfg, EngineConfig(device="cpu", max_context=128, seed=5), tp=TPGroup(dist.group.WORLD, rank, world))
        L = e.w.layers[0]
        assert L.q_norm.shape == (cfg.head_dim,) and L.w_qkv.shape[0] == cfg.qkv_size // world  # norms replicated
        p = [(i * 13) % 700 + 256 for i in range(24)]
        s = e.new_sequence()
        e.prefill([s], [p])
        logits = e.full_logits(s).clone().unsqueeze(0)
        e.free_sequence(s)
        gen = e.generate_ids(p, 6, temperature=0.0, stop_on_eos=False)
        if rank == 0:
            q.put((logits.tolist(), gen, L.q_norm.float().tolist()))  # plain lists: tensor handles die with the child
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_tp2_matches_tp1():
    """test_qwen2_cpu.py's harness on ``qwen3-tiny``: every rank normalises its own whole heads with
    the same replicated weights."""
    name = "qwen3-tiny"
    ref = Engine(FAMILIES[name], EngineConfig(device="cpu", max_context=128, seed=5))
    p = [(i * 13) % 700 + 256 for i in range(24)]
    s = ref.new_sequence()
    ref.prefill([s], [p])
    ref_logits = ref.full_logits(s).clone()
    ref.free_sequence(s)
    ref_gen = ref.generate_ids(p, 6, temperature=0.0, stop_on_eos=False)

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_tp_worker, args=(r, 2, port, name, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    for pr in procs:
        pr.join(timeout=240)
    for pr in procs:
        if pr.is_alive():
            pr.kill()
            pr.join()
    assert all(pr.exitcode == 0 for pr in procs), [pr.exitcode for pr in procs]
    logits, gen, g = q.get(timeout=10)
    logits = torch.tensor(logits)
    assert torch.equal(torch.tensor(g), ref.w.layers[0].q_norm.float())
    # TP sums partials in a different order (and rounds partials to bf16): small drift only
    assert (logits[0] - ref_logits).abs().max().item() < 0.05 * ref_logits.abs().max().item()
    top2 = torch.topk(ref_logits, 2).values
    if (top2[0] - top2[1]).item() > 0.05:
        assert gen[0] == ref_gen[0]


def test_list_models_shows_qk_norm():
    out = io.StringIO()
    with pytest.raises(SystemExit):
        cli.run(["--list-models"], stdout=out, stderr=io.StringIO())
    recs = {r["id"]: r for r in json.loads(out.getvalue())}
    r = recs["qwen3-8b"]
    assert r["qk_norm"] is True and "qkv_bias" not in r and r["arch"] == "llama" and 8.1e9 < r["params"] < 8.3e9
    assert r["context_length"] == 40960 and r["heads"] == 32 and r["kv_heads"] == 8 and r["head_dim"] == 128
    assert recs["qwen3-tiny"]["qk_norm"] is True and recs["qwen3-tiny"]["head_dim"] == 128
    for name, rec in recs.items():
        if not name.startswith("qwen3"):
            assert "qk_norm" not in rec, name
