"""Qwen2 / Qwen2.5 without a GPU: the loader and the q/k/v bias against ``transformers`` (a tiny
random Qwen2 checkpoint with NON-ZERO biases: ``Qwen2ForCausalLM`` initialises them to zero, and a
zero bias would pass with the bias dropped), the hub Qwen2.5-7B config, the refused variants, the
CPU engine's decode against its prefill on ``qwen2-tiny`` (GQA group 7), TP = 2 over gloo against
TP = 1 (the bias shard and pair-interleave), the catalog record and the weight layout."""

import io
import json
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from llm_consensus_amd import cli
from llm_consensus_amd.engine import Engine, EngineConfig
from llm_consensus_amd.models.checkpoint import CheckpointError, config_from_hf
from llm_consensus_amd.models.config import FAMILIES
from llm_consensus_amd.models.transformer import pair_interleave_heads

PROMPTS = [[5], [7, 100, 3, 9, 400], list(range(40, 140))]  # test_checkpoint.py's


def qwen2_checkpoint(tmp):
    """Tiny random Qwen2 (14 / 2 heads of 64: group 7) with std-1 q/k/v biases, saved to ``tmp``."""
    from transformers import Qwen2Config, Qwen2ForCausalLM

    c = Qwen2Config(vocab_size=512, hidden_size=896, intermediate_size=1024, num_hidden_layers=2,
                    num_attention_heads=14, num_key_value_heads=2, max_position_embeddings=2048, rms_norm_eps=1e-6,
                    rope_theta=1e6, tie_word_embeddings=False, bos_token_id=510, eos_token_id=511)
    torch.manual_seed(3)
    m = Qwen2ForCausalLM(c)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for layer in m.model.layers:
            for proj in (layer.self_attn.q_proj, layer.self_attn.k_proj, layer.self_attn.v_proj):
                proj.bias.copy_(torch.randn(proj.bias.shape, generator=g) * 1.0)
    m = m.to(torch.bfloat16)
    m.save_pretrained(tmp, safe_serialization=True)
    return m


def hf_last_logits(m, ids):
    mf = m.float()
    with torch.no_grad():
        out = mf(torch.tensor([ids])).logits[0, -1]
    m.to(torch.bfloat16)
    return out


def compare(eng, hf, prompts):
    """test_checkpoint.py's ``_compare`` with the argmax guarded by the top-2 gap (hidden 896 over a
    512-token vocabulary has near-ties a bf16 engine may flip)."""
    for ids in prompts:
        s = eng.new_sequence()
        eng.prefill([s], [ids])
        ours = eng.full_logits(s).float().cpu()
        eng.free_sequence(s)
        ref = hf_last_logits(hf, ids)
        cos = torch.nn.functional.cosine_similarity(ours, ref, dim=0).item()
        abs_err = (ours - ref).abs().max().item()
        err = abs_err / ref.abs().max().item()
        print(f"qwen2 parity: len {len(ids)} cos {cos:.6f} err {err:.5f}")
        assert cos > 0.999 and err < 0.05, (len(ids), cos, err)
        top2 = torch.topk(ref, 2).values
        if (top2[0] - top2[1]).item() > 2 * abs_err:
            assert ours.argmax().item() == ref.argmax().item()


def test_qwen2_checkpoint_matches_transformers(tmp_path):
    pytest.importorskip("transformers")
    hf = qwen2_checkpoint(str(tmp_path))
    cfg = config_from_hf(str(tmp_path), name="ck-qwen2")
    assert cfg.arch == "llama" and cfg.qkv_bias and cfg.n_heads == 14 and cfg.n_kv_heads == 2 and cfg.head_dim == 64
    assert cfg.sliding_window == 0 and cfg.bos_id == 510 and cfg.eos == (511,) and cfg.rms_eps == 1e-6
    eng = Engine(cfg, EngineConfig(device="cpu", max_context=512, use_graphs=False))
    assert all(L.b_qkv is not None and L.b_qkv.float().abs().max() > 1.0 for L in eng.w.layers)
    compare(eng, hf, PROMPTS)
    # the bias is what makes it match: with the biases dropped the logits are another model's
    for L in eng.w.layers:
        L.b_qkv = None
    s = eng.new_sequence()
    eng.prefill([s], [PROMPTS[-1]])
    ref = hf_last_logits(hf, PROMPTS[-1])
    assert torch.nn.functional.cosine_similarity(eng.full_logits(s).float(), ref, dim=0).item() < 0.9


def test_qwen2_decode_matches_transformers_greedy(tmp_path):
    pytest.importorskip("transformers")
    hf = qwen2_checkpoint(str(tmp_path))
    cfg = config_from_hf(str(tmp_path), name="ck-qwen2-g")
    eng = Engine(cfg, EngineConfig(device="cpu", max_context=512, use_graphs=False))
    prompt = [3, 14, 15, 92, 65]
    ours = eng.generate_ids(prompt, 12, temperature=0.0, stop_on_eos=False)
    # teacher-forced check of every generated token against transformers' next-token argmax
    with torch.no_grad():
        logits = hf.float()(torch.tensor([prompt + ours])).logits[0]
    for i, t in enumerate(ours):
        row = logits[len(prompt) - 1 + i]
        top2 = torch.topk(row, 2).values
        if (top2[0] - top2[1]).item() > 1e-2:  # skip numerical near-ties
            assert t == row.argmax().item(), i


QWEN25_7B_HUB = {  # the public Qwen2.5-7B-Instruct config.json
    "architectures": ["Qwen2ForCausalLM"], "model_type": "qwen2", "hidden_size": 3584, "intermediate_size": 18944,
    "num_hidden_layers": 28, "num_attention_heads": 28, "num_key_value_heads": 4, "vocab_size": 152064,
    "rope_theta": 1000000.0, "rms_norm_eps": 1e-06, "max_position_embeddings": 32768, "sliding_window": 131072,
    "max_window_layers": 28, "use_sliding_window": False, "bos_token_id": 151643, "eos_token_id": 151645,
    "tie_word_embeddings": False, "hidden_act": "silu", "attention_dropout": 0.0, "torch_dtype": "bfloat16",
}


def test_config_from_hf_qwen25_7b(tmp_path):
    (tmp_path / "config.json").write_text(json.dumps(QWEN25_7B_HUB))
    cfg = config_from_hf(str(tmp_path))
    fam = FAMILIES["qwen2.5-7b"]
    assert cfg.qkv_bias and cfg.sliding_window == 0 and cfg.arch == "llama"
    for f in ("n_layers", "hidden", "n_heads", "n_kv_heads", "head_dim", "intermediate", "vocab", "rope_theta",
              "rms_eps", "max_position", "n_experts", "qkv_bias", "sliding_window", "qkv_size"):
        assert getattr(cfg, f) == getattr(fam, f), f
    assert cfg.bos_id == 151643 and cfg.eos == (151645,) and not cfg.tie_embeddings
    assert cfg.num_params() == fam.num_params()


def test_refused_configs_still_raise(tmp_path):
    def write(d):
        (tmp_path / "config.json").write_text(json.dumps(d))

    llama = {"model_type": "llama", "hidden_size": 128, "intermediate_size": 256, "num_hidden_layers": 2,
             "num_attention_heads": 4, "num_key_value_heads": 2, "vocab_size": 512, "max_position_embeddings": 2048}
    write(llama)
    assert not config_from_hf(str(tmp_path)).qkv_bias
    for key in ("attention_bias", "mlp_bias"):  # a bias on o_proj / the MLP
        write(dict(llama, **{key: True}))
        with pytest.raises(CheckpointError):
            config_from_hf(str(tmp_path))
    write(dict(llama, model_type="mistral", attention_bias=True))
    with pytest.raises(CheckpointError):
        config_from_hf(str(tmp_path))
    # a qwen2 window that really applies to some layers only
    write(dict(QWEN25_7B_HUB, num_hidden_layers=2, use_sliding_window=True, sliding_window=16, max_window_layers=1))
    with pytest.raises(CheckpointError):
        config_from_hf(str(tmp_path))
    write(dict(QWEN25_7B_HUB, model_type="qwen2_moe"))
    with pytest.raises(CheckpointError):
        config_from_hf(str(tmp_path))
    # YaRN (the long-context Qwen variants) is refused as before
    write(dict(QWEN25_7B_HUB, rope_scaling={"type": "yarn", "factor": 4.0, "original_max_position_embeddings": 32768}))
    with pytest.raises(CheckpointError):
        config_from_hf(str(tmp_path))


def test_cpu_engine_decode_equals_prefill():
    """``qwen2-tiny`` (group 7, biased): greedy decode from a 40-token prompt; the logits each token
    was sampled from equal the prefill logits of the same prefix (test_sliding_window_cpu.py's
    check and bounds)."""
    cfg = FAMILIES["qwen2-tiny"]
    assert cfg.qkv_bias and cfg.n_heads // cfg.n_kv_heads == 7
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


def test_random_init_bias_is_not_zero_and_leaves_other_families_alone():
    eng = Engine(FAMILIES["qwen2-tiny"], EngineConfig(device="cpu", max_context=64, use_graphs=False, seed=5))
    c = eng.cfg
    for L in eng.w.layers:
        assert L.b_qkv.shape == (c.qkv_size,) and L.b_qkv.dtype == torch.bfloat16
        assert 0.8 < L.b_qkv.float().std().item() < 1.2
    assert not torch.equal(eng.w.layers[0].b_qkv, eng.w.layers[1].b_qkv)
    plain = Engine(FAMILIES["llama-tiny"], EngineConfig(device="cpu", max_context=64, use_graphs=False, seed=5))
    assert all(L.b_qkv is None for L in plain.w.layers)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _tp_worker(rank, world, port, name, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.set_num_threads(1)
        from llm_consensus_amd.parallel.comm import TPGroup

        cfg = FAMILIES[name]
        e = Engine(cfg, EngineConfig(device="cpu", max_context=128, seed=5), tp=TPGroup(dist.group.WORLD, rank, world))
        assert e.w.layers[0].b_qkv.shape == (cfg.qkv_size // world,)
        p = [(i * 13) % 700 + 256 for i in range(24)]
        s = e.new_sequence()
        e.prefill([s], [p])
        logits = e.full_logits(s).clone().unsqueeze(0)
        e.free_sequence(s)
        gen = e.generate_ids(p, 6, temperature=0.0, stop_on_eos=False)
        if rank == 0:
            q.put((logits.tolist(), gen))  # plain lists: tensor handles die with the child
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_tp2_matches_tp1():
    """test_tp_cpu.py's harness on ``qwen2-tiny``: a wrong bias shard or interleave moves the logits
    by far more than the summation-order drift allowed here."""
    name = "qwen2-tiny"
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
    logits, gen = q.get(timeout=10)
    logits = torch.tensor(logits)
    # TP sums partials in a different order (and rounds partials to bf16): small drift only
    assert (logits[0] - ref_logits).abs().max().item() < 0.05 * ref_logits.abs().max().item()
    top2 = torch.topk(ref_logits, 2).values
    if (top2[0] - top2[1]).item() > 0.05:
        assert gen[0] == ref_gen[0]


def test_list_models_shows_qkv_bias():
    out = io.StringIO()
    with pytest.raises(SystemExit):
        cli.run(["--list-models"], stdout=out, stderr=io.StringIO())
    recs = {r["id"]: r for r in json.loads(out.getvalue())}
    r = recs["qwen2.5-7b"]
    assert r["qkv_bias"] is True and r["arch"] == "llama" and 7.5e9 < r["params"] < 7.7e9
    assert r["context_length"] == 32768 and r["heads"] == 28 and r["kv_heads"] == 4 and "sliding_window" not in r
    assert recs["qwen2-tiny"]["qkv_bias"] is True
    for name in ("llama-3-8b", "phi-3-mini", "mixtral-8x7b", "mistral-7b", "llama-tiny"):
        assert "qkv_bias" not in recs[name]
    c = FAMILIES["qwen2.5-7b"]
    assert c.num_params() - c.with_(qkv_bias=False).num_params() == c.n_layers * c.qkv_size


def test_checkpoint_bias_layout_follows_the_weight_rows(tmp_path):
    """``b_qkv`` is the q | k | v biases permuted exactly as the rows of ``w_qkv``: the same shard
    ranges, ``pair_interleave_heads`` applied to the bias as a [N, 1] column."""
    pytest.importorskip("transformers")
    hf = qwen2_checkpoint(str(tmp_path))
    cfg = config_from_hf(str(tmp_path), name="ck-qwen2-layout")
    eng = Engine(cfg, EngineConfig(device="cpu", max_context=64, use_graphs=False))
    D, nq, nk = cfg.head_dim, cfg.q_size, cfg.kv_size
    for i, L in enumerate(eng.w.layers):
        a = hf.model.layers[i].self_attn
        col = torch.cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias]).detach().to(torch.bfloat16).view(-1, 1)
        want = torch.cat([pair_interleave_heads(col[:nq], D), pair_interleave_heads(col[nq:nq + nk], D), col[nq + nk:]])
        assert torch.equal(L.b_qkv, want.reshape(-1))
        W = torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight]).detach().to(torch.bfloat16)
        wantW = torch.cat([pair_interleave_heads(W[:nq], D), pair_interleave_heads(W[nq:nq + nk], D), W[nq + nk:]])
        assert torch.equal(L.w_qkv, wantW)
        # spot check of the permutation itself: row 1 of a head is its dim D / 2
        assert L.b_qkv[1] == a.q_proj.bias[D // 2].to(torch.bfloat16)
