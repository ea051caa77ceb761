"""Sliding-window attention without a GPU: the loader's window against ``transformers`` (tiny
random Mistral and windowed Phi-3 checkpoints), the CPU engine's decode against its prefill across
L = W, per-layer windows still refused, the catalog records."""

import io
import json

import pytest
import torch

from llm_consensus_amd import cli
from llm_consensus_amd.engine import Engine, EngineConfig
from llm_consensus_amd.models.checkpoint import CheckpointError, config_from_hf
from llm_consensus_amd.models.config import FAMILIES
from llm_consensus_amd.ops import oracle

PROMPTS = [[5], [7, 100, 3, 9, 400], list(range(40, 56)), list(range(40, 57)), list(range(40, 140))]  # 1, 5, 16, 17, 100


def _mistral(tmp, window=16):
    from transformers import MistralConfig, MistralForCausalLM

    c = MistralConfig(vocab_size=512, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, head_dim=32, max_position_embeddings=512, sliding_window=window,
                      rms_norm_eps=1e-5, tie_word_embeddings=False, pad_token_id=0, bos_token_id=1, eos_token_id=2,
                      attn_implementation="eager")
    torch.manual_seed(3)
    m = MistralForCausalLM(c).to(torch.bfloat16)
    m.save_pretrained(tmp, safe_serialization=True)
    return m


def _phi3(tmp, window=33, inter=256):
    from transformers import Phi3Config, Phi3ForCausalLM

    c = Phi3Config(vocab_size=512, hidden_size=192, intermediate_size=inter, num_hidden_layers=2, num_attention_heads=2,
                   num_key_value_heads=2, max_position_embeddings=2048, original_max_position_embeddings=2048,
                   rope_theta=10000.0, pad_token_id=0, bos_token_id=1, eos_token_id=2, tie_word_embeddings=False,
                   sliding_window=window, attn_implementation="eager")
    torch.manual_seed(2)
    m = Phi3ForCausalLM(c).to(torch.bfloat16)
    m.save_pretrained(tmp, safe_serialization=True)
    return m


def _hf_last_logits(m, ids):
    mf = m.float()
    with torch.no_grad():
        out = mf(torch.tensor([ids])).logits[0, -1]
    m.to(torch.bfloat16)
    return out


def _compare(eng, hf, prompts):
    for ids in prompts:
        s = eng.new_sequence()
        eng.prefill([s], [ids])
        ours = eng.full_logits(s).float().cpu()
        eng.free_sequence(s)
        ref = _hf_last_logits(hf, ids)
        cos = torch.nn.functional.cosine_similarity(ours, ref, dim=0).item()
        err = (ours - ref).abs().max().item() / ref.abs().max().item()
        assert cos > 0.999 and err < 0.05, (len(ids), cos, err)
        assert ours.argmax().item() == ref.argmax().item()


def test_mistral_checkpoint_matches_transformers(tmp_path):
    pytest.importorskip("transformers")
    hf = _mistral(str(tmp_path))
    cfg = config_from_hf(str(tmp_path), name="ck-mistral")
    assert cfg.arch == "llama" and cfg.sliding_window == 16 and cfg.head_dim == 32 and cfg.n_kv_heads == 2
    eng = Engine(cfg, EngineConfig(device="cpu", max_context=512, use_graphs=False))
    _compare(eng, hf, PROMPTS)
    # the window is what makes the 100-token prompt match: without it the logits move
    full = Engine(cfg.with_(sliding_window=0), EngineConfig(device="cpu", max_context=512, use_graphs=False),
                  weights=eng.w)
    s = full.new_sequence()
    full.prefill([s], [PROMPTS[-1]])
    ref = _hf_last_logits(hf, PROMPTS[-1])
    assert (full.full_logits(s).float() - ref).abs().max().item() / ref.abs().max().item() > 0.02


def test_phi3_windowed_checkpoint_matches_transformers(tmp_path):
    pytest.importorskip("transformers")
    hf = _phi3(str(tmp_path))
    cfg = config_from_hf(str(tmp_path), name="ck-phi3-swa")
    assert cfg.arch == "phi3" and cfg.sliding_window == 33 and cfg.head_dim == 96
    eng = Engine(cfg, EngineConfig(device="cpu", max_context=512, use_graphs=False))
    _compare(eng, hf, PROMPTS)


def test_window_not_shorter_than_context_is_no_window(tmp_path):
    pytest.importorskip("transformers")
    _mistral(str(tmp_path), window=512)  # == max_position_embeddings
    assert config_from_hf(str(tmp_path)).sliding_window == 0


@pytest.mark.parametrize("extra", [
    {"layer_types": ["sliding_attention", "full_attention"]},
    {"max_window_layers": 1},
])
def test_per_layer_window_still_raises(tmp_path, extra):
    pytest.importorskip("transformers")
    _mistral(str(tmp_path))
    p = tmp_path / "config.json"
    c = json.loads(p.read_text())
    c.update(extra)
    p.write_text(json.dumps(c))
    with pytest.raises(CheckpointError):
        config_from_hf(str(tmp_path))
    # the same keys describing one window for every layer load
    c.update({"layer_types": ["sliding_attention"] * 2} if "layer_types" in extra else {"max_window_layers": 0})
    p.write_text(json.dumps(c))
    assert config_from_hf(str(tmp_path)).sliding_window == 16


@pytest.mark.parametrize("name", ["mistral-tiny"])
def test_cpu_engine_decode_equals_prefill_across_the_window(name):
    """Greedy decode from a 40-token prompt through L = W = 48: the logits each token was sampled
    from equal the prefill logits of the same prefix (both run the fp32 oracle; they differ only in
    the summation order of the attention, far below bf16 rounding of the activations)."""
    cfg = FAMILIES[name]
    assert cfg.sliding_window == 48
    eng = Engine(cfg, EngineConfig(device="cpu", max_context=256, use_graphs=False, seed=5))
    prompt = [(i * 53) % (cfg.vocab - 300) + 256 for i in range(40)]
    n = 14
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


def test_oracle_window_semantics():
    """Position p attends keys (p - W, p]: W keys including itself; W = 0 and W >= L are all keys;
    decode at length L equals the prefill row at position L - 1."""
    torch.manual_seed(0)
    nh, nkv, D, bs, L = 4, 2, 32, 16, 50
    kc = torch.randn(8, nkv, bs, D).to(torch.bfloat16)
    vc = torch.randn(8, nkv, bs, D).to(torch.bfloat16)
    bt = torch.tensor([[3, 0, 5, 1]], dtype=torch.int32)
    q = torch.randn(L, nh * D).to(torch.bfloat16)
    z, n = torch.tensor([0], dtype=torch.int32), torch.tensor([L], dtype=torch.int32)

    def pre(W):
        return oracle.attn_prefill(q, kc, vc, bt, z, n, n, nh, nkv, D, bs, 0.2, torch.zeros(L, nh * D, dtype=torch.bfloat16),
                                   W)

    full = pre(0)
    assert torch.equal(pre(50), full) and torch.equal(pre(1000), full)
    assert not torch.equal(pre(49)[-1], full[-1]) and torch.equal(pre(49)[:-1], full[:-1])
    for W in (1, 16, 49):
        dec = oracle.attn_decode(q[-1:], kc, vc, bt, n, nh, nkv, D, bs, 0.2, W)
        assert torch.allclose(dec.float(), pre(W)[-1:].float(), atol=1e-2)
    # W = 1: a token attends itself only, so its output is its own V row
    v_last = vc[bt[0, (L - 1) // bs].long(), :, (L - 1) % bs].repeat_interleave(nh // nkv, dim=0).reshape(-1)
    assert torch.equal(pre(1)[-1], v_last)


def test_list_models_shows_the_window():
    out = io.StringIO()
    with pytest.raises(SystemExit):
        cli.run(["--list-models"], stdout=out, stderr=io.StringIO())
    recs = {r["id"]: r for r in json.loads(out.getvalue())}
    assert recs["mistral-7b"]["sliding_window"] == 4096 and recs["mistral-7b"]["arch"] == "llama"
    assert recs["mistral-7b"]["context_length"] == 32768 and 7.2e9 < recs["mistral-7b"]["params"] < 7.3e9
    assert recs["mistral-tiny"]["sliding_window"] == 48
    for name in ("llama-3-8b", "phi-3-mini", "mixtral-8x7b", "llama-tiny"):
        assert "sliding_window" not in recs[name]


def test_engine_drops_a_window_no_context_can_outgrow():
    """W >= the longest context the engine serves masks nothing: that engine runs unwindowed (and
    on the GPU keeps the fused launches); a longer context keeps the window."""
    cfg = FAMILIES["mistral-tiny"]
    assert Engine(cfg, EngineConfig(device="cpu", max_context=32, use_graphs=False)).window == 0
    assert Engine(cfg, EngineConfig(device="cpu", max_context=256, use_graphs=False)).window == 48
