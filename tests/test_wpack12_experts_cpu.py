"""The 12-bit twin of a MoE expert stack (``wpack.pack12_experts``) and the sizes that count it.

An ``[E, N, K]`` stack is packed as its ``[E * N, K]`` view, row by row, so the twin must be the
per-expert ``pack12_reference`` twins concatenated, planes and records, and ``unpack12_reference`` over
the view must restore the bits. ``pack_best`` takes a 3-D stack on whole 2048-weight units at 12 bits
only. A MoE model's ``packed_demand`` must be what ``pack_decode_weights`` allocates, and
``ModelConfig.packed_twin_bytes`` its upper bound from shapes alone.
"""

import pytest
import torch

from llm_consensus_amd.models.config import FAMILIES, ModelConfig
from llm_consensus_amd.models.transformer import TransformerWeights
from llm_consensus_amd.ops import wpack
from llm_consensus_amd.parallel.comm import TPGroup

# 2 layers, hidden 2048, 16 / 4 heads x 128, intermediate 2048, 4 experts, top-2, vocab 2048: every K one unit
MOE_P12 = ModelConfig("moe-p12-test", "mixtral", 2, 2048, 16, 4, 128, 2048, 2048, 1000000.0, max_position=4096,
                      n_experts=4, top_k_experts=2)
TINY = [0.0, -0.0, 1e-30, -3e-33]


def _stack(E, N, K):
    """Gaussian [E, N, K] with exceptions planted in chosen experts' rows, and one raw row
    (MAX_EXC + 1 planted values) in expert 1. -> (W, {(e, n): [k, ...]}, the raw (e, n))."""
    g = torch.Generator().manual_seed(E * 1000 + N + K)
    W = (torch.randn(E, N, K, generator=g) * K ** -0.5).to(torch.bfloat16)
    plan = {(0, 0): [0, K - 1], (E - 1, N - 1): [K // 2 + 1], (1, 3): [8 * 5 + 1, 8 * 5 + 6], (E - 1, 0): [K - 2048 + 100]}
    raw = (1, 7)
    W[raw] = ((1 + 0.9 * torch.rand(K, generator=g)) * K ** -0.5).to(torch.bfloat16)  # one exponent
    plan[raw] = [(i * K) // (wpack.MAX_EXC + 1) + 3 * i for i in range(wpack.MAX_EXC + 1)]
    for (e, n), ks in plan.items():
        for i, k in enumerate(ks):
            W[e, n, k] = TINY[i % 4]
    return W, plan, raw


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("E,N,K", [(4, 64, 2048), (3, 32, 6144)])
def test_pack12_experts_is_the_per_expert_twins_concatenated(E, N, K):
    W, plan, raw = _stack(E, N, K)
    pw = wpack.pack12_experts(W)
    assert isinstance(pw, wpack.PackedExperts12) and isinstance(pw, wpack.PackedWeight12)
    assert (pw.E, pw.rows, pw.N, pw.K) == (E, N, E * N, K)
    each = [wpack.pack12_reference(W[e]) for e in range(E)]
    assert torch.equal(pw.planes, torch.cat([p.planes for p in each]))
    assert torch.equal(pw.hdr, torch.cat([p.hdr for p in each]))
    assert pw.raw_rows == sum(p.raw_rows for p in each) and pw.exceptions == sum(p.exceptions for p in each)
    assert pw.nbytes() == wpack.packed12_nbytes(E * N, K)
    # each planted row took the intended path, at row e * N + n
    rec = pw.records().to(torch.int64) & 0xFFFFFFFF
    for (e, n), ks in plan.items():
        r = e * N + n
        base, cnt = int(rec[r, 0] & 0xFF), int(rec[r, 0] >> 8 & 0xFF)
        if (e, n) == raw:
            assert base == wpack.RAW and cnt == 0
        else:
            assert base != wpack.RAW and set(ks) <= set((rec[r, 1:1 + cnt] & 0xFFFF).tolist())
    assert 1 <= pw.raw_rows <= 1 + E * N // 100
    # the view's bits come back (the raw row from W)
    back = wpack.unpack12_reference(pw, W.view(E * N, K))
    assert torch.equal(_bits(back), _bits(W.view(E * N, K)))


def test_pack_best_on_expert_stacks():
    W, _, _ = _stack(4, 128, 2048)  # one raw row of 512: under MAX_RAW_SHARE
    pw = wpack.pack_best(W, fmt=12)
    assert isinstance(pw, wpack.PackedExperts12) and pw.raw_share <= wpack.MAX_RAW_SHARE
    assert torch.equal(pw.planes, wpack.pack12_experts(W).planes)
    assert wpack.pack_best(W, fmt=13) is None                       # no 13-bit expert format
    g = torch.Generator().manual_seed(5)
    for K in (2560, 1024, 256):                                      # off the unit: no tail for experts
        assert wpack.pack_best((torch.randn(2, 8, K, generator=g) * 0.02).to(torch.bfloat16), fmt=12) is None
    # more than MAX_RAW_SHARE raw rows: no twin (the stack of (4, 64): one raw row of 256 is 0.4 %, two of 64 are 3 %)
    few, _, _ = _stack(2, 32, 2048)
    few[0, 5] = few[1, 7]
    assert wpack.pack12_experts(few).raw_share > wpack.MAX_RAW_SHARE and wpack.pack_best(few, fmt=12) is None
    with pytest.raises(ValueError):
        wpack.pack12_experts(W.view(4 * 128, 2048))
    with pytest.raises(ValueError):
        wpack.pack12_experts(W[:, ::2])                              # not contiguous


def test_moe_model_packs_and_its_demand_is_what_it_allocates(monkeypatch):
    monkeypatch.delenv("LLMC_PACKED_FORMAT", raising=False)
    w = TransformerWeights(MOE_P12, TPGroup.single(), torch.device("cpu"), seed=3)
    for with_o in (True, False):
        need = w.packed_demand(with_o)
        st = w.pack_decode_weights(with_o)   # on the CPU: the reference packer
        L = w.layers[0]
        assert isinstance(L.p_gu, wpack.PackedExperts12) and isinstance(L.p_down, wpack.PackedExperts12)
        assert (L.p_gu.E, L.p_gu.rows, L.p_gu.K) == tuple(L.w_gu.shape) == (4, 4096, 2048)
        assert (L.p_down.E, L.p_down.rows, L.p_down.K) == tuple(L.w_down.shape) == (4, 2048, 2048)
        assert isinstance(L.p_qkv, wpack.PackedWeight12) and isinstance(w.p_lm_head, wpack.PackedWeight12)
        assert (L.p_o is not None) == with_o
        per_layer = 4 if with_o else 3
        assert st["tensors"] == st["packed"] == st["p12"] == 1 + 2 * per_layer and st["p13"] == st["tail"] == 0
        assert st["bytes"] == w.packed_nbytes() == need
        assert MOE_P12.packed_twin_bytes() >= need
    # the twin restores the expert stack
    L = w.layers[1]
    E, N, K = L.w_down.shape
    back = wpack.unpack12_reference(L.p_down, L.w_down.view(E * N, K))
    assert torch.equal(_bits(back), _bits(L.w_down.view(E * N, K)))


def test_packed_twin_bytes_counts_moe_from_shapes():
    assert FAMILIES["mixtral-tiny"].packed_twin_bytes() == 0        # K = 256 / 384: nothing packs
    c = FAMILIES["mixtral-8x7b"]
    h, i, E = c.hidden, c.intermediate, c.n_experts
    experts = sum(wpack.packed12_nbytes(E * n, k) for n, k in ((2 * i, h), (h, i)))
    dense = sum(n * k * 13 // 8 for n, k in ((c.qkv_size, h), (h, c.q_size)))
    assert c.packed_twin_bytes() == c.n_layers * (experts + dense) + c.vocab * h * 13 // 8 > 0
    assert 0.70 < c.packed_twin_bytes() / c.weight_bytes() < 0.8125
