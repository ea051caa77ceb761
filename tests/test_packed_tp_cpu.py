"""Packed decode twins on tensor-parallel ranks, the parts that need no GPU: the memory accounting from
shapes alone (``ModelConfig.packed_twin_bytes(tp)``, the placement demand) and a rank packing its own
shards with the reference packer."""

import pytest
import torch

from llm_consensus_amd.models.config import FAMILIES, LLAMA3_8B, LLAMA3_70B, MIXTRAL_8X7B, ModelConfig
from llm_consensus_amd.models.transformer import TransformerWeights
from llm_consensus_amd.ops import wpack
from llm_consensus_amd.parallel.comm import TPGroup
from llm_consensus_amd.provider.local import model_demand


def _bits(t):
    return t.contiguous().view(torch.int16)


def _unsharded_twin_bytes(c):
    """The unsharded count as it was before there was a ``tp``: 13/16 of a K on whole 2048-weight units, the
    12-bit twin with a tail and a 68-byte record per row for another multiple of 512 above 2048; a MoE
    model's expert stacks at 12 bits on whole units."""
    h, i = c.hidden, c.intermediate

    def twin(n, k):
        if k % 2048 == 0:
            return n * k * 13 // 8
        return n * k * 12 // 8 + 68 * n if k % 512 == 0 and k > 2048 else 0

    def experts(n, k):
        rows = c.n_experts * n
        return rows * k * 12 // 8 + 68 * rows if k % 2048 == 0 and k <= 65536 - 2048 else 0

    ffn = experts(2 * i, h) + experts(h, i) if c.is_moe else twin(2 * i, h) + twin(h, i)
    return c.n_layers * (twin(c.qkv_size, h) + twin(h, c.q_size) + ffn) + twin(c.vocab, h)


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_packed_twin_bytes_tp1_is_the_unsharded_count(name):
    c = FAMILIES[name]
    assert c.packed_twin_bytes(tp=1) == c.packed_twin_bytes() == _unsharded_twin_bytes(c)


def _sum(shapes):
    """Whole units: the 13-bit planes (the upper bound the unsharded count uses); a tail: the 12-bit twin."""
    tot = 0
    for N, K in shapes:
        tot += N * (K // wpack.UNIT_ELEMS) * wpack.UNIT_BYTES if K % 2048 == 0 else wpack.packed12_tail_nbytes(N, K)
    return tot


def test_packed_twin_bytes_counts_a_rank_s_shard_shapes():
    # Llama-3-70B on 4 ranks: qkv (64 + 2 * 8) * 128 / 4 rows, o_proj K = 8192 / 4, gate_up 2 * 28672 / 4
    # rows, down K = 28672 / 4 = 7168 (3 units and a 2-chunk tail), lm_head 128256 / 4 rows
    layer = [(2560, 8192), (8192, 2048), (14336, 8192), (8192, 7168)]
    assert wpack.packable12_tail_shape(8192, 7168) and 7168 % 2048 // 512 == 2
    assert LLAMA3_70B.packed_twin_bytes(tp=4) == 80 * _sum(layer) + _sum([(32064, 8192)])
    # ... on 8: down K = 3584, o_proj K = 1024 has no twin
    layer8 = [(1280, 8192), (7168, 8192), (8192, 3584)]
    assert LLAMA3_70B.packed_twin_bytes(tp=8) == 80 * _sum(layer8) + _sum([(16032, 8192)])
    # Llama-3-8B on 2 ranks: qkv 6144 / 2, o_proj K = 2048, gate_up 28672 / 2, down K = 7168, lm_head 128256 / 2
    layer = [(3072, 4096), (4096, 2048), (14336, 4096), (4096, 7168)]
    assert LLAMA3_8B.packed_twin_bytes(tp=2) == 32 * _sum(layer) + _sum([(64128, 4096)])
    # a rank's twin is no more than its share of the unsharded one (the records of a tail aside)
    assert LLAMA3_8B.packed_twin_bytes(tp=2) * 2 <= LLAMA3_8B.packed_twin_bytes() + 2 * 32 * 68 * 4096


def test_packed_twin_bytes_skips_shards_no_format_takes():
    # Llama-3-8B on 8 ranks: o_proj K = 512 (under 2048) and down K = 1792 (no multiple of 512): nothing
    assert not wpack.packable_shape(4096, 1792) and not wpack.packable12_tail_shape(4096, 1792)
    assert not wpack.packable12_tail_shape(4096, 512)
    layer = [(768, 4096), (3584, 4096)]
    assert LLAMA3_8B.packed_twin_bytes(tp=8) == 32 * _sum(layer) + _sum([(16032, 4096)])
    # on 4: o_proj K = 1024 has none, down K = 3584 has a tail
    layer = [(1536, 4096), (7168, 4096), (4096, 3584)]
    assert LLAMA3_8B.packed_twin_bytes(tp=4) == 32 * _sum(layer) + _sum([(32064, 4096)])
    # a MoE model's expert shards have no packed form under TP
    assert MIXTRAL_8X7B.packed_twin_bytes(tp=2) == 0 < MIXTRAL_8X7B.packed_twin_bytes()


def test_placement_demand_counts_the_twins_of_a_dense_tp_model(monkeypatch):
    monkeypatch.delenv("LLMC_PACKED_WEIGHTS", raising=False)
    c, ctx = LLAMA3_70B, 8192
    d = model_demand(c.name, c, ctx, 4, is_judge=True)
    # ModelDemand.weight_bytes is the model's over its GPUs: tp ranks' twins beside the bf16 weights
    assert d.tp == 4 and d.is_judge and d.kv_bytes == c.kv_bytes_per_token() * ctx
    assert d.weight_bytes == c.weight_bytes() + 4 * c.packed_twin_bytes(tp=4) > c.weight_bytes()
    assert model_demand(c.name, c, ctx, 1).weight_bytes == c.weight_bytes() + c.packed_twin_bytes()
    assert model_demand(c.name, c, ctx, 4, on_cpu=True).weight_bytes == c.weight_bytes()
    m = MIXTRAL_8X7B
    assert model_demand(m.name, m, ctx, 2).weight_bytes == m.weight_bytes()
    assert model_demand(m.name, m, ctx, 1).weight_bytes == m.weight_bytes() + m.packed_twin_bytes()
    monkeypatch.setenv("LLMC_PACKED_WEIGHTS", "off")
    assert model_demand(c.name, c, ctx, 4).weight_bytes == c.weight_bytes()
    assert model_demand(c.name, c, ctx, 1).weight_bytes == c.weight_bytes()


# K of the catalog's row-parallel shards (o_proj 2048: 70B TP = 4, 8B TP = 2; down 7168 and 3584) and of the
# column-parallel ones (4096, 8192), at a few rows: rows are packed one by one
@pytest.mark.parametrize("K", [2048, 3584, 7168, 4096, 8192])
def test_pack_best_of_a_shard_round_trips(monkeypatch, K):
    monkeypatch.delenv("LLMC_PACKED_FORMAT", raising=False)
    N = 128                        # one planted raw row stays under MAX_RAW_SHARE
    g = torch.Generator().manual_seed(K)
    full = (torch.randn(N, 2 * K, generator=g) / K ** 0.5).to(torch.bfloat16)
    full[3, K + 5] = 0.0           # an exception in the shard's first chunk
    full[3, 2 * K - 2] = 0.0       # ... and in its last (the tail's, where K has one)
    full[7, K:K + 40] = 0.0        # more than 16 exceptions: a raw row
    shard = full[:, K:]            # rank 1 of 2: a column slice, made contiguous before it is packed
    assert not shard.is_contiguous()
    W = shard.contiguous()
    pw = wpack.pack_best(W)        # on the CPU: the reference packer
    if K % 2048:
        assert type(pw) is wpack.PackedWeight12Tail
        back = wpack.unpack12_tail_reference(pw, W)
    else:
        assert type(pw) is wpack.PackedWeight12
        back = wpack.unpack12_reference(pw, W)
    assert (pw.N, pw.K) == (N, K) and pw.raw_rows >= 1 and pw.exceptions >= 2
    assert int(pw.records()[7, 0]) & 0xFF == 0xFF
    assert torch.equal(_bits(back), _bits(W))


def test_a_rank_packs_its_own_shards():
    """TransformerWeights of rank 1 of 2 on the CPU (the reference packer): every twin is that of the
    rank's shard, a tail where the shard's K has one, and ``packed_demand`` is what was allocated."""
    cfg = ModelConfig("llama-tp-pack-cpu-test", "llama", 1, 2048, 32, 2, 128, 5120, 1024, 500000.0, max_position=4096)
    w = TransformerWeights(cfg, TPGroup(None, 1, 2), torch.device("cpu"), seed=3)
    L = w.layers[0]
    assert tuple(L.w_o.shape) == (2048, 2048) and tuple(L.w_down.shape) == (2048, 2560)
    assert tuple(L.w_qkv.shape) == (2304, 2048) and tuple(w.lm_head.shape) == (512, 2048)
    need = w.packed_demand()
    st = w.pack_decode_weights()
    assert st["tensors"] == st["packed"] == st["p12"] == 5 and st["tail"] == 1 and st["p13"] == 0
    assert st["bytes"] == w.packed_nbytes() == need <= cfg.packed_twin_bytes(tp=2)
    assert type(L.p_down) is wpack.PackedWeight12Tail and (L.p_down.N, L.p_down.K) == (2048, 2560)
    assert type(L.p_o) is wpack.PackedWeight12 and (L.p_o.N, L.p_o.K) == (2048, 2048)
    assert torch.equal(_bits(wpack.unpack12_tail_reference(L.p_down, L.w_down)), _bits(L.w_down))
    assert torch.equal(_bits(wpack.unpack12_reference(L.p_o, L.w_o)), _bits(L.w_o))
    # twins nobody reads are not built, and the demand follows
    w2 = TransformerWeights(cfg, TPGroup(None, 1, 2), torch.device("cpu"), seed=3)
    assert w2.packed_demand(with_o=False, with_qkv=False) == need - L.p_o.nbytes() - L.p_qkv.nbytes()
    st2 = w2.pack_decode_weights(with_o=False, with_qkv=False)
    assert st2["packed"] == 3 and w2.layers[0].p_o is None and w2.layers[0].p_qkv is None
    assert w2.packed_nbytes() == w2.packed_demand(with_o=False, with_qkv=False)


def test_fused_allreduce_per_shape_rule():
    """Row-parallel shards that measured no faster packed in the fused all-reduce launch get no twin on an
    engine that runs it with that many rows (``ops.wpack.AR_STAYS_BF16``); elsewhere they are ordinary."""
    assert all(wpack.packable12_shape(*s) or wpack.packable12_tail_shape(*s) for s in wpack.AR_STAYS_BF16)
    assert wpack.ar_twin_wanted(8192, 7168, 2) and wpack.ar_twin_wanted(4096, 7168, 2)  # the down shards that won
    for (N, K), (rows, _, _) in wpack.AR_STAYS_BF16.items():
        assert not wpack.ar_twin_wanted(N, K, rows) and not wpack.ar_twin_wanted(N, K, 2)
        assert rows == 1 or wpack.ar_twin_wanted(N, K, rows - 1)
    # a rank whose o_proj shard is listed from two rows on: Llama-3-8B's shapes on 2 ranks, one layer
    cfg = ModelConfig("llama-8b-shapes-tp2-cpu-test", "llama", 1, 4096, 32, 2, 128, 1024, 512, 500000.0)
    w = TransformerWeights(cfg, TPGroup(None, 0, 2), torch.device("cpu"), seed=3)
    L = w.layers[0]
    assert tuple(L.w_o.shape) == (4096, 2048) and (4096, 2048) in wpack.AR_STAYS_BF16
    o_bytes = wpack.packed12_nbytes(4096, 2048)
    assert w.packed_demand() == w.packed_demand(fused_ar_rows=1) == w.packed_demand(fused_ar_rows=2) + o_bytes
    st = w.pack_decode_weights(fused_ar_rows=2)
    assert L.p_o is None and L.p_qkv is not None and st["bytes"] == w.packed_demand(fused_ar_rows=2)
