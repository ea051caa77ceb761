"""The 12-bit packed decode weight format with a row tail (``ops.wpack``, "P12 with a tail") on the
CPU: for a K that is a multiple of 512 off the 2048-weight unit the plain-torch packer round-trips
every bf16 bit, the planes have the documented row stride, exceptions in the tail are ordinary record
entries at their k, the raw fallback starts above ``MAX_EXC`` as without a tail, and ``pack_best``
and ``packed_demand`` take the tail shapes in under the 12-bit format only."""

import pytest
import torch

from llm_consensus_amd.models.config import ModelConfig
from llm_consensus_amd.models.transformer import TransformerWeights
from llm_consensus_amd.ops import wpack
from llm_consensus_amd.parallel.comm import TPGroup

E = wpack.MAX_EXC
TINY = [0.0, -0.0, 1e-30, -3e-33]  # far below any 16-exponent window of weights near 1


def _bits(t):
    return t.contiguous().view(torch.int16)


def _gauss(N, K, std, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, K, generator=g) * std).to(torch.bfloat16)


def _flat(N, K, seed=0):
    """Rows whose exponents all sit in one 8-code window: values in [1, 2), random signs."""
    g = torch.Generator().manual_seed(seed)
    return ((1 + 0.9 * torch.rand(N, K, generator=g)) * (torch.randint(0, 2, (N, K), generator=g) * 2 - 1)).to(torch.bfloat16)


def _hdr(pw):
    rec = pw.records().to(torch.int64) & 0xFFFFFFFF
    return rec[:, 0] & 0xFF, (rec[:, 0] >> 8) & 0xFF, rec[:, 1:]


@pytest.mark.parametrize("std", [0.02, 1.0])
@pytest.mark.parametrize("K", [2560, 3072, 3584, 6656, 18944])
def test_round_trip_gaussian(std, K):
    N = 48
    U, Q = K // 2048, K % 2048 // 512
    W = _gauss(N, K, std, seed=K + int(std * 100))
    pw = wpack.pack12_tail_reference(W)
    assert isinstance(pw, wpack.PackedWeight12Tail) and isinstance(pw, wpack.PackedWeight12)
    assert pw.planes.shape == (N, U * 3072 + Q * 768) and pw.planes.dtype == torch.uint8
    assert pw.planes.shape[1] % 256 == 0
    assert pw.hdr.shape == (N, 4 * (1 + E)) and pw.hdr.dtype == torch.uint8
    assert pw.nbytes() == wpack.packed12_tail_nbytes(N, K) == N * (U * 3072 + Q * 768 + 68)
    base, cnt, _ = _hdr(pw)
    print(f"K {K} std {std}: most exceptions in a row {int(cnt.max())}, share {pw.exception_share:.2e}")
    assert pw.raw_rows == 0 and int(cnt.max()) <= 12
    assert pw.exceptions == int(cnt.sum())
    assert torch.equal(_bits(wpack.unpack12_tail_reference(pw)), _bits(W))  # without W: nothing is raw


def test_the_whole_units_of_a_tail_row_are_the_unit_format():
    """The first U units of every row are byte for byte the planes of the same weights packed without
    a tail (one flat window: the base does not depend on the columns), and the tail is the unit cut
    short: a lane's low bytes of chunks 0 and 1 (block A), of chunk 2 (block B), its nibble dwords."""
    N = 6
    for Q in (1, 2, 3):
        K = 4096 + 512 * Q
        W = _flat(N, K, seed=4 + Q)
        pw = wpack.pack12_tail_reference(W)
        head = wpack.pack12_reference(W[:, :4096].contiguous())
        assert torch.equal(pw.planes[:, :2 * 3072], head.planes.reshape(N, 2 * 3072))
        tail = pw.planes[:, 2 * 3072:]
        assert tail.shape[1] == Q * 768
        base, _, _ = _hdr(pw)
        b = _bits(W).to(torch.int32) & 0xFFFF
        for r, c, lane in ((0, 0, 0), (1, Q - 1, 17), (5, Q // 2, 63)):
            k = 4096 + 512 * c + 8 * lane
            low = [int(b[r, k + e]) & 0xFF for e in range(8)]
            at = 1024 + 8 * lane if c == 2 else (8 if Q == 1 else 16) * lane + 8 * c
            assert tail[r, at:at + 8].tolist() == low
            # byte j of the lane's nibble dword c: code(e = j) | code(e = j + 4) << 4, sign in the code's top bit
            code = [((((int(b[r, k + e]) >> 8) & 0x7F) - int(base[r])) & 7) | (int(b[r, k + e]) >> 15) << 3 for e in range(8)]
            nib = tail[r, Q * 512 + 4 * (Q * lane + c):Q * 512 + 4 * (Q * lane + c) + 4].tolist()
            assert nib == [code[j] | code[j + 4] << 4 for j in range(4)]


@pytest.mark.parametrize("K", [2560, 3584, 6656])
def test_planted_exceptions_are_record_entries_at_their_k(K):
    U = K // 2048
    T = 2048 * U  # the first tail weight
    plan = {
        0: [T],                                        # the first tail weight
        1: [K - 1],                                    # the last weight
        2: [T + 8 * 3 + 2, T + 8 * 40 + 7],            # two in one tail chunk, different lanes
        3: [T + 8 * 5 + 1, T + 8 * 5 + 6],             # two in one lane's 8 weights
        4: [T - 512 + 8 * 10, T + 8 * 10 + 3],         # chunk 3 of the last whole unit and tail chunk 0
        5: [0, T, K - 1],
    }
    W = _flat(8, K, seed=K)
    for r, ks in plan.items():
        for i, k in enumerate(ks):
            W[r, k] = TINY[i % 4]
    pw = wpack.pack12_tail_reference(W)
    base, cnt, slots = _hdr(pw)
    wb = _bits(W).to(torch.int64) & 0xFFFF
    for r, ks in plan.items():
        assert base[r] != wpack.RAW and int(cnt[r]) == len(ks)
        ent = slots[r, :len(ks)]
        assert (ent & 0xFFFF).tolist() == sorted(ks)
        assert (ent >> 16).tolist() == [int(wb[r, k]) for k in sorted(ks)]
        assert int(slots[r, len(ks):].abs().sum()) == 0
    assert [int(k) >> 9 for k in (slots[4, :2] & 0xFFFF)] == [4 * U - 1, 4 * U]  # consecutive wave chunks
    assert int(cnt[6]) == 0 and int(cnt[7]) == 0
    assert pw.raw_rows == 0 and pw.exceptions == sum(len(ks) for ks in plan.values())
    assert torch.equal(_bits(wpack.unpack12_tail_reference(pw)), _bits(W))


def test_exactly_E_is_packed_and_E_plus_one_is_raw():
    K = 3584
    W = _flat(3, K, seed=2)
    pos = torch.cat([torch.arange(0, 9) * 200 + 1, 2048 + torch.arange(0, 8) * 190 + 5])  # 9 in the unit, 8 in the tail
    assert pos.numel() == E + 1 and int((pos >= 2048).sum()) == 8 and int(pos.max()) < K
    W[0, pos[1:]] = 0.0   # E: one in the unit fewer
    W[1, pos] = 0.0       # E + 1
    W[2, pos[-1:]] = 0.0
    pw = wpack.pack12_tail_reference(W)
    base, cnt, slots = _hdr(pw)
    assert base[0] != wpack.RAW and cnt[0] == E
    assert (slots[0, :E] & 0xFFFF).tolist() == pos[1:].tolist()
    assert base[1] == wpack.RAW and cnt[1] == 0 and int(slots[1].abs().sum()) == 0
    assert cnt[2] == 1
    assert pw.raw_rows == 1 and pw.exceptions == E + 1
    assert torch.equal(_bits(wpack.unpack12_tail_reference(pw, W)), _bits(W))
    ok = base != wpack.RAW
    assert torch.equal(_bits(wpack.unpack12_tail_reference(pw))[ok], _bits(W)[ok])


def test_shape_rules():
    for N, K in ((8, 2560), (4, 63488 - 512), (8, 18944)):
        assert wpack.packable12_tail_shape(N, K)
    for N, K in ((8, 1024), (8, 2048), (8, 4096), (8, 2048 + 256), (4, 65536 - 512)):
        assert not wpack.packable12_tail_shape(N, K)
        with pytest.raises(ValueError):
            wpack.pack12_tail_reference(torch.zeros(N, K, dtype=torch.bfloat16))
    # the names without a tail keep their rules
    assert not wpack.packable12_shape(8, 4608) and not wpack.packable_shape(8, 2560)
    with pytest.raises(ValueError):
        wpack.pack12_reference(torch.zeros(8, 4608, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        wpack.pack12(torch.zeros(8, 1024, dtype=torch.bfloat16))
    assert wpack.packed12_tail_nbytes(8, 2560) == 8 * (3072 + 768 + 68)


def test_pack_best(monkeypatch):
    monkeypatch.delenv("LLMC_PACKED_FORMAT", raising=False)
    W = _gauss(64, 2560, 0.02, seed=1)
    pw = wpack.pack_best(W)
    assert type(pw) is wpack.PackedWeight12Tail and pw.raw_rows == 0
    assert torch.equal(_bits(wpack.unpack12_tail_reference(pw)), _bits(W))
    assert type(wpack.pack_best(_gauss(64, 4096, 0.02, seed=2))) is wpack.PackedWeight12  # not the subclass
    assert wpack.pack_best(torch.zeros(8, 1024, dtype=torch.bfloat16)) is None
    assert wpack.pack_best(torch.zeros(8, 2304, dtype=torch.bfloat16)) is None
    # the 13-bit format has no tail, and a tail shape has no 13-bit fallback
    assert wpack.pack_best(W, fmt=13) is None
    monkeypatch.setenv("LLMC_PACKED_FORMAT", "13")
    assert wpack.pack_best(W) is None
    monkeypatch.delenv("LLMC_PACKED_FORMAT")
    # more than 1 % raw rows: no twin (2 of 100 rows with E + 1 zeros, some of them in the tail)
    W2 = _flat(100, 2560, seed=3)
    W2[:2, 1500:2500:50] = 0.0
    assert int((W2[0] == 0).sum()) == 20 > E
    assert wpack.pack12_tail_reference(W2).raw_rows == 2 > wpack.MAX_RAW_SHARE * 100
    assert wpack.pack_best(W2) is None
    W2[1] = W2[2]
    assert type(wpack.pack_best(W2)) is wpack.PackedWeight12Tail  # 1 of 100 is within the share


# hidden 2560 (qkv, gate_up, lm_head and, with 20 heads x 128, o_proj), intermediate 3584 (down)
LLAMA_TAIL = ModelConfig("llama-tail-test", "llama", 2, 2560, 20, 10, 128, 3584, 2048, 500000.0, max_position=4096)


def test_packed_demand_counts_the_tail_twins(monkeypatch):
    monkeypatch.delenv("LLMC_PACKED_FORMAT", raising=False)
    w = TransformerWeights(LLAMA_TAIL, TPGroup.single(), torch.device("cpu"), seed=3)
    need = w.packed_demand()
    assert need == (wpack.packed12_tail_nbytes(2048, 2560)
                    + 2 * (wpack.packed12_tail_nbytes(5120, 2560) + wpack.packed12_tail_nbytes(2560, 2560)
                           + wpack.packed12_tail_nbytes(7168, 2560) + wpack.packed12_tail_nbytes(2560, 3584)))
    assert w.packed_demand(with_o=False) == need - 2 * wpack.packed12_tail_nbytes(2560, 2560)
    st = w.pack_decode_weights()  # CPU tensors: the reference packer
    assert st["tensors"] == st["packed"] == st["p12"] == st["tail"] == 9 and st["p13"] == 0
    assert st["bytes"] == w.packed_nbytes() == need
    assert isinstance(w.p_lm_head, wpack.PackedWeight12Tail)
    assert all(isinstance(getattr(L, s), wpack.PackedWeight12Tail) for L in w.layers for s in L.PACKED)
    monkeypatch.setenv("LLMC_PACKED_FORMAT", "13")
    assert w.packed_demand() == 0
