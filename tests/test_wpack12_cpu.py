"""The 12-bit packed decode weight format (``ops.wpack``, P12) on the CPU: the plain-torch packer
round-trips every bf16 bit pattern, the planes and the row records have the documented layout, the
exception lists are sorted, in range and zero-padded, the window has the fewest exceptions of its
candidates, and the raw fallback starts exactly above ``MAX_EXC`` exceptions."""

import pytest
import torch

from llm_consensus_amd.ops import wpack

E = wpack.MAX_EXC


def _bits(t):
    return t.contiguous().view(torch.int16)


def _gauss(N, K, std, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, K, generator=g) * std).to(torch.bfloat16)


def _flat(N, K, seed=0):
    """Rows whose exponents all sit in one 8-code window: values in [1, 2), random signs."""
    g = torch.Generator().manual_seed(seed)
    return ((1 + 0.9 * torch.rand(N, K, generator=g)) * (torch.randint(0, 2, (N, K), generator=g) * 2 - 1)).to(torch.bfloat16)


def _bf(bits):
    """The bf16 scalar with these 16 bits."""
    return torch.tensor([bits - (1 << 16) if bits & 0x8000 else bits], dtype=torch.int16).view(torch.bfloat16)[0]


def _hdr(pw):
    rec = pw.records().to(torch.int64) & 0xFFFFFFFF
    return rec[:, 0] & 0xFF, (rec[:, 0] >> 8) & 0xFF, rec[:, 1:]


@pytest.mark.parametrize("std", [0.02, 1.0])
@pytest.mark.parametrize("K", [2048, 6144])
def test_round_trip_gaussian(std, K):
    N = 96
    W = _gauss(N, K, std, seed=K + int(std * 100))
    pw = wpack.pack12_reference(W)
    assert isinstance(pw, wpack.PackedWeight12)
    assert pw.planes.shape == (N, K // 2048, 3072) and pw.planes.dtype == torch.uint8
    assert pw.hdr.shape == (N, 4 * (1 + E)) and pw.hdr.dtype == torch.uint8
    assert pw.nbytes() == wpack.packed12_nbytes(N, K) == pw.planes.numel() + pw.hdr.numel()
    assert wpack.packed12_nbytes(N, K) < wpack.packed_nbytes(N, K)
    assert pw.raw_rows == 0, "Gaussian rows: no raw rows at all"
    assert torch.equal(_bits(wpack.unpack12_reference(pw)), _bits(W))  # without W: nothing is raw


def test_gaussian_exception_counts_stay_far_inside_the_list():
    """The figures the format's E = 16 rests on: Gaussian rows (std 0.02) of the flagship model's two
    K leave at most a handful of weights outside the window."""
    for N, K, most in ((1024, 4096, 8), (512, 14336, 10)):
        pw = wpack.pack12_reference(_gauss(N, K, 0.02, seed=K))
        _, cnt, _ = _hdr(pw)
        assert pw.raw_rows == 0
        assert int(cnt.max()) <= most < E, int(cnt.max())
        assert pw.exceptions == int(cnt.sum())
        assert pw.exception_share < 2e-4


def test_shapes_off_the_unit_are_not_packed():
    for N, K in ((8, 2047), (8, 4096 + 512), (8, 1024), (4, 65536)):
        assert not wpack.packable12_shape(N, K)
        with pytest.raises(ValueError):
            wpack.pack12_reference(torch.zeros(N, K, dtype=torch.bfloat16))
    assert wpack.pack_best(torch.zeros(8, 1024, dtype=torch.bfloat16)) is None
    assert wpack.packable12_shape(4, 63488)


def test_special_rows_round_trip():
    K = 2048
    W = _flat(9, K, seed=5)
    W[0] = 0.0                                     # all-zero
    W[1, ::4] = 0.0                                # +-0.0 in half the row: more than E exceptions
    W[1, 1::4] = -0.0
    W[2, 7] = 0.0                                  # a zero, a -0.0 beside normal weights
    W[2, 2040] = -0.0
    W[3, 100] = _bf(0x0040)                        # denormals
    W[3, 101] = _bf(0x8001)
    W[4, 5] = _bf(0x1E80)                          # a tiny normal (about 1.4e-20)
    W[5, 9] = float("inf")
    W[6, 9] = float("-inf")
    W[7, 11] = float("nan")
    W[8] = _bf(0x0023)                             # a row of denormals only
    pw = wpack.pack12_reference(W)
    base, cnt, _ = _hdr(pw)
    assert torch.equal(_bits(wpack.unpack12_reference(pw, W)), _bits(W))
    # what took which path: all-zero / all-denormal rows sit in the window at base 0; a few zeros,
    # denormals or a tiny weight are exceptions; an inf / NaN beside small weights pulls the window up
    # and leaves the row raw
    assert base[0] == 0 and cnt[0] == 0 and base[8] == 0 and cnt[8] == 0
    assert base[1] == wpack.RAW
    assert (cnt[2], cnt[3], cnt[4]) == (2, 2, 1) and all(base[r] != wpack.RAW for r in (2, 3, 4))
    assert all(base[r] == wpack.RAW for r in (5, 6, 7))
    assert pw.raw_rows == 4
    # without W the non-raw rows still round-trip
    ok = base != wpack.RAW
    assert torch.equal(_bits(wpack.unpack12_reference(pw))[ok], _bits(W)[ok])


def test_exactly_E_is_packed_and_E_plus_one_is_raw():
    K = 4096
    W = _flat(3, K, seed=2)
    pos = torch.randperm(K, generator=torch.Generator().manual_seed(3))[:E + 1]
    W[0, pos[:E]] = 0.0
    W[1, pos] = 0.0
    W[2, pos[:1]] = 0.0
    pw = wpack.pack12_reference(W)
    base, cnt, slots = _hdr(pw)
    assert base[0] != wpack.RAW and cnt[0] == E
    assert base[1] == wpack.RAW and cnt[1] == 0 and int(slots[1].abs().sum()) == 0
    assert cnt[2] == 1
    assert pw.raw_rows == 1 and pw.exceptions == E + 1
    assert torch.equal(_bits(wpack.unpack12_reference(pw, W)), _bits(W))


def test_lists_are_sorted_in_range_and_zero_padded():
    N, K = 64, 6144
    W = _gauss(N, K, 0.02, seed=11)
    g = torch.Generator().manual_seed(12)
    for r in range(N):
        n = r % (E + 1)
        W[r, torch.randperm(K, generator=g)[:n]] = 0.0
    W[5, 0] = 0.0
    W[5, K - 1] = 0.0
    pw = wpack.pack12_reference(W)
    base, cnt, slots = _hdr(pw)
    bits = _bits(W).to(torch.int64) & 0xFFFF
    for r in range(N):
        c = int(cnt[r])
        if base[r] == wpack.RAW:
            assert c == 0 and int(slots[r].sum()) == 0
            continue
        k = slots[r, :c] & 0xFFFF
        assert torch.all(k[1:] > k[:-1]), "sorted by k, no duplicates"
        assert c == 0 or int(k.max()) < K
        assert torch.equal(slots[r, :c] >> 16, bits[r, k])
        assert int(slots[r, c:].abs().sum()) == 0, "unused slots are zero"
        hi7 = (bits[r] >> 8) & 0x7F
        out = (hi7 < base[r]) | (hi7 > base[r] + 7)
        assert torch.equal(out.nonzero().flatten(), k)
    assert int(cnt[5]) >= 2 and int(slots[5, 0] & 0xFFFF) == 0 and int(slots[5, int(cnt[5]) - 1] & 0xFFFF) == K - 1
    assert torch.equal(_bits(wpack.unpack12_reference(pw, W)), _bits(W))


def test_window_has_the_fewest_exceptions_and_ties_stay_on_top():
    K = 2048
    W = _flat(4, K, seed=4)        # exponent 127: e7..e1 = 63
    # row 0: three larger weights (e7..e1 = 65): the top window [58, 65] still holds the bulk
    W[0, :3] = 20.0
    # row 1: the bulk 2^-16 (e7..e1 = 55) and 3 weights at 1.0 (63): the top-anchored base 56 excludes
    # the whole bulk, one step down (55) only the three
    W[1] = W[1] * 2.0 ** -16
    W[1, :3] = 1.0
    # row 2: the same count on top and one below -> tie -> top. bulk at 63, one weight at 64 (2.0..4.0)
    # and one at 56: top base 57 excludes the 56, base 56 excludes the 64
    W[2, 0] = 3.0
    W[2, 1] = 2.0 ** -14
    # row 3: beyond the search: the bulk 6 codes below what the top window reaches -> raw
    W[3] = W[3] * 2.0 ** -40
    W[3, 0] = 1.0
    pw = wpack.pack12_reference(W)
    base, cnt, _ = _hdr(pw)
    bases, counts = wpack.window_candidates(W)
    assert bases.shape == (4, wpack.WINDOW_STEPS)
    assert torch.equal(bases[:, 0], torch.tensor([65 - 7, 63 - 7, 64 - 7, 63 - 7], dtype=torch.int32))
    for r in range(3):
        assert int(cnt[r]) == int(counts[r].min())
        first = int((counts[r] == counts[r].min()).nonzero()[0])
        assert int(base[r]) == int(bases[r, first]), "ties go to the candidate nearest the top"
    assert (int(base[0]), int(cnt[0])) == (58, 0)
    assert (int(base[1]), int(cnt[1])) == (55, 3)
    assert (int(base[2]), int(cnt[2])) == (57, 1) and int(counts[2, 1]) == 1
    assert int(base[3]) == wpack.RAW
    assert torch.equal(_bits(wpack.unpack12_reference(pw, W)), _bits(W))


def test_pack_best_prefers_p12_then_p13_then_none(monkeypatch):
    monkeypatch.delenv("LLMC_PACKED_FORMAT", raising=False)
    W = _gauss(200, 2048, 0.02, seed=21)
    assert isinstance(wpack.pack_best(W), wpack.PackedWeight12)
    assert isinstance(wpack.pack_best(W, fmt=13), wpack.PackedWeight)
    monkeypatch.setenv("LLMC_PACKED_FORMAT", "13")
    assert isinstance(wpack.pack_best(W), wpack.PackedWeight)
    monkeypatch.setenv("LLMC_PACKED_FORMAT", "11")
    with pytest.raises(ValueError):
        wpack.pack_best(W)
    monkeypatch.delenv("LLMC_PACKED_FORMAT")
    # 17 weights 20 codes below the rest in 2 % of the rows: raw under P12, inside P13's 16 codes
    W2 = _flat(200, 2048, seed=22)
    W2[:4, :E + 1] = 2.0 ** -20
    assert wpack.pack12_reference(W2).raw_rows == 4 > wpack.MAX_RAW_SHARE * 200
    pw = wpack.pack_best(W2)
    assert isinstance(pw, wpack.PackedWeight) and pw.raw_rows == 0
    W2[:4, :E + 1] = 0.0   # zeros: raw under both
    assert wpack.pack_best(W2) is None
    assert wpack.MAX_RAW_SHARE == 0.01
