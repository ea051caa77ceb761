"""The 13-bit packed weight format (ops.wpack): the plain-torch reference packer and its inverse.

Pack then unpack must give back the int16 bits of every packable row; a row is raw exactly when a
weight lies below the 32-exponent window under the row's largest exponent; codes are 4 bits.
"""

import pytest
import torch

from llm_consensus_amd.ops import wpack


def _bits(t):
    return t.contiguous().view(torch.int16)


def _gauss(N, K, std, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, K, generator=g) * std).to(torch.bfloat16)


def _codes(pw):
    nib = pw.planes[..., 2048:3072].to(torch.int32)
    return torch.stack([nib & 0xF, nib >> 4])


def _window_violated(W):
    """The format's rule, written out per row with Python ints (independent of row_headers)."""
    hi7 = ((_bits(W).to(torch.int32) & 0xFFFF) >> 8) & 0x7F
    out = []
    for r in hi7.tolist():
        base = max(max(r) - 15, 0)
        out.append(min(r) < base)
    return torch.tensor(out)


@pytest.mark.parametrize("K", [2048, 6144])
@pytest.mark.parametrize("std", [0.02, 1.0])
def test_gaussian_rows_round_trip(K, std):
    W = _gauss(192, K, std, seed=K + int(std * 100))
    pw = wpack.pack_reference(W)
    assert pw.planes.shape == (192, K // 2048, 3328) and pw.planes.dtype == torch.uint8
    assert pw.planes.numel() * 8 == W.numel() * 13  # 13 bits per weight
    raw = pw.hdr[:192] == wpack.RAW
    assert torch.equal(raw, _window_violated(W))
    assert pw.raw_rows == int(raw.sum())
    assert pw.raw_share <= wpack.MAX_RAW_SHARE, f"raw share {pw.raw_share}"
    c = _codes(pw)
    assert int(c.min()) >= 0 and int(c.max()) <= 15
    # without the bf16 tensor: every packable row exactly; with it: every row
    back = wpack.unpack_reference(pw)
    assert torch.equal(_bits(back)[~raw], _bits(W)[~raw])
    assert torch.equal(_bits(wpack.unpack_reference(pw, W)), _bits(W))


def test_gaussian_raw_share_is_small():
    """The init's own weights: rows of K = 4096 at std 1/sqrt(K); the share of raw rows stays well
    under the 1 % cap (a raw row needs |w| < 2^-30 of the row's largest or an exact zero)."""
    W = _gauss(2048, 4096, 4096 ** -0.5, seed=7)
    pw = wpack.pack_reference(W)
    assert pw.raw_share <= wpack.MAX_RAW_SHARE
    assert torch.equal(_bits(wpack.unpack_reference(pw, W)), _bits(W))


def _special_rows():
    """[9, 2048] and the expected raw flags."""
    W = _gauss(9, 2048, 0.02, seed=3)
    one = torch.tensor(1.0)
    W[0] = 0.0                                   # all zero: base 0, code 0 -> packable
    W[1, 77] = 0.0                               # one zero beside normal weights -> raw
    W[2, 5] = float("inf")                       # inf beside normal weights -> raw
    W[3, 2047] = float("nan")                    # NaN -> raw
    W[4, 0] = torch.tensor(1e-40).to(torch.bfloat16)  # a denormal -> raw
    # exponents 2 b .. 2 b + 31 (16 values of e7..e1): packable; one more below: raw
    e = torch.arange(2048) % 32
    W[5] = (one * 2.0) ** (e - 20).float()       # biased exponents 107..138: e7..e1 = 53..69 -> 17 values
    W[6] = (one * 2.0) ** (e - 21).float()       # biased 106..137: e7..e1 = 53..68 -> 16 values
    W[7] = -W[6]                                 # the same, negative
    W[7, 0] = W[7, 0] * 2.0 ** -2                # the smallest, 106 -> 104: e7..e1 = 52, 17 values
    W[8] = W[6]
    W[8, 9] = W[8, 9] * 1.5                      # mantissa bits inside the window: still packable
    return W, torch.tensor([False, True, True, True, True, True, False, True, False])


def test_special_rows():
    W, want_raw = _special_rows()
    bits = (_bits(W).to(torch.int32) & 0xFFFF)
    e = (bits >> 7) & 0xFF
    assert int(e[6].max() - e[6].min()) == 31 and int(e[6].min()) % 2 == 0   # exactly 32 exponents, aligned
    assert int(e[5].max() - e[5].min()) == 31 and int(e[5].min()) % 2 == 1   # 32 exponents over 17 codes
    assert int(e[7].max() - e[7].min()) >= 32                                # 33 or more
    pw = wpack.pack_reference(W)
    raw = pw.hdr[:9] == wpack.RAW
    assert torch.equal(raw, want_raw)
    assert torch.equal(raw, _window_violated(W))
    assert pw.raw_rows == int(want_raw.sum())
    assert int(pw.hdr[0]) == 0                       # the all-zero row
    c = _codes(pw)
    assert int(c.min()) >= 0 and int(c.max()) <= 15
    back = wpack.unpack_reference(pw)
    assert torch.equal(_bits(back)[~raw], _bits(W)[~raw])
    full = wpack.unpack_reference(pw, W)
    assert torch.equal(_bits(full), _bits(W))        # NaN payloads included: compared as bits


def test_thirty_three_exponents_is_raw():
    W = torch.ones(2, 2048, dtype=torch.bfloat16)
    W[0, 1] = 2.0 ** -31     # biased 127 and 96: e7..e1 63 and 48 -> 16 values, packable
    W[1, 1] = 2.0 ** -32     # 127 and 95: e7..e1 63 and 47 -> raw
    pw = wpack.pack_reference(W)
    assert pw.hdr[:2].tolist() == [48, wpack.RAW]
    assert torch.equal(_bits(wpack.unpack_reference(pw))[0], _bits(W)[0])


def test_shapes_off_the_unit_are_not_packed():
    assert not wpack.packable_shape(64, 256) and wpack.packable_shape(64, 14336)
    pw, share = wpack.pack_if_worthwhile(torch.zeros(8, 256, dtype=torch.bfloat16))
    assert pw is None and share == 0.0
    with pytest.raises(ValueError):
        wpack.pack_reference(torch.zeros(8, 1024, dtype=torch.bfloat16))
    # more than 1 % raw rows: the tensor stays bf16 only, the share is still reported
    W = _gauss(50, 2048, 0.02, seed=1)
    W[:2, 0] = 0.0
    pw, share = wpack.pack_if_worthwhile(W)
    assert pw is None and share == pytest.approx(0.04)
    assert wpack.packed_nbytes(6, 4096) == 6 * 2 * 3328 + 8
