"""Lossless 13-bit and 12-bit planes of a bf16 weight matrix for the decode GEMV
(csrc/kernels/wpack.hip). The 13-bit format (P13) first; the 12-bit one (P12) and ``pack_best``,
which chooses between them, further down.

A bf16 weight is ``s | e7..e0 | m6..m0``. Per row: the low byte as it is, a 4-bit code
``(e7..e1) - base`` (``base`` = the row's largest ``e7..e1`` minus 15, clamped at 0: one header
byte) and the sign bit, 13 bits per weight. A row with a weight below that 32-exponent window is
*raw* (header ``RAW``): the GEMV reads it from the bf16 tensor. The byte layout (one 3328-byte wave
unit per 2048 weights) is described in ``wpack.hip``; ``pack_reference`` is the same layout in
plain torch, ``unpack_reference`` its inverse.
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch

UNIT_ELEMS = 2048   # weights per wave unit: 64 lanes x 4 chunks x 8
UNIT_BYTES = 3328   # 2 x 1024 low bytes + 1024 nibbles + 256 signs
RAW = 0xFF
MAX_RAW_SHARE = 0.01  # a tensor with more raw rows than this stays bf16 only


class PackedWeight:
    """The packed twin of a bf16 ``[N, K]`` tensor: ``planes`` uint8 [N, K / 2048, 3328], ``hdr``
    uint8 [N rounded up to 4] (base or RAW per row), ``raw_rows`` their count."""

    __slots__ = ("planes", "hdr", "raw_rows", "N", "K")

    def __init__(self, planes: torch.Tensor, hdr: torch.Tensor, raw_rows: int, N: int, K: int):
        self.planes, self.hdr, self.raw_rows, self.N, self.K = planes, hdr, int(raw_rows), N, K

    @property
    def raw_share(self) -> float:
        return self.raw_rows / max(1, self.N)

    def nbytes(self) -> int:
        return self.planes.numel() + self.hdr.numel()


def packable_shape(N: int, K: int) -> bool:
    return N > 0 and K > 0 and K % UNIT_ELEMS == 0


def packed_nbytes(N: int, K: int) -> int:
    return N * (K // UNIT_ELEMS) * UNIT_BYTES + (N + 3) // 4 * 4


def _bits(W: torch.Tensor) -> torch.Tensor:
    if W.dtype != torch.bfloat16 or W.dim() != 2:
        raise TypeError("wpack: a bf16 [N, K] tensor")
    return W.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def row_headers(W: torch.Tensor) -> torch.Tensor:
    """uint8 [N]: the row's base, or RAW when a weight lies below the window."""
    hi7 = (_bits(W) >> 8) & 0x7F
    base = (hi7.max(dim=1).values - 15).clamp(min=0)
    raw = hi7.min(dim=1).values < base
    return torch.where(raw, torch.full_like(base, RAW), base).to(torch.uint8)


def _lane_order(t: torch.Tensor, U: int) -> torch.Tensor:
    """[N, K] -> [N, U, 64 lanes, 32]: weight t = 8 c + e of lane l in unit u is k index
    8 (l + 64 (4 u + c)) + e."""
    N = t.shape[0]
    return t.view(N, U, 4, 64, 8).permute(0, 1, 3, 2, 4).reshape(N, U, 64, 32)


def pack_reference(W: torch.Tensor) -> PackedWeight:
    """Plain-torch packer (any device). Raw rows' codes are taken against base 0 and masked to 4
    bits, as the HIP packer writes them."""
    N, K = W.shape
    if not packable_shape(N, K):
        raise ValueError(f"wpack: K = {K} is not a multiple of {UNIT_ELEMS}")
    U = K // UNIT_ELEMS
    bits = _bits(W)
    hdr = row_headers(W)
    base = torch.where(hdr == RAW, torch.zeros_like(hdr), hdr).to(torch.int32)
    b = _lane_order(bits, U)
    low = (b & 0xFF).to(torch.uint8)                                    # [N, U, 64, 32]
    code = (((b >> 8) & 0x7F) - base.view(N, 1, 1, 1)) & 0xF            # groups of 4: [.., c, h, j]
    code = code.view(N, U, 64, 4, 2, 4)
    nib = (code[..., 0, :] | (code[..., 1, :] << 4)).to(torch.uint8)    # [N, U, 64, 4 c, 4 j]
    sign = (b >> 15).view(N, U, 64, 8, 4)                               # [.., g, j]
    sbyte = (sign << torch.arange(8, device=W.device).view(1, 1, 1, 8, 1)).sum(dim=3).to(torch.uint8)  # [.., j]
    planes = torch.cat([low[..., :16].reshape(N, U, 1024), low[..., 16:].reshape(N, U, 1024),
                        nib.reshape(N, U, 1024), sbyte.reshape(N, U, 256)], dim=2).contiguous()
    hdr_pad = torch.zeros((N + 3) // 4 * 4, dtype=torch.uint8, device=W.device)
    hdr_pad[:N] = hdr
    return PackedWeight(planes, hdr_pad, int((hdr == RAW).sum()), N, K)


def unpack_reference(pw: PackedWeight, W: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The bf16 tensor back from its planes; raw rows come from ``W`` (the bf16 tensor the GEMV
    reads them from), or, without it, from the planes with base 0 (not the original bits)."""
    N, K = pw.N, pw.K
    U = K // UNIT_ELEMS
    p = pw.planes.view(N, U, UNIT_BYTES).to(torch.int32)
    hdr = pw.hdr[:N].to(torch.int32)
    base = torch.where(hdr == RAW, torch.zeros_like(hdr), hdr).view(N, 1, 1, 1)
    low = torch.cat([p[..., :1024].reshape(N, U, 64, 16), p[..., 1024:2048].reshape(N, U, 64, 16)], dim=3)
    nib = p[..., 2048:3072].reshape(N, U, 64, 4, 4)
    code = torch.stack([nib & 0xF, nib >> 4], dim=4).reshape(N, U, 64, 32)   # [.., c, h, j]
    sb = p[..., 3072:].reshape(N, U, 64, 1, 4)
    sign = ((sb >> torch.arange(8, device=p.device).view(1, 1, 1, 8, 1)) & 1).reshape(N, U, 64, 32)  # [.., g, j]
    b = (sign << 15) | ((code + base) << 8) | low                            # [N, U, 64 l, 32 = (c, e)]
    bits = b.view(N, U, 64, 4, 8).permute(0, 1, 3, 2, 4).reshape(N, K)
    out = (bits - ((bits & 0x8000) << 1)).to(torch.int16).view(torch.bfloat16)
    if W is not None:
        rows = hdr == RAW
        out[rows] = W[rows].to(out.device)
    return out


def pack(W: torch.Tensor) -> PackedWeight:
    """Pack ``W`` where it lives: the HIP packer on the GPU, ``pack_reference`` on the CPU."""
    if not W.is_cuda:
        return pack_reference(W)
    from ..utils.native import kernels

    N, K = W.shape
    if W.dtype != torch.bfloat16 or not packable_shape(N, K):
        raise ValueError(f"wpack: bf16 [N, K] with K a multiple of {UNIT_ELEMS}, got {W.dtype} {tuple(W.shape)}")
    W = W.contiguous()
    planes = torch.empty(N, K // UNIT_ELEMS, UNIT_BYTES, dtype=torch.uint8, device=W.device)
    hdr = torch.zeros((N + 3) // 4 * 4, dtype=torch.uint8, device=W.device)
    raw = torch.zeros(1, dtype=torch.int32, device=W.device)
    kernels().wpack13(W.data_ptr(), planes.data_ptr(), hdr.data_ptr(), raw.data_ptr(), N, K,
                      torch.cuda.current_stream(W.device).cuda_stream)
    return PackedWeight(planes, hdr, int(raw.item()), N, K)


def pack_if_worthwhile(W: torch.Tensor) -> Tuple[Optional[PackedWeight], float]:
    """(twin or None, share of raw rows): None when the shape is off the unit size or more than
    MAX_RAW_SHARE of the rows are raw."""
    if W.dim() != 2 or not packable_shape(*W.shape):
        return None, 0.0
    pw = pack(W)
    return (pw if pw.raw_share <= MAX_RAW_SHARE else None), pw.raw_share


# ---- P12: 12 bits per weight, the row's few out-of-window weights patched from a list ----
#
# Per weight the low byte and a nibble ``s << 3 | k``, ``k = (e7..e1) - base`` in 3 bits: a window of
# 16 exponents. The unit is P13's without the sign plane (3072 bytes, same lane / chunk / element
# order). A weight outside the window is an *exception*: its code is written masked and its bits go
# to the row's record of ``REC12_DWORDS`` int32: ``[0] = base | count << 8`` (or ``RAW``, count 0,
# for a row with more than ``MAX_EXC`` exceptions, which the GEMV reads from the bf16 tensor), then
# ``MAX_EXC`` slots ``bits << 16 | k`` sorted by k, the unused ones zero. The window is the
# top-anchored one (``base = max(0, largest e7..e1 - 7)``) or up to ``WINDOW_STEPS - 1`` below it where
# that leaves fewer exceptions; ties stay with the higher base.

UNIT12_BYTES = 3072
MAX_EXC = 16
REC12_DWORDS = 1 + MAX_EXC
WINDOW_STEPS = 4
MAX_K12 = 65536 - UNIT_ELEMS  # positions are 16 bits; the reader's end mark is wave chunk 127


class PackedWeight12:
    """The 12-bit twin of a bf16 ``[N, K]`` tensor: ``planes`` uint8 [N, K / 2048, 3072], ``hdr``
    uint8 [N, 68] (the rows' records), ``raw_rows`` and ``exceptions`` (of the packed rows) counts."""

    __slots__ = ("planes", "hdr", "raw_rows", "exceptions", "N", "K")

    def __init__(self, planes: torch.Tensor, hdr: torch.Tensor, raw_rows: int, exceptions: int, N: int, K: int):
        self.planes, self.hdr, self.raw_rows, self.exceptions, self.N, self.K = \
            planes, hdr, int(raw_rows), int(exceptions), N, K

    @property
    def raw_share(self) -> float:
        return self.raw_rows / max(1, self.N)

    @property
    def exception_share(self) -> float:
        return self.exceptions / max(1, self.N * self.K)

    def records(self) -> torch.Tensor:
        """int32 [N, 17] view of ``hdr``."""
        return self.hdr.view(torch.int32).view(self.N, REC12_DWORDS)

    def nbytes(self) -> int:
        return self.planes.numel() + self.hdr.numel()


def packable12_shape(N: int, K: int) -> bool:
    return packable_shape(N, K) and K <= MAX_K12


def packed12_nbytes(N: int, K: int) -> int:
    return N * (K // UNIT_ELEMS) * UNIT12_BYTES + N * REC12_DWORDS * 4


def window_candidates(W: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(bases int32 [N, WINDOW_STEPS], exception counts int32 [N, WINDOW_STEPS]) of every row, the
    top-anchored base first."""
    hi7 = (_bits(W) >> 8) & 0x7F
    top = hi7.max(dim=1).values - 7
    bases = torch.stack([(top - d).clamp(min=0) for d in range(WINDOW_STEPS)], dim=1)
    counts = torch.stack([((hi7 < bases[:, d:d + 1]) | (hi7 > bases[:, d:d + 1] + 7)).sum(dim=1)
                          for d in range(WINDOW_STEPS)], dim=1)
    return bases.to(torch.int32), counts.to(torch.int32)


def pack12_reference(W: torch.Tensor) -> PackedWeight12:
    """Plain-torch P12 packer (any device), byte for byte what the HIP packer writes."""
    N, K = W.shape
    if not packable12_shape(N, K):
        raise ValueError(f"wpack12: K = {K} is not a multiple of {UNIT_ELEMS} up to {MAX_K12}")
    U = K // UNIT_ELEMS
    bits = _bits(W)
    hi7 = (bits >> 8) & 0x7F
    bases, counts = window_candidates(W)
    base, cnt = bases[:, 0].clone(), counts[:, 0].clone()
    for d in range(1, WINDOW_STEPS):  # strictly fewer only: ties stay with the higher base
        better = counts[:, d] < cnt
        base = torch.where(better, bases[:, d], base)
        cnt = torch.where(better, counts[:, d], cnt)
    raw = cnt > MAX_EXC
    rec = torch.zeros(N, REC12_DWORDS, dtype=torch.int64, device=W.device)
    rec[:, 0] = torch.where(raw, torch.full_like(cnt, RAW), base | (cnt << 8))
    exc = ((hi7 < base.view(N, 1)) | (hi7 > base.view(N, 1) + 7)) & ~raw.view(N, 1)
    rows, ks = exc.nonzero(as_tuple=True)                  # row-major: sorted by k within a row
    if rows.numel():
        first = torch.zeros(N + 1, dtype=torch.int64, device=W.device)
        first[1:] = exc.sum(dim=1).cumsum(0)
        rank = torch.arange(rows.numel(), device=W.device) - first[rows]
        rec[rows, 1 + rank] = (bits[rows, ks].to(torch.int64) << 16) | ks
    rec = (rec - ((rec & 0x80000000) << 1)).to(torch.int32)  # the dword's bits as int32
    pbase = torch.where(raw, torch.zeros_like(base), base)
    b = _lane_order(bits, U)
    low = (b & 0xFF).to(torch.uint8)
    code = ((((b >> 8) & 0x7F) - pbase.view(N, 1, 1, 1)) & 0x7) | ((b >> 15) << 3)
    code = code.view(N, U, 64, 4, 2, 4)
    nib = (code[..., 0, :] | (code[..., 1, :] << 4)).to(torch.uint8)
    planes = torch.cat([low[..., :16].reshape(N, U, 1024), low[..., 16:].reshape(N, U, 1024),
                        nib.reshape(N, U, 1024)], dim=2).contiguous()
    hdr = rec.contiguous().view(torch.uint8).view(N, REC12_DWORDS * 4)
    return PackedWeight12(planes, hdr, int(raw.sum()), int(cnt[~raw].sum()), N, K)


def unpack12_reference(pw: PackedWeight12, W: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The bf16 tensor back from the planes and the records; raw rows come from ``W`` (or, without
    it, from the planes with base 0: not the original bits)."""
    N, K = pw.N, pw.K
    U = K // UNIT_ELEMS
    p = pw.planes.view(N, U, UNIT12_BYTES).to(torch.int32)
    rec = pw.records().to(torch.int64) & 0xFFFFFFFF
    hb = rec[:, 0] & 0xFF
    raw = hb == RAW
    base = torch.where(raw, torch.zeros_like(hb), hb).view(N, 1, 1, 1).to(torch.int32)
    low = torch.cat([p[..., :1024].reshape(N, U, 64, 16), p[..., 1024:2048].reshape(N, U, 64, 16)], dim=3)
    nib = p[..., 2048:].reshape(N, U, 64, 4, 4)
    code = torch.stack([nib & 0xF, nib >> 4], dim=4).reshape(N, U, 64, 32)
    b = ((code >> 3) << 15) | (((code & 7) + base) << 8) | low
    bits = b.view(N, U, 64, 4, 8).permute(0, 1, 3, 2, 4).reshape(N, K).contiguous()
    cnt = torch.where(raw, torch.zeros_like(hb), (rec[:, 0] >> 8) & 0xFF)
    live = torch.arange(MAX_EXC, device=rec.device).view(1, MAX_EXC) < cnt.view(N, 1)
    rows, slot = live.nonzero(as_tuple=True)
    ent = rec[rows, 1 + slot]
    bits[rows, ent & 0xFFFF] = (ent >> 16).to(torch.int32)
    out = (bits - ((bits & 0x8000) << 1)).to(torch.int16).view(torch.bfloat16)
    if W is not None:
        out[raw] = W[raw].to(out.device)
    return out


def pack12(W: torch.Tensor) -> PackedWeight12:
    """P12-pack ``W`` where it lives: the HIP packer on the GPU, ``pack12_reference`` on the CPU."""
    if not W.is_cuda:
        return pack12_reference(W)
    from ..utils.native import kernels

    N, K = W.shape
    if W.dtype != torch.bfloat16 or not packable12_shape(N, K):
        raise ValueError(f"wpack12: bf16 [N, K] with K a multiple of {UNIT_ELEMS} up to {MAX_K12}, "
                         f"got {W.dtype} {tuple(W.shape)}")
    W = W.contiguous()
    planes = torch.empty(N, K // UNIT_ELEMS, UNIT12_BYTES, dtype=torch.uint8, device=W.device)
    hdr = torch.empty(N, REC12_DWORDS * 4, dtype=torch.uint8, device=W.device)
    counts = torch.zeros(2, dtype=torch.int32, device=W.device)
    kernels().wpack12(W.data_ptr(), planes.data_ptr(), hdr.data_ptr(), counts.data_ptr(), N, K,
                      torch.cuda.current_stream(W.device).cuda_stream)
    raw_rows, exceptions = counts.tolist()
    return PackedWeight12(planes, hdr, raw_rows, exceptions, N, K)


def packed_format() -> int:
    """12 or 13: the format ``pack_best`` tries first (``LLMC_PACKED_FORMAT``, A/B runs)."""
    from ..parallel.placement import packed_format as fmt

    return fmt()


def pack_best(W: torch.Tensor, fmt: Optional[int] = None):
    """The P12 twin of ``W``; where more than MAX_RAW_SHARE of its rows would be raw (or the shape
    is off P12's), the P13 twin; where that fails too, None. ``fmt`` 13 skips P12."""
    if W.dim() != 2 or not packable_shape(*W.shape):
        return None
    if (packed_format() if fmt is None else fmt) == 12 and packable12_shape(*W.shape):
        pw12 = pack12(W)
        if pw12.raw_share <= MAX_RAW_SHARE:
            return pw12
    pw = pack(W)
    return pw if pw.raw_share <= MAX_RAW_SHARE else None
