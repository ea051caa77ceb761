"""Lossless 13-bit planes of a bf16 weight matrix for the decode GEMV (csrc/kernels/wpack.hip).

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
