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
    bits, rec, raw, cnt, pbase = _records12(W)
    b = _lane_order(bits, U)
    low = (b & 0xFF).to(torch.uint8)
    code = ((((b >> 8) & 0x7F) - pbase.view(N, 1, 1, 1)) & 0x7) | ((b >> 15) << 3)
    code = code.view(N, U, 64, 4, 2, 4)
    nib = (code[..., 0, :] | (code[..., 1, :] << 4)).to(torch.uint8)
    planes = torch.cat([low[..., :16].reshape(N, U, 1024), low[..., 16:].reshape(N, U, 1024),
                        nib.reshape(N, U, 1024)], dim=2).contiguous()
    return PackedWeight12(planes, _rec_bytes(rec), int(raw.sum()), int(cnt[~raw].sum()), N, K)


def _rec_bytes(rec: torch.Tensor) -> torch.Tensor:
    return rec.contiguous().view(torch.uint8).view(rec.shape[0], REC12_DWORDS * 4)


def _records12(W: torch.Tensor):
    """(bits int32 [N, K], records int32 [N, 17], raw bool [N], exception counts [N], the base the
    planes' codes are taken against [N]) of ``W``'s rows, for any K."""
    N, K = W.shape
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
    return bits, rec, raw, cnt, pbase


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
    return _patched12(pw, bits, W)


def _patched12(pw: PackedWeight12, bits: torch.Tensor, W: Optional[torch.Tensor]) -> torch.Tensor:
    """``bits`` (int32 [N, K], decoded from the planes) with the records' exceptions written in, as
    bf16; raw rows from ``W``."""
    N = pw.N
    rec = pw.records().to(torch.int64) & 0xFFFFFFFF
    hb = rec[:, 0] & 0xFF
    raw = hb == RAW
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


# ---- P12 with a tail: K a multiple of 512 off the 2048-weight unit ----
#
# 512 weights are one wave chunk (64 lanes x 8), the granule of the GEMV's loop and of an exception's
# position, so a row may end in Q = (K / 512) % 4 = 1..3 chunks after its U = K // 2048 >= 1 whole units:
# the unit cut short, a lane's share of each plane contiguous (``wpack.hip``): ``A``, the lanes' low bytes
# of chunks 0 and 1 (8 or 16 per lane); for ``Q`` = 3 ``B``, those of chunk 2 (8 per lane); and at ``Q *
# 512`` the lanes' ``Q`` nibble dwords (byte j of dword c: ``code[e = j] | code[e = j + 4] << 4``, the
# unit's convention); the row stride is ``U * 3072 + Q * 768``. Records as above, the base chosen over the
# whole row.

CHUNK_ELEMS = 512        # weights per wave chunk
TAIL_CHUNK_BYTES = 768   # 512 low bytes + 256 nibble bytes


class PackedWeight12Tail(PackedWeight12):
    """The 12-bit twin of a bf16 ``[N, K]`` tensor with K off the 2048-weight unit: ``planes`` uint8
    [N, U * 3072 + Q * 768], every row its whole units and then its tail; the rest as the base class."""

    __slots__ = ()


def packable12_tail_shape(N: int, K: int) -> bool:
    return N > 0 and K % CHUNK_ELEMS == 0 and K % UNIT_ELEMS != 0 and UNIT_ELEMS < K <= MAX_K12


# The per-shape choice (profiles/r11_packed_tail.md section 1): catalog shapes on which the tail GEMV,
# cold and alone, was not faster than the bf16 GEMV by more than the spread of the two runs. They keep
# streaming bf16: ``pack_best`` builds no twin and ``tail_twin_wanted`` is what ``packed_demand`` asks.
# (N, K): tail time / bf16 time, spread
TAIL_STAYS_BF16 = {
    (3584, 3584): (0.972, 0.032),   # Qwen2.5-7B o_proj: 6.04 against 6.21 us
    (9216, 3072): (1.016, 0.014),   # Phi-3-mini qkv: 12.05 against 11.87 us
    (3072, 3072): (1.033, 0.046),   # Phi-3-mini o_proj: 5.25 against 5.08 us
    (16384, 3072): (1.095, 0.027),  # Phi-3-mini gate_up: 18.93 against 17.28 us
}


def tail_twin_wanted(N: int, K: int) -> bool:
    """A tail shape that ``pack_best`` packs: every one but the measured losers above."""
    return packable12_tail_shape(N, K) and (N, K) not in TAIL_STAYS_BF16


# The same choice for a TP rank's row-parallel shards (o_proj, down_proj) in the launch with the all-reduce
# in its epilogue (csrc/kernels/gemv_ar_p12.hip): shard shapes on which the packed launch, cold, two ranks
# each on half of the CUs (scripts/ar_packed_launch.py; profiles/r13_packed_tp.md section 3), was not
# faster than the bf16 launch by more than the spread of the runs. Such a shard gets no twin on an engine
# that runs the fused launch with that many decode rows; with separate all-reduce launches it is an
# ordinary GEMV and the rules above apply.
# (N, K): (fewest decode rows from which it stays bf16, packed / bf16 time at one row, at two rows)
AR_STAYS_BF16 = {
    (8192, 3584): (1, 1.051, 1.076),  # Llama-3-70B down on 8 ranks: 23.9 against 22.7 us
    (4096, 3584): (1, 1.040, 1.032),  # Llama-3-8B down on 4 ranks: 14.1 against 13.5 us
    (8192, 2048): (2, 0.952, 1.067),  # Llama-3-70B o_proj on 4 ranks: 15.0 against 15.8 us at one row, 17.8 against 16.6 at two
    (4096, 2048): (2, 0.946, 1.042),  # Llama-3-8B o_proj on 2 ranks: 9.4 against 10.0 us, 11.1 against 10.7 at two
}


def ar_twin_wanted(N: int, K: int, rows: int = 1) -> bool:
    """A row-parallel shard shape that keeps its twin under the fused all-reduce launch on an engine of
    ``rows`` decode rows (``max_batch``)."""
    return rows < AR_STAYS_BF16.get((N, K), (3,))[0]


def _row_bytes12(K: int) -> int:
    return K // UNIT_ELEMS * UNIT12_BYTES + K % UNIT_ELEMS // CHUNK_ELEMS * TAIL_CHUNK_BYTES


def packed12_tail_nbytes(N: int, K: int) -> int:
    return N * _row_bytes12(K) + N * REC12_DWORDS * 4


def _tail_error(shape) -> str:
    return (f"wpack12 tail: K a multiple of {CHUNK_ELEMS} off the {UNIT_ELEMS}-weight unit, above {UNIT_ELEMS} up to "
            f"{MAX_K12}, got {tuple(shape)}")


def pack12_tail_reference(W: torch.Tensor) -> PackedWeight12Tail:
    """Plain-torch packer of P12 with a tail (any device), byte for byte what the HIP packer writes."""
    N, K = W.shape
    if not packable12_tail_shape(N, K):
        raise ValueError(_tail_error(W.shape))
    U, Q = K // UNIT_ELEMS, K % UNIT_ELEMS // CHUNK_ELEMS
    bits, rec, raw, cnt, pbase = _records12(W)
    code = ((((bits >> 8) & 0x7F) - pbase.view(N, 1)) & 0x7) | ((bits >> 15) << 3)
    KU = U * UNIT_ELEMS
    b = _lane_order(bits[:, :KU].contiguous(), U)
    cu = _lane_order(code[:, :KU].contiguous(), U).view(N, U, 64, 4, 2, 4)
    low = (b & 0xFF).to(torch.uint8)
    nib = (cu[..., 0, :] | (cu[..., 1, :] << 4)).to(torch.uint8)
    ct = code[:, KU:].reshape(N, Q, 64, 2, 4)                               # [chunk, lane, half, j]
    tl = (bits[:, KU:] & 0xFF).to(torch.uint8).view(N, Q, 64, 8)            # [chunk, lane, element]
    QA = min(Q, 2)
    tail_low = torch.cat([tl[:, :QA].permute(0, 2, 1, 3).reshape(N, QA * 512), tl[:, QA:].reshape(N, (Q - QA) * 512)],
                         dim=1)                                             # A, B
    tn = (ct[..., 0, :] | (ct[..., 1, :] << 4)).to(torch.uint8)             # [chunk, lane, j]
    tail_nib = tn.permute(0, 2, 1, 3).reshape(N, Q * 256)                   # [lane, chunk, j]
    units = torch.cat([low[..., :16].reshape(N, U, 1024), low[..., 16:].reshape(N, U, 1024),
                       nib.reshape(N, U, 1024)], dim=2).reshape(N, U * UNIT12_BYTES)
    planes = torch.cat([units, tail_low, tail_nib], dim=1).contiguous()
    return PackedWeight12Tail(planes, _rec_bytes(rec), int(raw.sum()), int(cnt[~raw].sum()), N, K)


def unpack12_tail_reference(pw: PackedWeight12Tail, W: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``unpack12_reference`` for a twin with a tail."""
    N, K = pw.N, pw.K
    U, Q = K // UNIT_ELEMS, K % UNIT_ELEMS // CHUNK_ELEMS
    p = pw.planes.view(N, _row_bytes12(K)).to(torch.int32)
    hb = pw.records()[:, 0].to(torch.int32) & 0xFF
    base = torch.where(hb == RAW, torch.zeros_like(hb), hb)
    pu = p[:, :U * UNIT12_BYTES].reshape(N, U, UNIT12_BYTES)
    low = torch.cat([pu[..., :1024].reshape(N, U, 64, 16), pu[..., 1024:2048].reshape(N, U, 64, 16)], dim=3)
    nib = pu[..., 2048:].reshape(N, U, 64, 4, 4)
    code = torch.stack([nib & 0xF, nib >> 4], dim=4).reshape(N, U, 64, 32)
    b = ((code >> 3) << 15) | (((code & 7) + base.view(N, 1, 1, 1)) << 8) | low
    head = b.view(N, U, 64, 4, 8).permute(0, 1, 3, 2, 4).reshape(N, U * UNIT_ELEMS)
    pt = p[:, U * UNIT12_BYTES:]
    tnib = pt[:, Q * 512:].reshape(N, 64, Q, 4).permute(0, 2, 1, 3)          # [chunk, lane, j]
    tcode = torch.stack([tnib & 0xF, tnib >> 4], dim=3).reshape(N, Q * 512)  # [chunk, lane, half, j] = k order
    QA = min(Q, 2)
    tlow = torch.cat([pt[:, :QA * 512].reshape(N, 64, QA, 8).permute(0, 2, 1, 3).reshape(N, QA * 512),
                      pt[:, QA * 512:Q * 512]], dim=1)                       # A then B -> k order
    tail = ((tcode >> 3) << 15) | (((tcode & 7) + base.view(N, 1)) << 8) | tlow
    return _patched12(pw, torch.cat([head, tail], dim=1).contiguous(), W)


def pack12_tail(W: torch.Tensor) -> PackedWeight12Tail:
    """P12-with-a-tail-pack ``W`` where it lives: the HIP packer on the GPU, the reference on the CPU."""
    if not W.is_cuda:
        return pack12_tail_reference(W)
    from ..utils.native import kernels

    N, K = W.shape
    if W.dtype != torch.bfloat16 or not packable12_tail_shape(N, K):
        raise ValueError(_tail_error(W.shape) + f" {W.dtype}")
    W = W.contiguous()
    planes = torch.empty(N, _row_bytes12(K), dtype=torch.uint8, device=W.device)
    hdr = torch.empty(N, REC12_DWORDS * 4, dtype=torch.uint8, device=W.device)
    counts = torch.zeros(2, dtype=torch.int32, device=W.device)
    kernels().wpack12(W.data_ptr(), planes.data_ptr(), hdr.data_ptr(), counts.data_ptr(), N, K,
                      torch.cuda.current_stream(W.device).cuda_stream)
    raw_rows, exceptions = counts.tolist()
    return PackedWeight12Tail(planes, hdr, raw_rows, exceptions, N, K)


# ---- P12 of a MoE expert stack ----
#
# A contiguous ``[E, N, K]`` stack is packed as its ``[E * N, K]`` view: rows are packed one by one, so
# the planes and the records are the per-expert twins concatenated, and row n of expert e is row
# ``e * N + n``, which is how the expert GEMVs index it. Whole 2048-weight units only (no tail, no P13).


class PackedExperts12(PackedWeight12):
    """The 12-bit twin of a bf16 ``[E, N, K]`` expert stack: a ``PackedWeight12`` over its ``[E * N, K]``
    view (``N`` is E * N there), with ``E`` and ``rows``, the rows of one expert."""

    __slots__ = ("E", "rows")

    def __init__(self, pw: PackedWeight12, E: int):
        super().__init__(pw.planes, pw.hdr, pw.raw_rows, pw.exceptions, pw.N, pw.K)
        self.E, self.rows = E, pw.N // E


# Expert launches on which the packed stream, cold and alone, was not faster than bf16 by more than the spread
# of the two runs would be listed here as TAIL_STAYS_BF16 lists the tail shapes, (N, K) of one expert
# (profiles/r12_packed_experts.md section 3); ``pack_best`` builds no twin for them.
EXPERTS_STAY_BF16: dict = {}


def expert_twin_wanted(N: int, K: int) -> bool:
    """An expert shape ``[*, N, K]`` that ``pack_best`` packs."""
    return packable12_shape(N, K) and (N, K) not in EXPERTS_STAY_BF16


def pack12_experts(W: torch.Tensor) -> PackedExperts12:
    """P12-pack a contiguous bf16 ``[E, N, K]`` expert stack where it lives (``pack12`` of its ``[E * N, K]``
    view)."""
    if W.dim() != 3 or W.dtype != torch.bfloat16 or not W.is_contiguous() or not packable12_shape(*W.shape[1:]):
        raise ValueError(f"wpack12 experts: a contiguous bf16 [E, N, K] with K a multiple of {UNIT_ELEMS} up to "
                         f"{MAX_K12}, got {W.dtype} {tuple(W.shape)}")
    E, N, K = W.shape
    return PackedExperts12(pack12(W.view(E * N, K)), E)


def packed_format() -> int:
    """12 or 13: the format ``pack_best`` tries first (``LLMC_PACKED_FORMAT``, A/B runs)."""
    from ..parallel.placement import packed_format as fmt

    return fmt()


def pack_best(W: torch.Tensor, fmt: Optional[int] = None):
    """The P12 twin of ``W``; where more than MAX_RAW_SHARE of its rows would be raw (or the shape
    is off P12's), the P13 twin; where that fails too, None. ``fmt`` 13 skips P12. A K off the
    2048-weight unit has the 12-bit format with a tail only (``tail_twin_wanted``: a tail shape that did
    not measure slower than bf16): that twin, or None where too many rows are raw or ``fmt`` is 13.
    A 3-D ``[E, N, K]`` expert stack has the 12-bit format on whole units only: ``pack12_experts``' twin, or
    None likewise."""
    if W.dim() == 3:
        if (packed_format() if fmt is None else fmt) != 12 or not expert_twin_wanted(*W.shape[1:]):
            return None
        pwe = pack12_experts(W.contiguous())
        return pwe if pwe.raw_share <= MAX_RAW_SHARE else None
    if W.dim() != 2:
        return None
    if not packable_shape(*W.shape):
        if (packed_format() if fmt is None else fmt) == 12 and tail_twin_wanted(*W.shape):
            pwt = pack12_tail(W)
            return pwt if pwt.raw_share <= MAX_RAW_SHARE else None
        return None
    if (packed_format() if fmt is None else fmt) == 12 and packable12_shape(*W.shape):
        pw12 = pack12(W)
        if pw12.raw_share <= MAX_RAW_SHARE:
            return pw12
    pw = pack(W)
    return pw if pw.raw_share <= MAX_RAW_SHARE else None
