"""The decode GEMV's geometry rule (csrc/kernels/gemv_geom.h), asked through ``ops.gemv_plan`` (no GPU: the
rule and the kernel lookup are host code of the kernel library): which block (threads, rows per wave, 16-B
loads per lane in flight) a launch runs in every weight format, and that the library holds that kernel."""

import json
import os
import subprocess
import sys

import pytest

from llm_consensus_amd import ops
from llm_consensus_amd.models.config import FAMILIES
from llm_consensus_amd.ops import (EPI_AR, EPI_BF16, EPI_COMBINE, EPI_F32, EPI_RESADD, EPI_ROPE, EPI_SILU, GEMV_AR,
                                   GEMV_DENSE, GEMV_MOE_COMBINE, GEMV_MOE_PAIR, WF_BF16, WF_P12, WF_P13, wpack)

D, AR, PAIR, COMBINE = GEMV_DENSE, GEMV_AR, GEMV_MOE_PAIR, GEMV_MOE_COMBINE

# (op, M, N, K, epilogue, format) -> (nt, rpw, unroll): the parent's rule, transcribed shape by shape
PINNED = [
    (D, 1, 6144, 4096, EPI_ROPE, WF_BF16, (768, 2, 4)),        # 8B qkv
    (D, 2, 6144, 4096, EPI_ROPE, WF_BF16, (768, 2, 4)),
    (D, 3, 6144, 4096, EPI_ROPE, WF_BF16, (768, 1, 4)),
    (D, 1, 6144, 4096, EPI_BF16, WF_BF16, (768, 1, 4)),        # ... with the bf16 epilogue (Qwen3)
    (D, 1, 4096, 4096, EPI_RESADD, WF_BF16, (1024, 1, 4)),     # 8B o
    (D, 1, 28672, 4096, EPI_SILU, WF_BF16, (896, 2, 4)),       # 8B gate_up
    (D, 4, 28672, 4096, EPI_SILU, WF_BF16, (1024, 1, 4)),
    (D, 1, 4096, 14336, EPI_RESADD, WF_BF16, (1024, 1, 8)),    # 8B down
    (D, 2, 4096, 14336, EPI_RESADD, WF_BF16, (1024, 1, 8)),
    (D, 1, 128256, 4096, EPI_F32, WF_BF16, (768, 1, 4)),       # 8B lm_head
    (D, 1, 9216, 3072, EPI_ROPE, WF_BF16, (768, 1, 4)),        # Phi-3 qkv
    (D, 1, 16384, 3072, EPI_SILU, WF_BF16, (1024, 2, 4)),      # Phi-3 gate_up
    (D, 1, 3072, 8192, EPI_RESADD, WF_BF16, (768, 1, 4)),      # Phi-3 down
    (D, 1, 32064, 3072, EPI_F32, WF_BF16, (1024, 1, 4)),       # Phi-3 lm_head
    (D, 1, 2560, 8192, EPI_ROPE, WF_BF16, (640, 1, 8)),        # 70B TP=4 qkv
    (D, 1, 14336, 8192, EPI_SILU, WF_BF16, (896, 1, 4)),       # 70B TP=4 gate_up
    (D, 1, 768, 4096, EPI_ROPE, WF_BF16, (256, 1, 8)),         # 8B TP=8 qkv
    (D, 1, 3584, 4096, EPI_SILU, WF_BF16, (896, 1, 4)),        # 8B TP=8 gate_up
    (D, 1, 7168, 4096, EPI_SILU, WF_BF16, (896, 2, 4)),        # 8B TP=4 gate_up
    (D, 1, 4608, 3584, EPI_ROPE, WF_BF16, (768, 1, 4)),        # Qwen2.5-7B qkv
    (D, 1, 37888, 3584, EPI_SILU, WF_BF16, (512, 1, 4)),       # Qwen2.5-7B gate_up
    (D, 1, 3584, 18944, EPI_RESADD, WF_BF16, (1024, 1, 8)),    # Qwen2.5-7B down
    (D, 1, 2052, 4096, EPI_SILU, WF_BF16, (256, 2, 4)),
    (D, 1, 36, 512, EPI_SILU, WF_BF16, (256, 2, 4)),
    (D, 1, 64, 2048, EPI_BF16, WF_BF16, (256, 1, 8)),
    (AR, 1, 8192, 2048, EPI_AR, WF_BF16, (1024, 1, 4)),
    (AR, 1, 8192, 7168, EPI_AR, WF_BF16, (1024, 1, 4)),
    (AR, 1, 4096, 1792, EPI_AR, WF_BF16, (1024, 1, 4)),
    (AR, 2, 4096, 8192, EPI_AR, WF_BF16, (1024, 1, 8)),
    (AR, 2, 4096, 8192, EPI_AR, WF_P12, (1024, 1, 4)),         # packed EPI_AR, two rows: 4 loads per lane
    (AR, 1, 4096, 8192, EPI_AR, WF_P12, (1024, 1, 8)),
    (AR, 1, 2560, 8192, EPI_AR, WF_BF16, (640, 1, 8)),
    (AR, 1, 5120, 4096, EPI_AR, WF_BF16, (640, 1, 4)),
    (AR, 1, 64, 2048, EPI_AR, WF_BF16, (256, 1, 8)),
    (PAIR, 1, 28672, 4096, EPI_SILU, WF_BF16, (896, 2, 4)),
    (PAIR, 1, 4096, 14336, EPI_BF16, WF_BF16, (1024, 1, 4)),   # no 8 loads per lane in the pair form
    (PAIR, 1, 512, 2048, EPI_SILU, WF_BF16, (256, 1, 4)),      # ... nor in its 4-wave blocks
    (PAIR, 1, 4100, 2048, EPI_SILU, WF_BF16, (640, 1, 4)),
    (PAIR, 1, 16384, 2048, EPI_SILU, WF_BF16, (1024, 2, 4)),
    (COMBINE, 2, 4096, 14336, EPI_COMBINE, WF_BF16, (1024, 2, 4)),
    (COMBINE, 2, 30, 2048, EPI_COMBINE, WF_P12, (1024, 2, 4)),
    (D, 2, 4096, 14336, EPI_RESADD, WF_P12, (1024, 1, 8)),
    (D, 2, 4096, 14336, EPI_RESADD, WF_P13, (1024, 1, 8)),
    (D, 2, 4096, 14336, EPI_ROPE, WF_P12, (1024, 1, 4)),       # P12 with the RoPE epilogue, two rows
    (D, 2, 4096, 14336, EPI_ROPE, WF_P13, (1024, 1, 8)),
    (D, 2, 4096, 11264, EPI_RESADD, WF_P12, (1024, 1, 4)),     # P12 with a tail, two rows, every epilogue
    (D, 2, 4096, 11264, EPI_BF16, WF_P12, (1024, 1, 4)),
    (D, 2, 4096, 11264, EPI_F32, WF_P12, (1024, 1, 4)),
    (D, 2, 4096, 11264, EPI_SILU, WF_P12, (1024, 1, 4)),
    (D, 2, 4096, 11264, EPI_ROPE, WF_P12, (1024, 1, 4)),
    (D, 1, 4096, 14336, EPI_RESADD, WF_P12, (1024, 1, 8)),     # one row: 8 loads per lane stay
    (D, 1, 4096, 14336, EPI_ROPE, WF_P12, (1024, 1, 8)),
    (D, 1, 4096, 11264, EPI_RESADD, WF_P12, (1024, 1, 8)),
    (D, 1, 4096, 11264, EPI_ROPE, WF_P12, (1024, 1, 8)),
]


@pytest.mark.parametrize("op,M,N,K,epi,wf,geom", PINNED)
def test_pinned_geometry(op, M, N, K, epi, wf, geom):
    assert ops.gemv_plan(op, M, N, K, epi, wf) == geom + (True,)


def test_what_has_no_launch():
    none = (0, 0, 0, False)
    assert ops.gemv_plan(D, 5, 4096, 4096, EPI_BF16) == none          # the VALU form: up to 4 rows
    assert ops.gemv_plan(D, 3, 4096, 4096, EPI_BF16, WF_P12) == none  # packed: up to 2
    assert ops.gemv_plan(D, 1, 4097, 4096, EPI_SILU) == none          # a pair needs both rows
    assert ops.gemv_plan(D, 1, 4096, 4100, EPI_BF16) == none          # K: 16-B chunks
    assert ops.gemv_plan(D, 1, 4096, 4096, EPI_AR) == none            # an epilogue of another op
    assert ops.gemv_plan(AR, 3, 4096, 4096, EPI_AR) == none
    assert ops.gemv_plan(AR, 1, 4096, 4096, EPI_AR, WF_P13) == none   # P13: the dense op only
    assert ops.gemv_plan(PAIR, 1, 4096, 4096, EPI_SILU, WF_P13) == none
    assert ops.gemv_plan(D, 1, 4096, 3072, EPI_BF16, WF_P13) == none  # P13 has no tail
    assert ops.gemv_plan(D, 1, 4096, 1536, EPI_BF16, WF_P12) == none  # a tail needs a whole unit before it
    assert ops.gemv_plan(D, 1, 4096, 4352, EPI_BF16, WF_P12) == none  # ... and is whole 512-weight chunks
    assert ops.gemv_plan(PAIR, 1, 4096, 3072, EPI_SILU, WF_P12) == none  # expert stacks: whole units
    assert ops.gemv_plan(COMBINE, 2, 4096, 3072, EPI_COMBINE, WF_P12) == none
    assert ops.gemv_plan(PAIR, 1, 4096, 4096, EPI_F32) == none


OPS = [  # op, its epilogues, its row counts
    (D, (EPI_BF16, EPI_F32, EPI_RESADD, EPI_SILU, EPI_ROPE), (1, 2, 3, 4)),
    (AR, (EPI_AR,), (1, 2)),
    (PAIR, (EPI_BF16, EPI_SILU), (1,)),
    (COMBINE, (EPI_COMBINE,), (2,)),
]


def _packed_unroll(op, M, epi, K, wf, bf16):
    """The three documented demotions: two rows, 16 waves, one row per wave, 8 loads per lane run 4 at 12 bits
    with the RoPE epilogue, with a tail under every epilogue, and in the fused all-reduce launch."""
    if wf == WF_P12 and M == 2 and bf16 == (1024, 1, 8) and (epi == EPI_ROPE or K % 2048 != 0 or op == AR):
        return 4
    return bf16[2]


def test_no_hole_in_the_lists():
    """Every launch the rule can choose has its kernel: bf16 at every row count, and for M <= 2 every packed
    format the op has, in the bf16 launch's (nt, rpw) and, but for the demotions, its unroll."""
    plan = ops.kernels().gemv_plan
    seen = set()
    for op, epis, rows in OPS:
        for K in (4096, 8192, 8704):  # 8704: a tail on rows long enough for 8 loads per lane
            for epi in epis:
                for M in rows:
                    for N in range(2, 65537, 2):
                        bf16 = plan(op, M, N, K, epi, WF_BF16)
                        assert bf16[0] and bf16[3], (op, M, N, K, epi, bf16)
                        seen.add((op,) + bf16[:3])
                        if M > 2:
                            continue
                        for wf in (WF_P13, WF_P12):
                            got = plan(op, M, N, K, epi, wf)
                            if (wf == WF_P13 and (op != D or K % 2048)) or (K % 2048 and op in (PAIR, COMBINE)):
                                assert got == (0, 0, 0, False), (op, M, N, K, epi, wf, got)
                                continue
                            want = bf16[:2] + (_packed_unroll(op, M, epi, K, wf, bf16[:3]), True)
                            assert got == want, (op, M, N, K, epi, wf, got, want)
    # ... and the sweep reached every entry of the lists (csrc/kernels/gemv_geom.h)
    assert {g[1:] for g in seen if g[0] == D} == {(1024, 1, 4), (896, 1, 4), (768, 1, 4), (640, 1, 4), (512, 1, 4),
                                                  (256, 1, 8), (256, 2, 4), (1024, 2, 4), (896, 2, 4), (768, 2, 4),
                                                  (1024, 1, 8), (640, 1, 8)}
    assert {g[1:] for g in seen if g[0] == AR} == {(1024, 1, 4), (768, 1, 4), (640, 1, 4), (512, 1, 4), (256, 1, 8),
                                                   (1024, 1, 8), (640, 1, 8)}
    assert {g[1:] for g in seen if g[0] == PAIR} == {(1024, 1, 4), (768, 1, 4), (640, 1, 4), (512, 1, 4), (256, 1, 4),
                                                     (1024, 2, 4), (896, 2, 4), (896, 1, 4), (256, 2, 4)}
    assert {g[1:] for g in seen if g[0] == COMBINE} == {(1024, 2, 4)}


def _twin_formats(N, K):
    """The formats ``wpack.pack_best`` may give a dense [N, K] tensor (which of them depends on its raw rows)."""
    if wpack.packable_shape(N, K):
        return [WF_P13] + ([WF_P12] if wpack.packable12_shape(N, K) else [])
    return [WF_P12] if wpack.tail_twin_wanted(N, K) else []


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_every_twin_of_the_catalog_has_its_kernel(name):
    """Nothing that ``pack_decode_weights`` builds a twin for falls back through -8: at every TP degree the
    model shards over, every decode projection that gets a twin has a packed kernel in its plan, in every
    launch that may read it."""
    c = FAMILIES[name]
    h, i = c.hidden, c.intermediate
    checked = 0
    for tp in (1, 2, 4, 8):
        if c.n_heads % tp or c.n_kv_heads % tp or c.intermediate % tp or c.vocab % tp:
            continue
        if c.is_moe and tp != 1:  # expert shards under TP have no packed form (Engine: packed weights off)
            continue
        launches = [(D, c.vocab // tp, h, (EPI_F32,)),
                    (D, c.qkv_size // tp, h, (EPI_ROPE, EPI_BF16)),       # bf16: a qk_norm model's qkv
                    # o_proj (`with_o`: where the fused attention + o_proj launch does not cover it) and down:
                    # in place at TP = 1 and on rank 0, to a buffer on the other ranks ...
                    (D, h, c.q_size // tp, (EPI_RESADD, EPI_BF16))]
        if c.is_moe:
            launches += [(PAIR, 2 * i, h, (EPI_SILU,)), (PAIR, h, i, (EPI_BF16,)), (COMBINE, h, i, (EPI_COMBINE,))]
        else:
            launches += [(D, 2 * i // tp, h, (EPI_SILU,)), (D, h, i // tp, (EPI_RESADD, EPI_BF16))]
        for op, N, K, epis in launches:
            if op == D:
                formats = _twin_formats(N, K)
            else:
                formats = [WF_P12] if wpack.expert_twin_wanted(N, K) else []
            for wf in formats:
                for epi in epis:
                    for M in (1, 2):
                        got = ops.gemv_plan(op, M, N, K, epi, wf)
                        assert got[3], (name, tp, op, M, N, K, epi, wf, got)
                        checked += 1
        if tp > 1:  # ... or, with the all-reduce in the epilogue, the twins AR_STAYS_BF16 leaves
            for N, K in ((h, c.q_size // tp), (h, i // tp)):
                for rows in (1, 2):  # the engine's decode rows
                    if WF_P12 in _twin_formats(N, K) and wpack.ar_twin_wanted(N, K, rows):
                        for M in range(1, rows + 1):
                            got = ops.gemv_plan(AR, M, N, K, EPI_AR, WF_P12)
                            assert got[3], (name, tp, M, N, K, got)
                            checked += 1
    if c.hidden >= 2048:
        assert checked > 0


_CHILD = """
import json, sys
import llm_consensus_amd._lib._llmc_hip as k
print(json.dumps([k.gemv_plan(*r) for r in json.loads(sys.argv[1])]))
"""

# what each A/B switch changes among PINNED, from the parent's code: {row index: geometry with the switch set}
SWITCHES = {
    # no 10-wave blocks: 2560 rows fall back to 16 waves (dense; 8 loads per lane on long rows) or 12 (unpaired:
    # 214 blocks of 256 slots), 5120 rows to 12 waves, 4100 paired rows tile by nothing else
    "LLMC_GEMV_NO_W10": {(D, 1, 2560, 8192, EPI_ROPE, WF_BF16): (1024, 1, 8), (AR, 1, 2560, 8192, EPI_AR, WF_BF16): (768, 1, 4),
                         (AR, 1, 5120, 4096, EPI_AR, WF_BF16): (768, 1, 4), (PAIR, 1, 4100, 2048, EPI_SILU, WF_BF16): (256, 2, 4)},
    # no 14-wave blocks: 14336 rows tile exactly by 8 waves, 3584 rows stay on 16
    "LLMC_GEMV_NO_W14": {(D, 1, 14336, 8192, EPI_SILU, WF_BF16): (512, 1, 4), (D, 1, 3584, 4096, EPI_SILU, WF_BF16): (1024, 1, 4)},
    "LLMC_GEMV_ROPE_RPW1": {(D, 1, 6144, 4096, EPI_ROPE, WF_BF16): (768, 1, 4), (D, 2, 6144, 4096, EPI_ROPE, WF_BF16): (768, 1, 4)},
    "LLMC_GEMV_SILU_RPW1": {(D, 1, 28672, 4096, EPI_SILU, WF_BF16): (1024, 1, 4), (D, 1, 16384, 3072, EPI_SILU, WF_BF16): (1024, 1, 4),
                            (D, 1, 7168, 4096, EPI_SILU, WF_BF16): (896, 1, 4), (PAIR, 1, 28672, 4096, EPI_SILU, WF_BF16): (1024, 1, 4),
                            (PAIR, 1, 16384, 2048, EPI_SILU, WF_BF16): (1024, 1, 4)},
}


@pytest.mark.parametrize("switch", sorted(SWITCHES))
def test_ab_switch_changes_its_rows_only(switch):
    """The library reads each switch once per process, so a fresh child asks the plan with it set."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("LLMC_GEMV_")}
    env[switch] = "1"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    rows = [r[:6] for r in PINNED]
    out = subprocess.run([sys.executable, "-c", _CHILD, json.dumps(rows)], env=env, capture_output=True, text=True,
                         check=True).stdout
    changed = dict(SWITCHES[switch])
    for row, got in zip(PINNED, json.loads(out)):
        want = changed.pop(row[:6], row[6])
        assert tuple(got) == want + (True,), (switch, row, got)
    assert not changed, changed  # every row named above is one of PINNED
