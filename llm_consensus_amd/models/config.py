"""Architecture configs of the on-node model families (SURVEY.md §2.6 model shapes).

Weights are random-init (seeded per replica): there is no network to fetch checkpoints, and the
benchmark contract is "random-init weights of that architecture". Shapes are the public configs.
"""

from __future__ import annotations

import dataclasses
import math
from typing import Optional


@dataclasses.dataclass(frozen=True)
class RopeScaling:
    """Llama-3.1-style frequency-dependent RoPE scaling (for a judge context beyond 8k)."""

    factor: float = 8.0
    low_freq_factor: float = 1.0
    high_freq_factor: float = 4.0
    original_max_position: int = 8192


@dataclasses.dataclass(frozen=True)
class SamplingDefaults:
    """The sampling a checkpoint's ``generation_config.json`` asks for; used only on request
    (``--model-sampling``), for the knobs a request leaves neutral. The defaults here ARE neutral."""

    temperature: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    min_p: float = 0.0
    repetition_penalty: float = 1.0


@dataclasses.dataclass(frozen=True)
class ModelConfig:
    name: str
    arch: str  # "llama" (also Mistral, Qwen2, Qwen3: the same layer layout) | "mixtral" | "phi3"
    n_layers: int
    hidden: int
    n_heads: int
    n_kv_heads: int
    head_dim: int
    intermediate: int
    vocab: int
    rope_theta: float
    rms_eps: float = 1e-5
    max_position: int = 8192
    n_experts: int = 0
    top_k_experts: int = 0
    rope_scaling: Optional[RopeScaling] = None
    default_tp: int = 1
    # Hugging Face checkpoint directory (models/checkpoint.py); None = seeded random init
    checkpoint: Optional[str] = None
    bos_id: int = -1            # -1: the synthetic tokenizer's (vocab - 2)
    eos_ids: tuple = ()         # empty: the synthetic tokenizer's (vocab - 1)
    tie_embeddings: bool = False
    # sliding-window attention: position p attends keys (p - W, p]; 0 = every key (one window for
    # all layers)
    sliding_window: int = 0
    # a bias on the q, k and v projections (Qwen2 / Qwen2.5; o_proj and the MLP have none), added
    # before the rotation
    qkv_bias: bool = False
    # an RMSNorm over the head dimension on every q and every k head, after the projection and
    # before the rotation (Qwen3; weights [head_dim], one vector for the layer's q heads, one for
    # its k heads)
    qk_norm: bool = False
    # generation_config.json's sampling values (checkpoints only; see SamplingDefaults)
    sampling: Optional[SamplingDefaults] = None

    @property
    def eos(self) -> tuple:
        return self.eos_ids or (self.vocab - 1,)

    # -- derived sizes ---------------------------------------------------------------------
    @property
    def q_size(self) -> int:
        return self.n_heads * self.head_dim

    @property
    def kv_size(self) -> int:
        return self.n_kv_heads * self.head_dim

    @property
    def qkv_size(self) -> int:
        return self.q_size + 2 * self.kv_size

    @property
    def is_moe(self) -> bool:
        return self.n_experts > 0

    def num_params(self) -> int:
        h, i = self.hidden, self.intermediate
        attn = h * self.qkv_size + self.q_size * h + (self.qkv_size if self.qkv_bias else 0)
        mlp = 3 * h * i * (self.n_experts if self.is_moe else 1)
        router = h * self.n_experts if self.is_moe else 0
        per_layer = attn + mlp + router + 2 * h + (2 * self.head_dim if self.qk_norm else 0)
        return self.n_layers * per_layer + 2 * self.vocab * h + h

    def weight_bytes(self, dtype_bytes: int = 2) -> int:
        return self.num_params() * dtype_bytes

    def packed_twin_bytes(self, tp: int = 1) -> int:
        """Bytes of the packed decode twins ONE rank of a ``tp``-way engine builds beside its bf16 shards
        (``tp`` = 1, the default: the unsharded engine): the shapes below with the column-parallel outputs
        (qkv, gate_up), the row-parallel inputs (o_proj, down) and the vocabulary divided by ``tp``. A shard
        shape no format takes (K under 2048 or no multiple of 512) counts nothing; a MoE model has twins at
        ``tp`` = 1 only (0 above). Per shape:
        the bytes of the 13-bit packed decode twins (ops.wpack) an unsharded dense engine builds beside
        its bf16 weights: 13/16 of every decode GEMV weight whose K is a whole number of 2048-weight
        units (the o_proj twin counted too: the upper bound), and the 12-bit twin with a row tail
        (12/16 and a 68-byte record per row) of every one whose K is another multiple of 512 above
        2048 (an upper bound as well: ``ops.wpack.TAIL_STAYS_BF16`` leaves a few shapes bf16). A MoE model: the
        dense parts as above (the router has no twin) and the 12-bit twin of each expert stack whose K is a whole
        number of units (12/16 and a 68-byte record per row; no tail, so nothing for another K)."""
        h, i = self.hidden, self.intermediate
        if tp != 1 and self.is_moe:
            return 0

        def twin(n: int, k: int) -> int:
            if k % 2048 == 0:
                return n * k * 13 // 8
            return n * k * 12 // 8 + 68 * n if k % 512 == 0 and k > 2048 else 0

        def experts(n: int, k: int) -> int:
            rows = self.n_experts * n
            return rows * k * 12 // 8 + 68 * rows if k % 2048 == 0 and k <= 65536 - 2048 else 0

        shapes = [(self.qkv_size // tp, h), (h, self.q_size // tp)]
        ffn = experts(2 * i, h) + experts(h, i) if self.is_moe else twin(2 * i // tp, h) + twin(h, i // tp)
        return self.n_layers * (sum(twin(n, k) for n, k in shapes) + ffn) + twin(self.vocab // tp, h)

    def kv_bytes_per_token(self, dtype_bytes: int = 2) -> int:
        return 2 * self.n_layers * self.kv_size * dtype_bytes

    def active_weight_bytes(self, dtype_bytes: int = 2) -> int:
        """Bytes streamed per decode token at batch 1 (MoE: top-k experts only)."""
        if not self.is_moe:
            return self.weight_bytes(dtype_bytes) - self.vocab * self.hidden * dtype_bytes  # embed not streamed
        h, i = self.hidden, self.intermediate
        per_layer = h * self.qkv_size + self.q_size * h + 3 * h * i * self.top_k_experts + h * self.n_experts
        return (self.n_layers * per_layer + self.vocab * h) * dtype_bytes

    def with_(self, **kw) -> "ModelConfig":
        return dataclasses.replace(self, **kw)


LLAMA3_8B = ModelConfig("llama-3-8b", "llama", 32, 4096, 32, 8, 128, 14336, 128256, 500000.0,
                        max_position=131072, rope_scaling=RopeScaling())
LLAMA3_70B = ModelConfig("llama-3-70b", "llama", 80, 8192, 64, 8, 128, 28672, 128256, 500000.0,
                         max_position=131072, rope_scaling=RopeScaling(), default_tp=4)
MIXTRAL_8X7B = ModelConfig("mixtral-8x7b", "mixtral", 32, 4096, 32, 8, 128, 14336, 32000, 1000000.0,
                           max_position=32768, n_experts=8, top_k_experts=2)
PHI3_MINI = ModelConfig("phi-3-mini", "phi3", 32, 3072, 32, 32, 96, 8192, 32064, 10000.0,
                        max_position=4096)
MISTRAL_7B = ModelConfig("mistral-7b", "llama", 32, 4096, 32, 8, 128, 14336, 32000, 10000.0,
                         max_position=32768, sliding_window=4096)

# Tiny variants: same code paths and kernel shape classes (GQA, d=128/96, MoE), small enough
# for CPU tests and fast GPU numerics tests.
LLAMA_TINY = ModelConfig("llama-tiny", "llama", 2, 256, 4, 2, 64, 512, 1024, 500000.0, max_position=4096)
LLAMA_SMALL = ModelConfig("llama-small", "llama", 4, 1024, 8, 2, 128, 2816, 32000, 500000.0, max_position=8192)
MIXTRAL_TINY = ModelConfig("mixtral-tiny", "mixtral", 2, 256, 4, 2, 64, 384, 1024, 1000000.0,
                           max_position=4096, n_experts=4, top_k_experts=2)
PHI3_TINY = ModelConfig("phi3-tiny", "phi3", 2, 192, 2, 2, 96, 384, 1024, 10000.0, max_position=4096)
QWEN25_7B = ModelConfig("qwen2.5-7b", "llama", 28, 3584, 28, 4, 128, 18944, 152064, 1000000.0, rms_eps=1e-6,
                        max_position=32768, qkv_bias=True)
# Qwen2.5's shape class in small: a GQA group of 7 (14 / 2 heads, D = 64), q/k/v biases, every K a
# multiple of 128, heads / FFN / vocab shardable over TP = 2
QWEN2_TINY = ModelConfig("qwen2-tiny", "llama", 2, 896, 14, 2, 64, 1024, 1024, 1000000.0, rms_eps=1e-6,
                         max_position=4096, qkv_bias=True)
# Qwen3 (dense): no q/k/v bias, an explicit head_dim, a per-head RMSNorm on q and k before the rotation
QWEN3_8B = ModelConfig("qwen3-8b", "llama", 36, 4096, 32, 8, 128, 12288, 151936, 1000000.0, rms_eps=1e-6,
                       max_position=40960, qk_norm=True)
# Qwen3's shape class in small: heads of 128 over a hidden of 256 (q_size 512: the head_dim decoupled
# from hidden / heads, as in Qwen3-0.6B / 1.7B / 4B), heads / FFN / vocab shardable over TP = 2
QWEN3_TINY = ModelConfig("qwen3-tiny", "llama", 2, 256, 4, 2, 128, 512, 1024, 1000000.0, rms_eps=1e-6,
                         max_position=4096, qk_norm=True)
# llama-tiny with a window short enough that tiny prompts cross it
MISTRAL_TINY = LLAMA_TINY.with_(name="mistral-tiny", sliding_window=48)
# tiny stand-in for Llama-3-70B in TP=4 rehearsals (heads, kv heads, FFN and vocab shard over 4)
LLAMA_TINY_TP4 = ModelConfig("llama-tiny-tp4", "llama", 2, 512, 8, 4, 64, 1024, 1024, 500000.0, max_position=16384,
                             default_tp=4)

FAMILIES = {c.name: c for c in (LLAMA3_8B, LLAMA3_70B, MIXTRAL_8X7B, PHI3_MINI,
                                LLAMA_TINY, LLAMA_SMALL, MIXTRAL_TINY, PHI3_TINY, LLAMA_TINY_TP4,
                                MISTRAL_7B, MISTRAL_TINY, QWEN25_7B, QWEN2_TINY, QWEN3_8B, QWEN3_TINY)}


def rope_inv_freq(cfg: ModelConfig):
    """Inverse frequencies (float64 list) incl. Llama-3.1 scaling; shared by kernels and oracle."""
    d = cfg.head_dim
    inv = [1.0 / (cfg.rope_theta ** (2 * i / d)) for i in range(d // 2)]
    rs = cfg.rope_scaling
    if rs is None:
        return inv
    low_wl = rs.original_max_position / rs.low_freq_factor
    high_wl = rs.original_max_position / rs.high_freq_factor
    out = []
    for f in inv:
        wl = 2 * math.pi / f
        if wl < high_wl:
            out.append(f)
        elif wl > low_wl:
            out.append(f / rs.factor)
        else:
            smooth = (rs.original_max_position / wl - rs.low_freq_factor) / (rs.high_freq_factor - rs.low_freq_factor)
            out.append((1 - smooth) * f / rs.factor + smooth * f)
    return out
