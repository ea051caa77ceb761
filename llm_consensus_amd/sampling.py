"""What a request asks of the sampler (``SamplingParams``) and the launches that takes (``SamplingForm``).

Kept free of torch: the driver process derives the run's form from these (``provider/local.py``) and
must not pay torch's import before it spawns the workers. ``engine/engine.py`` re-exports both.
"""

from __future__ import annotations

import dataclasses
import math
from typing import Iterable, NamedTuple, Optional


class SamplingForm(NamedTuple):
    """The optional launches a decode step issues around the sampler. A step's form is launch-uniform
    (``of`` the rows it decodes); it is part of the decode graph's key and decides which per-row state
    the engine holds (``Engine._ensure_form_state``)."""

    topkp: bool = False      # the top-k/top-p launch (which also applies min-p)
    penalties: bool = False  # ``penalize_logits`` ahead of the sampler; the advance counts the sampled id
    logprobs: bool = False   # the two log-probability stages around the sampler

    @classmethod
    def of(cls, params: Iterable["SamplingParams"]) -> "SamplingForm":
        """The form of a step that decodes rows with these params: each launch any of them needs."""
        return cls(*map(any, zip(*(p.form for p in params))))  # field by field; no params: the default


@dataclasses.dataclass
class SamplingParams:
    max_tokens: int = 256
    temperature: float = 1.0
    top_p: float = 1.0
    top_k: int = 0
    seed: int = 0
    stop_on_eos: bool = True
    # sampled rows keep a token only if its probability is >= min_p x the most likely token's (0 = off)
    min_p: float = 0.0
    # over the ids of the context and the ids generated so far: l = l > 0 ? l / r : l * r (1 = off)
    repetition_penalty: float = 1.0
    # over the ids generated so far: l -= presence_penalty + frequency_penalty x (times generated)
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    # None = off; n in [0, 20]: report the raw log-probability of every generated token and of the n
    # most likely ids at its step (before penalties, temperature and truncation)
    logprobs: Optional[int] = None

    @property
    def penalised(self) -> bool:
        return self.repetition_penalty != 1.0 or self.presence_penalty != 0.0 or self.frequency_penalty != 0.0

    @property
    def topkp(self) -> bool:
        """Whether the row needs the top-k/top-p launch (which also applies min-p)."""
        return self.top_k > 0 or self.top_p < 1.0 or self.min_p > 0.0

    @property
    def form(self) -> SamplingForm:
        return SamplingForm(self.topkp, self.penalised, self.logprobs is not None)

    @property
    def ln_min_p(self) -> float:
        return math.log(self.min_p) if self.min_p > 0.0 else float("-inf")
