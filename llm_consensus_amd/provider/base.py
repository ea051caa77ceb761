"""Provider API (reference ``internal/provider/provider.go:8-55``).

``Provider.query_stream(ctx, req, callback) -> Response`` is the single contract every model
backend implements: the callback receives incremental text chunks and the returned
``content`` is their concatenation; ``latency`` spans request start → end of stream
(``openai.go:142, 208``).  ``FuncProvider`` is the test fake (``provider.go:37-55``): it calls
the function and then invokes the callback once with the full content.

Deviation: the JSON field ``latency_ms`` carries milliseconds; the raw
nanosecond value is kept in ``latency_ns`` for benches.
"""

from __future__ import annotations

import dataclasses
import math
from typing import Callable, Optional, Protocol

from ..context import Context

StreamCallback = Callable[[str], None]


@dataclasses.dataclass
class Request:
    model: str
    prompt: str
    # Engine knobs (no reference counterpart: the reference sends model+prompt only,
    # provider.go:24-27). ``None`` = engine default.
    max_tokens: Optional[int] = None
    temperature: Optional[float] = None
    top_p: Optional[float] = None
    top_k: Optional[int] = None
    seed: Optional[int] = None
    stop_on_eos: Optional[bool] = None  # None = stop at the model's EOS (benchmarks pin full lengths)
    # sampling penalties and min-p (local engines; the stub and the hosted providers ignore them)
    min_p: Optional[float] = None
    repetition_penalty: Optional[float] = None
    presence_penalty: Optional[float] = None
    frequency_penalty: Optional[float] = None
    # token log-probabilities (local engines): None = off, n in [0, 20] = the sampled token's raw
    # log-probability and the n most likely ids of every step (``Response.logprobs``)
    logprobs: Optional[int] = None


MAX_LOGPROBS = 20


def check_sampling(min_p=None, repetition_penalty=None, presence_penalty=None, frequency_penalty=None,
                   logprobs=None) -> None:
    """Raise ValueError("<name>: <why>") for a value no engine may see (``None`` = not given)."""
    def num(name, v):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"{name}: expected a finite number, got {v!r}")

    if min_p is not None:
        num("min_p", min_p)
        if not 0.0 <= min_p <= 1.0:
            raise ValueError(f"min_p: expected a value in [0, 1], got {min_p!r}")
    if repetition_penalty is not None:
        num("repetition_penalty", repetition_penalty)
        if not repetition_penalty > 0.0:
            raise ValueError(f"repetition_penalty: expected a value above 0, got {repetition_penalty!r}")
    if presence_penalty is not None:
        num("presence_penalty", presence_penalty)
    if frequency_penalty is not None:
        num("frequency_penalty", frequency_penalty)
    if logprobs is not None:
        if isinstance(logprobs, bool) or not isinstance(logprobs, int):
            raise ValueError(f"logprobs: expected an integer, got {logprobs!r}")
        if not 0 <= logprobs <= MAX_LOGPROBS:
            raise ValueError(f"logprobs: expected a value in [0, {MAX_LOGPROBS}], got {logprobs!r}")


@dataclasses.dataclass
class Response:
    model: str = ""
    content: str = ""
    provider: str = ""
    latency_ns: int = 0
    # Non-schema statistics (not serialised into result.json).
    prompt_tokens: int = 0
    output_tokens: int = 0
    ttft_ns: int = 0
    # None unless the request asked for ``logprobs``: one {"id", "token", "logprob", "top": [{"id",
    # "token", "logprob"}, ...]} per output token (raw values: before penalties, temperature, truncation)
    logprobs: Optional[list] = None

    @property
    def latency_ms(self) -> int:
        return self.latency_ns // 1_000_000

    @property
    def latency_s(self) -> float:
        return self.latency_ns / 1e9


class Provider(Protocol):
    def query(self, ctx: Context, req: Request) -> Response: ...

    def query_stream(self, ctx: Context, req: Request, callback: Optional[StreamCallback]) -> Response: ...


class FuncProvider:
    """Adapter turning ``fn(ctx, req) -> Response`` into a Provider (``provider.go:37-55``)."""

    def __init__(self, fn: Callable[[Context, Request], Response]):
        self._fn = fn

    def query(self, ctx: Context, req: Request) -> Response:
        return self._fn(ctx, req)

    def query_stream(self, ctx: Context, req: Request, callback: Optional[StreamCallback]) -> Response:
        resp = self._fn(ctx, req)
        if callback is not None:
            callback(resp.content)
        return resp
