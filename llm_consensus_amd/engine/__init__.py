from .engine import (Engine, EngineConfig, EngineError, GraphKey, SamplingForm, SamplingParams,  # noqa: F401
                     Sequence)
