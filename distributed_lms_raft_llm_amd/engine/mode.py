"""What a GPT-2 engine shape cannot serve, and the generation mode of one engine call.

Pure Python (no torch): the tutor server checks its flags with these before it builds an engine."""
from __future__ import annotations

from dataclasses import dataclass

from ..models.config import GenerationControls, SamplingParams

# feature -> (subject, why not under tensor parallelism, why not with fp8 weights, what to serve instead)
_UNSUPPORTED = {
    "sampling": ("sampling is", "the device sampler ranks one rank's whole vocabulary",
                 "the fp8 LM head has no f32-logits epilogue", "greedy"),
    "kv_fp8": ("the fp8 KV cache is", "the TP-fused decode path has no fp8-cache build",
               "the W8A8 QKV GEMM has no fp8-cache epilogue", "kv_dtype='bf16'"),
    "prefix": ("the prompt-prefix cache is", "the prefix store and its fill are built for one rank's whole cache",
               "the suffix-only prefill is verified on the bf16 GEMMs only", "prefix_capacity=0"),
    "controls": ("generation controls are", "the device bans work on one rank's whole vocabulary",
                 "the fp8 LM head has no f32-logits epilogue for the bans", "without controls"),
    "logprobs": ("log-probabilities are", "the device log-softmax reduces one rank's whole vocabulary",
                 "the fp8 LM head has no f32-logits epilogue to take them from", "without logprobs"),
}


def _unsupported(feature: str, what: str):
    subject, tp_why, fp8_why, instead = _UNSUPPORTED[feature]

    def why(tp_size: int, fp8_weights: bool) -> str | None:
        if tp_size > 1:
            return f"{subject} not supported with tensor parallelism (tp_size > 1): {tp_why}; serve {instead} or TP=1"
        if fp8_weights:
            return f"{subject} not supported with fp8 weights: {fp8_why}; serve {instead} or weight_dtype='bf16'"
        return None

    why.__name__ = why.__qualname__ = f"{feature}_unsupported"
    why.__doc__ = f"Why an engine of this shape cannot {what} (None: it can)."
    return why


sampling_unsupported = _unsupported("sampling", "sample")
kv_fp8_unsupported = _unsupported("kv_fp8", "hold an fp8 (e4m3) KV cache")
prefix_unsupported = _unsupported("prefix", "keep a prompt-prefix cache")
controls_unsupported = _unsupported("controls", "serve ``GenerationControls``")
logprobs_unsupported = _unsupported("logprobs", "return log-probabilities")

# greedy decoding through the sampler (bans, log-probabilities): its definition at top_k = 1, the
# largest unbanned key
GREEDY_AS_SAMPLING = SamplingParams(1.0, 1, 1.0, 0)


@dataclass(frozen=True)
class DecodeMode:
    """The generation mode of one public engine call: what its LM heads, updates, prefills and
    captured graphs depend on beyond their shapes.  The default is the greedy decode, exactly the
    calls made without any of the three."""

    sampling: SamplingParams | None = None
    controls: GenerationControls | None = None
    logprobs: bool = False

    @property
    def sampler(self) -> SamplingParams | None:
        """What the LM head's sampler runs with on f32 logits; None: the fused-argmax heads."""
        if self.sampling is not None:
            return self.sampling
        return GREEDY_AS_SAMPLING if self.bans or self.logprobs else None

    @property
    def bans(self) -> GenerationControls | None:
        """The controls when they ban tokens (-inf between the logits and the sampler), else None."""
        return self.controls if self.controls is not None and self.controls.bans else None

    @property
    def stop(self) -> tuple:
        """The stop sequences the update finishes a row at (empty: none)."""
        return self.controls.stop if self.controls is not None else ()

    @property
    def records_prompt_len(self) -> bool:
        """The prompts' lengths: what min_new_tokens and the stops count from, and where a slot's
        log-probabilities begin."""
        return self.controls is not None or self.logprobs

    @property
    def graph_key(self) -> tuple:
        """What a captured graph bakes in of the mode (the seed is a device word: not part of it)."""
        key = () if self.sampling is None else self.sampling.shape_key
        if self.controls is not None:
            key = key + self.controls.shape_key
        return key + ("logprobs",) if self.logprobs else key

    @property
    def dataflow_ok(self) -> bool:
        """The dataflow decode kernel's LM head is greedy, its commit block knows no controls, and it
        never materialises logits: launch-per-op serves every other mode."""
        return self.sampling is None and self.controls is None and not self.logprobs

    def check(self, tp_size: int, fp8_weights: bool) -> None:
        """``TypeError`` for a field of the wrong type, ``ValueError`` where an engine of this shape
        cannot serve the mode."""
        why = logprobs_unsupported(tp_size, fp8_weights) if self.logprobs else None
        if why:
            raise ValueError(why)
        if self.controls is not None:
            if not isinstance(self.controls, GenerationControls):
                raise TypeError("controls: a GenerationControls (models/config.py) or None")
            why = controls_unsupported(tp_size, fp8_weights)
            if why:
                raise ValueError(why)
        if self.sampling is not None:
            if not isinstance(self.sampling, SamplingParams):
                raise TypeError("sampling: a SamplingParams (models/config.py) or None")
            why = sampling_unsupported(tp_size, fp8_weights)
            if why:
                raise ValueError(why)
