"""Model configurations for the tutoring LLM (GPT-2 family) and the relevance gate (BERT).

The reference loads ``gpt2`` (124M) in ``tutoring_server.py:10-12`` and
``bert-base-uncased`` in ``lms_server.py:1258-1260``.  There is no network on the
build/GPU boxes, so weights are random-initialised (seeded) with the same
architecture, or loaded from a local safetensors file when one is supplied.
"""
from __future__ import annotations

from dataclasses import dataclass, asdict, field


@dataclass(frozen=True)
class GPT2Config:
    name: str = "gpt2"
    n_layer: int = 12
    n_embd: int = 768
    n_head: int = 12
    n_positions: int = 1024
    vocab_size: int = 50257
    layer_norm_epsilon: float = 1e-5
    eos_token_id: int = 50256
    initializer_range: float = 0.02

    @property
    def head_dim(self) -> int:
        return self.n_embd // self.n_head

    @property
    def n_inner(self) -> int:
        return 4 * self.n_embd

    @property
    def vocab_padded(self) -> int:
        # Padded to a multiple of 64 so the LM-head GEMM tiles evenly (50257 -> 50304).  (A
        # 256-multiple for 256x256 LM-head tiles measured 1 % slower in situ: profiles/r1_lmhead_256_ab.log)
        return (self.vocab_size + 63) // 64 * 64

    def kv_bytes_per_token(self, dtype_bytes: int = 2) -> int:
        return 2 * self.n_layer * self.n_embd * dtype_bytes

    def num_params(self) -> int:
        d, L, V, P = self.n_embd, self.n_layer, self.vocab_size, self.n_positions
        per_layer = 4 * d + (d * 3 * d + 3 * d) + (d * d + d) + (d * 4 * d + 4 * d) + (4 * d * d + d)
        return V * d + P * d + L * per_layer + 2 * d

    def to_dict(self) -> dict:
        return asdict(self)


GPT2_CONFIGS = {
    "gpt2": GPT2Config("gpt2", 12, 768, 12),
    "gpt2-small": GPT2Config("gpt2", 12, 768, 12),
    "gpt2-medium": GPT2Config("gpt2-medium", 24, 1024, 16),
    "gpt2-large": GPT2Config("gpt2-large", 36, 1280, 20),
    "gpt2-xl": GPT2Config("gpt2-xl", 48, 1600, 25),
    # tiny config for unit tests (fast on CPU, still exercises every code path)
    "gpt2-tiny": GPT2Config("gpt2-tiny", 2, 128, 2, n_positions=256, vocab_size=1000, eos_token_id=999),
}


def gpt2_config(name: str) -> GPT2Config:
    try:
        return GPT2_CONFIGS[name]
    except KeyError as e:
        raise ValueError(f"unknown GPT-2 config {name!r}; choose from {sorted(GPT2_CONFIGS)}") from e


@dataclass(frozen=True)
class BertConfig:
    name: str = "bert-base-uncased"
    n_layer: int = 12
    hidden: int = 768
    n_head: int = 12
    intermediate: int = 3072
    vocab_size: int = 30522
    max_position: int = 512
    type_vocab_size: int = 2
    layer_norm_eps: float = 1e-12
    pad_token_id: int = 0
    cls_token_id: int = 101
    sep_token_id: int = 102
    initializer_range: float = 0.02

    @property
    def head_dim(self) -> int:
        return self.hidden // self.n_head


BERT_CONFIGS = {
    "bert-base-uncased": BertConfig(),
    "bert-tiny": BertConfig("bert-tiny", 2, 128, 2, 512, vocab_size=1000, max_position=128),
}


def bert_config(name: str) -> BertConfig:
    try:
        return BERT_CONFIGS[name]
    except KeyError as e:
        raise ValueError(f"unknown BERT config {name!r}; choose from {sorted(BERT_CONFIGS)}") from e


SAMPLING_MAX_TOP_K = 256  # candidates the device sampler ranks per row (ops/csrc/sample.hip)


@dataclass(frozen=True)
class SamplingParams:
    """Seeded temperature / top-k / top-p sampling (HF's warper order: temperature, top-k, then
    top-p with ``min_tokens_to_keep=1``).  The draw of a token depends only on ``seed``, the
    request's stream id and the token's position (Philox4x32-10), never on the batch around it."""

    temperature: float = 0.7
    top_k: int = 50
    top_p: float = 0.9
    seed: int = 0

    def __post_init__(self):
        import math

        t, k, p, s = self.temperature, self.top_k, self.top_p, self.seed
        if isinstance(t, bool) or not isinstance(t, (int, float)) or not math.isfinite(t) or not t > 0:
            raise ValueError(f"temperature {t!r}: a finite number > 0")
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= SAMPLING_MAX_TOP_K:
            raise ValueError(f"top_k {k!r}: an integer in [1, {SAMPLING_MAX_TOP_K}]")
        if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0 < p <= 1:
            raise ValueError(f"top_p {p!r}: a number in (0, 1]")
        if isinstance(s, bool) or not isinstance(s, int) or not 0 <= s < 2 ** 64:
            raise ValueError(f"seed {s!r}: an integer in [0, 2^64)")

    @property
    def shape_key(self) -> tuple:
        """What a captured graph bakes in (the seed is a device word, not part of it)."""
        return (float(self.temperature), int(self.top_k), float(self.top_p))


CONTROLS_MAX_STOP = 4       # stop sequences per GenerationControls (ops/csrc/decode.hip STOP_MAX_SEQS)
CONTROLS_MAX_STOP_LEN = 8   # tokens per stop sequence (STOP_MAX_LEN)


@dataclass(frozen=True)
class GenerationControls:
    """Opt-in generation controls beside the repetition penalty, with HF's semantics
    (``NoRepeatNGramLogitsProcessor``, ``MinNewTokensLengthLogitsProcessor``, stop sequences on
    token ids); the definition is in ``ops/csrc/controls.hip`` and, in Python,
    ``models.gpt2.banned_tokens`` / ``stop_hit``.

    ``no_repeat_ngram_size`` n (0: off): no n-gram occurs twice in a sequence (prompt included).
    ``min_new_tokens``: EOS is banned until that many tokens have been generated.
    ``stop``: up to ``CONTROLS_MAX_STOP`` token sequences of 1 .. ``CONTROLS_MAX_STOP_LEN`` ids; a row
    finishes once its generated tokens end with one of them (the stop tokens stay in the output)."""

    no_repeat_ngram_size: int = 0
    min_new_tokens: int = 0
    stop: tuple = ()

    def __post_init__(self):
        n, m, stop = self.no_repeat_ngram_size, self.min_new_tokens, self.stop
        if isinstance(n, bool) or not isinstance(n, int) or n < 0:
            raise ValueError(f"no_repeat_ngram_size {n!r}: an integer >= 0 (0: off)")
        if isinstance(m, bool) or not isinstance(m, int) or m < 0:
            raise ValueError(f"min_new_tokens {m!r}: an integer >= 0")
        if isinstance(stop, (str, bytes)) or not isinstance(stop, (tuple, list)):
            raise ValueError(f"stop {stop!r}: a tuple of token-id tuples")
        if len(stop) > CONTROLS_MAX_STOP:
            raise ValueError(f"stop: at most {CONTROLS_MAX_STOP} sequences, got {len(stop)}")
        norm = []
        for s in stop:
            if isinstance(s, (str, bytes)) or not isinstance(s, (tuple, list)):
                raise ValueError(f"stop sequence {s!r}: a tuple of token ids")
            if not 1 <= len(s) <= CONTROLS_MAX_STOP_LEN:
                raise ValueError(f"stop sequence {s!r}: 1 .. {CONTROLS_MAX_STOP_LEN} token ids")
            for t in s:
                if isinstance(t, bool) or not isinstance(t, int) or not 0 <= t < 2 ** 31:
                    raise ValueError(f"stop sequence {s!r}: token ids are integers in [0, 2^31)")
            norm.append(tuple(s))
        object.__setattr__(self, "stop", tuple(norm))

    @property
    def bans(self) -> bool:
        """Whether tokens are banned (the LM head then writes f32 logits for ``logit_bans``)."""
        return self.no_repeat_ngram_size > 0 or self.min_new_tokens > 0

    @property
    def shape_key(self) -> tuple:
        """What a captured graph bakes in: all of it."""
        return ("ctl", self.no_repeat_ngram_size, self.min_new_tokens, self.stop)


@dataclass
class GenerationConfig:
    """Decode semantics of the reference ``model.generate`` call (tutoring_server.py:21-29).

    ``do_sample`` is unset there, so decoding is greedy by default.  With ``do_sample`` set,
    ``sampling()`` gives the ``SamplingParams`` (``temperature``/``top_k``/``top_p`` and
    ``seed``) that the engines, the scheduler and the tutor server take as ``sampling=``.
    ``controls()`` gives the ``GenerationControls`` (``no_repeat_ngram_size``, ``min_new_tokens``,
    ``stop``) they take as ``controls=``, or None when all three are off.  ``logprobs``: generation
    returns the chosen tokens' log-probabilities beside the tokens (``logprobs=True`` there).
    """

    max_length: int = 150  # total length, prompt included
    repetition_penalty: float = 1.2
    do_sample: bool = False
    temperature: float = 0.7
    top_k: int = 50
    top_p: float = 0.9
    eos_token_id: int | None = None
    extra: dict = field(default_factory=dict)
    seed: int = 0

    def sampling(self) -> "SamplingParams | None":
        if not self.do_sample:
            return None
        return SamplingParams(self.temperature, self.top_k, self.top_p, self.seed)

    no_repeat_ngram_size: int = 0
    min_new_tokens: int = 0
    stop: tuple = ()
    logprobs: bool = False

    def controls(self) -> "GenerationControls | None":
        if not (self.no_repeat_ngram_size or self.min_new_tokens or self.stop):
            return None
        return GenerationControls(self.no_repeat_ngram_size, self.min_new_tokens, tuple(self.stop))
