"""GPT-2 weights + a plain-PyTorch reference implementation.

This module is the CPU path (BASELINE config 1, "plumbing, no GPU") and the fp32
oracle that the HIP engine (``engine/gpt2_engine.py``) is checked against.

Parity target: ``GPT2LMHeadModel.generate(max_length=150, repetition_penalty=1.2)``
with ``do_sample`` unset, i.e. greedy decoding with a CTRL-style penalty
(``tutoring_server.py:21-29``).

Weights are held in the HF ``Conv1D`` layout ([in, out]) under the HF key names so
that ``transformers`` checkpoints (safetensors) load unchanged and the oracle tests
can push the same tensors into ``transformers.GPT2LMHeadModel``.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

from .config import GPT2Config


def gelu_new(x: torch.Tensor) -> torch.Tensor:
    # GPT-2's tanh-approximated GELU ("gelu_new").
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * torch.pow(x, 3.0))))


def init_gpt2_weights(cfg: GPT2Config, seed: int = 0, dtype=torch.float32) -> dict[str, torch.Tensor]:
    """Seeded random init with GPT-2's initializer (normal(0, 0.02); residual projections
    scaled by 1/sqrt(2L); LayerNorm = (1, 0)).  Returns HF-named tensors."""
    g = torch.Generator().manual_seed(seed)
    d, L, std = cfg.n_embd, cfg.n_layer, cfg.initializer_range
    proj_std = std / math.sqrt(2 * L)

    def normal(*shape, s=std):
        return (torch.randn(*shape, generator=g) * s).to(dtype)

    w: dict[str, torch.Tensor] = {
        "transformer.wte.weight": normal(cfg.vocab_size, d),
        "transformer.wpe.weight": normal(cfg.n_positions, d, s=0.01),
        "transformer.ln_f.weight": torch.ones(d, dtype=dtype),
        "transformer.ln_f.bias": torch.zeros(d, dtype=dtype),
    }
    for i in range(L):
        p = f"transformer.h.{i}."
        w[p + "ln_1.weight"] = torch.ones(d, dtype=dtype)
        w[p + "ln_1.bias"] = torch.zeros(d, dtype=dtype)
        w[p + "attn.c_attn.weight"] = normal(d, 3 * d)
        w[p + "attn.c_attn.bias"] = torch.zeros(3 * d, dtype=dtype)
        w[p + "attn.c_proj.weight"] = normal(d, d, s=proj_std)
        w[p + "attn.c_proj.bias"] = torch.zeros(d, dtype=dtype)
        w[p + "ln_2.weight"] = torch.ones(d, dtype=dtype)
        w[p + "ln_2.bias"] = torch.zeros(d, dtype=dtype)
        w[p + "mlp.c_fc.weight"] = normal(d, 4 * d)
        w[p + "mlp.c_fc.bias"] = torch.zeros(4 * d, dtype=dtype)
        w[p + "mlp.c_proj.weight"] = normal(4 * d, d, s=proj_std)
        w[p + "mlp.c_proj.bias"] = torch.zeros(d, dtype=dtype)
    return w


def perturb_norms_and_biases(w: dict[str, torch.Tensor], seed: int = 1, scale: float = 0.02) -> None:
    """Give LN gains/biases and linear biases non-trivial values so kernel tests
    exercise the affine/bias paths (an all-ones/zeros init would hide bugs)."""
    g = torch.Generator().manual_seed(seed)
    for k, v in w.items():
        if k.endswith(".bias") or (("ln_" in k) and k.endswith(".weight")):
            v.add_(torch.randn(v.shape, generator=g).to(v.dtype) * scale)


def load_safetensors_weights(path: str) -> dict[str, torch.Tensor]:
    from safetensors.torch import load_file

    raw = load_file(path)
    out = {}
    for k, v in raw.items():
        key = k if k.startswith("transformer.") or k.startswith("lm_head") else "transformer." + k
        out[key] = v.float()
    return out


@dataclass
class KVCache:
    """Contiguous per-slot KV cache for the reference path: [L, 2, B, H, Tmax, hd]."""

    data: torch.Tensor

    @classmethod
    def allocate(cls, cfg: GPT2Config, batch: int, max_len: int, dtype=torch.float32, device="cpu"):
        return cls(torch.zeros(cfg.n_layer, 2, batch, cfg.n_head, max_len, cfg.head_dim, dtype=dtype, device=device))


class GPT2Reference:
    """Plain-torch GPT-2 forward with a KV cache (batch, ragged prompt lengths)."""

    def __init__(self, cfg: GPT2Config, weights: dict[str, torch.Tensor], device="cpu", dtype=torch.float32,
                 kv_dtype: str = "bf16", act_dtype=None):
        """``kv_dtype="fp8"``: the model of the engines' fp8 KV cache -- k and v pass through
        ``quantize_kv_e4m3`` (and back to ``dtype``) where they are written into the cache, so every
        attention read sees the quantised values.  The default writes them as they are (the fp32
        oracle of the bf16-cache engines).
        ``act_dtype`` (measurement only, ``kv_fp8_margin``): round the activations a bf16 engine
        rounds (LN outputs, q, attention output, GELU output, final hidden) to that dtype."""
        if kv_dtype not in ("bf16", "fp8"):
            raise ValueError(f"kv_dtype {kv_dtype!r}: bf16 or fp8")
        self.cfg = cfg
        self.device = torch.device(device)
        self.dtype = dtype
        self.kv_dtype = kv_dtype
        self.act_dtype = act_dtype
        self.w = {k: v.to(device=self.device, dtype=dtype) for k, v in weights.items()}

    def _act(self, t: torch.Tensor) -> torch.Tensor:
        return t if self.act_dtype is None else t.to(self.act_dtype).to(t.dtype)

    def _ln(self, x, name):
        return torch.nn.functional.layer_norm(
            x, (self.cfg.n_embd,), self.w[name + ".weight"], self.w[name + ".bias"], self.cfg.layer_norm_epsilon
        )

    def forward(self, tokens: torch.Tensor, positions: torch.Tensor, cache: KVCache, rows: torch.Tensor) -> torch.Tensor:
        """Run ``tokens`` [B, S] at ``positions`` [B, S] for cache rows ``rows`` [B].

        Keys at cache positions ``<= position`` are attended (causal); returns the
        final hidden state after ``ln_f`` as [B, S, d].
        """
        cfg = self.cfg
        B, S = tokens.shape
        H, hd, d = cfg.n_head, cfg.head_dim, cfg.n_embd
        x = self.w["transformer.wte.weight"][tokens] + self.w["transformer.wpe.weight"][positions]
        Tmax = cache.data.shape[4]
        key_pos = torch.arange(Tmax, device=self.device)
        mask = key_pos[None, None, :] <= positions[:, :, None]  # [B, S, Tmax]
        bidx = rows[:, None].expand(B, S)
        for i in range(cfg.n_layer):
            p = f"transformer.h.{i}."
            h = self._act(self._ln(x, p + "ln_1"))
            qkv = h @ self.w[p + "attn.c_attn.weight"] + self.w[p + "attn.c_attn.bias"]
            q, k, v = qkv.split(d, dim=-1)
            q = self._act(q).view(B, S, H, hd)
            k = k.view(B, S, H, hd)
            v = v.view(B, S, H, hd)
            if self.kv_dtype == "fp8":
                k = quantize_kv_e4m3(k).to(x.dtype)
                v = quantize_kv_e4m3(v).to(x.dtype)
            elif self.act_dtype is not None:  # (measurement only) the bf16 cache of a bf16 engine
                k, v = self._act(k), self._act(v)
            cache.data[i, 0, bidx, :, positions] = k.to(cache.data.dtype)
            cache.data[i, 1, bidx, :, positions] = v.to(cache.data.dtype)
            K = cache.data[i, 0, rows].to(x.dtype)  # [B, H, Tmax, hd]
            V = cache.data[i, 1, rows].to(x.dtype)
            att = torch.einsum("bshd,bhtd->bhst", q, K) / math.sqrt(hd)
            att = att.masked_fill(~mask[:, None, :, :], float("-inf"))
            att = torch.softmax(att, dim=-1)
            a = self._act(torch.einsum("bhst,bhtd->bshd", att, V).reshape(B, S, d))
            x = x + a @ self.w[p + "attn.c_proj.weight"] + self.w[p + "attn.c_proj.bias"]
            h = self._act(self._ln(x, p + "ln_2"))
            f = self._act(gelu_new(h @ self.w[p + "mlp.c_fc.weight"] + self.w[p + "mlp.c_fc.bias"]))
            x = x + f @ self.w[p + "mlp.c_proj.weight"] + self.w[p + "mlp.c_proj.bias"]
        return self._act(self._ln(x, "transformer.ln_f"))

    def logits(self, hidden: torch.Tensor) -> torch.Tensor:
        return hidden @ self.w["transformer.wte.weight"].t()


def apply_repetition_penalty(logits: torch.Tensor, seen: torch.Tensor, penalty: float) -> torch.Tensor:
    """CTRL-style penalty (HF ``RepetitionPenaltyLogitsProcessor``): for every id already
    in the sequence, ``l < 0 ? l * p : l / p``.  ``seen`` is a bool mask [B, V]."""
    if penalty == 1.0:
        return logits
    pen = torch.where(logits < 0, logits * penalty, logits / penalty)
    return torch.where(seen, pen, logits)


@torch.no_grad()
def reference_generate(
    model: GPT2Reference,
    prompts: list[list[int]],
    max_length: int = 150,
    repetition_penalty: float = 1.2,
    eos_token_id: int | None = None,
    sampling=None,
    streams: list[int] | None = None,
    controls=None,
) -> list[list[int]]:
    """Batched greedy + repetition-penalty decode.  Returns full sequences (prompt
    echoed, as ``generate`` does), each stopping at EOS (inclusive) or ``max_length``.
    ``sampling`` (a ``SamplingParams``): every token is drawn by ``reference_sample`` instead, row b
    with stream id ``streams[b]`` (default b) at position = the index the token is written to.
    ``controls`` (a ``GenerationControls``): the logits of ``banned_tokens`` become -inf ahead of the
    penalty, and a row also stops once ``stop_hit``."""
    cfg = model.cfg
    eos = cfg.eos_token_id if eos_token_id is None else eos_token_id
    B = len(prompts)
    dev = model.device
    cache = KVCache.allocate(cfg, B, max_length, dtype=model.dtype, device=dev)
    rows = torch.arange(B, device=dev)
    seqs = [list(p) for p in prompts]
    seen = torch.zeros(B, cfg.vocab_size, dtype=torch.bool, device=dev)
    for b, p in enumerate(prompts):
        seen[b, torch.tensor(p, device=dev)] = True
    done = [len(p) >= max_length for p in prompts]
    # prefill each prompt (ragged lengths: run per-length groups padded on the right)
    maxp = max(len(p) for p in prompts)
    toks = torch.zeros(B, maxp, dtype=torch.long, device=dev)
    pos = torch.zeros(B, maxp, dtype=torch.long, device=dev)
    for b, p in enumerate(prompts):
        toks[b, : len(p)] = torch.tensor(p, device=dev)
        # pad positions repeat the last real position so they overwrite it with
        # identical k/v (harmless) instead of polluting later slots
        pos[b, : len(p)] = torch.arange(len(p), device=dev)
        pos[b, len(p):] = len(p) - 1
        toks[b, len(p):] = p[-1]
    hidden = model.forward(toks, pos, cache, rows)
    last = torch.tensor([len(p) - 1 for p in prompts], device=dev)
    h_last = hidden[rows, last]
    while True:
        logits = model.logits(h_last)
        if controls is not None and controls.bans:
            for b in range(B):
                if not done[b]:
                    ban = banned_tokens(seqs[b], len(prompts[b]), controls, eos)
                    if ban:
                        logits[b, torch.tensor(ban, device=dev)] = float("-inf")
        if sampling is None:
            nxt = torch.argmax(apply_repetition_penalty(logits, seen, repetition_penalty), dim=-1)
        else:
            z, sn = logits.float().cpu().numpy(), seen.cpu().numpy()
            nxt = [0 if done[b] else reference_sample(z[b], sn[b], repetition_penalty, sampling,
                                                      b if streams is None else streams[b], len(seqs[b]))[0]
                   for b in range(B)]
        for b in range(B):
            if done[b]:
                continue
            t = int(nxt[b])
            seqs[b].append(t)
            seen[b, t] = True
            if t == eos or len(seqs[b]) >= max_length:
                done[b] = True
            elif controls is not None and stop_hit(seqs[b], len(prompts[b]), controls.stop):
                done[b] = True
        if all(done):
            break
        cur_pos = torch.tensor([min(len(s) - 1, max_length - 1) for s in seqs], device=dev)
        cur_tok = torch.tensor([s[-1] for s in seqs], device=dev)
        hidden = model.forward(cur_tok[:, None], cur_pos[:, None], cache, rows)
        h_last = hidden[:, 0]
    return seqs


# ---------------------------------------------------------------------------------------------
# Generation controls: the normative Python definition (ops/csrc/controls.hip has the same text)
# ---------------------------------------------------------------------------------------------
def banned_tokens(seq, prompt_len: int, controls, eos: int) -> list[int]:
    """The token ids whose logit is -inf for the next token of ``seq`` (prompt of ``prompt_len``
    tokens included), sorted.  With L = len(seq) and n = ``controls.no_repeat_ngram_size``: if
    n > 0 and L + 1 >= n, ``seq[i+n-1]`` for every 0 <= i <= L-n with
    ``seq[i : i+n-1] == seq[L-n+1 : L]`` (n = 1: every token of ``seq``) -- HF's
    ``NoRepeatNGramLogitsProcessor``; and ``eos`` while ``L - prompt_len < controls.min_new_tokens``
    -- HF's ``MinNewTokensLengthLogitsProcessor``."""
    seq = [int(t) for t in seq]
    L, n = len(seq), int(controls.no_repeat_ngram_size)
    ban = set()
    if n > 0 and L + 1 >= n:
        tail = seq[L - n + 1: L]
        for i in range(L - n + 1):
            if seq[i: i + n - 1] == tail:
                ban.add(seq[i + n - 1])
    if L - int(prompt_len) < int(controls.min_new_tokens):
        ban.add(int(eos))
    return sorted(ban)


def stop_hit(seq, prompt_len: int, stop) -> bool:
    """Whether ``seq``, whose last token was just written at index p = len(seq) - 1, ends with one of
    the ``stop`` sequences wholly inside its generated part: for some s of length m,
    ``p + 1 - m >= prompt_len`` and ``seq[p+1-m : p+1] == s``."""
    L = len(seq)
    for s in stop:
        m = len(s)
        if m and L - m >= prompt_len and [int(t) for t in seq[L - m:]] == [int(t) for t in s]:
            return True
    return False


def _controls_rows(logits: torch.Tensor, seq: list[int], prompt_len: int, repetition_penalty: float, controls,
                   eos: int, eps: float) -> dict:
    """The margin rule on the oracle's ``logits`` rows (row j predicts ``seq[prompt_len + j]``)
    with the bans of ``controls`` applied at each position."""
    n = logits.shape[0]
    dev = logits.device
    logits = logits.clone()
    seen = torch.zeros(n, logits.shape[1], dtype=torch.bool, device=dev)
    banned_got = []
    for j in range(n):
        seen[j, torch.tensor(seq[: prompt_len + j], device=dev)] = True
        if controls is not None and controls.bans:
            ban = banned_tokens(seq[: prompt_len + j], prompt_len, controls, eos)
            if ban:
                logits[j, torch.tensor(ban, device=dev)] = float("-inf")
            if seq[prompt_len + j] in ban:
                banned_got.append(prompt_len + j)
    logits = apply_repetition_penalty(logits, seen, repetition_penalty)
    top = logits.topk(2, dim=-1)
    margin = (top.values[:, 0] - top.values[:, 1]).tolist()
    want = top.indices[:, 0].tolist()
    out = {"positions": n, "decisive": 0, "mismatches": [], "min_margin": min(margin)}
    for j in range(n):
        got = seq[prompt_len + j]
        if prompt_len + j in banned_got:  # whatever the margin: no sampler may pick a banned token
            out["mismatches"].append((prompt_len + j, got, want[j], float("inf")))
        if margin[j] > eps:
            out["decisive"] += 1
            if got != want[j] and prompt_len + j not in banned_got:
                out["mismatches"].append((prompt_len + j, got, want[j], margin[j]))
    return out


@torch.no_grad()
def teacher_forced_controls_check(model: GPT2Reference, seq: list[int], prompt_len: int,
                                  repetition_penalty: float = 1.2, controls=None, eps: float = 0.05,
                                  eos_token_id: int | None = None) -> dict:
    """``teacher_forced_check`` for a greedy sequence generated under ``controls``: the bans of
    ``banned_tokens`` are applied to the oracle's logits at each position (-inf ahead of the
    penalty); a position is decisive when top-1 minus top-2 among the unbanned penalised logits
    exceeds ``eps``, and there the token must be the oracle's choice.  A banned token in ``seq`` is a
    mismatch at any margin.  Same result dict."""
    return teacher_forced_controls_check_batch(model, [seq], [prompt_len], repetition_penalty, controls, eps,
                                               eos_token_id=eos_token_id)[0]


@torch.no_grad()
def teacher_forced_controls_check_batch(model: GPT2Reference, seqs: list[list[int]], prompt_lens: list[int],
                                        repetition_penalty: float = 1.2, controls=None, eps: float = 0.05,
                                        chunk: int = 16, eos_token_id: int | None = None) -> list[dict]:
    """``teacher_forced_controls_check`` for many sequences (one padded forward per ``chunk`` rows, as
    ``teacher_forced_check_batch`` runs it)."""
    cfg, dev = model.cfg, model.device
    eos = cfg.eos_token_id if eos_token_id is None else eos_token_id
    out: list[dict] = []
    for c0 in range(0, len(seqs), chunk):
        rows = seqs[c0: c0 + chunk]
        pls = prompt_lens[c0: c0 + chunk]
        Bc = len(rows)
        S = max(len(s) for s in rows)
        toks = torch.tensor([s + [s[-1]] * (S - len(s)) for s in rows], device=dev)
        pos = torch.arange(S, device=dev)[None].expand(Bc, S).contiguous()
        cache = KVCache.allocate(cfg, Bc, S, dtype=model.dtype, device=dev)
        hidden = model.forward(toks, pos, cache, torch.arange(Bc, device=dev))
        for b, (s, pl) in enumerate(zip(rows, pls)):
            if len(s) <= pl:
                out.append({"positions": 0, "decisive": 0, "mismatches": [], "min_margin": float("inf")})
                continue
            out.append(_controls_rows(model.logits(hidden[b, pl - 1: len(s) - 1]), s, pl, repetition_penalty,
                                      controls, eos, eps))
    return out


@torch.no_grad()
def teacher_forced_check(model: GPT2Reference, seq: list[int], prompt_len: int, repetition_penalty: float = 1.2,
                         eps: float = 0.05) -> dict:
    """Margin-aware exactness oracle for a generated sequence: run the fp32 reference once over
    ``seq`` (teacher forcing), and at every generated position compare the produced token with the
    reference's greedy choice under the repetition penalty of the prefix.  A position is
    *decisive* when the reference's top-1 minus top-2 penalised logit exceeds ``eps``; at every
    decisive position the token must be the reference's argmax.

    Returns {"positions", "decisive", "mismatches": [(i, got, want, margin)], "min_margin"}."""
    cfg = model.cfg
    dev = model.device
    S = len(seq)
    if S <= prompt_len:
        return {"positions": 0, "decisive": 0, "mismatches": [], "min_margin": float("inf")}
    cache = KVCache.allocate(cfg, 1, S, dtype=model.dtype, device=dev)
    toks = torch.tensor([seq], device=dev)
    pos = torch.arange(S, device=dev)[None]
    hidden = model.forward(toks, pos, cache, torch.zeros(1, dtype=torch.long, device=dev))[0]
    logits = model.logits(hidden[prompt_len - 1: S - 1])  # row j predicts seq[prompt_len + j]
    n = logits.shape[0]
    seen = torch.zeros(n, cfg.vocab_size, dtype=torch.bool, device=dev)
    for j in range(n):
        seen[j, torch.tensor(seq[: prompt_len + j], device=dev)] = True
    logits = apply_repetition_penalty(logits, seen, repetition_penalty)
    top = logits.topk(2, dim=-1)
    margin = (top.values[:, 0] - top.values[:, 1]).tolist()
    want = top.indices[:, 0].tolist()
    out = {"positions": n, "decisive": 0, "mismatches": [], "min_margin": min(margin)}
    for j in range(n):
        got = seq[prompt_len + j]
        if margin[j] > eps:
            out["decisive"] += 1
            if got != want[j]:
                out["mismatches"].append((prompt_len + j, got, want[j], margin[j]))
    return out


@torch.no_grad()
def teacher_forced_check_batch(model: GPT2Reference, seqs: list[list[int]], prompt_lens: list[int],
                               repetition_penalty: float = 1.2, eps: float = 0.05, chunk: int = 16) -> list[dict]:
    """``teacher_forced_check`` for many sequences at once (chunks of ``chunk`` rows, each padded on
    the right: causal attention keeps the padding out of every checked position).  The penalty
    mask of position j of a row is "first occurrence of v < prompt_len + j", built by one
    scatter-min instead of a loop of small launches.  Same result dicts, in order."""
    cfg, dev = model.cfg, model.device
    out: list[dict] = []
    for c0 in range(0, len(seqs), chunk):
        rows = seqs[c0: c0 + chunk]
        pls = prompt_lens[c0: c0 + chunk]
        Bc = len(rows)
        S = max(len(s) for s in rows)
        toks = torch.tensor([s + [s[-1]] * (S - len(s)) for s in rows], device=dev)
        pos = torch.arange(S, device=dev)[None].expand(Bc, S).contiguous()
        cache = KVCache.allocate(cfg, Bc, S, dtype=model.dtype, device=dev)
        hidden = model.forward(toks, pos, cache, torch.arange(Bc, device=dev))
        first = torch.full((Bc, cfg.vocab_size), S + 1, dtype=torch.long, device=dev)
        first.scatter_reduce_(1, toks, pos, reduce="amin")
        for b, (s, pl) in enumerate(zip(rows, pls)):
            n = len(s) - pl
            if n <= 0:
                out.append({"positions": 0, "decisive": 0, "mismatches": [], "min_margin": float("inf")})
                continue
            logits = model.logits(hidden[b, pl - 1: len(s) - 1])
            seen = first[b][None, :] < (pl + torch.arange(n, device=dev))[:, None]
            logits = apply_repetition_penalty(logits, seen, repetition_penalty)
            top = logits.topk(2, dim=-1)
            margin = (top.values[:, 0] - top.values[:, 1]).tolist()
            want = top.indices[:, 0].tolist()
            r = {"positions": n, "decisive": 0, "mismatches": [], "min_margin": min(margin)}
            for j in range(n):
                if margin[j] > eps:
                    r["decisive"] += 1
                    if s[pl + j] != want[j]:
                        r["mismatches"].append((pl + j, s[pl + j], want[j], margin[j]))
            out.append(r)
    return out


# ---------------------------------------------------------------------------------------------
# fp8 KV cache: the normative CPU definition of what the engines' e4m3 cache holds
# ---------------------------------------------------------------------------------------------
KV_E4M3_MAX = 448.0  # largest finite OCP e4m3fn value


def quantize_kv_e4m3(x: torch.Tensor) -> torch.Tensor:
    """The fp8 KV cache's content for the K / V values ``x`` (bias included, any float dtype):
    ``e4m3_rne(clamp(bf16_rne(x), -448, 448))`` as a ``torch.float8_e4m3fn`` tensor -- the bf16
    cache's content, saturated and rounded to nearest-even OCP e4m3, without scales.  The bf16
    rounding comes first (double rounding is part of the definition: the kernels quantise the
    bf16 values the bf16 cache would hold); the clamp keeps the result independent of a
    conversion's overflow behaviour and the NaN byte (0x7F / 0xFF) out of the cache.
    Dequantisation (``.float()`` / ``.to(bf16)``) is exact."""
    return x.to(torch.bfloat16).float().clamp(-KV_E4M3_MAX, KV_E4M3_MAX).to(torch.float8_e4m3fn)


@torch.no_grad()
def kv_fp8_margin(cfg: GPT2Config, weights: dict[str, torch.Tensor], prompts: list[list[int]], max_length: int,
                  repetition_penalty: float = 1.2, base_eps: float = 0.05) -> dict:
    """Derive, from the reference alone, the teacher-forced margin ``eps`` that an fp8-cache engine
    is held to.  An engine's K / V differ from the fp32 oracle's by bf16-arithmetic noise ahead of
    the quantiser; on the e4m3 grid that noise now and then flips a rounding by a whole step, so
    the logits deviate more than with a bf16 cache.  For each cache type the reference is
    evaluated teacher-forced on its own greedy generations twice -- exactly, and with the
    activations a bf16 engine rounds (LN outputs, q, attention output, GELU output, final hidden;
    for the bf16 cache also k and v) rounded to bf16 -- and the largest logit difference over the
    generated positions is taken.  ``eps`` = ``base_eps`` scaled by the ratio fp8 / bf16.

    Returns {"dev_fp8", "dev_bf16", "ratio", "eps", "positions", "decisive_share"(eps)}: the last
    is a function giving the share of the fp8 reference's positions that stay decisive at eps."""
    out: dict = {}
    margins: list[float] = []
    for kv in ("fp8", "bf16"):
        exact = GPT2Reference(cfg, weights, kv_dtype=kv)
        noisy = GPT2Reference(cfg, weights, kv_dtype=kv, act_dtype=torch.bfloat16)
        seqs = reference_generate(exact, prompts, max_length=max_length, repetition_penalty=repetition_penalty)
        dev, npos = 0.0, 0
        for s, p in zip(seqs, prompts):
            S, pl = len(s), len(p)
            if S <= pl:
                continue
            toks = torch.tensor([s])
            pos = torch.arange(S)[None]
            row = torch.zeros(1, dtype=torch.long)
            lg = []
            for m in (exact, noisy):
                cache = KVCache.allocate(cfg, 1, S, dtype=m.dtype)
                lg.append(m.logits(m.forward(toks, pos, cache, row)[0][pl - 1: S - 1]))
            dev = max(dev, float((lg[0] - lg[1]).abs().max()))
            npos += S - pl
            if kv == "fp8":
                seen = torch.zeros(S - pl, cfg.vocab_size, dtype=torch.bool)
                for j in range(S - pl):
                    seen[j, torch.tensor(s[: pl + j])] = True
                top = apply_repetition_penalty(lg[0], seen, repetition_penalty).topk(2, dim=-1).values
                margins += (top[:, 0] - top[:, 1]).tolist()
        out["dev_" + kv] = dev
        out["positions"] = npos
    out["ratio"] = out["dev_fp8"] / out["dev_bf16"]
    out["eps"] = base_eps * out["ratio"]
    out["decisive_share"] = lambda eps: sum(m > eps for m in margins) / max(1, len(margins))
    return out


# ---------------------------------------------------------------------------------------------
# Sampling: the normative CPU definition of the device sampler (ops/csrc/sample.hip)
# ---------------------------------------------------------------------------------------------
_PHILOX_M0, _PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_M32 = 0xFFFFFFFF


def philox4x32_10(counter, key) -> tuple[int, int, int, int]:
    """Philox4x32 with 10 rounds (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3"):
    ``counter`` 4 and ``key`` 2 32-bit words -> 4 32-bit words."""
    c0, c1, c2, c3 = (int(c) & _M32 for c in counter)
    k0, k1 = (int(k) & _M32 for k in key)
    for _ in range(10):
        p0, p1 = _PHILOX_M0 * c0, _PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + _PHILOX_W0) & _M32, (k1 + _PHILOX_W1) & _M32
    return c0, c1, c2, c3


def sampling_uniform(seed: int, stream: int, position: int) -> float:
    """The draw u in [0, 1) of (seed, request stream id, token position): 24 bits of Philox word 0."""
    r = philox4x32_10((position, stream & _M32, (stream >> 32) & _M32, 0), (seed & _M32, (seed >> 32) & _M32))
    return (r[0] >> 8) * 2.0 ** -24


def f32_ordered(x):
    """Order-preserving map of float32 values to uint32 (the high word of the argmax / sampler keys)."""
    import numpy as np

    bits = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def penalised_logits_f32(logits_f32, seen, penalty: float):
    """``seen(j) ? (z < 0 ? z * penalty : z / penalty) : z`` in float32, as the kernels compute it."""
    import numpy as np

    z = np.ascontiguousarray(logits_f32, dtype=np.float32)
    th = np.float32(penalty)
    with np.errstate(all="ignore"):
        pen = np.where(z < 0, z * th, z / th).astype(np.float32)
    return np.where(np.asarray(seen, dtype=bool), pen, z).astype(np.float32)


def sampling_candidates(l):
    """Token ids ordered by the key ``(f32_ordered(l_j) << 32) | ~j`` descending (ties: lower id first)."""
    import numpy as np

    key = (f32_ordered(l).astype(np.uint64) << np.uint64(32)) | (~np.arange(l.size, dtype=np.uint32)).astype(np.uint64)
    return np.argsort(key, kind="stable")[::-1]


def reference_sample(logits_f32, seen, penalty: float, params, stream: int, position: int,
                     margin: float = 1e-9) -> tuple[int, int, bool]:
    """One sampled token from the ``vocab`` float32 logits of a row, exactly as ``sample.hip``
    defines it, in numpy float64 from float32 inputs.  ``seen``: bool [vocab].  Returns
    ``(token, m, decisive)``: m is the nucleus size; ``decisive`` is False when moving the draw
    ``u * c_{m-1}`` or the nucleus cut ``top_p * W`` by +-``margin`` * W would change the result."""
    import numpy as np

    l = penalised_logits_f32(logits_f32, seen, penalty)
    k = min(int(params.top_k), l.size)
    order = sampling_candidates(l)[:k]
    lc = l[order]
    with np.errstate(all="ignore"):
        x = (lc - lc[0]).astype(np.float32).astype(np.float64)
    w = np.exp(x / float(params.temperature))
    c = np.empty(k, dtype=np.float64)
    acc = 0.0
    for i in range(k):  # prefix sums in candidate order, one double add each
        acc += float(w[i])
        c[i] = acc
    W = float(c[-1])
    d = margin * W

    def nucleus(cut):
        return int(np.searchsorted(c, cut, side="left")) + 1  # the smallest m with c[m-1] >= cut

    def pick(m, target):
        return int(np.searchsorted(c[:m], target, side="right"))  # the first i with c[i] > target

    top_p = float(params.top_p)
    decisive = True
    if top_p >= 1.0:
        m = k
    else:
        cut = top_p * W
        m = min(nucleus(cut), k)
        decisive = min(nucleus(cut - d), k) == m and min(nucleus(cut + d), k) == m
    u = sampling_uniform(int(params.seed), int(stream), int(position))
    target = u * float(c[m - 1])
    i = min(pick(m, target), m - 1)
    decisive = decisive and min(pick(m, target - d), m - 1) == i and min(pick(m, target + d), m - 1) == i
    return int(order[i]), m, bool(decisive)


@torch.no_grad()
def teacher_forced_sampling_check(model: GPT2Reference, seq: list[int], prompt_len: int, repetition_penalty: float,
                                  params, eps: float = 0.05, controls=None, eos_token_id: int | None = None) -> dict:
    """Oracle for a SAMPLED sequence: one fp32 forward over ``seq`` (teacher forcing); a generated
    token is a mismatch when the oracle says no sampler within a logit error of ``eps`` could have
    drawn it -- (a) its penalised oracle logit is more than ``eps`` below the ``top_k``-th largest,
    or (b) the oracle probability mass (softmax at the temperature over the top-k) of the tokens
    whose logit beats it by more than ``eps`` is >= ``top_p * exp(2 eps / T)``: those tokens rank
    above it under any eps-perturbation, and an eps-error scales a softmax ratio by at most
    exp(2 eps / T), so the nucleus closes before it.  ``controls``: the oracle's logits of
    ``banned_tokens`` are -inf at each position, so a banned token in ``seq`` is "below top-k".

    Returns {"positions", "mismatches": [(i, got, reason, value)]}."""
    cfg = model.cfg
    dev = model.device
    S = len(seq)
    out = {"positions": 0, "mismatches": []}
    if S <= prompt_len:
        return out
    cache = KVCache.allocate(cfg, 1, S, dtype=model.dtype, device=dev)
    toks = torch.tensor([seq], device=dev)
    pos = torch.arange(S, device=dev)[None]
    hidden = model.forward(toks, pos, cache, torch.zeros(1, dtype=torch.long, device=dev))[0]
    logits = model.logits(hidden[prompt_len - 1: S - 1]).float()  # row j predicts seq[prompt_len + j]
    n = logits.shape[0]
    seen = torch.zeros(n, cfg.vocab_size, dtype=torch.bool, device=dev)
    for j in range(n):
        seen[j, torch.tensor(seq[: prompt_len + j], device=dev)] = True
    if controls is not None and controls.bans:
        eos = cfg.eos_token_id if eos_token_id is None else eos_token_id
        for j in range(n):
            ban = banned_tokens(seq[: prompt_len + j], prompt_len, controls, eos)
            if ban:
                logits[j, torch.tensor(ban, device=dev)] = float("-inf")
    logits = apply_repetition_penalty(logits, seen, repetition_penalty).double()
    k = min(int(params.top_k), cfg.vocab_size)
    T, top_p = float(params.temperature), float(params.top_p)
    out["positions"] = n
    got = torch.tensor(seq[prompt_len:], device=dev)
    top = logits.topk(k, dim=-1).values  # [n, k], descending
    lg = logits.gather(1, got[:, None])  # [n, 1]
    short = (top[:, -1:] - lg)[:, 0]  # how far below the k-th largest
    p = torch.softmax(top / T, dim=-1)
    mass = (p * (top > lg + eps)).sum(dim=-1)  # oracle mass of the tokens that beat it by more than eps
    short, mass = short.tolist(), mass.tolist()
    for j in range(n):
        if short[j] > eps:
            out["mismatches"].append((prompt_len + j, seq[prompt_len + j], "below top-k", short[j]))
        elif top_p < 1.0 and mass[j] >= top_p * math.exp(2 * eps / T):
            out["mismatches"].append((prompt_len + j, seq[prompt_len + j], "outside nucleus", mass[j]))
    return out


# ---------------------------------------------------------------------------------------------
# Log-probabilities: the normative CPU definition of ops/csrc/logprob.hip
# ---------------------------------------------------------------------------------------------
def reference_logprob(logits_f32, seen, penalty: float, token=None):
    """The log-probability of ``token`` under the distribution that the logits processors leave of
    the ``vocab`` float32 logits of a row (banned columns hold -inf), at temperature 1, ahead of
    top-k / top-p, exactly as ``logprob.hip`` defines it: with the float32 penalised logits l_j
    (``penalised_logits_f32``) and m = max l_j, ``(l_tok - m) - log(sum_j exp(l_j - m))`` in numpy
    float64.  ``seen``: bool [vocab] (None: no column seen).  ``token`` None: every token's
    log-probability, float64 [vocab]."""
    import numpy as np

    z = np.ascontiguousarray(logits_f32, dtype=np.float32)
    l = penalised_logits_f32(z, np.zeros(z.shape, dtype=bool) if seen is None else seen, penalty).astype(np.float64)
    m = l.max()
    with np.errstate(divide="ignore"):
        lp = (l - m) - np.log(np.exp(l - m).sum())
    return lp if token is None else float(lp[int(token)])


@torch.no_grad()
def teacher_forced_logprobs(model: GPT2Reference, seq: list[int], prompt_len: int, repetition_penalty: float = 1.2,
                            controls=None, eos_token_id: int | None = None):
    """``reference_logprob`` of every generated token of ``seq`` (float64 [len(seq) - prompt_len]):
    one forward of ``model`` over ``seq`` (teacher forcing); position j sees the float32 logits that
    predict ``seq[prompt_len + j]``, with the bans of ``controls`` stored as -inf as
    ``reference_generate`` applies them, and the tokens before it as the seen set."""
    import numpy as np

    cfg, dev = model.cfg, model.device
    S = len(seq)
    if S <= prompt_len:
        return np.zeros(0, dtype=np.float64)
    eos = cfg.eos_token_id if eos_token_id is None else eos_token_id
    cache = KVCache.allocate(cfg, 1, S, dtype=model.dtype, device=dev)
    toks = torch.tensor([seq], device=dev)
    pos = torch.arange(S, device=dev)[None]
    hidden = model.forward(toks, pos, cache, torch.zeros(1, dtype=torch.long, device=dev))[0]
    logits = model.logits(hidden[prompt_len - 1: S - 1]).float().cpu().numpy()  # row j predicts seq[prompt_len + j]
    out = np.empty(S - prompt_len, dtype=np.float64)
    seen = np.zeros(cfg.vocab_size, dtype=bool)
    seen[np.asarray(seq[:prompt_len], dtype=np.int64)] = True
    for j in range(S - prompt_len):
        if controls is not None and controls.bans:
            ban = banned_tokens(seq[: prompt_len + j], prompt_len, controls, eos)
            if ban:
                logits[j, np.asarray(ban, dtype=np.int64)] = -np.inf
        out[j] = reference_logprob(logits[j], seen, repetition_penalty, seq[prompt_len + j])
        seen[seq[prompt_len + j]] = True
    return out


@torch.no_grad()
def logprob_noise(cfg: GPT2Config, weights: dict[str, torch.Tensor], prompts: list[list[int]], max_length: int,
                  penalty: float = 1.2, kv_dtype: str = "bf16") -> float:
    """The largest difference between ``teacher_forced_logprobs`` of the fp32 reference and of the
    same reference with the activations a bf16 engine rounds rounded to bf16 (``act_dtype``), over
    the fp32 reference's own greedy generations of ``prompts``: what rounding the activations alone
    moves a log-probability by.  From the reference alone, on the CPU, like ``kv_fp8_margin``; the
    tests hold an engine's log-probabilities to a multiple of it."""
    import numpy as np

    exact = GPT2Reference(cfg, weights, kv_dtype=kv_dtype)
    noisy = GPT2Reference(cfg, weights, kv_dtype=kv_dtype, act_dtype=torch.bfloat16)
    seqs = reference_generate(exact, prompts, max_length=max_length, repetition_penalty=penalty)
    dev = 0.0
    for s, p in zip(seqs, prompts):
        if len(s) > len(p):
            a = teacher_forced_logprobs(exact, s, len(p), penalty)
            b = teacher_forced_logprobs(noisy, s, len(p), penalty)
            dev = max(dev, float(np.abs(a - b).max()))
    return dev
