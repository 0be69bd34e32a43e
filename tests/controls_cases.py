"""Inputs and recorded figures shared by test_controls_cpu.py and test_controls_gpu.py."""
import numpy as np

# The engine cases of test_controls_gpu.py: (rows, max_length) -> the no_repeat_ngram_size values run.
# Prompts: tests/test_sampling_gpu.py::_prompts(cfg, rows, seed=3) on gpt2_config("gpt2"),
# init_gpt2_weights(seed=0) with bf16-rounded matrices, penalty 1.2.
ENGINE_CASES = {(1, 40): (1, 2), (2, 40): (1, 2), (9, 40): (1, 2), (16, 40): (1, 2), (256, 24): (1, 2),
                (4, 40): (2,)}  # 4 rows: the fp8-cache, prefix-cache and batcher cases

# (rows, max_length, n) -> (decisive, positions): the share of generated positions whose top-1 /
# top-2 margin among the unbanned penalised logits exceeds eps = 0.05, measured on the fp32
# reference alone (reference_generate(controls) checked by teacher_forced_controls_check on the
# CPU).  The GPU tests require MIN_DECISIVE of the engine's output; a case whose reference share is
# under 0.6 would be too close to that floor and needs other prompts (test_controls_cpu.py checks).
REFERENCE_DECISIVE = {
    (6, 40, 1): (146, 228), (6, 40, 2): (169, 228), (6, 40, 3): (177, 228),  # (the six-prompt case of the issue)
    (1, 40, 1): (24, 36), (1, 40, 2): (26, 36),
    (2, 40, 1): (47, 76), (2, 40, 2): (53, 76),
    (9, 40, 1): (218, 335), (9, 40, 2): (229, 335),
    (16, 40, 1): (381, 591), (16, 40, 2): (433, 591),
    (4, 40, 1): (95, 150), (4, 40, 2): (115, 150),
    (256, 24, 1): (3294, 5060), (256, 24, 2): (3611, 5060),
}
MIN_DECISIVE = 0.5
# The seed of _prompts per row count (default 3).  One row: seed 3's prompt gives 20/37 = 0.54 at
# n = 1 on the reference alone (seeds 4 .. 8: 0.62, 0.67, 0.54, 0.69, 0.78) -- under 0.6, so that
# case runs seed 5's prompt (24/36 and 26/36 above).
PROMPT_SEED = {1: 5}


def prompt_seed(rows: int) -> int:
    return PROMPT_SEED.get(rows, 3)


def repeated_ngrams(seq, prompt_len: int, n: int) -> list[int]:
    """The generated indices p at which ``seq`` completes an n-gram that occurred before:
    some i < p - n + 1 with seq[i : i+n] == seq[p-n+1 : p+1].  Empty: property (a)."""
    bad = []
    for p in range(max(prompt_len, n - 1), len(seq)):
        cur = seq[p - n + 1: p + 1]
        if any(seq[i: i + n] == cur for i in range(p - n + 1)):
            bad.append(p)
    return bad


def cut_at_stop(full, prompt_len: int, stop) -> list[int]:
    """``full`` cut right after the first generated occurrence of a stop sequence (whole if none)."""
    for end in range(prompt_len + 1, len(full) + 1):
        if any(end - len(s) >= prompt_len and list(full[end - len(s): end]) == list(s) for s in stop):
            return list(full[:end])
    return list(full)


def planted_sequences(n: int, vocab: int, seed: int, max_len: int = 30):
    """(seq, prompt_len, min_new_tokens) cases for ``banned_tokens``: random sequences over a small
    vocabulary (chance repeats), each also with its last n - 1 tokens overwritten by a copy of an
    earlier stretch (a planted repeat: a ban for certain); lengths 1, n - 1, n, n + 1 and random
    ones; min_new_tokens at L - P = min - 1, min and off."""
    g = np.random.default_rng(seed)
    cases = []
    for L in sorted({1, max(1, n - 1), n, n + 1, 2 * n + 1, max_len} | set(g.integers(1, max_len, 12).tolist())):
        for planted in (False, True):
            seq = g.integers(0, vocab - 1, L).tolist()
            if planted and n > 1 and L >= 2 * n:
                i = int(g.integers(0, L - 2 * n + 2))
                seq[L - n + 1:] = seq[i: i + n - 1]
            P = int(g.integers(1, L + 1))
            for mn in (0, L - P, L - P + 1):
                cases.append((seq, P, mn))
    return cases


def kernel_rows(rows: int, vocab: int, n: int, max_len: int, seed: int, shift: int = 0):
    """State of ``rows`` slots for the logit_bans test: lengths 0, 1, n - 1, n, max_len first (that
    list rotated left by ``shift``: a one-row case takes them in turn), then random; tokens over a
    12-id alphabet spread across the vocabulary (last id vocab - 1) with the last n - 1 tokens of
    every other row copied from an earlier stretch; prompt lengths random.
    Returns (out_tokens [rows, max_len] int32 -- random ids past each length --, lens, prompt_len)."""
    g = np.random.default_rng(seed)
    alphabet = np.unique(np.concatenate([g.integers(0, vocab, 11), [vocab - 1]]))
    wanted = [0, 1, max(0, n - 1), n, max_len]
    wanted = wanted[shift:] + wanted[:shift]
    lens = np.array([wanted[r] if r < len(wanted) else int(g.integers(0, max_len + 1)) for r in range(rows)])
    lens = np.minimum(lens, max_len)
    toks = alphabet[g.integers(0, alphabet.size, (rows, max_len))]
    for r in range(rows):
        L = int(lens[r])
        if r % 2 == 0 and n > 1 and L >= 2 * n:
            i = int(g.integers(0, L - 2 * n + 2))
            toks[r, L - n + 1: L] = toks[r, i: i + n - 1]
    plen = np.array([int(g.integers(0, L + 1)) for L in lens])
    return toks.astype(np.int32), lens.astype(np.int32), plen.astype(np.int32)
