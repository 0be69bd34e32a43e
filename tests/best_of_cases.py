"""Shared by tests/test_best_of_cpu.py and tests/test_best_of_gpu.py: the prompts, seeds, completion
counts and kernel geometries of the best-of-n tests.

The engine cases run GPT-2-124M (random init, bf16-exact matrices: logprob_cases.bf16_exact_weights)
at max_batch 16, max_length 40, penalty 1.2, SamplingParams(0.7, 50, 0.9, 7), prompts of 1-8 tokens
(logprob_cases.prompts, seed 3).  The oracle is the fp32 ``GPT2Reference`` through
``teacher_forced_sampling_check`` at the project's eps = 0.05 and ``teacher_forced_logprobs`` within
logprob_cases.LOGPROB_EPS: best of n adds a copy of bytes and a choice of stream ids, no arithmetic,
so no new tolerance exists.  The GPU tests assert that the k completions of a prompt are not all
equal; tests/test_best_of_cpu.py checks on the reference alone that they are in fact pairwise distinct
for every case here (k streams at temperature 0.7 over up to 39 draws).
"""
import numpy as np

PEN = 1.2
SAMPLING = (0.7, 50, 0.9, 7)  # temperature, top_k, top_p, seed
MAX_BATCH, T = 16, 40
# (prompts, completions per prompt): 2 rows (the latency step), 12 rows (the mid path, 16-row bucket), 16 rows
ENGINE_CASES = [(1, 2), (3, 4), (2, 8)]
# the order slots are handed to admit() in: neither contiguous nor ascending, parents included
SLOT_ORDER = [11, 3, 14, 0, 7, 9, 2, 15, 5, 12, 1, 8, 13, 4, 10, 6]


def slots_for(n_prompts: int, k: int) -> list[int]:
    return SLOT_ORDER[: n_prompts * k]


# ------------------------------------------------------------------ ops.kv_fork
# cache [L][2][S][H][T][64]; pairs (src, dst, len)
# out of order, a shared parent, len = T (the last key), len = 1, src = dst, and a pair with len 0.
# With six slots, five of them named by the first four pairs, the len-0 pair has to be a self pair as
# well (any other would write a slot twice or read a written one, which the host refuses);
# EXACT_EXTRA covers a len-0 pair between two different slots.
EXACT = dict(L=2, S=6, H=3, T=8, pairs=[(4, 1, 8), (4, 5, 8), (0, 2, 1), (3, 3, 7), (0, 0, 0)])
# len 0 between different slots, and a length past T (the kernel clamps it to T)
EXACT_EXTRA = dict(L=1, S=8, H=2, T=5, pairs=[(6, 7, 0), (2, 0, 100), (2, 5, 3)])
# 128 children x 24 (layer, k/v) units = 3072 units: more than the launcher's 2048 workgroups, so they stride
STRIDE = dict(L=12, S=160, H=12, T=40, parents=32, children=4)


def stride_pairs():
    """32 parents with 4 children each over a permutation of the 160 slots; lengths from 1 .. 40,
    1 and 40 among them."""
    g = np.random.default_rng(15)
    c = STRIDE
    perm = g.permutation(c["S"])
    parents, kids = perm[: c["parents"]], perm[c["parents"]:].reshape(c["parents"], c["children"])
    lens = g.integers(1, c["T"] + 1, c["parents"])
    lens[0], lens[1] = 1, c["T"]
    pairs = [(int(p), int(d), int(n)) for p, ds, n in zip(parents, kids, lens) for d in ds]
    order = g.permutation(len(pairs))
    return [pairs[i] for i in order]


def random_cache(geom, dtype_bytes: int, seed: int) -> np.ndarray:
    """Every byte random: uint8 [L, 2, S, H, T, 64 * dtype_bytes]."""
    g = np.random.default_rng(seed)
    return g.integers(0, 256, (geom["L"], 2, geom["S"], geom["H"], geom["T"], 64 * dtype_bytes), dtype=np.uint8)


def forked(cache: np.ndarray, pairs) -> np.ndarray:
    """What ``kv_fork`` must leave: the indexed copies and every other byte as it was."""
    out = cache.copy()
    T = cache.shape[4]
    for s, d, n in pairs:
        n = min(n, T)
        out[:, :, d, :, :n] = cache[:, :, s, :, :n]
    return out


# ------------------------------------------------------------------ pick_best
# (lists, index): means, ties to the lowest index, an empty list, NaN
NAN = float("nan")
PICK_CASES = [
    ([[-1.0, -3.0], [-1.5, -1.5], [-0.5, -4.0]], 1),  # means -2, -1.5, -2.25
    ([[-2.0], [-1.0, -3.0], [-2.0, -2.0]], 0),  # a three-way tie
    ([[-3.0], [-1.0], [-1.0]], 1),
    ([[-0.1] * 3 + [-9.0], [-2.0]], 1),  # the mean, not the sum and not the best token
    ([[], [-50.0]], 1),  # an empty list ranks below every non-empty one
    ([[], []], 0),
    ([[NAN, -0.1], [-7.0], [-6.0, NAN]], 1),  # a NaN ranks a list below all lists without one
    ([[-0.1, NAN], []], 1),
    ([[NAN], [NAN, NAN]], 0),
    ([[-2.5]], 0),
]
