"""Inputs and recorded figures shared by test_logprobs_cpu.py and test_logprobs_gpu.py."""
import numpy as np

PEN = 1.2

# ------------------------------------------------------------------ the kernel against reference_logprob
# (vocab, padded row stride): float4 chunks per thread NJ = 1, 4 and 13; no vocab is a multiple of 4
KERNEL_SHAPES = [(1000, 1024), (5001, 5008), (50257, 50304)]
KERNEL_ROWS = [1, 5]
KERNEL_MAX_LEN = 12  # columns of out_logprob in the decode-mode tests
# f32 arithmetic at |l| <= 100: the argument rounding of l_j - m is <= 2^-24 * 88 ~ 5e-6 relative per
# term, expf adds a few ulp, the summation tree < 1e-5 relative on the sum (the same absolute error
# on its log), l_tok - m <= 1 ulp at 100 ~ 8e-6: under 5e-5 in total; 1e-4 leaves a factor 2
KERNEL_TOL = 1e-4
SENTINEL = -12345.0


def kernel_rows(rows: int, vocab: int, ld: int, seed: int, pad: float):
    """``rows`` x 8 cases of f32 logits [rows * 8, ld] with their seen masks and chosen tokens.  Per
    block of ``rows`` rows, in order: N(0, 2^2) logits; the same with 100 columns at -inf; one logit
    40 above the rest (the chosen one: logprob ~ 0); a constant row (-log(vocab)); a row shifted by
    +80; then three more random blocks whose tokens are 0, vocab - 1 and random.  About half the
    columns are seen; the chosen token alternates seen / unseen, and the random logits have both
    signs at seen columns.  Columns >= vocab hold ``pad`` (1e30 or NaN)."""
    g = np.random.default_rng(seed)
    n = rows * 8
    z = (g.standard_normal((n, ld)) * 2).astype(np.float32)
    seen = g.random((n, ld)) < 0.5
    tok = g.integers(0, vocab, n)
    for r in range(rows):
        z[rows + r, g.choice(vocab, 100, replace=False)] = -np.inf
        z[2 * rows + r, tok[2 * rows + r]] = z[2 * rows + r, :vocab].max() + 40.0
        z[3 * rows + r, :] = 1.5
        z[4 * rows + r, :] += 80.0
        tok[5 * rows + r] = 0
        tok[6 * rows + r] = vocab - 1
    for i in range(n):
        while not np.isfinite(z[i, tok[i]]):  # (never score a banned token: it is never chosen)
            tok[i] = (tok[i] + 1) % vocab
        seen[i, tok[i]] = i % 2 == 0
    z[:, vocab:] = pad
    seen[:, vocab:] = False
    return z, seen, tok.astype(np.int64)


def pack_seen(seen: np.ndarray) -> np.ndarray:
    """bool [n, ld] -> the engines' int32 bitmap words [n, ceil(ld / 32)] (bit c % 32 of word c // 32)."""
    n, ld = seen.shape
    words = (ld + 31) // 32
    padded = np.zeros((n, words * 32), dtype=bool)
    padded[:, :ld] = seen
    return np.packbits(padded.reshape(n, words, 32), axis=-1, bitorder="little").view(np.uint32) \
        .reshape(n, words).view(np.int32)


def sampler_keys(l_tok: np.ndarray, tok: np.ndarray) -> np.ndarray:
    """What the sampler writes per row: (f32_ordered(l_tok) << 32) | ~tok, as int64."""
    from distributed_lms_raft_llm_amd.models.gpt2 import f32_ordered

    hi = f32_ordered(np.asarray(l_tok, dtype=np.float32)).astype(np.uint64)
    lo = (~np.asarray(tok, dtype=np.uint32)).astype(np.uint64)
    return ((hi << np.uint64(32)) | lo).view(np.int64)


# ------------------------------------------------------------------ the engine against the fp32 reference
# The engine cases: (kind, rows) with the engines of tests/test_controls_gpu.py::_make; prompts
# _prompts(cfg, rows, seed=3) (lengths 1-8) on gpt2_config("gpt2"), init_gpt2_weights(seed=0) with
# bf16-rounded matrices, penalty 1.2.
ENGINE_CASES = [("small", 1), ("small", 2), ("small", 9), ("overlap", 16), ("panel", 256)]
NOISE_ROWS, NOISE_T = 9, 40
# models.gpt2.logprob_noise over the 9-row, T = 40 case: the largest difference between the fp32
# reference's teacher-forced log-probabilities and those of the same reference with bf16-rounded
# activations, on the fp32 reference's own greedy sequences (measured on the CPU; the reference
# alone -- test_logprobs_cpu.py reproduces them)
LOGPROB_NOISE = {"bf16": 0.006494434976703545, "fp8": 0.03891034727780607}
# The engine is held to 4 x the noise: the act_dtype model rounds activations only, the engine also
# differs in accumulation order, its exp2 / rcp GELU and its softmax
LOGPROB_EPS = 4 * LOGPROB_NOISE["bf16"]  # ~ 0.026
LOGPROB_EPS_FP8 = 4 * LOGPROB_NOISE["fp8"]  # ~ 0.16


def prompts(cfg, n: int, seed: int = 3):
    """tests/test_controls_gpu.py::_prompts."""
    import torch

    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, cfg.vocab_size - 1, (int(L),), generator=g).tolist()
            for L in torch.randint(1, 9, (n,), generator=g)]


def bf16_exact_weights(cfg):
    import torch

    from distributed_lms_raft_llm_amd.models.gpt2 import init_gpt2_weights

    w = init_gpt2_weights(cfg, seed=0)
    for k, v in w.items():  # bf16-exact weights: the oracle sees exactly what the kernels see
        if v.dim() == 2:
            w[k] = v.to(torch.bfloat16).float()
    return w
