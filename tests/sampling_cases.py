"""Inputs shared by the sampler tests (test_sampling_cpu.py checks the reference on them,
test_sampling_gpu.py the kernel against the reference): logits rows of several kinds mixed within
one launch, a seen bitmap, and a (stream, position) pair per row."""
import numpy as np

# (vocab, row stride, rows)
SHAPES = [(50257, 50304, 1), (50257, 50304, 5), (50257, 50304, 67), (1000, 1024, 3)]
# (top_k, top_p, temperature)
PARAMS = [(50, 0.9, 0.7), (1, 1.0, 1.0), (2, 0.1, 1.0), (64, 0.5, 1.0), (256, 0.9, 2.0), (256, 1.0, 1.0)]
PENALTY = 1.2
SEED = 0x9E3779B97F4A7C15  # (above 2^63: the seed word's top bit is exercised)
KINDS = ("normal", "halves", "equal", "spike", "seen")


def row_kind(r: int, case: int, top_p: float) -> str:
    kind = KINDS[(r + case) % len(KINDS)]
    # all-equal rows only where the nucleus is the whole top-k: at top_p < 1 the cut falls exactly on
    # a boundary of equal weights
    return "normal" if kind == "equal" and top_p < 1.0 else kind


def make_case(vocab: int, ld: int, rows: int, top_p: float, case: int):
    """-> logits f32 [rows, ld] (padding columns hold 1e30 / NaN), seen bool [rows, vocab],
    streams int64 [rows], positions int32 [rows]."""
    g = np.random.default_rng(1000 + case)
    z = np.empty((rows, ld), dtype=np.float32)
    seen = np.zeros((rows, vocab), dtype=bool)
    for r in range(rows):
        kind = row_kind(r, case, top_p)
        v = (g.standard_normal(vocab) * 3.0).astype(np.float32)
        if kind == "halves":
            v = (np.round(v * 2.0) / 2.0).astype(np.float32)
        elif kind == "equal":
            v[:] = np.float32(g.standard_normal() * 3.0)
        elif kind == "spike":
            v[int(g.integers(vocab))] = np.float32(30.0)
        elif kind == "seen":
            seen[r] = g.random(vocab) < 0.2
        else:
            seen[r, g.integers(vocab, size=3)] = True  # a few penalised tokens on every other kind
        z[r, :vocab] = v
    pad = np.where(np.arange(ld - vocab) % 2 == 0, np.float32(1e30), np.float32(np.nan))
    z[:, vocab:] = pad
    streams = (np.arange(rows, dtype=np.int64) * 7 + 3) + (np.arange(rows, dtype=np.int64) % 3 == 2) * (1 << 40)
    positions = (5 + 11 * np.arange(rows)) % 150
    return z, seen, streams, positions.astype(np.int32)


def all_cases():
    case = 0
    for vocab, ld, rows in SHAPES:
        for top_k, top_p, temperature in PARAMS:
            yield case, vocab, ld, rows, top_k, top_p, temperature
            case += 1


def seen_words(seen: np.ndarray, words: int) -> np.ndarray:
    """bool [rows, vocab] -> the kernels' int32 bitmap [rows, words] (bit t % 32 of word t // 32)."""
    rows, vocab = seen.shape
    bits = np.zeros((rows, words * 32), dtype=np.uint8)
    bits[:, :vocab] = seen
    return np.packbits(bits.reshape(rows, words, 32), axis=-1, bitorder="little").view(np.uint32).reshape(
        rows, words).view(np.int32)
