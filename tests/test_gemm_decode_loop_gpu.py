"""Exact checks of the tiled GEMM's K loop (gemm.hip: host-computed tile map, ring prologue, tail
drain, whole-step fragment reads with counted waits) on the 64-row decode tiles.

A, W and the bias hold small integers in [-3, 3] (exact in bf16).  With K <= 3072 every partial sum
is an integer of magnitude <= 9 * 3072 + 3 < 2^24, exact in fp32 whatever the summation order, so the
kernel must EQUAL a torch fp64 product rounded the same way (fp32 slabs for the split-K epilogue, one
round-to-nearest-even to bf16 for the bf16 / QKV epilogues): any wrong fragment, ring stage, tile
index or K-slice bound changes an integer.  K = 64 ... 768 are 1, 2, 3 (= ring depth - 1), 4, 5 and 12
ring steps: prologue-only, tail-drain and steady-state paths of the 4-deep ring."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ops():
    from distributed_lms_raft_llm_amd import ops

    ops.lib()
    return ops


def _ints(*shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(-3, 4, shape, generator=g)


@functools.lru_cache(maxsize=None)
def _case(M, N, K):
    """(a bf16, w bf16, bias f32, a @ w.T in fp64 without the bias) -- computed once per shape, read-only."""
    a, w, bias = _ints(M, K, seed=K + M), _ints(N, K, seed=7 * K + N), _ints(N, seed=N)
    a, w, bias = a.to(DEV), w.to(DEV), bias.to(DEV)
    ref = a.double() @ w.double().t()
    assert float(ref.abs().max()) + 3 < 2 ** 24
    return a.to(torch.bfloat16), w.to(torch.bfloat16), bias.float(), ref


def _rne_bf16(x64):
    return x64.float().to(torch.bfloat16)  # integers < 2^24: fp64 -> fp32 is exact, then one RNE


@pytest.mark.parametrize("K", [64, 128, 192, 256, 320, 768])
@pytest.mark.parametrize("N", [96, 192, 384])
@pytest.mark.parametrize("M", [257, 320, 512])
def test_decode_tile_bf16_exact(M, N, K):
    """Production dispatch of a decode row half (256 < M <= 512): the 64x96 4-stage tile, ragged and
    full last row tiles, two and four column tiles, every ring phase.  The GEMM's contract is
    N % 64 == 0 (every dispatch falls back to 64-wide tiles), so a lone 96-column tile cannot be
    launched: N = 96 must be refused on the host, before any launch."""
    ops = _ops()
    a, w, bias, ref = _case(M, N, K)
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    ops.gemm_tile_reset()
    if N % 64:
        with pytest.raises(ValueError):
            ops.gemm(a, w, ops.EPI_BF16, bias=bias, out=out)
        assert ops.gemm_tile_count(64, 96) == 0
        return
    ops.gemm(a, w, ops.EPI_BF16, bias=bias, out=out)
    assert ops.gemm_tile_count(64, 96) == 1
    assert torch.equal(out, _rne_bf16(ref + bias.double()))


@pytest.mark.parametrize("M,N,K,split,tile", [(512, 768, 2048, 4, (64, 96)), (257, 768, 2048, 4, (64, 96)),
                                              (512, 768, 768, 2, (64, 64))])
def test_decode_split_k_slabs_exact(M, N, K, split, tile):
    """EPI_PARTIAL: c_proj's split 4 on the smallest shape the 64x96 split rule takes, and the
    out-projection's split 2 on 64x64 tiles; every fp32 slab equals its K slice's product."""
    ops = _ops()
    a, w, _, _ = _case(M, N, K)
    out = torch.full((split, M, N), float("nan"), device=DEV)
    ops.gemm_tile_reset()
    ops.gemm(a, w, ops.EPI_PARTIAL, out=out, split_k=split)
    assert ops.gemm_tile_count(*tile) == 1
    kc = K // split
    for s in range(split):
        ref = a[:, s * kc:(s + 1) * kc].double() @ w[:, s * kc:(s + 1) * kc].double().t()
        assert torch.equal(out[s], ref.float()), f"slab {s}"


def test_decode_qkv_scatter_exact():
    """EPI_QKV on the 64x96 tile (N = 3 x 192): q rows and the K/V rows scattered to permuted slots and
    positions; q_out and both whole caches (nothing else written) equal the reference."""
    ops = _ops()
    M, D, K, T = 320, 192, 320, 11
    H = D // 64
    a, w, bias, ref = _case(M, 3 * D, K)
    ref = _rne_bf16(ref + bias.double())
    g = torch.Generator(device="cpu").manual_seed(5)
    slot = torch.randperm(M, generator=g).to(torch.int32).to(DEV)
    pos = ((torch.arange(M) * 7 + 3) % T).to(torch.int32).to(DEV)
    q = torch.full((M, D), float("nan"), dtype=torch.bfloat16, device=DEV)
    kc = torch.zeros(M, H, T, 64, dtype=torch.bfloat16, device=DEV)
    vc = torch.zeros_like(kc)
    ops.gemm_tile_reset()
    ops.gemm(a, w, ops.EPI_QKV, bias=bias, q_out=q, k_cache=kc, v_cache=vc, row_slot=slot, row_pos=pos)
    assert ops.gemm_tile_count(64, 96) == 1
    assert torch.equal(q, ref[:, :D])
    want_k, want_v = torch.zeros_like(kc), torch.zeros_like(vc)
    want_k[slot.long(), :, pos.long()] = ref[:, D:2 * D].reshape(M, H, 64)
    want_v[slot.long(), :, pos.long()] = ref[:, 2 * D:].reshape(M, H, 64)
    assert torch.equal(kc, want_k)
    assert torch.equal(vc, want_v)


def test_decode_tile_gelu_tanh():
    """EPI_GELU_TANH on the 64x96 tile, random inputs, the tolerance of test_kernels_gpu.test_gemm_gelu."""
    ops = _ops()
    M, N, K = 320, 192, 768
    g = torch.Generator(device="cpu").manual_seed(9)
    a = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16).to(DEV)
    bias = (torch.randn(N, generator=g) * 0.1).to(DEV)
    ops.gemm_tile_reset()
    out = ops.gemm(a, w, ops.EPI_GELU_TANH, bias=bias)
    assert ops.gemm_tile_count(64, 96) == 1
    ref = torch.nn.functional.gelu(a.float() @ w.float().t() + bias, approximate="tanh")
    torch.testing.assert_close(out.float(), ref, atol=2e-2, rtol=2e-2)


# forced tile id -> (BM, BN): ring depths 6, 4, 2, 6 on 32/64-row 64-wide tiles, 4 on 32x128, 4, 3, 6 on 64x96
FORCED = {0: (32, 64), 1: (64, 64), 4: (64, 64), 7: (64, 64), 15: (32, 128), 17: (64, 96), 18: (64, 96),
          19: (64, 96)}


@pytest.mark.parametrize("tile", sorted(FORCED))
def test_forced_tiles_exact_and_repeatable(tile):
    """M = 65 (a one-row last tile), N = 384, K = 320 (5 ring steps: shorter than, equal to and longer
    than the rings) on every ring depth of the small tiles; launched twice on the same buffers, the
    second result must equal the first (a screen for a DMA / fragment-read race)."""
    ops = _ops()
    L = ops.lib()
    M, N, K = 65, 384, 320
    a, w, bias, ref = _case(M, N, K)
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    ops.gemm_tile_reset()
    L.dlms_gemm_force_tile(tile)
    try:
        ops.gemm(a, w, ops.EPI_BF16, bias=bias, out=out)
        first = out.clone()
        ops.gemm(a, w, ops.EPI_BF16, bias=bias, out=out)
    finally:
        L.dlms_gemm_force_tile(-1)
    assert ops.gemm_tile_count(*FORCED[tile]) == 2
    assert torch.equal(first, _rne_bf16(ref + bias.double()))
    assert torch.equal(out, first)
