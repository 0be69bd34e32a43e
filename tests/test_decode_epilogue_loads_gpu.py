"""Checks of the decode kernels whose epilogue operands are requested ahead of the main loop
(gemm.hip: bias values and QKV scatter indices held in registers across the K loop; gemm_ps.hip:
the LM head's seen-bitmap words fetched ahead of a tile's weight loads and exchanged through LDS;
decode.hip: unconditional, clamped key / embedding loads).

The GEMM checks are exact, by the method of test_gemm_decode_loop_gpu.py: A, W and the bias hold
integers in [-3, 3] (exact in bf16), every partial sum stays below 2^24 (exact in fp32 in any order),
so the kernel must EQUAL a torch fp64 product rounded once.  K = 64 ... 768 are 1, 2, 3, 4 and 12 steps
of the 4-deep ring: the prefetched values are outstanding across a prologue-only, a draining and a
steady-state loop."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
KS = [64, 128, 192, 256, 768]


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
    a, w, bias = _ints(M, K, seed=3 * K + M), _ints(N, K, seed=5 * K + N), _ints(N, seed=N + 1)
    a, w, bias = a.to(DEV), w.to(DEV), bias.to(DEV)
    ref = a.double() @ w.double().t()
    assert float(ref.abs().max()) + 3 < 2 ** 24
    return a.to(torch.bfloat16), w.to(torch.bfloat16), bias.float(), ref


def _rne_bf16(x64):
    return x64.float().to(torch.bfloat16)  # integers < 2^24: fp64 -> fp32 is exact, then one RNE


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M", [257, 512])
def test_qkv_scatter_exact(M, K):
    """EPI_QKV on the 64x96 tile (N = 3 x 192), ragged and full last row tile: q rows and the K/V rows
    scattered to permuted slots and positions; q_out and both whole caches equal the reference."""
    ops = _ops()
    D, T = 192, 11
    H = D // 64
    a, w, bias, ref = _case(M, 3 * D, K)
    ref = _rne_bf16(ref + bias.double())
    g = torch.Generator(device="cpu").manual_seed(5 + K)
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


@pytest.mark.parametrize("K", KS)
def test_bf16_without_bias_exact(K):
    """EPI_BF16 with a null bias pointer (the prefetch must not touch it), one-row last tile."""
    ops = _ops()
    M, N = 65, 384
    a, w, _, ref = _case(M, N, K)
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    ops.gemm_tile_reset()
    ops.gemm(a, w, ops.EPI_BF16, out=out)
    assert ops.gemm_tile_count(64, 64) == 1
    assert torch.equal(out, _rne_bf16(ref))


@pytest.mark.parametrize("K", KS)
def test_partial_exact(K):
    """EPI_PARTIAL (no bias by construction), one K slice, one-row last tile: the fp32 slab."""
    ops = _ops()
    M, N = 65, 384
    a, w, _, ref = _case(M, N, K)
    out = torch.full((1, M, N), float("nan"), device=DEV)
    ops.gemm_tile_reset()
    ops.gemm(a, w, ops.EPI_PARTIAL, out=out, split_k=1)
    assert ops.gemm_tile_count(64, 64) == 1
    assert torch.equal(out[0], ref.float())


# forced tile id -> (BM, BN), as in test_gemm_decode_loop_gpu.py
FORCED = {0: (32, 64), 1: (64, 64), 4: (64, 64), 7: (64, 64), 15: (32, 128), 17: (64, 96), 18: (64, 96),
          19: (64, 96)}


@pytest.mark.parametrize("K", [128, 320])
@pytest.mark.parametrize("tile", sorted(FORCED))
def test_forced_tiles_bias_exact_and_repeatable(tile, K):
    """EPI_BF16 with a bias on every forced small tile (ring depths 2 ... 6; K = 128 is shorter than
    every ring but the 2-deep one, 320 longer than most), launched twice: equal results."""
    ops = _ops()
    L = ops.lib()
    M, N = 65, 384
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


def _penalised(logits, seen, p):
    bits = ((seen.long().unsqueeze(-1) >> torch.arange(32, device=DEV)) & 1).reshape(seen.shape[0], -1).bool()
    bits = bits[:, :logits.shape[1]]
    return torch.where(bits, torch.where(logits < 0, logits * p, logits / p), logits)


def _first_argmax(x):
    """Lowest index among the maxima of each row."""
    n = x.shape[1]
    idx = torch.arange(n, device=x.device).expand_as(x)
    return torch.where(x == x.max(dim=1, keepdim=True).values, idx, n).min(dim=1).values


# (4, 2, 1) with K % 256 == 0 is the 8-k-block instance (one and three chunks per tile); the others
# run 4-k-block chunks, (5, 2, 1) on an 80-row panel with two seen words per lane
@pytest.mark.parametrize("M", [65, 128])
@pytest.mark.parametrize("geo,K", [((4, 2, 1), 256), ((4, 2, 1), 768), ((4, 2, 1), 128), ((4, 2, 1), 384),
                                   ((5, 2, 1), 128), ((5, 2, 1), 384)])
def test_lm_head_argmax_exact(geo, K, M):
    """gemm_ps EPI_ARGMAX on 8 wave slots, N = 608 = 19 column tiles (a ragged last round), vocab 600:
    integer logits (many ties: the lowest index wins), a seen bitmap that penalises the unpenalised
    argmax of every other row; the token equals torch's on fp32 logits with the same penalty rule."""
    ops = _ops()
    N, V, P = 608, 600, 1.2
    a, w, _, ref = _case(M, N, K)
    logits = ref.float()
    logits[:, V:] = -float("inf")
    top = _first_argmax(logits)
    seen = torch.zeros(M, N // 32, dtype=torch.int64, device=DEV)
    rows = torch.arange(0, M, 2, device=DEV)
    seen[rows, top[rows] >> 5] = 1 << (top[rows] & 31)
    seen[:, 3] |= 0x00F0F00F  # ... and a fixed pattern in every row
    seen = torch.where(seen >= 2 ** 31, seen - 2 ** 32, seen).to(torch.int32)
    want = _first_argmax(_penalised(logits, seen, P))
    keys = torch.zeros(M, 8 * geo[2], dtype=torch.int64, device=DEV)
    ops.gemm_ps(a, ops.shuffle_weight(w), ops.EPI_ARGMAX, argmax_out=keys, seen=seen, vocab=V, penalty=P,
                geometry=geo)
    tok = (~ops.argmax_reduce(keys)) & 0xFFFFFFFF
    assert torch.equal(tok, want)
    assert (want[rows] != top[rows]).any()  # the penalty moved some argmax


def _u64_max(keys):
    """Row-wise max of int64 keys compared as unsigned."""
    flip = torch.tensor(-2 ** 63, dtype=torch.int64, device=keys.device)
    return (keys ^ flip).max(dim=1).values ^ flip


@functools.lru_cache(maxsize=None)
def _keys(B, nparts, V):
    g = torch.Generator(device="cpu").manual_seed(31 + nparts)
    hi = torch.randint(0, 2 ** 32, (B, nparts), generator=g)  # both halves of the unsigned range
    tok = torch.randint(0, V, (B, nparts), generator=g)
    k = (hi << 32) | (~tok & 0xFFFFFFFF)  # wraps into the signed range: the same 64 bits
    return k.to(DEV)


NPARTS = [1, 63, 64, 65, 256, 800, 1025]


@pytest.mark.parametrize("nparts", NPARTS)
def test_argmax_reduce_unsigned_max(nparts):
    ops = _ops()
    keys = _keys(5, nparts, 3000)
    assert torch.equal(ops.argmax_reduce(keys), _u64_max(keys))


@pytest.mark.parametrize("nparts", NPARTS)
def test_decode_update_key_rounds(nparts):
    """decode_update over 1 ... 1025 partial keys per row (less than a lane round, one, two rounds),
    B = 5 (two workgroups) with one finished row: the token is the max-key token, x the embedding sum
    and the fused LN row what add_layernorm writes from the stored row."""
    ops = _ops()
    V, P, D, B, T = 3000, 64, 768, 5, 40
    g = torch.Generator(device="cpu").manual_seed(41)
    wte = torch.randn(V, D, generator=g).to(torch.bfloat16).to(DEV)
    wpe = torch.randn(P, D, generator=g).to(torch.bfloat16).to(DEV)
    gam, bet = torch.randn(D, generator=g).to(DEV), torch.randn(D, generator=g).to(DEV)
    keys = _keys(B, nparts, V)
    lens = torch.tensor([3, 17, 1, 9, 22], dtype=torch.int32, device=DEV)
    fin = torch.tensor([0, 0, 0, 1, 0], dtype=torch.int32, device=DEV)
    out = torch.randint(0, V, (B, T), generator=g).to(torch.int32).to(DEV)
    out0 = out.clone()
    seen = torch.zeros(B, (V + 31) // 32, dtype=torch.int32, device=DEV)
    ct, cp, ck = (torch.zeros(B, dtype=torch.int32, device=DEV) for _ in range(3))
    x = torch.zeros(B, D, device=DEV)
    h = torch.full((B, D), float("nan"), dtype=torch.bfloat16, device=DEV)
    ops.decode_update(keys, lens, fin, out, seen, ct, cp, ck, wte, wpe, x, eos=V, t_max=T, ln=(gam, bet, 1e-5), h=h)
    want = ((~_u64_max(keys)) & 0xFFFFFFFF).to(torch.int32)
    want[3] = out0[3, 8]  # the finished row repeats its last token
    assert torch.equal(ct, want)
    assert lens.tolist() == [4, 18, 2, 9, 23] and cp.tolist() == [3, 17, 1, 8, 22] and ck.tolist() == [4, 18, 2, 9, 23]
    for b in (0, 1, 2, 4):
        assert out[b, cp[b]].item() == want[b].item()
    assert torch.equal(out[3], out0[3])
    torch.testing.assert_close(x, wte[ct.long()].float() + wpe[cp.long()].float())
    ref = torch.empty_like(h)
    ops.add_layernorm(x.clone(), gam, bet, 1e-5, out_bf16=ref)
    assert torch.equal(h.view(torch.int16), ref.view(torch.int16))

