"""Write-through (``sc1``) output stores of the decode GEMM epilogues (csrc/common.h ``st_wt*``, mask
``DLMS_WT_STORES`` / ``ops.wt_stores``): a store moved through L2 must move exactly the same bytes.
(Of the five kernel families measured, docs/PERFORMANCE.md round 9, only the GEMM epilogues kept
such stores; the others have no switch to test.)

Every kernel test runs one GEMM twice on the same inputs, first with the family's bit off, then on,
in one process.  Every output buffer lies between two guard bands of a sentinel pattern and starts
out filled with the pattern itself, and the two runs' whole allocations -- bands, outputs, rows and
slots the kernel must not touch -- have to be equal byte for byte (and the bands intact), so a store
helper with a wrong width or address shows as a changed or a missing byte somewhere.  Shapes are the
smallest that reach every store path."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 256  # bytes on either side of an output (keeps the 16-byte alignment of the buffer inside)


def _ops():
    from distributed_lms_raft_llm_amd import ops

    ops.lib()
    return ops


def _guarded(shape, dtype, init=None):
    """(raw uint8 allocation, view of its middle as ``shape`` / ``dtype``): sentinel bytes 1 ... 251
    everywhere, ``init`` copied into the view when the kernel also reads the buffer."""
    n = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
    raw = ((torch.arange(n + 2 * GUARD, dtype=torch.int64) * 37 + 11) % 251 + 1).to(torch.uint8).to(DEV)
    view = raw[GUARD:GUARD + n].view(dtype).view(shape)
    if init is not None:
        view.copy_(init)
    return raw, view


def _off_on(make, bit):
    """``make()`` -> (launch, [raw allocations]) on fresh, identical buffers.  Runs it with the mask 0
    and with ``bit``; checks the guard bands, that the kernel wrote something, and that the two runs
    left the same bytes everywhere."""
    ops = _ops()
    runs = []
    for mask in (0, bit):
        launch, raws = make()
        before = [r.clone() for r in raws]
        old = ops.wt_stores(mask)
        try:
            assert ops.wt_stores() == mask
            launch()
            torch.cuda.synchronize()
        finally:
            ops.wt_stores(old)
        for r, b in zip(raws, before):
            assert torch.equal(r[:GUARD], b[:GUARD]) and torch.equal(r[-GUARD:], b[-GUARD:]), "guard band overwritten"
            assert not torch.equal(r, b), "an output buffer was not written at all"
        runs.append(raws)
    for i, (a, b) in enumerate(zip(*runs)):
        assert torch.equal(a, b), f"output {i}: {(a != b).sum().item()} bytes differ between plain and write-through"


def _rand_bf16(*shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).to(DEV)


def _forced(ops, tile, fn):
    L = ops.lib()
    L.dlms_gemm_force_tile(tile)
    try:
        fn()
    finally:
        L.dlms_gemm_force_tile(-1)


# forced tile ids (gemm.hip launch_forced): 1 = 64x64, 17 = 64x96, both 4 ring stages
TILES = {1: (64, 64), 17: (64, 96)}


@pytest.mark.parametrize("tile", sorted(TILES))
@pytest.mark.parametrize("K,split", [(256, 2), (512, 4)])
def test_gemm_partial_slabs(K, split, tile):
    """EPI_PARTIAL: 70 rows (a ragged second 64-row tile) x 192 columns, every slab whole -- the slabs
    hold 72 rows, so rows >= M, which the kernel must leave alone, are compared as well."""
    ops = _ops()
    M, N = 70, 192
    a, w = _rand_bf16(M, K, seed=K), _rand_bf16(N, K, seed=K + 1)

    def make():
        raw, out = _guarded((split, M + 2, N), torch.float32)

        def launch():
            ops.gemm_tile_reset()
            _forced(ops, tile, lambda: ops.gemm(a, w, ops.EPI_PARTIAL, out=out, split_k=split))
            assert ops.gemm_tile_count(*TILES[tile]) == 1
        return launch, [raw]

    _off_on(make, ops.WT_GEMM)


@pytest.mark.parametrize("tile", sorted(TILES))
def test_gemm_gelu_rows(tile):
    """EPI_GELU_TANH (c_fc): 70 x 192, K = 128."""
    ops = _ops()
    M, N, K = 70, 192, 128
    a, w = _rand_bf16(M, K, seed=3), _rand_bf16(N, K, seed=4, scale=0.1)
    bias = torch.linspace(-1, 1, N, device=DEV)

    def make():
        raw, out = _guarded((M + 2, N), torch.bfloat16)
        return (lambda: _forced(ops, tile, lambda: ops.gemm(a, w, ops.EPI_GELU_TANH, bias=bias, out=out))), [raw]

    _off_on(make, ops.WT_GEMM)


@pytest.mark.parametrize("kv,tile", [("bf16", 1), ("bf16", 17), ("e4m3", -1)])
def test_gemm_qkv_scatter(kv, tile):
    """EPI_QKV: 70 rows, 2 heads (N = 384), K = 128, t_max = 8, rows scattered to non-contiguous slots
    and different positions; q and both whole caches (80 slots, 10 of them never written) compared.
    The e4m3 cache has no forced-tile build: the heuristic's tile (BM <= 64 at 70 rows)."""
    ops = _ops()
    M, H, K, T, S = 70, 2, 128, 8, 80
    a, w = _rand_bf16(M, K, seed=5), _rand_bf16(3 * H * 64, K, seed=6, scale=0.2)
    bias = torch.linspace(-2, 2, 3 * H * 64, device=DEV)
    g = torch.Generator(device="cpu").manual_seed(7)
    slot = torch.randperm(S, generator=g)[:M].to(torch.int32).to(DEV)
    pos = ((torch.arange(M) * 5 + 3) % T).to(torch.int32).to(DEV)
    cdt = ops.FP8 if kv == "e4m3" else torch.bfloat16

    def make():
        rq, q = _guarded((M + 2, H * 64), torch.bfloat16)
        rk, kc = _guarded((S, H, T, 64), cdt)
        rv, vc = _guarded((S, H, T, 64), cdt)

        def launch():
            _forced(ops, tile, lambda: ops.gemm(a, w, ops.EPI_QKV, bias=bias, q_out=q, k_cache=kc, v_cache=vc,
                                                row_slot=slot, row_pos=pos))
        return launch, [rq, rk, rv]

    _off_on(make, ops.WT_GEMM)


def test_engine_overlapped_step_tokens_equal():
    """The overlapped two-stream decode step at 16 queries (8 steps per graph, 4-token prompts to 24
    tokens): tokens and lengths with every write-through store off equal those with the default mask
    (the GEMM epilogues' bit, unless the environment says otherwise)."""
    from distributed_lms_raft_llm_amd.engine.gpt2_engine import HipGPT2Engine
    from distributed_lms_raft_llm_amd.models.config import gpt2_config
    from distributed_lms_raft_llm_amd.models.gpt2 import init_gpt2_weights

    ops = _ops()
    cfg = gpt2_config("gpt2")
    w = init_gpt2_weights(cfg, seed=0)
    g = torch.Generator().manual_seed(9)
    prompts = [torch.randint(0, cfg.vocab_size - 1, (4,), generator=g).tolist() for _ in range(16)]
    default = ops.wt_stores()
    if not os.environ.get("DLMS_WT_STORES"):
        assert default == ops.WT_GEMM
    got = {}
    for mask in (0, ops.WT_GEMM):
        ops.wt_stores(mask)
        try:
            eng = HipGPT2Engine(cfg, w, max_batch=16, max_length=24, overlap=True, overlap_min_batch=2, overlap_parts=2)
            eng.mid_max = 0  # (the mid path would take the 16-row steps ahead of the overlapped one)
            assert eng._overlap_ok(16) and eng.steps_per_graph == 8
            got[mask] = eng.generate(prompts)
            eng.close()
        finally:
            ops.wt_stores(default)
    assert got[0] == got[ops.WT_GEMM]
    assert all(4 < len(o) <= 24 for o in got[0])
