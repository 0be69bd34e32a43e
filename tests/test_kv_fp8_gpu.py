"""fp8 (e4m3) KV cache on the GPU: the QKV GEMM's e4m3 scatter (bit-exact against the quantiser on
the bf16 cache's content), the fp8 decode attention kernels and the fp8 tile attention (against
fp32 torch attention over the dequantised cache, the bf16 kernels' tolerance: dequantisation is
exact, so the arithmetic error is the same), and ``HipGPT2Engine(kv_dtype="fp8")`` against
``GPT2Reference(kv_dtype="fp8")`` with the teacher-forced margin rule.

The margin ``eps`` is derived on the CPU from the reference alone (kv_fp8_cases.py, recomputed by
tests/test_kv_fp8_cpu.py): GPT-2-124M 0.25 (fp8 deviation 0.0588 against bf16 0.0119 -> 0.247),
gpt2-tiny 0.10 (0.0042 / 0.0022 -> 0.094), gpt2-medium 0.29 (0.0972 / 0.0171 -> 0.285)."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

import kv_fp8_cases as kc

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_BYTE = 0x7F


def _ops():
    from distributed_lms_raft_llm_amd import ops

    ops.lib()
    return ops


def _quant(x):
    from distributed_lms_raft_llm_amd.models.gpt2 import quantize_kv_e4m3

    return quantize_kv_e4m3(x)


def _nan_filled(*shape):
    return torch.full(shape, NAN_BYTE, dtype=torch.uint8, device=DEV).view(torch.float8_e4m3fn)


# ------------------------------------------------------------------------------------------------
# QKV GEMM: e4m3 scatter
# ------------------------------------------------------------------------------------------------
# (M, d, heads, the tile the launcher must have taken)
SCATTER_CASES = [(1, 768, 12, (32, 64)), (63, 768, 12, (32, 64)), (65, 768, 12, (64, 64)), (257, 768, 12, (64, 96)),
                 (512, 768, 12, (64, 96)), (4096, 768, 12, (256, 256)), (8192, 768, 12, (128, 128)),
                 (16384, 768, 12, (256, 256)), (65, 1600, 25, (64, 64))]


@pytest.mark.parametrize("M,d,H,tile", SCATTER_CASES)
def test_qkv_scatter_is_the_quantised_bf16_cache(M, d, H, tile):
    """The same QKV GEMM into a bf16 cache and into an fp8 cache pre-filled with the NaN byte: the
    written fp8 values are the quantiser applied to the bf16 cache's values there, exactly; every
    other byte is untouched; q is identical.  96-column tiles straddle the 64-wide heads; M = 512
    takes the 64x96 tiles, 8192 the 128x128 ones, 16384 the 8-phase kernel (4096: 256x256)."""
    ops = _ops()
    T = 19  # not a multiple of 16
    S = M // T + 3
    g = torch.Generator().manual_seed(M + d)
    a = torch.randn(M, d, generator=g).to(DEV).bfloat16()
    w = (torch.randn(3 * d, d, generator=g) * 0.05).to(DEV).bfloat16()
    bias = torch.randn(3 * d, generator=g).to(DEV)
    # columns that pin the edges of the format: zero weights, so the value is the bias itself --
    # saturation on both sides, the smallest subnormal, the tie below it, a tie at step 2
    edge = [1000.0, -1e9, 448.0, -449.0, 2.0 ** -9, 2.0 ** -10, -3 * 2.0 ** -10, 17.0, 19.0, 1e-6, 0.0, 464.0]
    cols = [d + 5 + 61 * i for i in range(len(edge))] + [2 * d + 3 + 59 * i for i in range(len(edge))]
    w[cols] = 0
    bias[cols] = torch.tensor(edge + edge, device=DEV)
    # rows -> distinct (slot, position) pairs: slots a permutation, positions ragged, 0 and T - 1 used
    need = torch.tensor([(S - 1) * T + (T - 1)] + ([2 * T] if M > 1 else []))  # position T - 1, position 0
    perm = torch.randperm(S * T, generator=g)
    pairs = torch.cat([need, perm[~torch.isin(perm, need)][: M - need.numel()]])
    pairs = pairs[torch.randperm(M, generator=g)]
    slot = (pairs // T).to(torch.int32).to(DEV)
    pos = (pairs % T).to(torch.int32).to(DEV)
    assert int(pos.max()) == T - 1 and (M == 1 or int(pos.min()) == 0) and pairs.unique().numel() == M

    k16 = torch.zeros(S, H, T, 64, dtype=torch.bfloat16, device=DEV)
    v16 = torch.zeros_like(k16)
    q16 = torch.zeros(M, d, dtype=torch.bfloat16, device=DEV)
    ops.gemm(a, w, ops.EPI_QKV, bias=bias, q_out=q16, k_cache=k16, v_cache=v16, row_slot=slot, row_pos=pos)
    k8, v8 = _nan_filled(S, H, T, 64), _nan_filled(S, H, T, 64)
    q8 = torch.zeros_like(q16)
    ops.gemm_tile_reset()
    ops.gemm(a, w, ops.EPI_QKV, bias=bias, q_out=q8, k_cache=k8, v_cache=v8, row_slot=slot, row_pos=pos)
    assert ops.gemm_tile_count(*tile) == 1, tile
    assert torch.equal(q8, q16)
    written = torch.zeros(S, T, dtype=torch.bool, device=DEV)
    written[slot.long(), pos.long()] = True
    wmask = written[:, None, :, None].expand(S, H, T, 64)
    for c8, c16 in ((k8, k16), (v8, v16)):
        raw = c8.view(torch.uint8)
        assert bool((raw[~wmask] == NAN_BYTE).all())
        got = raw[wmask]
        assert not bool(((got == 0x7F) | (got == 0xFF)).any())
        torch.testing.assert_close(c8.float()[wmask], _quant(c16).float()[wmask], atol=0, rtol=0)
    # the edge columns did reach the cache as the definition says (head, dim of column d + 5: 0, 5)
    row0 = (int(slot[0]), int(pos[0]))
    assert k8[row0[0], 0, row0[1], 5].float().item() == 448.0 and k16[row0[0], 0, row0[1], 5].float().item() == 1000.0


def test_ops_refuse_mixed_and_unbuilt_fp8_caches():
    ops = _ops()
    H, T = 2, 32
    k8, v8 = _nan_filled(2, H, T, 64), _nan_filled(2, H, T, 64)
    k16 = torch.zeros(2, H, T, 64, dtype=torch.bfloat16, device=DEV)
    q = torch.zeros(2, H * 64, dtype=torch.bfloat16, device=DEV)
    idx = torch.zeros(2, dtype=torch.int32, device=DEV)
    one = torch.ones(2, dtype=torch.int32, device=DEV)
    a = torch.zeros(2, 128, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(3 * H * 64, 128, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError):
        ops.gemm(a, w, ops.EPI_QKV, q_out=q, k_cache=k8, v_cache=k16, row_slot=idx, row_pos=idx)
    with pytest.raises(ValueError):  # W8A8 weights x fp8 cache: no such build
        ops.gemm(a.to(ops.FP8), w.to(ops.FP8), ops.EPI_QKV, q_out=q, k_cache=k8, v_cache=v8, row_slot=idx, row_pos=idx,
                 a_scale=torch.ones(2, device=DEV), w_scale=torch.ones(w.shape[0], device=DEV))
    for impl in ("wave", "persist"):
        with pytest.raises(ValueError):
            ops.row_attention(q, k16, v8, idx, one, impl=impl)
    with pytest.raises(ValueError):  # the LDS two-pass kernel is not ported
        ops.row_attention(q, k8, v8, idx, one, impl="lds")
    with pytest.raises(ValueError):
        ops.tile_attention(q, k8, k16, idx, one, ops.AttnTiles([2], DEV))


# ------------------------------------------------------------------------------------------------
# decode attention (wave and persistent kernels)
# ------------------------------------------------------------------------------------------------
KVLENS = [1, 2, 15, 16, 17, 31, 33, 63, 64, 65, 150, 1024]  # around 16 keys / instruction, 64- and 128-key blocks
ATT_T = 1024
ATT_SLOTS = 16


@functools.lru_cache(maxsize=None)
def _attn_case(H):
    """One fp8 cache per head count, shared by the attention tests (never modified): slot s holds
    kvlen KVLENS[s % 12] valid keys; ``nan`` caches hold the NaN byte at every later position, the
    ``plain`` ones ordinary values there."""
    g = torch.Generator().manual_seed(100 + H)
    S, T = ATT_SLOTS, ATT_T
    kvlen = torch.tensor([KVLENS[s % len(KVLENS)] for s in range(S)])
    k = _quant(torch.randn(S, H, T, 64, generator=g).to(DEV))
    v = _quant((torch.randn(S, H, T, 64, generator=g) * 2).to(DEV))
    tail = (torch.arange(T)[None, :] >= kvlen[:, None]).to(DEV)[:, None, :, None].expand(S, H, T, 64)
    kn, vn = k.clone(), v.clone()
    kn.view(torch.uint8)[tail] = NAN_BYTE
    vn.view(torch.uint8)[tail] = NAN_BYTE
    q = torch.randn(300, H * 64, generator=g).to(DEV).bfloat16()
    return dict(k=k, v=v, kn=kn, vn=vn, q=q, kvlen=kvlen)


def _attn_ref(c, H, row_slot):
    """fp32 torch attention over the dequantised cache, per row."""
    out = torch.empty(row_slot.numel(), H * 64, device=DEV)
    for s in row_slot.unique().tolist():
        rows = (row_slot == s).nonzero()[:, 0]
        L = int(c["kvlen"][s])
        K, V = c["k"][s, :, :L].float(), c["v"][s, :, :L].float()
        qq = c["q"][rows].float().view(-1, H, 64)
        p = torch.softmax(torch.einsum("rhd,htd->rht", qq, K) / 8.0, -1)
        out[rows] = torch.einsum("rht,htd->rhd", p, V).reshape(-1, H * 64)
    return out


@pytest.mark.parametrize("impl", ["wave", "persist"])
@pytest.mark.parametrize("H", [12, 25])
@pytest.mark.parametrize("R", [1, 5, 12, 300])
def test_fp8_decode_attention(R, H, impl):
    """H = 25: the last workgroup of a row has idle waves; R = 300 with 64 persistent workgroups:
    the grid (256 waves) is smaller than the pair count; slots permuted; R = 12 / 300 reach every
    kvlen of KVLENS."""
    ops = _ops()
    c = _attn_case(H)
    row_slot = torch.tensor([11 - r if R == 12 else (7 * r + 3) % ATT_SLOTS for r in range(R)], dtype=torch.int32,
                            device=DEV)
    kvl = c["kvlen"][row_slot.cpu().long()].to(torch.int32).to(DEV)
    if R >= 12:
        assert set(kvl.tolist()) == set(KVLENS)
    q = c["q"][:R]
    kw = dict(impl=impl, blocks=64)
    out = ops.row_attention(q, c["kn"], c["vn"], row_slot, kvl, **kw)
    assert torch.isfinite(out.float()).all()
    torch.testing.assert_close(out.float(), _attn_ref(c, H, row_slot), atol=2e-2, rtol=2e-2)
    # the bytes past kvlen are never used: the same output over ordinary values there, and again
    assert torch.equal(out, ops.row_attention(q, c["k"], c["v"], row_slot, kvl, **kw))
    assert torch.equal(out, ops.row_attention(q, c["kn"], c["vn"], row_slot, kvl, **kw))


def test_fp8_decode_attention_kernels_agree_with_the_bf16_kernels():
    """The same (dequantised) cache through the bf16 kernels: the fp8 kernels' results are as close
    to them as two summation orders of the same products are."""
    ops = _ops()
    H = 12
    c = _attn_case(H)
    row_slot = torch.arange(12, dtype=torch.int32, device=DEV)
    kvl = c["kvlen"][:12].to(torch.int32).to(DEV)
    k16, v16 = c["k"].to(torch.bfloat16), c["v"].to(torch.bfloat16)
    for impl in ("wave", "persist"):
        a = ops.row_attention(c["q"][:12], c["k"], c["v"], row_slot, kvl, impl=impl)
        b = ops.row_attention(c["q"][:12], k16, v16, row_slot, kvl, impl=impl)
        torch.testing.assert_close(a.float(), b.float(), atol=1.6e-2, rtol=1.6e-2)


def test_fp8_tile_attention_matches_fp32():
    ops = _ops()
    H, T = 5, 40
    lens = [1, 7, 16, 17, 32, 33]
    R, n = sum(lens), len(lens)
    g = torch.Generator().manual_seed(7)
    q = torch.randn(R, H * 64, generator=g).to(DEV).bfloat16()
    k = _quant(torch.randn(n + 2, H, T, 64, generator=g).to(DEV))
    v = _quant((torch.randn(n + 2, H, T, 64, generator=g) * 2).to(DEV))
    slots = [(3 * b + 1) % (n + 2) for b in range(n)]
    assert len(set(slots)) == n
    kn, vn = k.clone(), v.clone()
    for b, L in enumerate(lens):  # the NaN byte past every sequence's end
        kn.view(torch.uint8)[slots[b], :, L:] = NAN_BYTE
        vn.view(torch.uint8)[slots[b], :, L:] = NAN_BYTE
    row_slot = torch.tensor([slots[b] for b, L in enumerate(lens) for _ in range(L)], dtype=torch.int32, device=DEV)
    kvl = torch.tensor([i + 1 for L in lens for i in range(L)], dtype=torch.int32, device=DEV)
    tiles = ops.AttnTiles(lens, DEV)
    out = ops.tile_attention(q, kn, vn, row_slot, kvl, tiles)
    assert torch.isfinite(out.float()).all()
    row = 0
    for b, L in enumerate(lens):
        s = slots[b]
        K, V = k[s, :, :L].float(), v[s, :, :L].float()
        qq = q[row: row + L].float().view(L, H, 64).transpose(0, 1)
        sc = (torch.einsum("hqd,hkd->hqk", qq, K) / 8.0).masked_fill(torch.ones(L, L, device=DEV).triu(1).bool(),
                                                                     float("-inf"))
        ref = torch.einsum("hqk,hkd->hqd", torch.softmax(sc, -1), V).transpose(0, 1).reshape(L, H * 64)
        torch.testing.assert_close(out[row: row + L].float(), ref, atol=2e-2, rtol=2e-2)
        row += L
    assert torch.equal(out, ops.tile_attention(q, kn, vn, row_slot, kvl, tiles))
    # widening to bf16 is exact: the bf16 kernel on the dequantised cache gives the same bits
    assert torch.equal(out, ops.tile_attention(q, k.to(torch.bfloat16), v.to(torch.bfloat16), row_slot, kvl, tiles))


# ------------------------------------------------------------------------------------------------
# engine
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(name):
    from distributed_lms_raft_llm_amd.models.gpt2 import GPT2Reference

    cfg, w = kc.setup(name)
    return cfg, w, GPT2Reference(cfg, w, device=DEV, kv_dtype="fp8")


def _engine(name, **kw):
    from distributed_lms_raft_llm_amd.engine.gpt2_engine import HipGPT2Engine

    cfg, w, _ = _model(name)
    return HipGPT2Engine(cfg, w, kv_dtype="fp8", **kw)


def _assert_teacher_forced(name, outs, prompts, T):
    from distributed_lms_raft_llm_amd.models.gpt2 import teacher_forced_check_batch

    _, _, model = _model(name)
    eps = kc.KV_FP8_EPS[name]
    for o, p in zip(outs, prompts):
        assert o[: len(p)] == p and len(o) <= T
    res = teacher_forced_check_batch(model, outs, [len(p) for p in prompts], 1.2, eps)
    total, decisive = sum(r["positions"] for r in res), sum(r["decisive"] for r in res)
    bad = [(i, r["mismatches"][:2]) for i, r in enumerate(res) if r["mismatches"]]
    print(f"{name} batch {len(prompts)}: {decisive} / {total} positions decisive at eps {eps}, "
          f"{sum(len(r['mismatches']) for r in res)} mismatches")
    assert not bad, bad[:4]
    assert total > 0 and decisive > 0 and decisive >= kc.MIN_DECISIVE[name] * total, (decisive, total)


@pytest.mark.parametrize("batch", [1, 3, 9, 64, 512])
def test_fp8_engine_matches_the_fp8_reference(batch):
    """GPT-2-124M, T = 48: every batch size runs the tiled step (wave attention; 512: the overlapped
    parts with the persistent attention), held to ``GPT2Reference(kv_dtype="fp8")``."""
    ops = _ops()
    T = 48
    eng = _engine("gpt2", max_batch=max(8, batch), max_length=T)
    assert eng.kv.dtype == ops.FP8 and eng.kv_dtype == "fp8"
    assert not eng.dataflow and eng.small_max == 0 and eng.mid_max == 0 and not eng.fuse_ao and not eng.fused_mlp
    assert not eng._small_ok(batch) and not eng._mid_ok(batch) and not eng._df_ok(batch)
    assert eng._overlap_ok(batch) == (batch == 512) and eng.persist_attn_blocks > 0
    cfg = eng.cfg
    lens = ([5, 20, 11, 1, 30, 8, 16, 2] * ((batch + 7) // 8))[:batch]
    prompts = kc.prompts(cfg, lens)
    got = eng.generate(prompts, repetition_penalty=1.2)
    _assert_teacher_forced("gpt2", got, prompts, T)


@pytest.mark.parametrize("name", ["gpt2-tiny", "gpt2-medium"])
def test_fp8_engine_other_widths(name):
    T = 48
    eng = _engine(name, max_batch=8, max_length=T)
    prompts = kc.prompts(eng.cfg, [5, 20, 11])
    _assert_teacher_forced(name, eng.generate(prompts, repetition_penalty=1.2), prompts, T)


def test_fp8_engine_cache_bytes_and_planner():
    from distributed_lms_raft_llm_amd.engine.gpt2_engine import HipGPT2Engine
    from distributed_lms_raft_llm_amd.engine.memory import kv_bytes

    cfg, w, _ = _model("gpt2-tiny")
    a = HipGPT2Engine(cfg, w, max_batch=4, max_length=24)
    b = HipGPT2Engine(cfg, w, max_batch=4, max_length=24, kv_dtype="fp8")
    assert a.kv.dtype == torch.bfloat16 and a.kv_dtype == "bf16"
    assert 2 * b.kv_cache_bytes() == a.kv_cache_bytes() == 4 * kv_bytes(cfg, 24)
    assert b.kv_cache_bytes() == 4 * kv_bytes(cfg, 24, kv_dtype="fp8")


def test_fp8_engine_graph_replay_equals_eager_and_reruns():
    cfg, _, _ = _model("gpt2")
    prompts = kc.prompts(cfg, [32] * 5 + [9, 17])
    eng = _engine("gpt2", max_batch=8, max_length=64, use_graph=True)
    a = eng.generate(prompts)
    assert eng._graphs
    assert eng.generate(prompts) == a
    assert _engine("gpt2", max_batch=8, max_length=64, use_graph=False).generate(prompts) == a


def test_fp8_engine_continuous_batching_matches_serving_alone():
    """Staggered admissions into a running batch (8 slots, 12 requests; the prefill split-K pinned,
    as tests/test_engine_gpu.py does) produce what serving each prompt alone produces."""
    from distributed_lms_raft_llm_amd.engine.scheduler import ContinuousBatcher

    cfg, _, _ = _model("gpt2")
    T = 48
    prompts = kc.prompts(cfg, [3, 30, 12, 1, 25, 7, 40, 16, 2, 33, 9, 47], seed=3)
    eng = _engine("gpt2", max_batch=8, max_length=T, prefill_split=2)
    cb = ContinuousBatcher(eng, repetition_penalty=1.2, chunk=4)
    try:
        got = [f.result(120) for f in [cb.submit(p) for p in prompts]]
    finally:
        cb.stop()
    solo = _engine("gpt2", max_batch=1, max_length=T, prefill_split=2)
    for g_, p in zip(got, prompts):
        assert g_ == solo.generate([p], repetition_penalty=1.2)[0]
    assert cb.completed == len(prompts)


def test_fp8_engine_samples_reproducibly():
    from distributed_lms_raft_llm_amd.models.config import SamplingParams

    cfg, _, _ = _model("gpt2")
    prompts = kc.prompts(cfg, [5, 20, 11])
    eng = _engine("gpt2", max_batch=8, max_length=40)
    sp = SamplingParams(0.7, 50, 0.9, 11)
    a = eng.generate(prompts, sampling=sp)
    assert all(o[: len(p)] == p and len(p) < len(o) <= 40 for o, p in zip(a, prompts))
    assert eng.generate(prompts, sampling=sp) == a
    assert eng.generate(prompts, sampling=SamplingParams(0.7, 50, 0.9, 12)) != a
    assert eng.kv.dtype == torch.float8_e4m3fn  # the sampler does not touch the cache


def test_fp8_engine_refuses_tp_and_fp8_weights():
    from distributed_lms_raft_llm_amd.engine.gpt2_engine import HipGPT2Engine

    cfg, w, _ = _model("gpt2-tiny")
    with pytest.raises(ValueError, match="fp8 weights"):
        HipGPT2Engine(cfg, w, max_batch=4, max_length=24, kv_dtype="fp8", weight_dtype="fp8")
    with pytest.raises(ValueError, match="tensor parallelism"):
        HipGPT2Engine(cfg, w, max_batch=4, max_length=24, kv_dtype="fp8", tp_group=object())
    with pytest.raises(ValueError):
        HipGPT2Engine(cfg, w, max_batch=4, max_length=24, kv_dtype="int8")


CHECKED_SCRIPT = r"""
import json, sys, torch
sys.path.insert(0, "tests")
import kv_fp8_cases as kc
from distributed_lms_raft_llm_amd import ops
from distributed_lms_raft_llm_amd.engine.gpt2_engine import HipGPT2Engine
assert ops.checked_mode()
cfg, w = kc.setup("gpt2-tiny")
eng = HipGPT2Engine(cfg, w, max_batch=8, max_length=40, kv_dtype="fp8")
out = eng.generate(kc.prompts(cfg, [5, 20, 11, 1, 17]))
print("RESULT " + json.dumps({"lens": [len(o) for o in out], "errors": ops.device_errors(),
                              "dtype": str(eng.kv.dtype)}))
"""


def test_fp8_engine_checked_build_reports_no_device_errors():
    env = dict(os.environ, DLMS_KERNEL_CHECKS="1", PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-c", CHECKED_SCRIPT], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert res["errors"] == [] and res["dtype"] == "torch.float8_e4m3fn" and all(n <= 40 for n in res["lens"]), res
