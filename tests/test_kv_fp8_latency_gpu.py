"""fp8 (e4m3) KV cache on the latency and mid-batch decode paths: the skinny / fused add+LN / mid QKV
epilogues' e4m3 scatter (bit-exact against the quantiser on the bf16 cache's content), the split
attention and the fused attention + out-projection kernels reading the byte cache (against fp32
torch attention over the dequantised cache at the bf16 kernels' tolerances: dequantisation is exact,
so the arithmetic error class is the same), and ``HipGPT2Engine(kv_dtype="fp8", latency_path=True)``
against ``GPT2Reference(kv_dtype="fp8")`` with the teacher-forced margin rule.

The fp8 builds of the three attention kernels keep the bf16 kernels' lane mapping (lane (g, c) owns
dims [8c, 8c + 8) of key 8i + g, with 8-byte loads) and widen exactly, so every product and every
sum is the bf16 kernel's on ``cache.to(bfloat16)``: those comparisons are ``torch.equal``.

The cache, reference and engine helpers are those of tests/test_kv_fp8_gpu.py (one cached fp8 cache
per head count, never modified); the engine prompts are kv_fp8_latency_cases.py's."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

import kv_fp8_cases as kc
import kv_fp8_latency_cases as lc
from test_kv_fp8_gpu import (ATT_SLOTS, KVLENS, NAN_BYTE, _assert_teacher_forced, _attn_case, _attn_ref, _engine, _model,
                             _nan_filled, _ops, _quant)

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-5


# ------------------------------------------------------------------------------------------------
# 1. QKV epilogues: e4m3 scatter, bit-exact
# ------------------------------------------------------------------------------------------------
def _run_qkv(ops, op, x, w_sh, g, b, bias, q, k, v, slot, pos):
    kw = dict(bias=bias, q_out=q, k_cache=k, v_cache=v, row_slot=slot, row_pos=pos)
    if op == "skinny":
        ops.skinny_gemm(x, w_sh, ops.EPI_QKV, ln=(g, b, EPS), **kw)
    elif op == "addln":
        ops.skinny_addln_gemm(x, w_sh, ops.EPI_QKV, g, b, EPS, **kw)
    else:
        ops.mid_ln_gemm(x, w_sh, ops.EPI_QKV, g, b, EPS, **kw)


# M = -1: skinny_addln_max_rows(d); mid 17: a ragged second row tile
SCATTER_CASES = [("skinny", 1, 768, 12), ("skinny", 5, 768, 12), ("skinny", 32, 768, 12), ("skinny", 5, 1024, 16),
                 ("addln", 1, 768, 12), ("addln", -1, 768, 12), ("addln", -1, 1024, 16),
                 ("mid", 3, 768, 12), ("mid", 17, 768, 12), ("mid", 64, 768, 12), ("mid", 17, 1024, 16)]


@pytest.mark.parametrize("op,M,d,H", SCATTER_CASES)
def test_latency_qkv_scatter_is_the_quantised_bf16_cache(op, M, d, H):
    """The recipe of test_kv_fp8_gpu.py::test_qkv_scatter_is_the_quantised_bf16_cache for the three
    small-batch QKV kernels: the same op into a bf16 cache and into an fp8 cache pre-filled with the
    NaN byte -- the written bytes are the quantiser applied to the bf16 cache's values, exactly;
    every other byte is untouched; no NaN byte is written; q is identical."""
    ops = _ops()
    if M < 0:
        M = ops.skinny_addln_max_rows(d)
        assert M >= 4
    T = 19
    S = M // T + 3
    g = torch.Generator().manual_seed(1000 * len(op) + M + d)
    x = (torch.randn(M, d, generator=g) * 2 + 0.3).to(DEV)
    gam, bet = (1 + 0.2 * torch.randn(d, generator=g)).to(DEV), (0.1 * torch.randn(d, generator=g)).to(DEV)
    w = (torch.randn(3 * d, d, generator=g) * 0.05).to(DEV).bfloat16()
    bias = torch.randn(3 * d, generator=g).to(DEV)
    # zero weight columns whose value is the bias itself: saturation on both sides, the smallest
    # subnormal, the tie below it, a tie at step 2, 464 (the first value a direct conversion would NaN)
    edge = [1000.0, -1e9, 448.0, -449.0, 2.0 ** -9, 2.0 ** -10, -3 * 2.0 ** -10, 17.0, 19.0, 1e-6, 0.0, 464.0]
    cols = [d + 5 + 61 * i for i in range(len(edge))] + [2 * d + 3 + 59 * i for i in range(len(edge))]
    w[cols] = 0
    bias[cols] = torch.tensor(edge + edge, device=DEV)
    w_sh = ops.shuffle_weight(w)
    # rows -> distinct (slot, position) pairs: slots permuted, positions ragged, 0 and T - 1 used
    need = torch.tensor([(S - 1) * T + (T - 1)] + ([2 * T] if M > 1 else []))
    perm = torch.randperm(S * T, generator=g)
    pairs = torch.cat([need, perm[~torch.isin(perm, need)][: M - need.numel()]])
    pairs = pairs[torch.randperm(M, generator=g)]
    slot = (pairs // T).to(torch.int32).to(DEV)
    pos = (pairs % T).to(torch.int32).to(DEV)
    assert int(pos.max()) == T - 1 and (M == 1 or int(pos.min()) == 0) and pairs.unique().numel() == M

    k16 = torch.zeros(S, H, T, 64, dtype=torch.bfloat16, device=DEV)
    v16 = torch.zeros_like(k16)
    q16 = torch.zeros(M, d, dtype=torch.bfloat16, device=DEV)
    _run_qkv(ops, op, x, w_sh, gam, bet, bias, q16, k16, v16, slot, pos)
    k8, v8 = _nan_filled(S, H, T, 64), _nan_filled(S, H, T, 64)
    q8 = torch.zeros_like(q16)
    _run_qkv(ops, op, x, w_sh, gam, bet, bias, q8, k8, v8, slot, pos)
    assert torch.equal(q8, q16) and bool(q16.any())
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
    s0, p0 = int(slot[0]), int(pos[0])
    assert k8[s0, 0, p0, 5].float().item() == 448.0 and k16[s0, 0, p0, 5].float().item() == 1000.0


# ------------------------------------------------------------------------------------------------
# 2. attention_split on the fp8 cache
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bf16_cache(H):
    c = _attn_case(H)
    return c["k"].to(torch.bfloat16), c["v"].to(torch.bfloat16)


@pytest.mark.parametrize("H", [12, 25])
@pytest.mark.parametrize("R", [1, 5, 12, 64])
def test_fp8_attention_split(R, H):
    """Every wave count, one workgroup per pair and four (through a workspace); slots permuted;
    R = 12 / 64 reach every kvlen of KVLENS (1 ... 1024: slices with no keys, ragged last groups)."""
    ops = _ops()
    c = _attn_case(H)
    k16, v16 = _bf16_cache(H)
    row_slot = torch.tensor([11 - r if R == 12 else (7 * r + 3) % ATT_SLOTS for r in range(R)], dtype=torch.int32,
                            device=DEV)
    kvl = c["kvlen"][row_slot.cpu().long()].to(torch.int32).to(DEV)
    if R >= 12:
        assert set(kvl.tolist()) == set(KVLENS)
    q = c["q"][:R]
    ref = _attn_ref(c, H, row_slot)
    for waves in (2, 4, 8, 16):
        for splits in (1, 4):
            ws = ops.AttnSplitWorkspace(R * H, splits, DEV) if splits > 1 else None
            kw = dict(waves=waves, splits=splits, workspace=ws)
            out = ops.attention_split(q, c["kn"], c["vn"], row_slot, kvl, **kw)
            assert torch.isfinite(out.float()).all(), (waves, splits)
            torch.testing.assert_close(out.float(), ref, atol=2e-2, rtol=2e-2)
            # the bytes past kvlen are never used: the same output over ordinary values there, and again
            assert torch.equal(out, ops.attention_split(q, c["k"], c["v"], row_slot, kvl, **kw)), (waves, splits)
            assert torch.equal(out, ops.attention_split(q, c["kn"], c["vn"], row_slot, kvl, **kw)), (waves, splits)
            # the (g, c) lane mapping is kept and widening is exact: the bf16 kernel's bits
            assert torch.equal(out, ops.attention_split(q, k16, v16, row_slot, kvl, **kw)), (waves, splits)


# ------------------------------------------------------------------------------------------------
# 3. fused attention + out-projection on the fp8 cache
# ------------------------------------------------------------------------------------------------
def _rows_attn_ref(q, k, v, slot, kvlen):
    """fp32 torch attention over the dequantised cache, per row (tests/test_skinny_gpu.py::_attn_ref)."""
    R, H = q.shape[0], k.shape[1]
    out = torch.empty(R, H * 64, device=DEV)
    for r in range(R):
        s, n = int(slot[r]), int(kvlen[r])
        kk, vv = k[s, :, :n].float(), v[s, :, :n].float()
        p = torch.softmax((q[r].float().reshape(H, 1, 64) @ kk.transpose(1, 2)) / 8.0, dim=-1)
        out[r] = (p @ vv).reshape(-1)
    return out


def _oproj_case(H, T, S, seed):
    g = torch.Generator().manual_seed(seed)
    k = _quant(torch.randn(S, H, T, 64, generator=g).to(DEV))
    v = _quant((torch.randn(S, H, T, 64, generator=g) * 2).to(DEV))
    q = torch.randn(4, H * 64, generator=g).to(DEV).bfloat16()
    wo = (torch.randn(H * 64, H * 64, generator=g) * 0.05).to(DEV).bfloat16()
    return k, v, q, wo


def _nan_tail(k, v, slot, kvlen):
    kn, vn = k.clone(), v.clone()
    for s in range(k.shape[0]):  # slots no row uses: all NaN bytes
        L = 0
        for r in range(slot.numel()):
            if int(slot[r]) == s:
                L = int(kvlen[r])
        kn.view(torch.uint8)[s, :, L:] = NAN_BYTE
        vn.view(torch.uint8)[s, :, L:] = NAN_BYTE
    return kn, vn


@pytest.mark.parametrize("T", [64, 512])
@pytest.mark.parametrize("H", [12, 16])
@pytest.mark.parametrize("M", [1, 2, 4])
def test_fp8_attention_oproj(M, H, T):
    """Slab h == fp32 attention of head h over the dequantised cache -> bf16 -> @ W_o[:, head h]^T,
    the slabs sum to the out-projection; ragged kvlens with 1 and T (one row: each in turn)."""
    ops = _ops()
    N, S = H * 64, 6
    k, v, q, wo = _oproj_case(H, T, S, 200 + H + T)
    q = q[:M]
    wo_sh = ops.shuffle_weight(wo)
    slot = torch.tensor([4, 1, 5, 2][:M], dtype=torch.int32, device=DEV)
    for lens in ([[T], [1]] if M == 1 else [[T, 1, T // 2 + 3, 17][:M]]):
        kvlen = torch.tensor(lens, dtype=torch.int32, device=DEV)
        kn, vn = _nan_tail(k, v, slot, kvlen)
        parts = torch.full((H, 4, N), 7.0, device=DEV)
        ops.attention_oproj(q, kn, vn, slot, kvlen, wo_sh, parts)
        assert torch.isfinite(parts).all()
        o = _rows_attn_ref(q, k, v, slot, kvlen).to(torch.bfloat16).float().reshape(M, H, 64)
        for h in range(H):
            ref_h = o[:, h] @ wo.float()[:, 64 * h:64 * h + 64].t()
            torch.testing.assert_close(parts[h, :M], ref_h, atol=2e-2, rtol=2e-2)
        torch.testing.assert_close(parts[:, :M].sum(0), o.reshape(M, -1) @ wo.float().t(), atol=5e-2, rtol=2e-2)
        assert torch.all(parts[:, M:] == 7.0)  # rows >= M untouched
        # the bytes past kvlen are never used; and the bf16 kernel's bits on the widened cache
        for kk, vv in ((k, v), (k.to(torch.bfloat16), v.to(torch.bfloat16))):
            again = torch.full((H, 4, N), 7.0, device=DEV)
            ops.attention_oproj(q, kk, vv, slot, kvlen, wo_sh, again)
            assert torch.equal(again, parts)


@pytest.mark.parametrize("H,hg,tiles", [(12, 3, 3), (12, 3, 1), (16, 4, 4), (16, 4, 2), (12, 4, 3)])
@pytest.mark.parametrize("T", [1, 37, 150])
def test_fp8_attention_oproj_grouped(H, hg, tiles, T):
    """One row, heads in groups of hg: slab g == sum over its heads of attn_h(q) -> bf16 -> @ W_o[:, h]^T."""
    ops = _ops()
    N, S, Tmax = H * 64, 5, 150
    k, v, q, wo = _oproj_case(H, Tmax, S, 300 + H)
    q = q[:1]
    wo_sh = ops.shuffle_weight(wo)
    slot = torch.tensor([3], dtype=torch.int32, device=DEV)
    kvlen = torch.tensor([T], dtype=torch.int32, device=DEV)
    kn, vn = _nan_tail(k, v, slot, kvlen)
    parts = torch.full((H // hg, 2, N), 7.0, device=DEV)
    ops.attention_oproj_grouped(q, kn, vn, slot, kvlen, wo_sh, parts, hg, tiles=tiles)
    assert torch.isfinite(parts).all()
    o = _rows_attn_ref(q, k, v, slot, kvlen).to(torch.bfloat16).float().reshape(H, 64)
    for g in range(H // hg):
        ref = sum(o[h] @ wo.float()[:, 64 * h:64 * h + 64].t() for h in range(g * hg, g * hg + hg))
        torch.testing.assert_close(parts[g, 0], ref, atol=3e-2, rtol=2e-2)
    assert torch.all(parts[:, 1] == 7.0)
    for kk, vv in ((k, v), (k.to(torch.bfloat16), v.to(torch.bfloat16))):
        again = torch.full((H // hg, 2, N), 7.0, device=DEV)
        ops.attention_oproj_grouped(q, kk, vv, slot, kvlen, wo_sh, again, hg, tiles=tiles)
        assert torch.equal(again, parts)


# ------------------------------------------------------------------------------------------------
# 4. refusals, and bf16 dispatch untouched
# ------------------------------------------------------------------------------------------------
def _six_ops(ops, k, v, kq=None, vq=None):
    """The six ops on caches (k, v) for the attention side and (kq, vq) for the QKV side (d = 768,
    2 rows; 1 row for the grouped kernel): yields (name, call), each call returning the op's output."""
    H, d, M = 12, 768, 2
    kq, vq = (k, v) if kq is None else (kq, vq)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(M, d, generator=g).to(DEV)
    gam, bet = torch.ones(d, device=DEV), torch.zeros(d, device=DEV)
    w_sh = ops.shuffle_weight((torch.randn(3 * d, d, generator=g) * 0.05).to(DEV).bfloat16())
    wo_sh = ops.shuffle_weight((torch.randn(d, d, generator=g) * 0.05).to(DEV).bfloat16())
    q = torch.randn(M, d, generator=g).to(DEV).bfloat16()
    slot = torch.tensor([1, 0], dtype=torch.int32, device=DEV)
    pos = torch.tensor([3, 0], dtype=torch.int32, device=DEV)
    kvl = torch.tensor([4, 1], dtype=torch.int32, device=DEV)
    for op in ("skinny", "addln", "mid"):
        qo = torch.zeros(M, d, dtype=torch.bfloat16, device=DEV)
        yield op, lambda qo=qo, op=op: (_run_qkv(ops, op, x, w_sh, gam, bet, None, qo, kq, vq, slot, pos), qo)[1]
    yield "split", lambda: ops.attention_split(q, k, v, slot, kvl, waves=4)
    yield "oproj", lambda: ops.attention_oproj(q, k, v, slot, kvl, wo_sh, torch.zeros(H, 4, d, device=DEV)).clone()
    yield "grouped", lambda: ops.attention_oproj_grouped(q[:1], k, v, slot, kvl, wo_sh,
                                                         torch.zeros(4, 1, d, device=DEV), 3).clone()


def test_six_ops_refuse_mixed_and_misplaced_fp8_caches():
    ops = _ops()
    H, T = 12, 8
    k8 = _quant(torch.randn(2, H, T, 64, generator=torch.Generator().manual_seed(1)).to(DEV))
    k16 = k8.to(torch.bfloat16)
    for name, call in _six_ops(ops, k8, k16):  # mixed K / V dtypes
        with pytest.raises(ValueError):
            call()
    for name, call in _six_ops(ops, k16, k8):
        with pytest.raises(ValueError):
            call()
    wide = _quant(torch.randn(2, H, T, 128, generator=torch.Generator().manual_seed(2)).to(DEV))
    strided = wide[..., :64]  # not contiguous
    assert strided.shape == k8.shape and not strided.is_contiguous()
    for name, call in _six_ops(ops, strided, strided):
        with pytest.raises(ValueError):
            call()
    flat = torch.zeros(k8.numel() + 16, dtype=torch.uint8, device=DEV).view(ops.FP8)
    odd = flat[4: 4 + k8.numel()].view(k8.shape)  # contiguous, 4 bytes off the 8-byte loads' alignment
    assert odd.is_contiguous() and odd.data_ptr() % 8 == 4
    for name, call in _six_ops(ops, odd, odd, k8.clone(), k8.clone()):
        if name in ("split", "oproj", "grouped"):
            with pytest.raises(ValueError):
                call()


def test_six_ops_bf16_and_fp8_calls_repeat_bit_for_bit():
    """Dispatch does not cross: a bf16 call gives what a second bf16 call gives (and what it gave
    before an fp8 call ran in between); the attention ops give the fp8 call's bits (exact widening)."""
    ops = _ops()
    H, T = 12, 8
    k8 = _quant(torch.randn(2, H, T, 64, generator=torch.Generator().manual_seed(3)).to(DEV))
    v8 = _quant(torch.randn(2, H, T, 64, generator=torch.Generator().manual_seed(4)).to(DEV))
    k16, v16 = k8.to(torch.bfloat16), v8.to(torch.bfloat16)
    # (the QKV ops scatter into caches of their own: the attention ops read k8 / k16 as they are)
    first = {name: call() for name, call in _six_ops(ops, k16, v16, k16.clone(), v16.clone())}
    fp8 = {name: call() for name, call in _six_ops(ops, k8, v8, k8.clone(), v8.clone())}
    second = {name: call() for name, call in _six_ops(ops, k16, v16, k16.clone(), v16.clone())}
    for name in first:
        assert torch.equal(first[name], second[name]), name
        assert torch.equal(first[name], fp8[name]), name  # q of the QKV ops; the attention outputs


# ------------------------------------------------------------------------------------------------
# 5. engine against GPT2Reference(kv_dtype="fp8")
# ------------------------------------------------------------------------------------------------
FP8_MID_MAX = 32  # the fp8 engine's default mid-path range (measured: docs/PERFORMANCE.md "fp8 KV cache")


@pytest.mark.parametrize("n", lc.BATCHES)
def test_fp8_latency_engine_matches_the_fp8_reference(n, monkeypatch):
    """GPT-2-124M, T = 48: 1 and 2 rows run the latency step (fused attention + out-projection and
    the fused MLP at one row), 3 ... 64 the mid path, all over the e4m3 cache.  An fp8 engine's
    default dispatch ends the mid path at 32 rows (beyond, the fp8 tiled step measured faster); the
    kernels serve up to 64, so the 33- and 64-row cases widen it with ``DLMS_MID_MAX_ROWS`` and are
    held to the same reference."""
    ops = _ops()
    if n > FP8_MID_MAX:
        dflt = _engine("gpt2", latency_path=True, max_batch=n, max_length=lc.T)
        assert dflt.mid_max == FP8_MID_MAX and not dflt._mid_ok(n) and dflt._mid_ok(FP8_MID_MAX)
        monkeypatch.setenv("DLMS_MID_MAX_ROWS", "64")
    eng = _engine("gpt2", latency_path=True, max_batch=max(8, n), max_length=lc.T)
    assert eng.mid_max == (64 if n > FP8_MID_MAX else FP8_MID_MAX)
    assert eng.kv.dtype == ops.FP8 and eng.kv_fp8_latency
    assert eng.small_max > 0 and eng.mid_max > 0 and not eng.dataflow
    assert eng._small_ok(n) or eng._mid_ok(n)
    assert not eng._df_ok(n)
    if n == 1:
        assert eng.fuse_ao and eng.fused_mlp
    prompts = lc.batch(eng.cfg, n)
    got = eng.generate(prompts, repetition_penalty=1.2)
    _assert_teacher_forced("gpt2", got, prompts, lc.T)


def test_fp8_engine_default_stays_tiled_and_env_does_not_override_explicit(monkeypatch):
    eng = _engine("gpt2", max_batch=8, max_length=lc.T)
    assert eng.small_max == 0 and eng.mid_max == 0 and not eng.kv_fp8_latency and not eng.fuse_ao and not eng.fused_mlp
    off = _engine("gpt2", latency_path=False, max_batch=8, max_length=lc.T)
    assert off.small_max == 0 and off.mid_max == 0
    monkeypatch.setenv("DLMS_LATENCY_PATH", "0")
    on = _engine("gpt2", latency_path=True, max_batch=8, max_length=lc.T)
    assert on.small_max > 0 and on.mid_max > 0 and on.kv_fp8_latency
    monkeypatch.setenv("DLMS_LATENCY_PATH", "1")  # the environment does not turn the fp8 default on either
    assert _engine("gpt2", max_batch=8, max_length=lc.T).small_max == 0


@pytest.mark.parametrize("n", [1, 24])
def test_fp8_latency_engine_medium(n):
    """gpt2-medium (d 1024, 16 heads): the margin rule at its eps 0.29, no floor (kc.MIN_DECISIVE)."""
    eng = _engine("gpt2-medium", latency_path=True, max_batch=max(8, n), max_length=lc.T)
    assert eng.small_max > 0 and eng.mid_max > 0 and (eng._small_ok(n) or eng._mid_ok(n)) and not eng.dataflow
    prompts = lc.batch(eng.cfg, n)
    _assert_teacher_forced("gpt2-medium", eng.generate(prompts, repetition_penalty=1.2), prompts, lc.T)


# ------------------------------------------------------------------------------------------------
# 6.-8. graphs, continuous batching, sampling
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 17])
def test_fp8_latency_engine_graph_replay_equals_eager_and_reruns(n):
    cfg, _, _ = _model("gpt2")
    prompts = lc.batch(cfg, n)
    eng = _engine("gpt2", latency_path=True, max_batch=max(8, n), max_length=lc.T, use_graph=True)
    assert eng._mid_ok(n)
    a = eng.generate(prompts)
    assert eng._graphs
    assert eng.generate(prompts) == a
    assert _engine("gpt2", latency_path=True, max_batch=max(8, n), max_length=lc.T, use_graph=False).generate(prompts) == a


def test_fp8_latency_engine_continuous_batching_passes_the_margin_rule():
    """Staggered admissions into a running batch (8 slots, the 12 requests of the fp8 batching test):
    as rows come and go the bucket moves through the latency and mid paths, over slots whose earlier
    keys the tiled prefill wrote.  Different row counts run different kernels, so the answers are held
    to the reference by the margin rule (no floor), not to a solo engine's tokens."""
    from distributed_lms_raft_llm_amd.engine.scheduler import ContinuousBatcher
    from distributed_lms_raft_llm_amd.models.gpt2 import teacher_forced_check_batch

    cfg, _, model = _model("gpt2")
    T = 48
    prompts = kc.prompts(cfg, [3, 30, 12, 1, 25, 7, 40, 16, 2, 33, 9, 47], seed=3)
    eng = _engine("gpt2", latency_path=True, max_batch=8, max_length=T, prefill_split=2)
    assert eng.small_max > 0 and eng.mid_max >= 8
    cb = ContinuousBatcher(eng, repetition_penalty=1.2, chunk=4)
    try:
        got = [f.result(120) for f in [cb.submit(p) for p in prompts]]
    finally:
        cb.stop()
    for o, p in zip(got, prompts):
        assert o[: len(p)] == p and len(p) < len(o) <= T
    res = teacher_forced_check_batch(model, got, [len(p) for p in prompts], 1.2, kc.KV_FP8_EPS["gpt2"])
    print("decisive", sum(r["decisive"] for r in res), "of", sum(r["positions"] for r in res))
    bad = [(i, r["mismatches"][:2]) for i, r in enumerate(res) if r["mismatches"]]
    assert not bad, bad
    assert cb.completed == 12


def test_fp8_latency_engine_samples_reproducibly():
    from distributed_lms_raft_llm_amd.models.config import SamplingParams

    cfg, _, _ = _model("gpt2")
    prompts = lc.batch(cfg, 3)
    eng = _engine("gpt2", latency_path=True, max_batch=8, max_length=40)
    assert eng._mid_ok(3)
    sp = SamplingParams(0.7, 50, 0.9, 11)
    a = eng.generate(prompts, sampling=sp)
    assert all(o[: len(p)] == p and len(p) < len(o) <= 40 for o, p in zip(a, prompts))
    assert eng.generate(prompts, sampling=sp) == a
    assert eng.generate(prompts, sampling=SamplingParams(0.7, 50, 0.9, 12)) != a
    assert eng.kv.dtype == torch.float8_e4m3fn


# ------------------------------------------------------------------------------------------------
# 9. checked build
# ------------------------------------------------------------------------------------------------
CHECKED_SCRIPT = r"""
import json, sys, torch
sys.path.insert(0, "tests")
import kv_fp8_cases as kc
import kv_fp8_latency_cases as lc
from distributed_lms_raft_llm_amd import ops
from distributed_lms_raft_llm_amd.engine.gpt2_engine import HipGPT2Engine
assert ops.checked_mode()
cfg, w = kc.setup("gpt2")
eng = HipGPT2Engine(cfg, w, max_batch=16, max_length=40, kv_dtype="fp8", latency_path=True)
paths = [bool(eng._small_ok(1) and eng.fuse_ao and eng.fused_mlp), bool(eng._mid_ok(9))]
lens = [len(o) for n in (1, 9) for o in eng.generate(lc.batch(cfg, n))]
print("RESULT " + json.dumps({"lens": lens, "errors": ops.device_errors(), "dtype": str(eng.kv.dtype), "paths": paths}))
"""


def test_fp8_latency_engine_checked_build_reports_no_device_errors():
    """1 row (latency step) and 9 rows (mid path) under the range-checked kernel build."""
    env = dict(os.environ, DLMS_KERNEL_CHECKS="1", PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-c", CHECKED_SCRIPT], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert res["errors"] == [] and res["dtype"] == "torch.float8_e4m3fn" and res["paths"] == [True, True], res
    assert len(res["lens"]) == 10 and all(n <= 40 for n in res["lens"]), res
