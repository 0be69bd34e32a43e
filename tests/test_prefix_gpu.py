"""Prompt-prefix cache on the GPU: ``ops.kv_prefix_fill`` (bit-exact copies, every other byte of the
cache untouched) and ``HipGPT2Engine(prefix_capacity=...)`` with ``set_prompt_prefix`` -- held to the
unchanged fp32 ``GPT2Reference`` under the teacher-forced margin rule (eps 0.05, >= 70 % decisive
positions; prompts and floor: prefix_cases.py, the floor recomputed by tests/test_prefix_cpu.py), the
fp8 cache to ``GPT2Reference(kv_dtype="fp8")`` at kv_fp8_cases.KV_FP8_EPS.

Every slot holds all of its keys (the store's rows are copied into it at admission), so every decode
path works as it is; the wave and the persistent decode attention on a bf16 cache read the shared
keys from the store instead (``ops.row_attention(prefix=...)``), bit-identically: the tiled step from
(row, head) pair 1025 on -- 96 rows here -- and the overlapped step, counted by
``prefix_decode_launches``.  At 64 rows and below the mid / latency / dataflow paths and their split
attention read the slots, as does everything on an fp8 cache, so the count stays 0 there."""
import functools
import json
import os
import subprocess
import sys
import time

import pytest
import torch

import attention_cases as ac
import kv_fp8_cases as kc
import prefix_cases as pc

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ops():
    from distributed_lms_raft_llm_amd import ops

    ops.lib()
    return ops


# ------------------------------------------------------------------------------------------------
# kv_prefix_fill
# ------------------------------------------------------------------------------------------------
def _random_bytes(shape, dtype, seed):
    """Distinct random bytes viewed as ``dtype`` (compared as bytes: NaN patterns included)."""
    g = torch.Generator().manual_seed(seed)
    n = 1
    for s in shape:
        n *= s
    nbytes = n * torch.empty(0, dtype=dtype).element_size()
    raw = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, generator=g).to(DEV)
    return raw.view(dtype).view(*shape)


@pytest.mark.parametrize("pfx", [[0, 1, 7], [16, 32, 0], [32, 7, 16], [1, 0, 32]])
@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("H", [12, 25])
def test_kv_prefix_fill_copies_the_store_and_nothing_else(H, dtype, pfx):
    ops = _ops()
    L, S, T, C = 2, 8, 48, 32
    dt = torch.bfloat16 if dtype == "bf16" else ops.FP8
    kv = _random_bytes((L, 2, S, H, T, 64), dt, 1 + H)
    store = _random_bytes((L, 2, H, C, 64), dt, 2 + H)
    slots = [5, 0, 3]
    before = kv.clone()
    out = ops.kv_prefix_fill(kv, store, torch.tensor(slots, dtype=torch.int32, device=DEV),
                             torch.tensor(pfx, dtype=torch.int32, device=DEV))
    assert out is kv
    raw, raw0, sraw = (t.view(torch.uint8) for t in (kv, before, store))
    touched = torch.zeros(L, 2, S, H, T, dtype=torch.bool, device=DEV)
    for s, p in zip(slots, pfx):
        touched[:, :, s, :, :p] = True
        assert torch.equal(raw[:, :, s, :, :p], sraw[:, :, :, :p])  # the filled region is the store, bit for bit
    assert int(touched.sum()) == L * 2 * H * sum(pfx)
    # keys >= pfx, the other slots and the slots with pfx = 0: unchanged
    assert torch.equal(raw[~touched], raw0[~touched])
    assert torch.equal(sraw, _random_bytes((L, 2, H, C, 64), dt, 2 + H).view(torch.uint8))  # the store is only read


def test_kv_prefix_fill_refuses_bad_arguments():
    ops = _ops()
    kv = torch.zeros(2, 2, 4, 3, 16, 64, dtype=torch.bfloat16, device=DEV)
    store = torch.zeros(2, 2, 3, 8, 64, dtype=torch.bfloat16, device=DEV)
    i32 = dict(dtype=torch.int32, device=DEV)
    slots, pfx = torch.tensor([1, 2], **i32), torch.tensor([3, 0], **i32)
    ops.kv_prefix_fill(kv, store, slots, pfx)
    with pytest.raises(ValueError):  # one cache dtype
        ops.kv_prefix_fill(kv, store.to(ops.FP8), slots, pfx)
    with pytest.raises(ValueError):  # another head count
        ops.kv_prefix_fill(kv, torch.zeros(2, 2, 4, 8, 64, dtype=torch.bfloat16, device=DEV), slots, pfx)
    with pytest.raises(ValueError):  # one length per slot
        ops.kv_prefix_fill(kv, store, slots, pfx[:1])
    with pytest.raises(ValueError):  # a strided cache
        ops.kv_prefix_fill(kv[:, :, ::2], store, slots, pfx)
    with pytest.raises(TypeError):
        ops.kv_prefix_fill(kv, store, slots.long(), pfx)


# ------------------------------------------------------------------------------------------------
# decode attention reading the shared keys from the store (wave and persistent kernels, bf16 cache)
# ------------------------------------------------------------------------------------------------
PFX_CHOICES = [0, 1, 7, 8, 9, 16, 21]
PFX_S, PFX_T, PFX_C = 16, 64, 24


def _nan_bf16(t):
    t.view(torch.int16).fill_(ac.NAN_BF16)


@functools.lru_cache(maxsize=None)
def _pfx_attn_case(H):
    """16 slots of T = 64: slot s takes its first PFX_CHOICES[s % 7] keys from the store and holds
    kvlen = pfx + 1 (s % 3 == 0), T (s % 3 == 1) or something between.  ``full``: the slots hold the
    store's rows (what the existing kernels read); ``nan``: NaN there, and NaN in the store's rows no
    slot may use -- a read from the wrong place shows."""
    g = torch.Generator().manual_seed(300 + H)
    S, T, C = PFX_S, PFX_T, PFX_C
    pfx = torch.tensor([PFX_CHOICES[s % len(PFX_CHOICES)] for s in range(S)], dtype=torch.int32)
    kvlen = torch.tensor([int(p) + 1 if s % 3 == 0 else T if s % 3 == 1 else
                          int(torch.randint(int(p) + 2, T, (1,), generator=g)) for s, p in enumerate(pfx)],
                         dtype=torch.int32)
    mk = lambda *shape, f=1.0: (torch.randn(*shape, generator=g) * f).to(DEV).bfloat16()  # noqa: E731
    pk, pv = mk(H, C, 64), mk(H, C, 64, f=2.0)
    k, v = mk(S, H, T, 64), mk(S, H, T, 64, f=2.0)
    kn, vn = k.clone(), v.clone()
    for s, p in enumerate(pfx.tolist()):
        k[s, :, :p], v[s, :, :p] = pk[:, :p], pv[:, :p]
        _nan_bf16(kn[s, :, :p])
        _nan_bf16(vn[s, :, :p])
    pkn, pvn = pk.clone(), pv.clone()
    _nan_bf16(pkn[:, max(PFX_CHOICES):])
    _nan_bf16(pvn[:, max(PFX_CHOICES):])
    q = torch.randn(300, H * 64, generator=g).to(DEV).bfloat16()
    return dict(k=k, v=v, kn=kn, vn=vn, pk=pkn, pv=pvn, q=q, pfx=pfx, kvlen=kvlen)


@pytest.mark.parametrize("impl", ["wave", "persist"])
@pytest.mark.parametrize("H", [12, 25])
@pytest.mark.parametrize("R", [1, 5, 300])
def test_prefix_attention_is_bit_identical_to_the_slot_kernels(R, H, impl):
    """Reference: the existing kernel on slots that hold the store's rows.  R = 300 with 64
    persistent workgroups: fewer waves than pairs; H = 25: idle waves in a row's last workgroup."""
    ops = _ops()
    c = _pfx_attn_case(H)
    row_slot = torch.tensor([(5 * r + 2) % PFX_S for r in range(R)], dtype=torch.int32)
    kvl = c["kvlen"][row_slot.long()].to(DEV)
    if R == 300:
        used = c["pfx"][row_slot.long()]
        assert set(used.tolist()) == set(PFX_CHOICES)
        assert bool((kvl.cpu() == used + 1).any()) and bool((kvl == PFX_T).any())
    row_slot = row_slot.to(DEV)
    q = c["q"][:R]
    kw = dict(impl=impl, blocks=64)
    want = ops.row_attention(q, c["k"], c["v"], row_slot, kvl, **kw)
    assert torch.isfinite(want.float()).all()
    got = ops.row_attention(q, c["kn"], c["vn"], row_slot, kvl, prefix=(c["pk"], c["pv"], c["pfx"].to(DEV)), **kw)
    assert torch.equal(got, want)
    # with every count 0 the slots are read
    zero = torch.zeros(PFX_S, dtype=torch.int32, device=DEV)
    plain = ops.row_attention(q, c["k"], c["v"], row_slot, kvl, prefix=(c["pk"], c["pv"], zero), **kw)
    assert torch.equal(plain, want)


def test_prefix_attention_refuses_other_kernels_and_caches():
    ops = _ops()
    c = _pfx_attn_case(12)
    idx = torch.zeros(2, dtype=torch.int32, device=DEV)
    one = torch.ones(2, dtype=torch.int32, device=DEV)
    pre = (c["pk"], c["pv"], c["pfx"].to(DEV))
    with pytest.raises(ValueError):
        ops.row_attention(c["q"][:2], c["k"], c["v"], idx, one, impl="lds", prefix=pre)
    with pytest.raises(ValueError):  # the fp8 cache has no such build
        ops.row_attention(c["q"][:2], c["k"].to(ops.FP8), c["v"].to(ops.FP8), idx, one, prefix=pre)
    with pytest.raises(ValueError):  # another head count
        ops.row_attention(c["q"][:2], c["k"], c["v"], idx, one, prefix=(c["pk"][:5], c["pv"][:5], pre[2]))
    with pytest.raises(ValueError):  # a count per slot
        ops.row_attention(c["q"][:2], c["k"], c["v"], idx, one, prefix=(c["pk"], c["pv"], pre[2][:3]))


STRUCT_KVLENS = (9, 33, 65, 257)


def _moved_into_store(case, pfx, cap=32):
    """The case's bf16 caches with the first ``pfx`` keys of the rows' slot moved into a store
    (NaN left behind in the slot, NaN in the store's unused rows)."""
    slot = int(case.row_slot[0])
    assert bool((case.row_slot == slot).all()) and pfx < min(case.row_kvlen.tolist())
    k, v = ac.cache(case.k, "bf16").to(DEV), ac.cache(case.v, "bf16").to(DEV)
    pk = torch.empty(case.H, cap, 64, dtype=torch.bfloat16, device=DEV)
    pv = torch.empty_like(pk)
    _nan_bf16(pk)
    _nan_bf16(pv)
    pk[:, :pfx], pv[:, :pfx] = k[slot, :, :pfx], v[slot, :, :pfx]
    _nan_bf16(k[slot, :, :pfx])
    _nan_bf16(v[slot, :, :pfx])
    slot_pfx = torch.zeros(k.shape[0], dtype=torch.int32, device=DEV)
    slot_pfx[slot] = pfx
    return k, v, (pk, pv, slot_pfx)


@pytest.mark.parametrize("impl", ["wave", "persist"])
@pytest.mark.parametrize("pfx", [1, 7, 8])
def test_prefix_attention_count_and_comb_families(pfx, impl):
    """tests/attention_cases.py's count (both codes) and comb families at kvlens 9 / 33 / 65 / 257
    with the first ``pfx`` keys served from the store, under the comparators and bounds defined
    there for the row kernels (one bf16 ulp; relative 2^-7 against the fp64 softmax)."""
    ops = _ops()
    H = 12
    kw = dict(impl=impl, blocks=64)
    for code in ("A", "B"):
        case = ac.count_case(H, code, kvlens=STRUCT_KVLENS)
        k, v, pre = _moved_into_store(case, pfx)
        out = ops.row_attention(case.q.to(DEV).bfloat16(), k, v, case.row_slot.to(DEV), case.row_kvlen.to(DEV),
                                prefix=pre, **kw)
        assert not ac.count_mismatches(out, case, ulps=1), (code, ac.count_mismatches(out, case, ulps=1))
    case = ac.comb_case(H, kvlens=STRUCT_KVLENS)
    k, v, pre = _moved_into_store(case, pfx)
    out = ops.row_attention(case.q.to(DEV).bfloat16(), k, v, case.row_slot.to(DEV), case.row_kvlen.to(DEV),
                            prefix=pre, **kw)
    ref, pav = ac.reference(case.q.to(DEV), case.k.to(DEV), case.v.to(DEV), case.row_slot.to(DEV),
                            case.row_kvlen.to(DEV))
    bad = ac.close_mismatches(out, ref, pav, rel=ac.REL)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------
# engine
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(kv_dtype="bf16"):
    from distributed_lms_raft_llm_amd.models.gpt2 import GPT2Reference

    cfg, w = kc.setup("gpt2")
    return cfg, w, GPT2Reference(cfg, w, device=DEV, kv_dtype=kv_dtype)


def _engine(prefix=None, capacity=pc.CAPACITY, kv_dtype="bf16", **kw):
    from distributed_lms_raft_llm_amd.engine.gpt2_engine import HipGPT2Engine

    cfg, w, _ = _model()
    kw.setdefault("max_length", pc.T)
    eng = HipGPT2Engine(cfg, w, prefix_capacity=capacity, kv_dtype=kv_dtype, **kw)
    if prefix is not None:
        eng.set_prompt_prefix(prefix)
    return eng


def _assert_margin_rule(outs, prompts, T, kv_dtype="bf16", eps=pc.EPS, floor=pc.MIN_DECISIVE):
    from distributed_lms_raft_llm_amd.models.gpt2 import teacher_forced_check_batch

    _, _, model = _model(kv_dtype)
    for o, p in zip(outs, prompts):
        assert o[: len(p)] == p and len(p) < len(o) <= T
    res = teacher_forced_check_batch(model, outs, [len(p) for p in prompts], 1.2, eps)
    total, decisive = sum(r["positions"] for r in res), sum(r["decisive"] for r in res)
    bad = [(i, r["mismatches"][:2]) for i, r in enumerate(res) if r["mismatches"]]
    print(f"batch {len(prompts)} ({kv_dtype} cache): {decisive} / {total} positions decisive at eps {eps}, "
          f"{sum(len(r['mismatches']) for r in res)} mismatches")
    assert not bad, bad[:4]
    assert total > 0 and decisive >= floor * total, (decisive, total)


def _predicted(prompts, prefix):
    from distributed_lms_raft_llm_amd.engine.gpt2_engine import split_prefix

    pfx = split_prefix(prompts, prefix)
    return sum(1 for k in pfx if k), sum(pfx)


@pytest.mark.parametrize("batch", [1, 3, 9, 64, 96, 512])
@pytest.mark.parametrize("P", pc.P_VALUES)
def test_prefix_engine_matches_the_fp32_reference(P, batch):
    """GPT-2-124M, T = 64, bf16 cache: one row (the dataflow decode), 3, 9 and 64 rows (the mid path
    and its split attention), 96 (the tiled step, one wave per row and head), 512 (the overlapped
    step, the persistent attention) -- every decode path reads slots the fill completed."""
    cfg, _, _ = _model()
    prefix, base = pc.prefix_and_prompts(cfg, P)
    prompts = pc.cycled(base, batch)
    eng = _engine(prefix, max_batch=max(8, batch))
    assert eng.prompt_prefix == prefix and eng.prefix_hits == 0
    got = eng.generate(prompts, repetition_penalty=1.2)
    _assert_margin_rule(got, prompts, pc.T)
    hits, rows = _predicted(prompts, prefix)
    assert hits == sum(1 for i in range(batch) if i % 13 < 8) and rows == hits * P
    assert (eng.prefix_hits, eng.prefix_rows_skipped, eng.prefix_prompts) == (hits, rows, batch)
    # the store is read by the wave (tiled step, > 1024 (row, head) pairs) and the persistent kernel
    # (overlapped step); the dataflow, latency and mid paths' attention kernels read the slots
    assert (eng.prefix_decode_launches > 0) == (batch >= 96), eng.prefix_decode_launches
    assert eng.slot_pfx[:batch].tolist() == [P if i % 13 < 8 else 0 for i in range(batch)]


@pytest.mark.parametrize("batch", [3, 64])
def test_prefix_engine_fp8_cache_matches_the_fp8_reference(batch):
    ops = _ops()
    cfg, _, _ = _model()
    prefix, base = pc.prefix_and_prompts(cfg, 16)
    prompts = pc.cycled(base, batch)
    eng = _engine(prefix, kv_dtype="fp8", max_batch=max(8, batch))
    assert eng.kv.dtype == ops.FP8 and eng.pfx_store.dtype == ops.FP8
    got = eng.generate(prompts, repetition_penalty=1.2)
    _assert_margin_rule(got, prompts, pc.T, kv_dtype="fp8", eps=kc.KV_FP8_EPS["gpt2"], floor=kc.MIN_DECISIVE["gpt2"])
    assert (eng.prefix_hits, eng.prefix_rows_skipped) == _predicted(prompts, prefix)
    assert eng.prefix_decode_launches == 0


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_slot_and_store_contents_after_an_admission(kv_dtype):
    """The sharing slots' first P keys are the store's, bit for bit, and the store is what a plain
    engine's slot holds after prefilling the prefix alone as a one-prompt batch."""
    from distributed_lms_raft_llm_amd.engine.memory import kv_bytes, prefix_store_bytes

    cfg, _, _ = _model()
    P = 13
    prefix, base = pc.prefix_and_prompts(cfg, P)
    eng = _engine(prefix, kv_dtype=kv_dtype, max_batch=8)
    assert eng.kv_cache_bytes() == 8 * kv_bytes(cfg, pc.T, kv_dtype=kv_dtype) + \
        prefix_store_bytes(cfg, pc.CAPACITY, kv_dtype=kv_dtype)
    store = eng.pfx_store.view(torch.uint8).clone()
    addr = (eng.pfx_store.data_ptr(), eng.slot_pfx.data_ptr())
    prompts = [base[0], base[8], base[3], base[11], base[12]]  # share, not, share, bare prefix, near miss
    slots = [6, 1, 2, 4, 0]
    eng.admit(prompts, slots)
    assert eng.slot_pfx.tolist() == [0, 0, P, 0, 0, 0, P, 0]
    raw = eng.kv.view(torch.uint8)
    for s in (6, 2):
        assert torch.equal(raw[:, :, s, :, :P], store[:, :, :, :P])
    assert torch.equal(eng.pfx_store.view(torch.uint8), store)
    assert eng.collect([6])[0][: len(base[0])] == base[0] and eng.lens[6].item() == len(base[0]) + 1
    plain = _engine(None, capacity=0, kv_dtype=kv_dtype, max_batch=8)
    assert plain.pfx_store is None and plain.slot_pfx is None
    assert plain.kv_cache_bytes() == 8 * kv_bytes(cfg, pc.T, kv_dtype=kv_dtype)
    plain.admit([prefix], [3])
    assert torch.equal(plain.kv.view(torch.uint8)[:, :, 3, :, :P], store[:, :, :, :P])
    # replacing the prefix keeps the addresses captured graphs hold
    eng.decode(8, pc.T)
    eng.set_prompt_prefix(prefix[:5])
    assert addr == (eng.pfx_store.data_ptr(), eng.slot_pfx.data_ptr()) and eng.slot_pfx.tolist() == [0] * 8
    eng.close()
    assert eng.pfx_store is None and eng.slot_pfx is None


def test_graph_replay_equals_eager_and_reruns():
    cfg, _, _ = _model()
    prefix, base = pc.prefix_and_prompts(cfg, 16)
    prompts = base[:5] + base[8:10] + base[11:]
    eng = _engine(prefix, max_batch=16, use_graph=True)
    a = eng.generate(prompts)
    assert eng._graphs
    assert eng.generate(prompts) == a
    assert eng.generate(prompts) == a and eng._pgraphs  # (the third call replays the captured prefill)
    assert _engine(prefix, max_batch=16, use_graph=False).generate(prompts) == a
    assert eng.prefix_hits == 3 * _predicted(prompts, prefix)[0]


def test_continuous_batching_matches_serving_alone(monkeypatch):
    """8 slots, 12 staggered requests (sharing and not), the prefill split-K pinned as the existing
    continuous-batching tests pin it: each result equals that prompt served alone on an engine
    with the same prefix.  (Launch-per-op throughout, as in tests/test_engine_gpu.py: the one-row
    dataflow decode sums in another order.)"""
    from distributed_lms_raft_llm_amd.engine.scheduler import ContinuousBatcher

    monkeypatch.setenv("DLMS_DATAFLOW", "0")
    cfg, _, _ = _model()
    prefix, base = pc.prefix_and_prompts(cfg, 16)
    prompts = base[:12]
    eng = _engine(prefix, max_batch=8, prefill_split=2)
    cb = ContinuousBatcher(eng, repetition_penalty=1.2, chunk=4)
    try:
        futs = []
        for i, p in enumerate(prompts):
            futs.append(cb.submit(p))
            if i % 4 == 3:
                time.sleep(0.02)  # (the next four join a running batch, as in tests/test_engine_gpu.py)
        got = [f.result(120) for f in futs]
    finally:
        cb.stop()
    solo = _engine(prefix, max_batch=1, prefill_split=2)
    for g_, p in zip(got, prompts):
        assert g_ == solo.generate([p], repetition_penalty=1.2)[0]
    assert cb.completed == len(prompts)
    assert (eng.prefix_hits, eng.prefix_rows_skipped) == _predicted(prompts, prefix) == (8, 128)
    assert solo.prefix_hits == 8


def test_prefix_is_refused_while_a_slot_is_live_then_replaced():
    cfg, _, _ = _model()
    prefix, base = pc.prefix_and_prompts(cfg, 16)
    other, base2 = pc.prefix_and_prompts(cfg, 13, seed=8)
    eng = _engine(prefix, max_batch=8)
    eng.admit(base[:2], [0, 1])
    with pytest.raises(RuntimeError):
        eng.set_prompt_prefix(other)
    with pytest.raises(RuntimeError):
        eng.set_prompt_prefix(None)
    assert eng.prompt_prefix == prefix
    eng.decode(8, pc.T)
    assert all(eng.finished_flags(8))
    _assert_margin_rule(eng.collect([0, 1]), base[:2], pc.T)
    eng.set_prompt_prefix(other)
    assert eng.prompt_prefix == other and eng.prefix_hits == 2
    new = base2[:8]
    _assert_margin_rule(eng.generate(new, repetition_penalty=1.2), new, pc.T)
    assert eng.prefix_hits == 10 and eng.prefix_rows_skipped == 2 * 16 + 8 * 13
    old = base[:8]  # prompts of the old prefix take the full path
    _assert_margin_rule(eng.generate(old, repetition_penalty=1.2), old, pc.T)
    assert eng.prefix_hits == 10 and eng.slot_pfx.tolist() == [0] * 8
    eng.set_prompt_prefix(None)
    assert eng.prompt_prefix is None
    _assert_margin_rule(eng.generate(new, repetition_penalty=1.2), new, pc.T)
    assert eng.prefix_hits == 10
    for bad in ([], list(range(pc.CAPACITY + 1)), [cfg.vocab_size], [-1]):
        with pytest.raises(ValueError):
            eng.set_prompt_prefix(bad)
    with pytest.raises(ValueError):  # max_length - 2 caps it below the capacity
        _engine(None, max_batch=2, max_length=20).set_prompt_prefix(list(range(19)))
    with pytest.raises(ValueError):  # an engine without a store
        _engine(None, capacity=0, max_batch=2).set_prompt_prefix(prefix)


def test_prefix_engine_refuses_tp_and_fp8_weights():
    from distributed_lms_raft_llm_amd.engine.gpt2_engine import HipGPT2Engine

    cfg, w = kc.setup("gpt2-tiny")
    with pytest.raises(ValueError, match="fp8 weights"):
        HipGPT2Engine(cfg, w, max_batch=4, max_length=24, prefix_capacity=8, weight_dtype="fp8")
    with pytest.raises(ValueError, match="tensor parallelism"):
        HipGPT2Engine(cfg, w, max_batch=4, max_length=24, prefix_capacity=8, tp_group=object())
    with pytest.raises(ValueError):
        HipGPT2Engine(cfg, w, max_batch=4, max_length=24, prefix_capacity=-1)


def test_prefix_engine_samples_reproducibly():
    from distributed_lms_raft_llm_amd.models.config import SamplingParams

    cfg, _, _ = _model()
    prefix, base = pc.prefix_and_prompts(cfg, 16)
    prompts = base[:3] + base[8:10]
    eng = _engine(prefix, max_batch=8)
    sp = SamplingParams(0.7, 50, 0.9, 11)
    a = eng.generate(prompts, sampling=sp)
    assert all(o[: len(p)] == p and len(p) < len(o) <= pc.T for o, p in zip(a, prompts))
    assert eng.generate(prompts, sampling=sp) == a
    assert eng.generate(prompts, sampling=SamplingParams(0.7, 50, 0.9, 12)) != a
    assert eng.prefix_hits == 9
    # the draws are those of an engine without the feature wherever the logits agree: same stream ids
    assert eng.rng_stream[:5].tolist() == list(range(5))


CHECKED_SCRIPT = r"""
import json, sys, torch
sys.path.insert(0, "tests")
import kv_fp8_cases as kc
import prefix_cases as pc
from distributed_lms_raft_llm_amd import ops
from distributed_lms_raft_llm_amd.engine.gpt2_engine import HipGPT2Engine
assert ops.checked_mode()
cfg, w = kc.setup("gpt2-tiny")
prefix, prompts = pc.prefix_and_prompts(cfg, 13)
errors = []
for kv_dtype in ("bf16", "fp8"):
    eng = HipGPT2Engine(cfg, w, max_batch=16, max_length=pc.T, prefix_capacity=pc.CAPACITY, kv_dtype=kv_dtype)
    eng.set_prompt_prefix(prefix)
    out = eng.generate(prompts)
    out2 = eng.generate(prompts)
    errors += ops.device_errors()
# the store-reading decode attention, which 16 rows of the tiny model never reach
H, S, T = 2, 4, 16
z = lambda *shape: torch.zeros(*shape, dtype=torch.bfloat16, device="cuda")
i32 = dict(dtype=torch.int32, device="cuda")
for impl in ("wave", "persist"):
    ops.row_attention(z(3, H * 64), z(S, H, T, 64), z(S, H, T, 64), torch.tensor([3, 0, 2], **i32),
                      torch.tensor([16, 9, 1], **i32), impl=impl,
                      prefix=(z(H, 8, 64), z(H, 8, 64), torch.tensor([8, 0, 1, 5], **i32)))
errors += ops.device_errors()
print("RESULT " + json.dumps({"lens": [len(o) for o in out], "errors": errors, "hits": eng.prefix_hits,
                              "same": out == out2}))
"""


def test_prefix_engine_checked_build_reports_no_device_errors():
    env = dict(os.environ, DLMS_KERNEL_CHECKS="1", PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-c", CHECKED_SCRIPT], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert res["errors"] == [] and res["hits"] == 16 and res["same"] and all(n <= pc.T for n in res["lens"]), res
