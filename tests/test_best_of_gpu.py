"""Best of n on the GPU: ``ops.kv_fork`` (bit-exact copies, every other byte of the cache untouched),
then ``HipGPT2Engine.admit / generate(..., n=k)`` -- the fork of a freshly prefilled slot into its
siblings, held to the fp32 oracle exactly as the sampled decode is (tests/test_sampling_gpu.py,
tests/test_logprobs_gpu.py) -- on the bf16 cache, the fp8 cache and with a prompt prefix, and
``ContinuousBatcher(n=, select=)``.  Cases: tests/best_of_cases.py."""
import math

import numpy as np
import pytest
import torch

import best_of_cases as bc
import kv_fp8_cases as kc
import logprob_cases as lc

pytestmark = pytest.mark.gpu

DEV = "cuda"
PEN = bc.PEN


def _ops():
    from distributed_lms_raft_llm_amd import ops

    return ops


def _sp(seed=None):
    from distributed_lms_raft_llm_amd.models.config import SamplingParams

    t, k, p, s = bc.SAMPLING
    return SamplingParams(t, k, p, s if seed is None else seed)


# ------------------------------------------------------------------ ops.kv_fork
def _cache(geom, dtype, seed):
    ops = _ops()
    host = bc.random_cache(geom, 2 if dtype == "bf16" else 1, seed)
    dev = torch.from_numpy(host).to(DEV).view(torch.bfloat16 if dtype == "bf16" else ops.FP8)
    assert dev.shape == (geom["L"], 2, geom["S"], geom["H"], geom["T"], 64)
    return host, dev


def _fork(kv, pairs):
    cols = [torch.tensor(c, dtype=torch.int32, device=DEV) for c in zip(*pairs)]
    return _ops().kv_fork(kv, *cols)


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("geom", [bc.EXACT, bc.EXACT_EXTRA], ids=["issue", "len0-and-clamp"])
def test_kv_fork_copies_the_named_runs_and_nothing_else(geom, dtype):
    host, kv = _cache(geom, dtype, seed=1)
    out = _fork(kv, geom["pairs"])
    assert out.data_ptr() == kv.data_ptr()
    want = bc.forked(host, geom["pairs"])
    assert not np.array_equal(want, host)
    assert np.array_equal(kv.view(torch.uint8).cpu().numpy(), want)


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_kv_fork_strides_over_more_units_than_workgroups(dtype):
    geom, pairs = bc.STRIDE, bc.stride_pairs()
    lens = [n for _, _, n in pairs]
    assert len(pairs) == 128 and min(lens) == 1 and max(lens) == geom["T"]
    assert len(pairs) * 2 * geom["L"] > 2048  # (the launcher's grid cap)
    host, kv = _cache(geom, dtype, seed=2)
    _fork(kv, pairs)
    assert np.array_equal(kv.view(torch.uint8).cpu().numpy(), bc.forked(host, pairs))


def test_kv_fork_refuses_bad_arguments():
    ops = _ops()
    _, kv = _cache(bc.EXACT, "bf16", seed=3)
    before = kv.clone()

    def t(*v):
        return torch.tensor(v, dtype=torch.int32, device=DEV)

    ops.kv_fork(kv, t(4), t(4), t(3))  # (a self pair: accepted, copies nothing)
    with pytest.raises(ValueError, match="twice"):  # a destination listed twice
        ops.kv_fork(kv, t(4, 0), t(1, 1), t(2, 2))
    with pytest.raises(ValueError, match="read and written"):  # slot 1 is written by one pair and read by another
        ops.kv_fork(kv, t(4, 1), t(1, 2), t(2, 2))
    for args in ((t(4, 0), t(1), t(2, 2)), (t(4), t(1), t(2, 2)), (t(4, 0), t(1, 2), t(2))):
        with pytest.raises(ValueError, match="differ in length"):
            ops.kv_fork(kv, *args)
    with pytest.raises(ValueError):  # a slot outside the cache
        ops.kv_fork(kv, t(4), t(6), t(2))
    with pytest.raises(ValueError):  # not the whole, contiguous cache
        ops.kv_fork(kv[:, :, ::2], t(0), t(1), t(2))
    with pytest.raises(TypeError):
        ops.kv_fork(kv, t(4).long(), t(1), t(2))
    with pytest.raises(ValueError):
        ops.kv_fork(kv.float(), t(4), t(1), t(2))
    assert torch.equal(kv.view(torch.uint8), before.view(torch.uint8))


# ------------------------------------------------------------------ engine
@pytest.fixture(scope="module")
def model():
    from distributed_lms_raft_llm_amd.models.config import gpt2_config
    from distributed_lms_raft_llm_amd.models.gpt2 import GPT2Reference

    cfg = gpt2_config("gpt2")
    w = lc.bf16_exact_weights(cfg)
    return cfg, w, GPT2Reference(cfg, w, device=DEV)


@pytest.fixture(scope="module")
def engines(model):
    from distributed_lms_raft_llm_amd.engine.gpt2_engine import HipGPT2Engine

    cfg, w, _ = model
    made = {}

    def get(kind):
        if kind not in made:
            kw = {"bf16": {}, "fp8": dict(kv_dtype="fp8"), "prefix": dict(prefix_capacity=16)}[kind]
            made[kind] = HipGPT2Engine(cfg, w, max_batch=bc.MAX_BATCH, max_length=bc.T, **kw)
        return made[kind]

    yield get
    for e in made.values():
        e.close()


def _check_fork(eng, prompts, slots, k, first):
    """After ``admit(prompts, slots, n=k)``: every child holds its parent's prompt keys byte for byte
    and its bookkeeping, and draws on its own stream."""
    from distributed_lms_raft_llm_amd.engine.gpt2_engine import seen_bitmap

    torch.cuda.synchronize()
    kvb = eng.kv.view(torch.uint8)
    toks, lens = eng.out_tokens.cpu(), eng.lens.cpu().tolist()
    seen, plen, streams = eng.seen.cpu().numpy(), eng.prompt_len.cpu().tolist(), eng.rng_stream.cpu().tolist()
    for i, p in enumerate(prompts):
        group = slots[i * k: (i + 1) * k]
        parent, n = group[0], len(p)
        assert bool(kvb[:, :, parent, :, :n].any())
        for j, s in enumerate(group):
            assert torch.equal(kvb[:, :, s, :, :n], kvb[:, :, parent, :, :n]), (i, j, "K/V bytes")
            assert toks[s, :n].tolist() == p and lens[s] == lens[parent] == n + 1 and plen[s] == plen[parent] == n
            # the prompt's bits and the slot's own first token's, nothing else
            assert np.array_equal(seen[s], seen_bitmap(p + [int(toks[s, n])], eng.seen_words)), (i, j, "seen")
            assert streams[s] == first + i * k + j, (i, j, streams[s])


def _reset(eng):
    eng._reset_slots(0, eng.max_batch)


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("n_prompts,k", bc.ENGINE_CASES)
def test_admit_forks_the_parent_into_its_siblings(model, engines, n_prompts, k, graph):
    cfg, _, _ = model
    eng = engines("bf16")
    eng.use_graph = graph
    prompts, slots, sp = lc.prompts(cfg, n_prompts), bc.slots_for(n_prompts, k), _sp(seed=100 + k)
    try:
        for sighting in range(3 if graph else 1):  # (the second sighting of a shape captures its prefill graph)
            _reset(eng)
            eng.reseed(sp.seed)
            eng.admit([prompts[0]], [slots[-1]], PEN, sampling=sp, logprobs=True)  # takes stream 0
            first = eng._rng_count
            assert first == 1
            eng.kv.view(torch.uint8)[:, :, slots] = 0  # (nothing of an earlier sighting is left to pass for a copy)
            eng.admit(prompts, slots, PEN, sampling=sp, logprobs=True, n=k)
            assert eng._rng_count == first + n_prompts * k
            _check_fork(eng, prompts, slots, k, first)
        if graph:
            from distributed_lms_raft_llm_amd.engine.mode import DecodeMode

            with eng._mode_scope(DecodeMode(sp, None, True)):
                key = eng._pkey(sum(map(len, prompts)), n_prompts, k)
            assert key[:3] == (sum(map(len, prompts)), n_prompts, k)
            assert key in eng._pgraphs and eng._pgraphs[key]["graph"] is not None
    finally:
        _reset(eng)
        eng.use_graph = True


def _check_completions(oracle, prompts, toks, lps, k, T, eps=0.05, lp_eps=lc.LOGPROB_EPS, what=""):
    from distributed_lms_raft_llm_amd.models.gpt2 import teacher_forced_logprobs, teacher_forced_sampling_check

    sp = _sp()
    worst = 0.0
    assert len(toks) == len(lps) == len(prompts)
    for p, group, glp in zip(prompts, toks, lps):
        assert len(group) == len(glp) == k
        for o, lp in zip(group, glp):
            assert o[: len(p)] == p and len(p) < len(o) <= T
            r = teacher_forced_sampling_check(oracle, o, len(p), PEN, sp, eps=eps)
            assert r["positions"] == len(o) - len(p) and not r["mismatches"], r["mismatches"]
            assert len(lp) == len(o) - len(p) and all(isinstance(v, float) and math.isfinite(v) for v in lp), lp
            worst = max(worst, float(np.abs(np.asarray(lp) - teacher_forced_logprobs(oracle, o, len(p), PEN)).max()))
        assert len({tuple(o) for o in group}) > 1, "the k completions of a prompt are all equal"
    print(f"best of n {what}: largest |engine - oracle| log-probability {worst:.5f} (tolerance {lp_eps:.5f})")
    assert worst <= lp_eps


@pytest.mark.parametrize("n_prompts,k", bc.ENGINE_CASES)
def test_generate_n_completions(model, engines, n_prompts, k):
    from distributed_lms_raft_llm_amd.engine.mode import DecodeMode

    cfg, _, oracle = model
    eng = engines("bf16")
    prompts, sp = lc.prompts(cfg, n_prompts), _sp()
    res = {}
    try:
        for graph in (True, False):
            eng.use_graph = graph
            toks, lps = eng.generate(prompts, repetition_penalty=PEN, sampling=sp, logprobs=True, n=k)
            # the same call twice gives the same output (with graphs: the second replays a captured prefill)
            assert eng.generate(prompts, repetition_penalty=PEN, sampling=sp, logprobs=True, n=k) == (toks, lps)
            only = eng.generate(prompts, repetition_penalty=PEN, sampling=sp, n=k)
            assert [len(g) for g in only] == [k] * n_prompts and all(isinstance(o, list) for g in only for o in g)
            if graph:
                _check_completions(oracle, prompts, toks, lps, k, eng.max_length, what=f"{n_prompts} x {k}")
                R = sum(map(len, prompts))
                with eng._mode_scope(DecodeMode(sp, None, True)):
                    key_n, key_1 = eng._pkey(R, n_prompts, k), eng._pkey(R, n_prompts)
                assert key_n in eng._pgraphs and eng._pgraphs[key_n]["graph"] is not None
                # the n = 1 prefill of the same (rows, prompts) is another entry, with today's key
                assert key_1 == (R, n_prompts) + key_n[3:] and key_1 != key_n
                flat = eng.generate(prompts, repetition_penalty=PEN, sampling=sp, logprobs=True)
                assert eng.generate(prompts, repetition_penalty=PEN, sampling=sp, logprobs=True) == flat
                assert key_1 in eng._pgraphs and eng._pgraphs[key_1] is not eng._pgraphs[key_n]
            res[graph] = (toks, lps)
    finally:
        eng.use_graph = True
    assert res[True] == res[False], "graph replay and eager disagree"


def test_generate_n_leaves_the_other_calls_as_they_were(model, engines):
    cfg, _, _ = model
    eng = engines("bf16")
    eng.use_graph = True
    prompts, sp = lc.prompts(cfg, 3), _sp()
    greedy = eng.generate(prompts, repetition_penalty=PEN)
    sampled = eng.generate(prompts, repetition_penalty=PEN, sampling=sp)
    groups = eng.generate(prompts, repetition_penalty=PEN, sampling=sp, n=4)
    assert [len(g) for g in groups] == [4, 4, 4]
    assert eng.generate(prompts, repetition_penalty=PEN) == greedy
    assert eng.generate(prompts, repetition_penalty=PEN, sampling=sp) == sampled
    assert eng.generate(prompts, repetition_penalty=PEN, sampling=sp, n=1) == sampled
    # more completions than slots run in chunks of whole groups; a pass-through prompt yields n copies
    long = list(range(eng.max_length))
    many = lc.prompts(cfg, 5, seed=9) + [long]
    out = eng.generate(many, repetition_penalty=PEN, sampling=sp, n=8)
    assert [len(g) for g in out] == [8] * 6 and out[5] == [long] * 8
    assert all(o[: len(p)] == p and len(o) > len(p) for g, p in zip(out[:5], many) for o in g)
    # (the first chunk is prompts 0-1 on streams 0 .. 15: what the two-prompt call draws)
    assert out[:2] == eng.generate(many[:2], repetition_penalty=PEN, sampling=sp, n=8)


def test_n_needs_sampling_and_slots(model, engines):
    cfg, _, _ = model
    eng = engines("bf16")
    prompts, sp = lc.prompts(cfg, 2), _sp()
    for call in (lambda: eng.generate(prompts, n=2), lambda: eng.admit(prompts, [0, 1, 2, 3], n=2),
                 lambda: eng.generate(prompts, logprobs=True, n=2)):
        with pytest.raises(ValueError, match="sampling"):
            call()
    for call in (lambda: eng.generate(prompts, sampling=sp, n=bc.MAX_BATCH + 1),
                 lambda: eng.admit(prompts, list(range(16)), sampling=sp, n=bc.MAX_BATCH + 1)):
        with pytest.raises(ValueError, match="max_batch"):
            call()
    with pytest.raises(ValueError):
        eng.generate(prompts, sampling=sp, n=0)
    with pytest.raises(ValueError):  # n slots per prompt
        eng.admit(prompts, [0, 1, 2], sampling=sp, n=2)
    with pytest.raises(ValueError):  # distinct slots
        eng.admit(prompts, [0, 1, 1, 2], sampling=sp, n=2)


def test_best_of_on_the_fp8_cache(model, engines):
    from distributed_lms_raft_llm_amd.models.gpt2 import GPT2Reference

    cfg, w, _ = model
    eng = engines("fp8")
    assert eng.kv.dtype == _ops().FP8
    n_prompts, k = 3, 4
    prompts, slots, sp = lc.prompts(cfg, n_prompts), bc.slots_for(n_prompts, k), _sp()
    eng.reseed(sp.seed)
    eng.admit(prompts, slots, PEN, sampling=sp, logprobs=True, n=k)
    _check_fork(eng, prompts, slots, k, 0)  # (byte equality of the forked e4m3 rows)
    _reset(eng)
    toks, lps = eng.generate(prompts, repetition_penalty=PEN, sampling=sp, logprobs=True, n=k)
    oracle8 = GPT2Reference(cfg, w, device=DEV, kv_dtype="fp8")
    _check_completions(oracle8, prompts, toks, lps, k, eng.max_length, eps=kc.KV_FP8_EPS["gpt2"],
                       lp_eps=lc.LOGPROB_EPS_FP8, what="fp8 cache 3 x 4")


def test_best_of_with_a_prompt_prefix(model, engines):
    cfg, _, oracle = model
    eng = engines("prefix")
    g = torch.Generator().manual_seed(15)

    def draw(n):
        return torch.randint(0, cfg.vocab_size - 1, (n,), generator=g).tolist()

    P, k = 8, 4
    prefix = draw(P)
    prompts = [prefix + draw(3), draw(5), prefix + draw(9)]  # hit, miss, hit
    slots, sp = bc.slots_for(3, k), _sp()
    eng.set_prompt_prefix(prefix)
    eng.reseed(sp.seed)
    eng.kv.zero_()
    eng.admit(prompts, slots, PEN, sampling=sp, logprobs=True, n=k)
    _check_fork(eng, prompts, slots, k, 0)
    # the hits are counted per prompt, not per completion; a child's slot holds the store's rows too
    assert (eng.prefix_prompts, eng.prefix_hits, eng.prefix_rows_skipped) == (3, 2, 2 * P)
    store = eng.pfx_store.view(torch.uint8)
    kvb = eng.kv.view(torch.uint8)
    for i, hit in enumerate((True, False, True)):
        for s in slots[i * k: (i + 1) * k]:
            assert int(eng.slot_pfx[s]) == (P if hit else 0)
            if hit:
                assert torch.equal(kvb[:, :, s, :, :P], store[:, :, :, :P])
    _reset(eng)
    toks, lps = eng.generate(prompts, repetition_penalty=PEN, sampling=sp, logprobs=True, n=k)
    assert eng.generate(prompts, repetition_penalty=PEN, sampling=sp, logprobs=True, n=k) == (toks, lps)
    assert eng.generate(prompts, repetition_penalty=PEN, sampling=sp, logprobs=True, n=k) == (toks, lps)  # (a replay)
    assert (eng.prefix_prompts, eng.prefix_hits) == (12, 8)
    _check_completions(oracle, prompts, toks, lps, k, eng.max_length, what="prefix store 3 x 4")


def test_continuous_batching_serves_groups_and_picks_the_best(model, engines):
    """16 slots, five requests of four completions: the fifth waits for a free group.  Every completion
    is held to the oracle; with ``select`` the future resolves to what ``pick_best`` picks from the
    run without it (same seed, same admissions)."""
    from distributed_lms_raft_llm_amd.engine.scheduler import ContinuousBatcher, pick_best

    cfg, _, oracle = model
    eng = engines("bf16")
    eng.use_graph = True
    prompts, sp, k = lc.prompts(cfg, 5, seed=4), _sp(), 4
    runs = {}
    for select in (None, "mean_logprob"):
        _reset(eng)
        eng.reseed(sp.seed)
        cb = ContinuousBatcher(eng, PEN, chunk=4, n=k, select=select, sampling=sp, logprobs=True)
        try:
            with cb._cv:  # (all five queued before the scheduler looks: four fit)
                futs = [cb.submit(p) for p in prompts]
            runs[select] = [f.result(120) for f in futs]
            assert cb.completed == 5 and cb.active == 0
        finally:
            cb.stop()
    groups = runs[None]
    assert all(isinstance(g, list) and len(g) == k for g in groups)
    _check_completions(oracle, prompts, [[o for o, _ in g] for g in groups], [[lp for _, lp in g] for g in groups], k,
                       eng.max_length, what="continuous batching 5 x 4")
    for g, chosen in zip(groups, runs["mean_logprob"]):
        assert chosen == g[pick_best([lp for _, lp in g])]
