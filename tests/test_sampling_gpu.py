"""Seeded temperature / top-k / top-p sampling on the GPU: the sampler kernel (ops/csrc/sample.hip)
against the CPU definition (models/gpt2.py reference_sample), then the engine through every decode
path, graphs and eager, held to the fp32 oracle; continuous batching; unsupported combinations."""
import functools

import numpy as np
import pytest
import torch

import sampling_cases as sc

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ kernel
@functools.lru_cache(maxsize=None)
def _reference(case):
    """The case's inputs and, per row, reference_sample's (token, m, decisive) + the key's high word:
    computed once, shared by the tests below."""
    from distributed_lms_raft_llm_amd.models.config import SamplingParams
    from distributed_lms_raft_llm_amd.models.gpt2 import f32_ordered, penalised_logits_f32, reference_sample

    _, vocab, ld, rows, k, p, T = next(c for c in sc.all_cases() if c[0] == case)
    z, seen, streams, positions = sc.make_case(vocab, ld, rows, p, case)
    sp = SamplingParams(T, k, p, sc.SEED)
    ref = []
    for r in range(rows):
        tok, m, dec = reference_sample(z[r, :vocab], seen[r], sc.PENALTY, sp, int(streams[r]), int(positions[r]))
        hi = int(f32_ordered(penalised_logits_f32(z[r, tok:tok + 1], seen[r, tok:tok + 1], sc.PENALTY))[0])
        ref.append((tok, m, dec, hi))
    return (vocab, ld, rows, sp), (z, seen, streams, positions), ref


def _device_inputs(z, seen, streams, positions, ld):
    dev = "cuda"
    return (torch.from_numpy(z).to(dev), torch.from_numpy(sc.seen_words(seen, ld // 32)).to(dev),
            torch.from_numpy(positions).to(dev), torch.from_numpy(streams).to(dev),
            torch.tensor([sc.SEED - 2 ** 64], dtype=torch.int64, device=dev))  # (the int64 with SEED's bits)


def _run(sp, vocab, zd, sd, lens, streams, seed, slot_map=None):
    from distributed_lms_raft_llm_amd import ops

    keys = torch.zeros(zd.shape[0], 3, dtype=torch.int64, device="cuda")
    ops.sample_topk_topp(zd, sd, lens, streams, seed, sc.PENALTY, sp.temperature, sp.top_k, sp.top_p, vocab, keys,
                         slot_map=slot_map)
    k = keys[:, 0].cpu().numpy().view(np.uint64)
    assert not keys[:, 1:].any()  # one key per row, nothing beside it
    return [(int(~np.uint32(x & np.uint64(0xffffffff))), int(x >> np.uint64(32))) for x in k]


def test_device_philox_known_answers():
    from distributed_lms_raft_llm_amd import ops

    ck = torch.tensor([[0, 0, 0, 0, 0, 0], [0xffffffff] * 6,
                       [0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0]], device="cuda")
    assert ops.philox4x32_10(ck).tolist() == [[0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8],
                                              [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd],
                                              [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]]


@pytest.mark.parametrize("case", [c[0] for c in sc.all_cases()])
def test_kernel_matches_reference(case):
    (vocab, ld, rows, sp), inputs, ref = _reference(case)
    got = _run(sp, vocab, *_device_inputs(*inputs, ld))
    print(f"case {case}: vocab {vocab} rows {rows} {sp}: decisive {sum(r[2] for r in ref)}/{rows}, "
          f"token matches {sum(g[0] == r[0] for g, r in zip(got, ref))}, nucleus sizes {[r[1] for r in ref][:8]}")
    for r, ((tok, hi), (rtok, _, dec, rhi)) in enumerate(zip(got, ref)):
        assert 0 <= tok < vocab, (r, tok)
        if dec:
            assert (tok, hi) == (rtok, rhi), (case, r, sc.row_kind(r, case, sp.top_p), (tok, hi), (rtok, rhi))
    assert sum(not r[2] for r in ref) <= 0.03 * rows


def test_row_and_slot_map_do_not_change_the_draw():
    case = next(c[0] for c in sc.all_cases() if c[3] == 5 and c[4] == 50)
    (vocab, ld, rows, sp), (z, seen, streams, positions), ref = _reference(case)
    zd, sd, lens, st, seed = _device_inputs(z, seen, streams, positions, ld)
    direct = _run(sp, vocab, zd, sd, lens, st, seed)
    # row 3 of 5 alone as row 0, same stream and position
    alone = _run(sp, vocab, zd[3:4].clone(), sd[3:4].clone(), lens[3:4].clone(), st[3:4].clone(), seed)
    assert alone[0] == direct[3]
    # through a slot map: row i's state lives in slot perm[i] of 8
    perm = [6, 0, 7, 3, 2]
    lens8 = torch.full((8,), 149, dtype=torch.int32, device="cuda")
    st8 = torch.full((8,), 12345, dtype=torch.int64, device="cuda")
    idx = torch.tensor(perm, device="cuda")
    lens8[idx], st8[idx] = lens, st
    mapped = _run(sp, vocab, zd, sd, lens8, st8, seed, slot_map=torch.tensor(perm, dtype=torch.int32, device="cuda"))
    assert mapped == direct
    # and the draw does depend on stream, position and seed
    other = _run(sp, vocab, zd, sd, lens + 1, st, seed)
    assert other != direct and _run(sp, vocab, zd, sd, lens, st + 1, seed) != direct
    assert _run(sp, vocab, zd, sd, lens, st, seed + 1) != direct


# ------------------------------------------------------------------ engine
PEN = 1.2


@pytest.fixture(scope="module")
def model():
    from distributed_lms_raft_llm_amd.models.config import gpt2_config
    from distributed_lms_raft_llm_amd.models.gpt2 import GPT2Reference, init_gpt2_weights

    cfg = gpt2_config("gpt2")
    w = init_gpt2_weights(cfg, seed=0)
    for k, v in w.items():  # bf16-exact weights: the oracle sees exactly what the kernels see
        if v.dim() == 2:
            w[k] = v.to(torch.bfloat16).float()
    return cfg, w, GPT2Reference(cfg, w, device="cuda")


@pytest.fixture(scope="module")
def engines(model):
    from distributed_lms_raft_llm_amd.engine.gpt2_engine import HipGPT2Engine

    cfg, w, _ = model
    made = {}

    def get(kind):
        if kind not in made:
            if kind == "small":  # 1 row, 2 rows (latency path), 9 rows (mid path)
                made[kind] = HipGPT2Engine(cfg, w, max_batch=16, max_length=40)
            elif kind == "panel":  # 256 rows: the panel-resident LM head
                made[kind] = HipGPT2Engine(cfg, w, max_batch=256, max_length=24)
            else:  # two row parts on two streams: the LM head at a row offset
                made[kind] = HipGPT2Engine(cfg, w, max_batch=16, max_length=40, overlap=True, overlap_min_batch=2,
                                           overlap_parts=2)
                # (the mid path would take single 16-row steps -- every eager step -- ahead of the
                # overlapped one: off, as DLMS_MID_PATH=0 does, so graph and eager run the same kernels)
                made[kind].mid_max = 0
        return made[kind]

    yield get
    for e in made.values():
        e.close()


def _prompts(cfg, n, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, cfg.vocab_size - 1, (int(L),), generator=g).tolist()
            for L in torch.randint(1, 9, (n,), generator=g)]


@pytest.mark.parametrize("kind,n", [("small", 1), ("small", 2), ("small", 9), ("panel", 256), ("overlap", 16)])
def test_engine_sampling(model, engines, kind, n):
    from distributed_lms_raft_llm_amd.models.config import SamplingParams
    from distributed_lms_raft_llm_amd.models.gpt2 import teacher_forced_check_batch, teacher_forced_sampling_check

    cfg, _, oracle = model
    eng = engines(kind)
    prompts = _prompts(cfg, n)
    sp = SamplingParams(0.7, 50, 0.9, 7)
    if kind == "panel":
        assert eng.ps_lm and n >= eng.PS_LM_MIN_ROWS
    if kind == "overlap":
        assert eng._overlap_ok(16) and not eng._small_ok(16)
    outs = {}
    for graph in (True, False):
        eng.use_graph = graph
        greedy = eng.generate(prompts, repetition_penalty=PEN)
        a = eng.generate(prompts, repetition_penalty=PEN, sampling=sp)
        assert a == eng.generate(prompts, repetition_penalty=PEN, sampling=sp), "same seed, other output"
        other = eng.generate(prompts, repetition_penalty=PEN, sampling=SamplingParams(0.7, 50, 0.9, 8))
        assert any(x != y for x, y in zip(a, other)), "another seed, same output"
        k1 = eng.generate(prompts, repetition_penalty=PEN, sampling=SamplingParams(0.7, 1, 0.9, 7))
        assert eng.generate(prompts, repetition_penalty=PEN) == greedy, "a sampled call changed greedy decoding"
        for o, p in zip(a, prompts):
            assert o[: len(p)] == p and len(p) < len(o) <= eng.max_length
            if not graph:  # (held to be the graph run's sequences below: checked there)
                continue
            r = teacher_forced_sampling_check(oracle, o, len(p), PEN, sp)
            assert r["positions"] == len(o) - len(p) and not r["mismatches"], r["mismatches"]
        for r in teacher_forced_check_batch(oracle, k1, [len(p) for p in prompts], PEN, eps=0.05):
            assert not r["mismatches"], (graph, r["mismatches"])
        assert any(x != y for x, y in zip(a, greedy))
        outs[graph] = a
    eng.use_graph = True
    assert outs[True] == outs[False], "graph replay and eager disagree"


def test_sampling_bypasses_the_dataflow_decode(model, engines, monkeypatch):
    """One row: greedy decodes on the persistent dataflow kernel (where the engine has it), a sampled
    call never launches it."""
    from distributed_lms_raft_llm_amd.engine.mode import DecodeMode
    from distributed_lms_raft_llm_amd.models.config import SamplingParams

    cfg, _, _ = model
    eng = engines("small")
    eng.use_graph = True
    launches = []
    run = eng._df_run
    monkeypatch.setattr(eng, "_df_run", lambda *a: launches.append(a) or run(*a))
    with eng._mode_scope(DecodeMode(sampling=SamplingParams())):
        assert not eng._df_ok(1)
    prompts = _prompts(cfg, 1)
    eng.generate(prompts, repetition_penalty=PEN, sampling=SamplingParams(0.7, 50, 0.9, 1))
    eng.decode(1, 2, PEN, sampling=SamplingParams(0.7, 50, 0.9, 1))
    assert not launches
    eng.generate(prompts, repetition_penalty=PEN)
    assert bool(launches) == bool(eng.dataflow)


def test_continuous_batching_is_batch_invariant(model):
    """The same request, reseeded to the same stream id, alone and among three others: the same
    tokens.  "Alone": its three companions are prompts one token short of max_length, which finish
    at admission, so it decodes with no live row beside it; "among": three live companions.  In both
    runs it is the fourth admission (stream 3, slot 3, the 4-row bucket), so its arithmetic is the
    same kernels on the same rows, and with it the draws must be."""
    from distributed_lms_raft_llm_amd.engine.gpt2_engine import HipGPT2Engine
    from distributed_lms_raft_llm_amd.engine.scheduler import ContinuousBatcher
    from distributed_lms_raft_llm_amd.models.config import SamplingParams
    from distributed_lms_raft_llm_amd.models.gpt2 import teacher_forced_sampling_check

    cfg, w, oracle = model
    T = 32
    sp = SamplingParams(0.7, 50, 0.9, 21)
    eng = HipGPT2Engine(cfg, w, max_batch=4, max_length=T, prefill_split=1)
    g = torch.Generator().manual_seed(11)
    leaving = [torch.randint(0, cfg.vocab_size - 1, (T - 1,), generator=g).tolist() for _ in range(3)]
    staying = _prompts(cfg, 3, seed=5)
    request = [464, 3290, 318, 257]
    cb = ContinuousBatcher(eng, PEN, chunk=4, sampling=sp)
    try:
        eng.reseed(sp.seed)
        cb._cv.acquire()  # (admit the four together: the request is the fourth)
        try:
            futs = [cb.submit(p) for p in leaving + [request]]
        finally:
            cb._cv.release()
        alone = [f.result(60) for f in futs]
        assert cb.active == 0
        eng.reseed(sp.seed)  # (the batcher is idle) stream ids start over
        cb._cv.acquire()
        try:
            futs = [cb.submit(p) for p in staying + [request]]
        finally:
            cb._cv.release()
        among = [f.result(60) for f in futs]
    finally:
        cb.stop()
        eng.close()
    assert all(len(o) == T for o in alone[:3])
    for o, p in zip(alone + among, leaving + [request] + staying + [request]):
        r = teacher_forced_sampling_check(oracle, o, len(p), PEN, sp)
        assert o[: len(p)] == p and r["positions"] > 0 and not r["mismatches"], r["mismatches"]
    assert len(alone[3]) > len(request) + 1 and among[3] == alone[3]
    assert any(len(o) > len(p) + 1 for o, p in zip(among[:3], staying))


def test_unsupported_combinations_raise(model, engines):
    from distributed_lms_raft_llm_amd.engine.gpt2_engine import HipGPT2Engine, sampling_unsupported
    from distributed_lms_raft_llm_amd.models.config import SamplingParams

    cfg, w, _ = model
    sp = SamplingParams()
    e8 = HipGPT2Engine(cfg, w, max_batch=2, max_length=24, weight_dtype="fp8")
    try:
        for call in (lambda: e8.generate([[1, 2]], sampling=sp), lambda: e8.admit([[1, 2]], [0], sampling=sp),
                     lambda: e8.decode(2, 1, sampling=sp), lambda: e8.warm_decode_graphs(sampling=sp)):
            with pytest.raises(ValueError, match="fp8"):
                call()
        assert len(e8.generate([[1, 2]])[0]) > 2  # greedy still serves
    finally:
        e8.close()
    eng = engines("small")
    eng.tp_size = 2  # (what a TP rank's engine reports; the check runs before any device work)
    try:
        with pytest.raises(ValueError, match="tensor parallelism"):
            eng.generate([[1, 2]], sampling=sp)
    finally:
        eng.tp_size = 1
    assert "tensor parallelism" in sampling_unsupported(8, False)
    with pytest.raises(TypeError):
        eng.generate([[1, 2]], sampling=(0.7, 50, 0.9))
