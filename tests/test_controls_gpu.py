"""Generation controls on the GPU: the logit_bans kernel (ops/csrc/controls.hip) against the Python
definition (models/gpt2.py banned_tokens), the stop-checking decode_update against a numpy model
and the plain kernel, then the engine through every decode path, graphs and eager, held to the
fp32 oracle with the bans applied; with sampling, the fp8 cache, the prefix cache and continuous
batching; unsupported combinations."""
import dataclasses

import numpy as np
import pytest
import torch

import controls_cases as cc

pytestmark = pytest.mark.gpu
DEV = "cuda"
PEN = 1.2


def _gc(*a, **k):
    from distributed_lms_raft_llm_amd.models.config import GenerationControls

    return GenerationControls(*a, **k)


# ------------------------------------------------------------------ logit_bans
MAX_LEN, MIN_NEW = 24, 3


def _ban_case(rows, vocab, ld, n, shift):
    """State, logits and, per row, the reference's banned ids.  Rows of length >= MIN_NEW sit at
    L - P = MIN_NEW - 1 (EOS banned) or MIN_NEW (not), alternating."""
    from distributed_lms_raft_llm_amd.models.gpt2 import banned_tokens

    toks, lens, plen = cc.kernel_rows(rows, vocab, n, MAX_LEN, seed=1000 * n + rows + 7 * shift, shift=shift)
    for r in range(rows):
        if lens[r] >= MIN_NEW:
            plen[r] = lens[r] - (MIN_NEW - 1 if (r + n + shift) % 2 else MIN_NEW)
        else:
            plen[r] = min(plen[r], lens[r])
    g = np.random.default_rng(5 + n)
    z = (g.standard_normal((rows, ld)) * 3).astype(np.float32)
    eos = vocab - 1
    ct = _gc(n, MIN_NEW)
    want = [banned_tokens(toks[r, : lens[r]].tolist(), int(plen[r]), ct, eos) for r in range(rows)]
    return toks, lens, plen, z, eos, ct, want


def _check_banned(z0, z1, want, vocab, skip=()):
    """The set of -inf columns is the reference's and every other logit keeps its bits."""
    for r in range(z0.shape[0]):
        ninf = np.nonzero(np.isneginf(z1[r]))[0].tolist()
        assert ninf == ([] if r in skip else want[r]), (r, ninf, want[r])
        keep = np.ones(z0.shape[1], dtype=bool)
        keep[ninf] = False
        assert np.array_equal(z0[r, keep].view(np.uint32), z1[r, keep].view(np.uint32)), r


@pytest.mark.parametrize("n", [1, 2, 3, 5])
@pytest.mark.parametrize("vocab,ld", [(1000, 1024), (50257, 50304)])
@pytest.mark.parametrize("rows", [1, 5])
def test_logit_bans_matches_banned_tokens(rows, vocab, ld, n):
    from distributed_lms_raft_llm_amd import ops
    from distributed_lms_raft_llm_amd.models.config import SamplingParams
    from distributed_lms_raft_llm_amd.models.gpt2 import reference_sample

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    planted = 0
    for shift in (range(5) if rows == 1 else (0,)):  # (one row: each of the lengths 0, 1, n-1, n, max_len in turn)
        toks, lens, plen, z, eos, ct, want = _ban_case(rows, vocab, ld, n, shift)
        planted += sum(len(w) for w in want)
        fin = np.zeros(rows, dtype=np.int32)
        zd = t(z)
        ops.logit_bans(zd[:, :vocab], t(lens), t(fin), t(plen), t(toks), n, MIN_NEW, eos, vocab)
        banned = zd.cpu().numpy()
        _check_banned(z, banned, want, vocab)
        # a finished row is left alone
        fin[rows // 2] = 1
        zd2 = t(z)
        ops.logit_bans(zd2[:, :vocab], t(lens), t(fin), t(plen), t(toks), n, MIN_NEW, eos, vocab)
        _check_banned(z, zd2.cpu().numpy(), want, vocab, skip=(rows // 2,))
        # through a slot map: row i's state lives in slot perm[i] of 8; the other slots hold a
        # sequence that would ban other columns
        perm = [6, 0, 7, 3, 2][:rows]
        toks8 = np.full((8, MAX_LEN), 1, dtype=np.int32)
        lens8, plen8, fin8 = (np.full(8, v, dtype=np.int32) for v in (MAX_LEN, 0, 0))
        toks8[perm], lens8[perm], plen8[perm] = toks, lens, plen
        zd3 = t(z)
        ops.logit_bans(zd3[:, :vocab], t(lens8), t(fin8), t(plen8), t(toks8), n, MIN_NEW, eos, vocab,
                       slot_map=t(np.asarray(perm, dtype=np.int32)))
        assert torch.equal(zd3.view(torch.int32), zd.view(torch.int32))
        # the existing sampler on the banned logits is reference_sample on the same: a banned token is
        # never picked, and top_k = 1 is the best unbanned token
        seen = np.zeros((rows, ld), dtype=bool)
        for r in range(rows):
            seen[r, toks[r, : lens[r]]] = True
        words = np.packbits(seen.reshape(rows, ld // 32, 32), axis=-1, bitorder="little").view(np.uint32)
        sd = t(words.reshape(rows, ld // 32).view(np.int32))
        streams = torch.arange(rows, dtype=torch.int64, device=DEV) + 11
        seed = torch.tensor([77], dtype=torch.int64, device=DEV)
        for sp in (SamplingParams(1.0, 1, 1.0, 77), SamplingParams(0.7, 50, 0.9, 77)):
            keys = torch.zeros(rows, 1, dtype=torch.int64, device=DEV)
            ops.sample_topk_topp(zd[:, :vocab], sd, t(lens), streams, seed, PEN, sp.temperature, sp.top_k, sp.top_p,
                                 vocab, keys)
            got = [int(~np.uint32(np.uint64(k) & np.uint64(0xffffffff))) for k in keys[:, 0].cpu().numpy().view(np.uint64)]
            for r in range(rows):
                tok, _, dec = reference_sample(banned[r, :vocab], seen[r, :vocab], PEN, sp, 11 + r, int(lens[r]))
                assert got[r] not in want[r], (r, got[r])
                if dec or sp.top_k == 1:
                    assert got[r] == tok, (r, sp, got[r], tok)
    assert planted > 0


def test_logit_bans_refuses_bad_arguments():
    from distributed_lms_raft_llm_amd import ops

    z = torch.zeros(2, 64, device=DEV)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=DEV)  # noqa: E731
    ops.logit_bans(z, i32(2), i32(2), i32(2), i32(2, 8), 2, 0, 63, 64)
    for bad in (lambda: ops.logit_bans(z, i32(1), i32(2), i32(2), i32(2, 8), 2, 0, 63, 64),
                lambda: ops.logit_bans(z, i32(2), i32(2), i32(2), i32(1, 8), 2, 0, 63, 64),
                lambda: ops.logit_bans(z, i32(2), i32(2), i32(2), i32(2, 8), -1, 0, 63, 64),
                lambda: ops.logit_bans(z, i32(2), i32(2), i32(2), i32(2, 8), 2, 0, 64, 64),
                lambda: ops.logit_bans(z, i32(2), i32(2), i32(2), i32(2, 8), 2, 0, 63, 65),
                lambda: ops.logit_bans(z, i32(2), i32(2), i32(2), i32(2, 8), 2, 0, 63, 64, slot_map=i32(1))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        ops.logit_bans(z.half(), i32(2), i32(2), i32(2), i32(2, 8), 2, 0, 63, 64)


# ------------------------------------------------------------------ the stop-checking decode_update
STOPS = ((5, 6), (7,), (9, 5, 6), (1, 2, 3, 4, 5, 6, 7, 8))
UP_T, UP_V, UP_D, UP_EOS = 16, 96, 64, 95
# (prompt length, tokens so far, finished, chosen token) -> finishes?
UPDATE_ROWS = [
    (3, [4, 4, 4, 5], 0, 6, True),                      # (5, 6) starts exactly at P
    (4, [4, 4, 4, 5], 0, 6, False),                     # ... one token before P
    (2, [4] * 14 + [5], 0, 6, True),                    # completed at the last index of max_len
    (1, [4, 4, 5, 6], 1, 6, None),                      # a finished row: left alone
    (1, [4], 0, 7, True),                               # a one-token stop as the first generated token
    (1, [4, 1, 2, 3, 4, 5, 6, 7], 0, 8, True),          # the longest stop, from index P
    (2, [4, 1, 2, 3, 4, 5, 6, 7], 0, 8, False),         # ... reaching into the prompt
    (1, [4, 9, 5], 0, 6, True),                         # a stop that is a suffix of another
    (1, [4, 4, 5], 0, 11, False),                       # no match
    (1, [4, 5], 0, UP_EOS, True),                       # EOS stops a row as before
    (1, [4] * 15, 0, 11, True),                         # max_len stops a row as before
]


def _update_state(slot_of):
    from distributed_lms_raft_llm_amd.models.gpt2 import f32_ordered

    B, S = len(UPDATE_ROWS), max(slot_of) + 1
    g = torch.Generator().manual_seed(3)
    st = dict(lens=torch.ones(S, dtype=torch.int32), finished=torch.ones(S, dtype=torch.int32),
              out_tokens=torch.zeros(S, UP_T, dtype=torch.int32), seen=torch.zeros(S, UP_V // 32, dtype=torch.int32),
              cur_tok=torch.zeros(S, dtype=torch.int32), cur_pos=torch.zeros(S, dtype=torch.int32),
              cur_kvlen=torch.ones(S, dtype=torch.int32), x=torch.zeros(S, UP_D), plen=torch.zeros(S, dtype=torch.int32),
              h=torch.zeros(S, UP_D, dtype=torch.bfloat16))
    keys = np.zeros((B, 3), dtype=np.uint64)
    for i, (P, toks, fin, tok, _) in enumerate(UPDATE_ROWS):
        b = slot_of[i]
        st["lens"][b], st["finished"][b], st["plen"][b] = len(toks), fin, P
        st["out_tokens"][b, : len(toks)] = torch.tensor(toks, dtype=torch.int32)
        for part, (v, t) in enumerate(((0.5, 20 + i), (2.0, tok), (-1.0, 3))):  # the chosen token has the largest value
            hi = int(f32_ordered(np.array([v], dtype=np.float32))[0])
            keys[i, part] = np.uint64((hi << 32) | (~t & 0xffffffff))
    wte = torch.randn(UP_V, UP_D, generator=g).to(torch.bfloat16)
    wpe = torch.randn(UP_T, UP_D, generator=g).to(torch.bfloat16)
    ln = (torch.randn(UP_D, generator=g), torch.randn(UP_D, generator=g), 1e-5)
    return ({k: v.to(DEV) for k, v in st.items()}, torch.from_numpy(keys.view(np.int64)).to(DEV), wte.to(DEV),
            wpe.to(DEV), tuple(t.to(DEV) if isinstance(t, torch.Tensor) else t for t in ln))


def _run_update(st, keys, wte, wpe, ln, stops, slot_map, fused):
    from distributed_lms_raft_llm_amd import ops

    st = {k: v.clone() for k, v in st.items()}
    args = (keys, st["lens"], st["finished"], st["out_tokens"], st["seen"], st["cur_tok"], st["cur_pos"],
            st["cur_kvlen"], wte, wpe, st["x"], UP_EOS, UP_T)
    kw = dict(slot_map=slot_map)
    if fused:
        kw.update(ln=ln, h=st["h"])
    if stops is None:
        ops.decode_update(*args, **kw)
    else:
        ops.decode_update_stop(*args, st["plen"], *ops.stop_table(stops, DEV), **kw)
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("mapped", [False, True])
def test_decode_update_stop_against_the_numpy_model(mapped, fused):
    from distributed_lms_raft_llm_amd.models.gpt2 import stop_hit

    B = len(UPDATE_ROWS)
    slot_of = [(5 * i + 3) % 13 for i in range(B)] if mapped else list(range(B))  # (13 slots, 11 rows: distinct)
    assert len(set(slot_of)) == B
    slot_map = torch.tensor(slot_of, dtype=torch.int32, device=DEV) if mapped else None
    st0, keys, wte, wpe, ln = _update_state(slot_of)
    plain = _run_update(st0, keys, wte, wpe, ln, None, slot_map, fused)
    got = _run_update(st0, keys, wte, wpe, ln, STOPS, slot_map, fused)
    none = _run_update(st0, keys, wte, wpe, ln, (), slot_map, fused)
    # with no stops given: bit-identical to ops.decode_update, the stop flags included
    for k in st0:
        assert torch.equal(none[k].view(torch.int16 if none[k].dtype == torch.bfloat16 else none[k].dtype),
                           plain[k].view(torch.int16 if plain[k].dtype == torch.bfloat16 else plain[k].dtype)), k
    # the numpy model of the state: lens, finished, out_tokens, seen, cur_*, x
    lens, fin, out = (st0[k].cpu().numpy().copy() for k in ("lens", "finished", "out_tokens"))
    seen, ctok, cpos, ckv = (st0[k].cpu().numpy().copy() for k in ("seen", "cur_tok", "cur_pos", "cur_kvlen"))
    x = st0["x"].cpu().clone()
    for i, (P, toks, f, tok, want_fin) in enumerate(UPDATE_ROWS):
        b = slot_of[i]
        if f:
            t, pos = toks[-1], len(toks) - 1
        else:
            t, pos = tok, len(toks)
            out[b, pos] = t
            seen.view(np.uint32)[b, t >> 5] |= np.uint32(1 << (t & 31))
            lens[b] = pos + 1
            hit = stop_hit(toks + [t], P, STOPS)
            assert (t == UP_EOS or pos + 1 >= UP_T or hit) == want_fin, i  # (the table above says the same)
            fin[b] = int(want_fin)
        pos = min(pos, UP_T - 1)
        ctok[b], cpos[b], ckv[b] = t, pos, pos + 1
        x[b] = wte[t].float().cpu() + wpe[pos].float().cpu()
    for k, want in (("lens", lens), ("finished", fin), ("out_tokens", out), ("seen", seen), ("cur_tok", ctok),
                    ("cur_pos", cpos), ("cur_kvlen", ckv)):
        assert np.array_equal(got[k].cpu().numpy(), want), (k, got[k].cpu().numpy(), want)
    assert torch.equal(got["x"].cpu().view(torch.int32), x.view(torch.int32))
    # everything but the stop flags is what decode_update writes, bit for bit: the fused LN rows too
    for k in st0:
        if k != "finished":
            assert torch.equal(got[k].view(torch.int16 if got[k].dtype == torch.bfloat16 else got[k].dtype),
                               plain[k].view(torch.int16 if plain[k].dtype == torch.bfloat16 else plain[k].dtype)), k
    if fused:
        assert got["h"].abs().sum() > 0
    stopped = (got["finished"] != plain["finished"]).sum().item()
    assert stopped == 4  # rows 0, 4, 5 and 7 of the table: the rows only a stop sequence finishes
    with pytest.raises(ValueError):
        _run_update(st0, keys, wte, wpe, ln, STOPS + ((1,),), slot_map, fused)


# ------------------------------------------------------------------ engine
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


def _make(cfg, w, kind):
    from distributed_lms_raft_llm_amd.engine.gpt2_engine import HipGPT2Engine

    if kind == "small":  # 1 row, 2 rows (latency path), 9 rows (mid path)
        return HipGPT2Engine(cfg, w, max_batch=16, max_length=40)
    if kind == "panel":  # 256 rows: the panel-resident LM head
        return HipGPT2Engine(cfg, w, max_batch=256, max_length=24)
    # two row parts on two streams: the LM head at a row offset (the mid path off, as
    # tests/test_sampling_gpu.py has it, so graph and eager run the same kernels)
    eng = HipGPT2Engine(cfg, w, max_batch=16, max_length=40, overlap=True, overlap_min_batch=2, overlap_parts=2)
    eng.mid_max = 0
    return eng


def _engine_pool(model):
    cfg, w, _ = model
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = _make(cfg, w, kind)
        return made[kind]

    return made, get


@pytest.fixture(scope="module")
def engines(model):
    """The engines of the banning tests."""
    made, get = _engine_pool(model)
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def stop_engines(model):
    """Engines that only ever see stop-only controls (they must never allocate the logits buffer)."""
    made, get = _engine_pool(model)
    yield get
    for e in made.values():
        e.close()


def _prompts(cfg, n, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, cfg.vocab_size - 1, (int(L),), generator=g).tolist()
            for L in torch.randint(1, 9, (n,), generator=g)]


def _margin_rule(oracle, outs, prompts, ct, eps=0.05, floor=None, eos=None):
    """(b) no mismatch at a decisive position, bans applied; (c) with ``floor``: the decisive share."""
    from distributed_lms_raft_llm_amd.models.gpt2 import teacher_forced_controls_check_batch

    rs = teacher_forced_controls_check_batch(oracle, outs, [len(p) for p in prompts], PEN, ct, eps=eps,
                                             eos_token_id=eos)
    d, n = sum(r["decisive"] for r in rs), sum(r["positions"] for r in rs)
    print(f"controls {ct}: decisive {d}/{n}")
    for r, o, p in zip(rs, outs, prompts):
        assert r["positions"] == len(o) - len(p) and not r["mismatches"], r["mismatches"]
    if floor is not None:
        assert n > 0 and d / n >= floor, (d, n)


@pytest.mark.parametrize("kind,n", [("small", 1), ("small", 2), ("small", 9), ("overlap", 16), ("panel", 256)])
def test_engine_no_repeat_ngram(model, engines, kind, n):
    cfg, _, oracle = model
    eng = engines(kind)
    T = eng.max_length
    assert (n, T) in cc.ENGINE_CASES
    prompts = _prompts(cfg, n, cc.prompt_seed(n))
    if kind == "panel":
        assert eng.ps_lm and n >= eng.PS_LM_MIN_ROWS
    if kind == "overlap":
        assert eng._overlap_ok(16) and not eng._small_ok(16)
    outs = {}
    for graph in (True, False):
        eng.use_graph = graph
        greedy = eng.generate(prompts, repetition_penalty=PEN)
        for size in cc.ENGINE_CASES[(n, T)]:
            ct = _gc(no_repeat_ngram_size=size)
            a = eng.generate(prompts, repetition_penalty=PEN, controls=ct)
            # (a) exact: no generated token completes an n-gram seen before
            for o, p in zip(a, prompts):
                assert o[: len(p)] == p and len(p) < len(o) <= T
                assert cc.repeated_ngrams(o, len(p), size) == [], (size, o)
            # (d) a repeated call returns equal output
            assert a == eng.generate(prompts, repetition_penalty=PEN, controls=ct)
            if graph:  # (b), (c): the eager run is held to be these sequences below
                _margin_rule(oracle, a, prompts, ct, floor=cc.MIN_DECISIVE)
            outs[graph, size] = a
        # without the bans this model loops: the bigram ban changed something
        assert any(cc.repeated_ngrams(o, len(p), 2) for o, p in zip(greedy, prompts))
        # (e) a greedy call without controls afterwards returns what it returned before
        assert eng.generate(prompts, repetition_penalty=PEN) == greedy
    eng.use_graph = True
    for size in cc.ENGINE_CASES[(n, T)]:  # (d) graph replay and eager agree
        assert outs[True, size] == outs[False, size], size


def test_controls_bypass_the_dataflow_decode(model, engines, monkeypatch):
    """(f) one row: greedy decodes on the persistent dataflow kernel (where the engine has it), a call
    with controls -- banning or stop-only -- never launches it."""
    from distributed_lms_raft_llm_amd.engine.mode import DecodeMode

    cfg, _, _ = model
    eng = engines("small")
    eng.use_graph = True
    launches = []
    run = eng._df_run
    monkeypatch.setattr(eng, "_df_run", lambda *a: launches.append(a) or run(*a))
    prompts = _prompts(cfg, 1, cc.prompt_seed(1))
    for ct in (_gc(no_repeat_ngram_size=2), _gc(min_new_tokens=2), _gc(stop=((1, 2),))):
        with eng._mode_scope(DecodeMode(controls=ct)):
            assert not eng._df_ok(1)
        eng.generate(prompts, repetition_penalty=PEN, controls=ct)
        eng.decode(1, 2, PEN, controls=ct)
    assert not launches
    eng.generate(prompts, repetition_penalty=PEN)
    assert bool(launches) == bool(eng.dataflow)


@pytest.mark.parametrize("kind,n", [("small", 1), ("small", 2), ("small", 9), ("overlap", 16)])
def test_engine_stop_sequences(model, stop_engines, monkeypatch, kind, n):
    from distributed_lms_raft_llm_amd.models.gpt2 import stop_hit

    cfg, _, oracle = model
    eng = stop_engines(kind)
    T = eng.max_length
    prompts = _prompts(cfg, n, cc.prompt_seed(n))
    outs = {}
    # (one row: the uncontrolled output that the stop is taken from comes from the launch-per-op
    # path too -- the dataflow kernel, which controls bypass, may differ where the margin is thin)
    monkeypatch.setattr(eng, "dataflow", False)
    for graph in (True, False):
        eng.use_graph = graph
        plain = eng.generate(prompts, repetition_penalty=PEN)
        P0 = len(prompts[0])
        assert len(plain[0]) >= P0 + 6
        stop = (tuple(plain[0][P0 + 4: P0 + 6]),)  # generated positions 4-5 of row 0
        ct = _gc(stop=stop)
        a = eng.generate(prompts, repetition_penalty=PEN, controls=ct)
        assert a == eng.generate(prompts, repetition_penalty=PEN, controls=ct)
        for o, p, full in zip(a, prompts, plain):
            # ends right after its first generated occurrence of the stop, else at EOS or max_length
            assert o[: len(p)] == p and len(o) > len(p) and o == cc.cut_at_stop(o, len(p), stop), (o, stop)
            assert stop_hit(o, len(p), stop) or o[-1] == cfg.eos_token_id or len(o) == T, o
            assert o == cc.cut_at_stop(full, len(p), stop)  # (greedy and deterministic: the plain row, cut)
        assert len(a[0]) <= P0 + 6 < T and any(len(o) < T for o in a)
        if graph:
            _margin_rule(oracle, a, prompts, ct)  # (b), with no bans
        assert eng.generate(prompts, repetition_penalty=PEN) == plain
        outs[graph] = a
    eng.use_graph = True
    assert outs[True] == outs[False], "graph replay and eager disagree"
    assert eng._logits is None, "stop-only controls ran the logits LM head"  # the fused-argmax LM head ran


def test_engine_minimum_length(model):
    """An engine whose EOS is the token row 0 generates at generated index 2: it ends there; with
    min_new_tokens = 6 it goes on for at least 6."""
    from distributed_lms_raft_llm_amd.engine.gpt2_engine import HipGPT2Engine
    from distributed_lms_raft_llm_amd.models.gpt2 import GPT2Reference

    cfg, w, _ = model
    prompts = _prompts(cfg, 2)
    probe = HipGPT2Engine(cfg, w, max_batch=2, max_length=40)
    try:
        row = probe.generate(prompts, repetition_penalty=PEN)[0]
    finally:
        probe.close()
    P = len(prompts[0])
    cfg2 = dataclasses.replace(cfg, eos_token_id=row[P + 2])
    assert cfg2.eos_token_id not in row[: P + 2]
    oracle2 = GPT2Reference(cfg2, w, device="cuda")
    eng = HipGPT2Engine(cfg2, w, max_batch=2, max_length=40)
    try:
        for graph in (True, False):
            eng.use_graph = graph
            short = eng.generate(prompts, repetition_penalty=PEN)
            assert short[0] == row[: P + 3]
            ct = _gc(min_new_tokens=6)
            a = eng.generate(prompts, repetition_penalty=PEN, controls=ct)
            assert len(a[0]) >= P + 6 and cfg2.eos_token_id not in a[0][P: P + 6]
            for o, p in zip(a, prompts):
                assert len(o) - len(p) >= min(6, 40 - len(p))
            _margin_rule(oracle2, a, prompts, ct, eos=cfg2.eos_token_id)
            assert eng.generate(prompts, repetition_penalty=PEN) == short
    finally:
        eng.close()


def test_engine_controls_with_sampling(model, engines):
    from distributed_lms_raft_llm_amd.models.config import SamplingParams
    from distributed_lms_raft_llm_amd.models.gpt2 import teacher_forced_sampling_check

    cfg, _, oracle = model
    eng = engines("small")
    eng.use_graph = True
    prompts = _prompts(cfg, 9)
    sp, ct = SamplingParams(0.7, 50, 0.9, 7), _gc(no_repeat_ngram_size=2)
    a = eng.generate(prompts, repetition_penalty=PEN, sampling=sp, controls=ct)
    assert a == eng.generate(prompts, repetition_penalty=PEN, sampling=sp, controls=ct)
    assert a != eng.generate(prompts, repetition_penalty=PEN, controls=ct)
    for o, p in zip(a, prompts):
        assert o[: len(p)] == p and cc.repeated_ngrams(o, len(p), 2) == [], o
        r = teacher_forced_sampling_check(oracle, o, len(p), PEN, sp, controls=ct)
        assert r["positions"] == len(o) - len(p) and not r["mismatches"], r["mismatches"]
    eng.use_graph = False
    assert a == eng.generate(prompts, repetition_penalty=PEN, sampling=sp, controls=ct)
    eng.use_graph = True


def test_engine_controls_on_the_fp8_cache(model):
    import kv_fp8_cases as kc
    from distributed_lms_raft_llm_amd.engine.gpt2_engine import HipGPT2Engine
    from distributed_lms_raft_llm_amd.models.gpt2 import GPT2Reference

    cfg, w, _ = model
    prompts = _prompts(cfg, 4)
    ct = _gc(no_repeat_ngram_size=2, min_new_tokens=4)
    eng = HipGPT2Engine(cfg, w, max_batch=4, max_length=40, kv_dtype="fp8")
    try:
        a = eng.generate(prompts, repetition_penalty=PEN, controls=ct)
        assert a == eng.generate(prompts, repetition_penalty=PEN, controls=ct)
    finally:
        eng.close()
    for o, p in zip(a, prompts):
        assert cc.repeated_ngrams(o, len(p), 2) == [], o
    _margin_rule(GPT2Reference(cfg, w, device="cuda", kv_dtype="fp8"), a, prompts, ct, eps=kc.KV_FP8_EPS["gpt2"])


def test_engine_controls_with_the_prefix_cache(model):
    from distributed_lms_raft_llm_amd.engine.gpt2_engine import HipGPT2Engine

    cfg, w, oracle = model
    prefix = _prompts(cfg, 1, seed=9)[0] + [17, 4242, 17, 4242, 17]  # (repeats inside the prefix: bans see them)
    prompts = [prefix + s for s in _prompts(cfg, 4)]
    ct = _gc(no_repeat_ngram_size=2, stop=((50000, 50001),))
    eng = HipGPT2Engine(cfg, w, max_batch=4, max_length=40, prefix_capacity=64)
    try:
        eng.set_prompt_prefix(prefix)
        a = eng.generate(prompts, repetition_penalty=PEN, controls=ct)
        assert eng.prefix_hits == 4
        assert a == eng.generate(prompts, repetition_penalty=PEN, controls=ct)
    finally:
        eng.close()
    for o, p in zip(a, prompts):
        assert o[: len(p)] == p and cc.repeated_ngrams(o, len(p), 2) == [], o
    _margin_rule(oracle, a, prompts, ct)


def test_continuous_batching_with_controls(model):
    """Chunk 4, four requests through ContinuousBatcher(controls=): every result has no repeated
    bigram and obeys the stop rule (the stop: generated tokens 4-5 of request 0 in a static batch of
    the four under the bigram ban alone)."""
    from distributed_lms_raft_llm_amd.engine.gpt2_engine import HipGPT2Engine
    from distributed_lms_raft_llm_amd.engine.scheduler import ContinuousBatcher
    from distributed_lms_raft_llm_amd.models.gpt2 import stop_hit

    cfg, w, oracle = model
    T = 40
    prompts = _prompts(cfg, 4)
    ban = _gc(no_repeat_ngram_size=2)
    eng = HipGPT2Engine(cfg, w, max_batch=4, max_length=T, prefill_split=1)
    try:
        first = eng.generate(prompts, repetition_penalty=PEN, controls=ban)[0]
        P0 = len(prompts[0])
        stop = (tuple(first[P0 + 4: P0 + 6]),)
        ct = _gc(no_repeat_ngram_size=2, stop=stop)
        cb = ContinuousBatcher(eng, PEN, chunk=4, controls=ct)
        try:
            cb._cv.acquire()  # (admit the four together, as the static batch above prefilled them)
            try:
                futs = [cb.submit(p) for p in prompts]
            finally:
                cb._cv.release()
            outs = [f.result(60) for f in futs]
        finally:
            cb.stop()
    finally:
        eng.close()
    for o, p in zip(outs, prompts):
        assert o[: len(p)] == p and len(o) > len(p)
        assert cc.repeated_ngrams(o, len(p), 2) == [], o
        assert o == cc.cut_at_stop(o, len(p), stop)
        assert stop_hit(o, len(p), stop) or o[-1] == cfg.eos_token_id or len(o) == T, o
    assert any(stop_hit(o, len(p), stop) for o, p in zip(outs, prompts))
    _margin_rule(oracle, outs, prompts, ct)


def test_unsupported_combinations_raise(model, engines):
    from distributed_lms_raft_llm_amd.engine.gpt2_engine import HipGPT2Engine, controls_unsupported

    cfg, w, _ = model
    ct = _gc(no_repeat_ngram_size=2, stop=((1, 2),))
    e8 = HipGPT2Engine(cfg, w, max_batch=2, max_length=24, weight_dtype="fp8")
    try:
        for call in (lambda: e8.generate([[1, 2]], controls=ct), lambda: e8.admit([[1, 2]], [0], controls=ct),
                     lambda: e8.decode(2, 1, controls=ct), lambda: e8.warm_decode_graphs(controls=ct)):
            with pytest.raises(ValueError, match="fp8"):
                call()
        assert len(e8.generate([[1, 2]])[0]) > 2  # greedy still serves
    finally:
        e8.close()
    eng = engines("small")
    eng.tp_size = 2  # (what a TP rank's engine reports; the check runs before any device work)
    try:
        with pytest.raises(ValueError, match="tensor parallelism"):
            eng.generate([[1, 2]], controls=ct)
    finally:
        eng.tp_size = 1
    assert len(eng.generate([[1, 2]])[0]) > 2
    assert "tensor parallelism" in controls_unsupported(8, False) and controls_unsupported(1, False) is None
    with pytest.raises(TypeError):
        eng.generate([[1, 2]], controls=(2, 0, ()))
    with pytest.raises(ValueError):  # a row could be banned completely
        HipGPT2Engine(cfg, w, max_batch=1, max_length=cfg.vocab_size - 1)
