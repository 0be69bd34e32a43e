"""Best of n on the CPU: the reference engine's definition of n completions per prompt, that the GPU
cases' completions are pairwise distinct on the reference, ``pick_best``, the continuous batcher's
groups of slots on a fake engine, and the tutor server's flag checks."""
from types import SimpleNamespace

import pytest

import best_of_cases as bc
import logprob_cases as lc
from distributed_lms_raft_llm_amd.engine.gpt2_engine import TorchGPT2Engine
from distributed_lms_raft_llm_amd.engine.scheduler import ContinuousBatcher, GainMeter, pick_best
from distributed_lms_raft_llm_amd.models.config import SamplingParams, gpt2_config
from distributed_lms_raft_llm_amd.models.gpt2 import init_gpt2_weights

SP = SamplingParams(*bc.SAMPLING)


# ------------------------------------------------------------------ the reference engine
def _tiny():
    """test_sampling_cpu.py's 2-layer model with logits spread over a few units."""
    cfg = gpt2_config("gpt2-tiny")
    w = init_gpt2_weights(cfg, seed=0)
    w["transformer.wte.weight"] = w["transformer.wte.weight"] * 20.0
    for k in w:
        if k.endswith("c_proj.weight"):
            w[k] = w[k] * 200.0
    return cfg, w


PROMPTS = [[1, 2, 3, 1, 2], [7, 8], [5], list(range(30))]  # (the last only passes through at max_length 24)


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("logprobs", [False, True])
def test_torch_engine_n_is_each_prompt_repeated_n_times(k, logprobs):
    cfg, w = _tiny()
    eng = TorchGPT2Engine(cfg, w, max_length=24)
    got = eng.generate(PROMPTS, repetition_penalty=bc.PEN, sampling=SP, n=k, logprobs=logprobs)
    flat = eng.generate([p for p in PROMPTS for _ in range(k)], repetition_penalty=bc.PEN, sampling=SP,
                        logprobs=logprobs)
    toks, flat_t = (got[0], flat[0]) if logprobs else (got, flat)
    assert len(toks) == len(PROMPTS) and all(len(g) == k for g in toks)
    assert [o for g in toks for o in g] == flat_t
    if logprobs:
        assert [lp for g in got[1] for lp in g] == flat[1]
        assert all(len(lp) == len(o) - len(p) for g, gl, p in zip(toks, got[1], PROMPTS) for o, lp in zip(g, gl))
    assert toks[3] == [PROMPTS[3]] * k  # a prompt that only passes through yields n copies
    assert any(len({tuple(o) for o in g}) > 1 for g in toks[:3])  # the streams differ
    # n = 1 is the call without n
    assert eng.generate(PROMPTS, repetition_penalty=bc.PEN, sampling=SP, n=1) == \
        eng.generate(PROMPTS, repetition_penalty=bc.PEN, sampling=SP)


def test_torch_engine_refuses_n_without_sampling():
    cfg, w = _tiny()
    eng = TorchGPT2Engine(cfg, w, max_length=24)
    with pytest.raises(ValueError, match="sampling"):
        eng.generate(PROMPTS, n=2)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            eng.generate(PROMPTS, sampling=SP, n=bad)


def test_the_gpu_cases_completions_are_pairwise_distinct_on_the_reference():
    """What tests/test_best_of_gpu.py relies on when it asserts that the k completions of a prompt are
    not all equal: on the fp32 reference, for every engine case, they are pairwise distinct."""
    cfg = gpt2_config("gpt2")
    eng = TorchGPT2Engine(cfg, lc.bf16_exact_weights(cfg), max_length=bc.T)
    for n_prompts, k in bc.ENGINE_CASES:
        prompts = lc.prompts(cfg, n_prompts)
        outs = eng.generate(prompts, repetition_penalty=bc.PEN, sampling=SP, n=k)
        for p, group in zip(prompts, outs):
            assert all(o[: len(p)] == p and len(o) > len(p) for o in group)
            assert len({tuple(o) for o in group}) == k, (n_prompts, k, group)


# ------------------------------------------------------------------ pick_best
@pytest.mark.parametrize("lists,want", bc.PICK_CASES)
def test_pick_best(lists, want):
    assert pick_best(lists) == want
    assert pick_best(tuple(tuple(lp) for lp in lists)) == want


def test_pick_best_needs_a_candidate_and_the_gain_is_chosen_minus_group_mean():
    with pytest.raises(ValueError):
        pick_best([])
    m = GainMeter()
    assert m.mean is None
    m.add([[-1.0, -3.0], [-1.0], [-6.0]], 1)  # means -2, -1, -6: the group's average is -3
    assert m.mean == pytest.approx(2.0)
    m.add([[-4.0], [-2.0], [], [bc.NAN]], 1)  # the lists that cannot be judged are left out: (-4 - 2) / 2
    assert m.mean == pytest.approx((2.0 + 1.0) / 2) and m.answers == 2
    m.add([[], []], 0)  # nothing to judge: not counted
    assert m.answers == 2


# ------------------------------------------------------------------ the continuous batcher
EOS, V = 99, 100


def fake_completion(prompt, j, max_length):
    """Completion j of ``prompt`` on the fake engine: 2 + 3 j tokens, each a function of the sequence
    so far and of j."""
    seq = list(prompt)
    want = min(max_length, len(prompt) + 2 + 3 * j)
    while len(seq) < want:
        seq.append((sum(seq) * 31 + 7 * j + len(seq)) % (V - 1))
    return seq


def fake_logprobs(prompt, seq):
    return [-((t % 7) + 1) / 4 for t in seq[len(prompt):]]


class FakeGroupEngine:
    """A slot engine that knows ``admit(..., n=)``: completion j of a prompt takes 2 + 3 j tokens, so
    siblings finish at different steps."""

    def __init__(self, max_batch=4, max_length=40):
        self.max_batch, self.max_length = max_batch, max_length
        self.cfg = SimpleNamespace(eos_token_id=EOS)
        self.seqs = [[EOS] for _ in range(max_batch)]
        self.plan = [[EOS] for _ in range(max_batch)]
        self.prompts = [[EOS] for _ in range(max_batch)]
        self.fin = [1] * max_batch
        self.admissions = []  # (slots, extra keyword arguments, slots live at the time)
        self.collected = []

    def admit(self, prompts, slots, penalty, **kw):
        live = [s for s in range(self.max_batch) if not self.fin[s]]
        self.admissions.append((list(slots), dict(kw), live))
        k = kw.get("n", 1)
        assert len(slots) == k * len(prompts) and len(set(slots)) == len(slots)
        for i, p in enumerate(prompts):
            for j, s in enumerate(slots[i * k: (i + 1) * k]):
                assert self.fin[s], "admitted into a live slot"
                self.prompts[s], self.plan[s] = list(p), fake_completion(p, j, self.max_length)
                self.seqs[s], self.fin[s] = list(p), 0
                self._step(s)

    def _step(self, s):
        if not self.fin[s]:
            self.seqs[s].append(self.plan[s][len(self.seqs[s])])
            self.fin[s] = int(len(self.seqs[s]) == len(self.plan[s]))

    def decode(self, B, steps, penalty, **kw):
        assert all(self.fin[s] for s in range(B, self.max_batch)), "live slot outside bucket"
        for _ in range(steps):
            for s in range(B):
                self._step(s)

    def finished_flags(self, B):
        return self.fin[:B]

    def collect(self, slots, logprobs=False):
        self.collected.append((list(slots), [self.fin[s] for s in slots]))
        toks = [list(self.seqs[s]) for s in slots]
        return (toks, [fake_logprobs(self.prompts[s], self.seqs[s]) for s in slots]) if logprobs else toks


REQUESTS = [[3, 1, 4], [1, 5, 9, 2, 6]]


def _submit_together(cb, prompts):
    with cb._cv:  # (both queued before the scheduler looks)
        return [cb.submit(p) for p in prompts]


@pytest.mark.parametrize("logprobs", [False, True])
def test_batcher_groups_take_and_free_their_slots_together(logprobs):
    eng = FakeGroupEngine(max_batch=4)
    cb = ContinuousBatcher(eng, chunk=2, n=3, logprobs=logprobs)
    try:
        outs = [f.result(30) for f in _submit_together(cb, REQUESTS)]
    finally:
        cb.stop()
    want = [[fake_completion(p, j, eng.max_length) for j in range(3)] for p in REQUESTS]
    if logprobs:
        want = [[(o, fake_logprobs(p, o)) for o in g] for g, p in zip(want, REQUESTS)]
    assert outs == want and all(isinstance(o, list) and len(o) == 3 for o in outs)
    # four slots, three per request: admitted one after the other, the second only once all three
    # slots of the first were free again -- none was live, none shared
    assert len(eng.admissions) == 2
    (s0, kw0, live0), (s1, kw1, live1) = eng.admissions
    assert kw0.get("n") == 3 and kw1.get("n") == 3
    assert len(set(s0)) == 3 and len(set(s1)) == 3 and live0 == [] and live1 == []
    # one collect per group, of its three slots, every one of them finished
    assert [sorted(c[0]) for c in eng.collected] == [sorted(s0), sorted(s1)]
    assert all(all(c[1]) for c in eng.collected)
    assert cb.completed == 2 and cb.active == 0


def test_batcher_select_resolves_to_the_best_completion():
    eng = FakeGroupEngine(max_batch=4)
    cb = ContinuousBatcher(eng, chunk=2, n=3, logprobs=True, select="mean_logprob")
    try:
        outs = [f.result(30) for f in _submit_together(cb, REQUESTS)]
        long = cb.submit(list(range(eng.max_length))).result(5)  # passes through: nothing to choose from
    finally:
        cb.stop()
    bests = []
    for p, got in zip(REQUESTS, outs):
        group = [fake_completion(p, j, eng.max_length) for j in range(3)]
        lps = [fake_logprobs(p, o) for o in group]
        bests.append(pick_best(lps))
        assert got == (group[bests[-1]], lps[bests[-1]])
    assert any(bests), "the fake's best is always completion 0: the choice is not tested"
    assert long == (list(range(eng.max_length)), [])
    assert cb.gain.answers == 2 and cb.gain.mean >= 0


def test_batcher_refuses_what_it_cannot_serve_and_n_1_is_the_old_call():
    eng = FakeGroupEngine(max_batch=4)
    with pytest.raises(ValueError, match="logprobs"):
        ContinuousBatcher(eng, n=3, select="mean_logprob")
    with pytest.raises(ValueError, match="slots"):
        ContinuousBatcher(eng, n=5)
    with pytest.raises(ValueError):
        ContinuousBatcher(eng, n=0)
    with pytest.raises(ValueError, match="select"):
        ContinuousBatcher(eng, n=2, logprobs=True, select="longest")
    cb = ContinuousBatcher(eng, chunk=2)
    try:
        out = cb.submit(REQUESTS[0]).result(30)
    finally:
        cb.stop()
    assert out == fake_completion(REQUESTS[0], 0, eng.max_length)
    assert [kw for _, kw, _ in eng.admissions] == [{}]  # no n argument: engines without it are served as before


# ------------------------------------------------------------------ the tutor server's flags
def test_tutor_best_of_implies_sampling_and_logprobs():
    from distributed_lms_raft_llm_amd.tutor.server import apply_best_of, arg_parser, sampling_from_args

    args = arg_parser().parse_args(["--best-of", "4"])
    assert args.best_of == 4 and not args.sample and not args.logprobs
    apply_best_of(args)
    assert args.sample and args.logprobs and sampling_from_args(args) == SamplingParams(0.7, 50, 0.9, 0)
    plain = arg_parser().parse_args([])
    apply_best_of(plain)
    assert plain.best_of == 1 and not plain.sample and not plain.logprobs and sampling_from_args(plain) is None
    for bad in (["--best-of", "0"], ["--best-of", "4", "--max-batch", "2"]):
        with pytest.raises(ValueError):
            apply_best_of(arg_parser().parse_args(bad))


def test_tutor_cli_refuses_best_of_on_tp_or_fp8_before_any_engine(capsys, monkeypatch):
    from distributed_lms_raft_llm_amd.engine.mode import sampling_unsupported
    from distributed_lms_raft_llm_amd.tutor import server

    def no_engine(*a, **kw):
        raise AssertionError("an engine was built")

    monkeypatch.setattr(server, "make_engine", no_engine)
    for extra, why in ((["--tp", "2"], sampling_unsupported(2, False)),
                       (["--weight-dtype", "fp8"], sampling_unsupported(1, True))):
        with pytest.raises(SystemExit) as e:
            server.main(["--best-of", "4"] + extra)
        assert e.value.code == 2 and why in " ".join(capsys.readouterr().err.split())
    with pytest.raises(SystemExit) as e:
        server.main(["--best-of", "4", "--max-batch", "2"])
    assert e.value.code == 2


def test_window_batcher_serves_the_best_of_n():
    from distributed_lms_raft_llm_amd.tutor.server import Batcher, generation_config

    cfg, w = _tiny()
    eng = TorchGPT2Engine(cfg, w, max_length=24)
    gen = generation_config(24, bc.PEN, SP, None, True)
    with pytest.raises(ValueError):
        Batcher(eng, generation_config(24, bc.PEN, None, None, True), best_of=3)
    b = Batcher(eng, gen, max_batch=4, window_ms=1.0, best_of=3)
    try:
        toks, lps = b.submit(PROMPTS[0]).result(60)
    finally:
        b.stop()
    group_t, group_l = eng.generate(PROMPTS[:1], repetition_penalty=bc.PEN, sampling=SP, logprobs=True, n=3)
    best = pick_best(group_l[0])
    assert (toks, lps) == (group_t[0][best], group_l[0][best])
    assert b.gain.answers == 1 and b.gain.mean >= 0


@pytest.mark.parametrize("batching", ["window", "continuous"])
def test_tutoring_server_answers_once_per_query_and_reports_the_gain(batching):
    from distributed_lms_raft_llm_amd import wire
    from distributed_lms_raft_llm_amd.tokenizer import GPT2BPE
    from distributed_lms_raft_llm_amd.tutor.server import TutoringServer, build_prompt
    from distributed_lms_raft_llm_amd.wire import pb

    if batching == "window":
        cfg, w = _tiny()
        eng, T = TorchGPT2Engine(cfg, w, max_length=112), 112  # (the wrapped prompt is 95 byte-level tokens)
    else:
        eng, T = FakeGroupEngine(max_batch=4, max_length=112), 112
    with pytest.raises(ValueError, match="sampling"):
        TutoringServer(eng, port=0, host="127.0.0.1", max_length=T, batching=batching, best_of=3)
    srv = TutoringServer(eng, port=0, host="127.0.0.1", max_length=T, window_ms=1, batching=batching, chunk=2,
                         tokenizer=GPT2BPE(eos_token_id=eng.cfg.eos_token_id), sampling=SP, best_of=3).start()
    try:
        assert srv.gen.logprobs and srv.best_of == 3
        stub = wire.Stub("Tutoring", wire.channel(f"127.0.0.1:{srv.port}"))
        r = stub.GetLLMAnswer(pb.QueryRequest(token="t", query="hi"), timeout=60)
        assert r.success and r.response.startswith(build_prompt("hi"))
        h = srv._health()
        assert h["best_of"] == 3 and isinstance(h["best_of_gain"], float) and h["best_of_gain"] >= 0
        assert h["mean_token_logprob"] is not None
    finally:
        srv.stop()
    if batching == "continuous":
        assert [kw.get("n") for _, kw, _ in eng.admissions] == [3]
