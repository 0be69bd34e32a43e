"""Continuous (in-flight) batching scheduler for the tutoring decode engine.

The reference serves one ``model.generate`` per request (SURVEY.md §3.3,
reference ``tutoring_server.py``: GetLLMAnswer -> tokenizer -> generate(max_length=150)),
so concurrent students queue behind each other.  Here one scheduler thread owns the engine's
KV-cache slots: a request is prefilled into the lowest free slot as soon as one exists (packed
varlen prefill, ``HipGPT2Engine.admit``), every live sequence advances together in graph-replayed
decode chunks over the smallest batch bucket covering the occupied slots, and a finished
sequence frees its slot at the next chunk boundary -- so a late request never waits for an
earlier batch to drain.

The loop is PIPELINED one chunk deep: chunk k+1 is enqueued before the host reads chunk k's stop
flags (a pinned copy behind chunk k, ``flags_async``), and finished sequences are gathered by a
copy enqueued behind chunk k+1 (``collect_async``: a finished row never changes), so the GPU
always has the next chunk queued while the host retires requests and prepares admissions (the
admission's host->device copies go through pinned memory and never block on the stream).  A
finished slot is reusable at once: its re-admission is stream-ordered behind the gather.

Engine protocol (``HipGPT2Engine`` implements it; tests use a CPU fake):
    max_batch, max_length, cfg.eos_token_id
    admit(prompts, slots, repetition_penalty)   prefill + first token into those slots
    decode(B, steps, repetition_penalty)        ``steps`` decode steps over slots [0, B)
                                                (both with ``sampling=`` when the batcher samples and
                                                ``controls=`` when it has generation controls,
                                                ``logprobs=True`` when it returns log-probabilities;
                                                ``admit`` alone with ``n=n`` when the batcher serves
                                                n > 1 completions per request: n slots per prompt)
    finished_flags(B) -> list[int]              per-slot stop flags
    collect(slots) -> list[list[int]]           prompt + generated tokens (``logprobs=True``, only
                                                then passed: ``(tokens, logprobs)``)
    flags_async(B), collect_async(slots)        optional: the same as handles with .result()
"""
from __future__ import annotations

import heapq
import math
import os
import threading
import time
from collections import deque
from concurrent.futures import Future
from dataclasses import dataclass, field

import torch

from ..utils.metrics import METRICS
from ..utils.trace import TRACER, roctx_range
from .gpt2_engine import _bucket


class _Ready:
    def __init__(self, value):
        self.value = value

    def result(self):
        return self.value


def flags_async(eng, B: int):
    f = getattr(eng, "flags_async", None)
    return f(B) if f is not None else _Ready(eng.finished_flags(B))


def health_async(eng):
    f = getattr(eng, "health_async", None)
    return f() if f is not None else None


def dataflow_status_async(eng):
    f = getattr(eng, "dataflow_status_async", None)
    return f() if f is not None else None


class PeerStalled(RuntimeError):
    """A tensor-parallel peer never reached a collective: the affected chunk's tokens are garbage."""


def collect_async(eng, slots: list[int], **mode):
    f = getattr(eng, "collect_async", None)
    return f(slots, **mode) if f is not None else _Ready(eng.collect(slots, **mode))


@dataclass
class _Req:
    prompt: list[int]
    future: Future
    t_submit: float = field(default_factory=time.perf_counter)
    t_first: float = 0.0
    steps_left: int = 0  # decode steps until max_length (an upper bound: EOS may come first)
    slots: tuple = ()  # the KV slots it holds once admitted: one, or its n completions' (parent first)


class Overloaded(RuntimeError):
    """``submit`` refused a query: the admission queue already holds ``max_queue`` queries (the
    servers answer RESOURCE_EXHAUSTED at once, so an overloaded replica sheds load in
    microseconds instead of queueing queries until their client deadlines expire)."""


SELECTORS = ("mean_logprob",)


def pick_best(logprob_lists) -> int:
    """Best of n by mean log-probability: the index of the list with the largest arithmetic mean.
    The lists are judged as the engine returned them, EOS and stop tokens included.  Ties go to the
    lowest index.  An empty list (nothing was generated) ranks below every non-empty list that can
    be judged; a list with a NaN in it cannot be judged and ranks below every list without one, the
    empty ones included."""
    best, best_key = 0, None
    for i, lp in enumerate(logprob_lists):
        lp = [float(v) for v in lp]
        if any(math.isnan(v) for v in lp):
            key = (0, 0.0)
        elif not lp:
            key = (1, 0.0)
        else:
            key = (2, math.fsum(lp) / len(lp))
        if best_key is None or key > best_key:
            best, best_key = i, key
    if best_key is None:
        raise ValueError("pick_best: no candidates")
    return best


class GainMeter:
    """What best of n bought: the running mean, over the answered requests, of the chosen
    completion's mean log-probability minus the average of the means over its group (the lists
    that can be judged: non-empty, no NaN).  A request whose chosen list cannot be judged is not
    counted."""

    def __init__(self):
        self._lock = threading.Lock()
        self.answers = 0
        self._sum = 0.0

    def add(self, logprob_lists, chosen: int):
        means = [math.fsum(lp) / len(lp) if len(lp) and not any(math.isnan(v) for v in lp) else None
                 for lp in logprob_lists]
        if means[chosen] is None:
            return
        judged = [m for m in means if m is not None]
        with self._lock:
            self.answers += 1
            self._sum += means[chosen] - math.fsum(judged) / len(judged)

    @property
    def mean(self) -> float | None:
        with self._lock:
            return self._sum / self.answers if self.answers else None


class ContinuousBatcher:
    def __init__(self, engine, repetition_penalty: float = 1.2, chunk: int = 8, max_admit: int | None = None,
                 name: str = "tutor", stream_priority: int | None = None, max_queue: int = 0, sampling=None,
                 controls=None, logprobs: bool = False, n: int = 1, select: str | None = None):
        """``max_queue``: queries allowed to wait for a free KV slot before ``submit`` raises
        ``Overloaded`` (0 = unbounded; the tutoring servers default to one batch of slots).
        ``sampling`` (a ``SamplingParams``): tokens are drawn instead of greedy; it is forwarded to
        the engine's ``admit`` / ``decode`` as ``sampling=`` -- only when set, so greedy engines are
        called exactly as before.  ``controls`` (a ``GenerationControls``): n-gram blocking, a minimum
        length and stop sequences, forwarded the same way as ``controls=`` (results keep their stop
        tokens, as they keep EOS).  ``logprobs``: every future resolves to ``(tokens, logprobs)``,
        one float per generated token; forwarded as ``logprobs=True`` the same way, to ``collect`` /
        ``collect_async`` too.
        ``n`` > 1: n completions per request from one prefill.  A request takes n slots at admission
        (it waits, at the head of the queue, until n are free; the engine's ``admit`` gets ``n=n`` --
        only then, so engines without the argument are called exactly as before) and retires as a
        group: when all n slots are flagged finished they are collected in one ``collect_async`` and
        freed together.  A sibling that finishes early idles as an inert row until then; freeing it
        early is not done.  ``{name}_tokens`` counts every completion's tokens, ``{name}_request_ms``
        requests.  ``select=None``: the future resolves to the list of the n results (each ``tokens`` or
        ``(tokens, logprobs)``); ``select="mean_logprob"`` (needs ``logprobs=True``): to the one result
        ``pick_best`` chooses."""
        if isinstance(n, bool) or not isinstance(n, int) or n < 1:
            raise ValueError(f"n: a positive integer, got {n!r}")
        if n > engine.max_batch:
            raise ValueError(f"n = {n} completions per request do not fit the engine's {engine.max_batch} slots")
        if select is not None and select not in SELECTORS:
            raise ValueError(f"select: None or one of {SELECTORS}, got {select!r}")
        if select is not None and not logprobs:
            raise ValueError(f"select={select!r} needs logprobs=True")
        self.n = n
        self.select = select
        self._admit_n = {"n": n} if n > 1 else {}
        self.gain = GainMeter()  # (select set: chosen mean log-probability over its group's average)
        self.engine = engine
        self.sampling = sampling
        self.controls = controls
        self._mode = {} if sampling is None else {"sampling": sampling}
        if controls is not None:
            self._mode["controls"] = controls
        self.logprobs = bool(logprobs)
        self._collect_mode = {"logprobs": True} if self.logprobs else {}
        self._mode.update(self._collect_mode)
        self.max_queue = int(max_queue or 0)
        self.rejected = 0
        env_prio = os.environ.get("DLMS_BATCHER_STREAM_PRIORITY")
        self.stream_priority = int(env_prio) if env_prio else stream_priority
        self.penalty = float(repetition_penalty)
        self.chunk = max(1, int(chunk))
        self.max_admit = max_admit or engine.max_batch
        self.name = name
        self._queue: deque[_Req] = deque()
        self._cv = threading.Condition()
        self._free = list(range(engine.max_batch))
        heapq.heapify(self._free)
        self._active: dict[int, _Req] = {}
        self._stop = False
        self._error: BaseException | None = None
        self.steps = 0
        self.completed = 0
        # side work run on this thread between decode chunks (gate/service.py GateWorker: the relevance
        # gate's encoder passes go on the decode stream right behind a chunk, never interleaved
        # kernel by kernel with it): work(idle) is called once per loop iteration, pending() says
        # whether it has anything queued or in flight (so an idle batcher does not sleep on it)
        self._side_work = None
        self._side_pending = None
        self._thread = threading.Thread(target=self._run, name=f"{name}-batcher", daemon=True)
        self._thread.start()

    def attach_side_work(self, work, pending):
        with self._cv:
            self._side_work, self._side_pending = work, pending
            self._cv.notify()

    def kick(self):
        """Wake the scheduler thread (new side work arrived)."""
        with self._cv:
            self._cv.notify()

    # ------------------------------------------------------------------ client side
    def submit(self, prompt: list[int]) -> Future:
        fut: Future = Future()
        eos, T = self.engine.cfg.eos_token_id, self.engine.max_length
        p = list(prompt) if len(prompt) else [eos]
        if len(p) >= T:  # nothing to generate (generate() pass-through semantics)
            fut.set_result(self._resolve([(p, []) if self.logprobs else p for _ in range(self.n)]))
            return fut
        with self._cv:
            if self._stop:
                raise RuntimeError("batcher stopped")
            if self._error is not None:
                raise RuntimeError("batcher failed") from self._error
            if self.max_queue and len(self._queue) >= self.max_queue:
                self.rejected += 1
                METRICS.inc(f"{self.name}_rejected_total")
                raise Overloaded(f"{len(self._queue)} queries already waiting for a KV slot")
            self._queue.append(_Req(p, fut))
            self._cv.notify()
        return fut

    def _resolve(self, items: list):
        """What a future resolves to, from its request's n results."""
        if self.select is not None:
            lps = [lp for _, lp in items]
            best = pick_best(lps)
            self.gain.add(lps, best)
            return items[best]
        return items[0] if self.n == 1 else items

    @property
    def failed(self) -> BaseException | None:
        """The error that stopped the batcher (None while it serves)."""
        return self._error

    def generate(self, prompts: list[list[int]], timeout: float | None = None) -> list[list[int]]:
        futs = [self.submit(p) for p in prompts]
        return [f.result(timeout) for f in futs]

    def stop(self, timeout: float = 10.0):
        with self._cv:
            self._stop = True
            self._cv.notify()
        self._thread.join(timeout)

    @property
    def active(self) -> int:
        """Occupied KV slots (n per live request)."""
        return len(self._active)

    # ------------------------------------------------------------------ scheduler thread
    def _run(self):
        try:
            dev = getattr(self.engine, "device", None)
            if dev is not None and getattr(dev, "type", None) == "cuda" and dev.index is not None:
                torch.cuda.set_device(dev)
            if self.stream_priority is not None and dev is not None and getattr(dev, "type", None) == "cuda":
                # serving beside other GPU processes on the same device (the LMS nodes' relevance
                # gates): the decode chunks go on a stream of this priority (lower = higher; the
                # graphs are replayed on it).  LMS path at 3.5 k q/s, 3 Raft nodes + BERT gates:
                # p50 863 -> 614 ms, p99 1189 -> 927, same tok/s (profiles/r4_serving_grpc.jsonl)
                torch.cuda.set_stream(torch.cuda.Stream(device=dev, priority=int(self.stream_priority)))
            with torch.no_grad():
                self._loop()
        except BaseException as e:  # fail every waiter loudly instead of hanging them
            # (the engine's device state is suspect after this -- e.g. a PeerStalled chunk left
            # garbage in the KV cache and the xGMI error word set -- so the batcher does not try
            # to continue: callers see `failed`, and the serving process exits for its supervisor
            # to restart it fresh; tutor/server.py)
            with self._cv:
                self._error = e
                waiters = list(self._active.values()) + list(self._queue)
                self._active.clear()
                self._queue.clear()
            for r in waiters:
                if not r.future.done():
                    r.future.set_exception(e)

    def _loop(self):
        eng = self.engine
        prev = None  # (flags handle, {slot: request} live when that chunk was enqueued) of the last chunk
        retiring = None  # (requests, collect handle) of sequences found finished
        while True:
            with self._cv:
                while not self._stop and not self._queue and not self._active and prev is None and retiring is None \
                        and not (self._side_pending is not None and self._side_pending()):
                    self._cv.wait()
                if self._stop:
                    waiters = list(self._queue) + list(self._active.values()) + \
                        ([r for _, r in retiring[0]] if retiring else [])
                    self._queue.clear()
                    self._active.clear()
                    for r in waiters:
                        if not r.future.done():
                            r.future.set_exception(RuntimeError("batcher stopped"))
                    return
                admits: list[tuple[int, _Req]] = []  # (first slot, request)
                while self._queue and len(self._free) >= self.n and len(admits) < self.max_admit:
                    r = self._queue.popleft()
                    # RUNNING from here on: a caller's cancel() (a gRPC deadline, asyncio.wait_for
                    # timing out on a wrap_future) can no longer race the result; a request
                    # cancelled while it queued is dropped
                    if r.future.set_running_or_notify_cancel():
                        r.slots = tuple(heapq.heappop(self._free) for _ in range(self.n))
                        admits.append((r.slots[0], r))
            if admits:
                ta = time.perf_counter()
                with roctx_range("prefill"):
                    eng.admit([r.prompt for _, r in admits], [s for _, r in admits for s in r.slots], self.penalty,
                              **self._mode, **self._admit_n)
                TRACER.complete("tutor.admit", ta, cat="tutor", n=len(admits),
                                tokens=sum(len(r.prompt) for _, r in admits))
                t_first = time.perf_counter()  # prefill (first token included) is enqueued
                for _, r in admits:
                    for s in r.slots:
                        self._active[s] = r
                    r.t_first = t_first
                    r.steps_left = max(0, eng.max_length - len(r.prompt) - 1)  # prefill made token 1
                    METRICS.observe(f"{self.name}_queue_ms", (ta - r.t_submit) * 1e3)
                    METRICS.observe(f"{self.name}_ttft_ms", (t_first - r.t_submit) * 1e3)
            cur = None
            # never decode far past the point where every live sequence has hit max_length: the last
            # chunk is cut to the longest remaining budget, and once every budget is spent only a
            # single step runs while the in-flight flags retire them (one step, not a whole no-op
            # chunk, on every query's latency at low load; at least one step keeps the loop making
            # progress even if a sequence's flag were late)
            steps = 0
            if self._active:
                steps = max(1, min(self.chunk, max(r.steps_left for r in self._active.values())))
            if steps > 0:
                B = min(_bucket(max(self._active) + 1), eng.max_batch)
                td = time.perf_counter()
                # the budget each live request actually gives up to this chunk (a request near its
                # max_length gives less than `steps`): an aborted chunk refunds exactly that
                taken = {}
                for s, r in self._active.items():
                    if s == r.slots[0]:  # once per request, under its first slot
                        taken[s] = min(steps, r.steps_left)
                        r.steps_left -= taken[s]
                with roctx_range("decode_chunk"):
                    eng.decode(B, steps, self.penalty, **self._mode)
                    cur = (flags_async(eng, B), dict(self._active), health_async(eng), dataflow_status_async(eng),
                           taken)
                self.steps += steps
                TRACER.complete("tutor.decode_chunk", td, cat="tutor", bucket=B, live=len(self._active),
                                steps=steps)
            if self._side_work is not None:  # behind the chunk just enqueued, before the next one
                self._side_work(cur is None and prev is None)
            if retiring is not None:  # gathered behind the chunk before `cur`: ready or nearly
                self._retire(*retiring)
                retiring = None
            if prev is not None:  # chunk k's flags while chunk k+1 runs
                flags = prev[0].result()
                if prev[2] is not None and prev[2].result():
                    # fail every live request (the _run handler) rather than return wrong tokens
                    METRICS.inc(f"{self.name}_peer_stalls")
                    raise PeerStalled("a tensor-parallel peer timed out in an xGMI collective")
                if prev[3] is not None and prev[3].result():
                    # the persistent dataflow kernel aborted that chunk before committing anything:
                    # no row advanced (the engine serves launch-per-op for a while); give the
                    # requests their step budget back so later chunks are not cut short
                    METRICS.inc(f"{self.name}_dataflow_aborts")
                    for s, r in prev[1].items():
                        if s == r.slots[0] and self._active.get(s) is r:
                            r.steps_left += prev[4].get(s, 0)
                # by identity: a slot retired one chunk earlier may already hold a new request
                # (a request is done when every one of its slots is flagged)
                reqs = [(s, r) for s, r in prev[1].items() if s == r.slots[0] and self._active.get(s) is r
                        and all(t < len(flags) and flags[t] for t in r.slots)]
                if reqs:
                    done = [t for _, r in reqs for t in r.slots]
                    handle = collect_async(eng, done, **self._collect_mode)
                    with self._cv:
                        for s in done:
                            del self._active[s]
                            heapq.heappush(self._free, s)
                    retiring = (reqs, handle)
                    METRICS.set(f"{self.name}_active", len(self._active))
                    METRICS.set(f"{self.name}_kv_slot_occupancy", len(self._active) / eng.max_batch)
            prev = cur

    def _retire(self, reqs, handle):
        outs = handle.result()
        lps = None
        if self.logprobs:
            outs, lps = outs
        now = time.perf_counter()
        n = self.n
        for i, (s, r) in enumerate(reqs):
            group = outs[i * n: (i + 1) * n]  # the request's n completions, in slot (= stream) order
            self.completed += 1
            new = [len(out) - len(r.prompt) for out in group]
            METRICS.observe(f"{self.name}_request_ms", (now - r.t_submit) * 1e3)
            if max(new) > 1:  # time per output token after the first (of the longest completion)
                METRICS.observe(f"{self.name}_tpot_ms", (now - r.t_first) * 1e3 / (max(new) - 1))
            METRICS.inc(f"{self.name}_tokens", sum(new))
            if not r.future.done():
                r.future.set_result(self._resolve(group if lps is None else
                                                  list(zip(group, lps[i * n: (i + 1) * n]))))
