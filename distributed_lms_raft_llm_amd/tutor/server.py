"""Tutoring service (``lms.Tutoring.GetLLMAnswer``) backed by the MI355X GPT-2 engine.

Reference behaviour (``tutoring_server.py:15-49``): wrap the query in a fixed prompt, run GPT-2
``generate(max_length=150, repetition_penalty=1.2)`` (greedy), return the decoded sequence -- prompt
included -- with ``success=True``; listen on ``[::]:50054`` with 10 worker threads.

Here concurrent queries are batched.  On the GPU engine the default is continuous batching
(``engine/scheduler.py``): a query is prefilled into a free KV-cache slot of the running batch as
soon as it arrives and leaves at its own EOS/max_length, every live query advancing in
hipGraph-replayed decode chunks.  The window batcher (``--batching window``, and the only mode of
the CPU torch reference engine, BASELINE config 1) collects requests for up to
``batch_window_ms`` (or until ``max_batch``) and runs them as one batched ``generate``.
Per-request latency, batch sizes and tokens/s land in the metrics registry.
"""
from __future__ import annotations

import argparse
import dataclasses
import logging
import os
import queue
import signal
import threading
import time
from concurrent import futures
from dataclasses import dataclass

import grpc
import torch

from .. import wire
from ..engine.scheduler import Overloaded
from ..models.config import (CONTROLS_MAX_STOP, CONTROLS_MAX_STOP_LEN, GenerationConfig, GenerationControls,
                             SamplingParams, gpt2_config)
from ..models.gpt2 import init_gpt2_weights, load_safetensors_weights
from ..tokenizer import GPT2BPE
from ..utils.config import parse_with_config
from ..utils.debug_rpc import debug_handler
from ..utils.metrics import METRICS
from ..wire import pb

log = logging.getLogger("dlms.tutor")

PROMPT_TEMPLATE = ("You are an intelligent assistant. Answer the following question in detail:\n"
                   "Question: {query}\nAnswer:")


def default_max_queue(engine, max_queue: int | None) -> int:
    """Admission limit of a serving replica: queries that may wait for a KV slot beyond the
    engine's slots (one batch of slots by default -- about one generation of queueing delay)
    before it answers RESOURCE_EXHAUSTED; 0 = unbounded."""
    return engine.max_batch if max_queue is None else int(max_queue)


def build_prompt(query: str) -> str:
    return PROMPT_TEMPLATE.format(query=query)


# --prefix-cache on: queries whose wrapped prompts are encoded to find the tokens every prompt starts
# with (different first characters, a digit, a lower-case word: the template's last shared token must
# not depend on how the query begins)
PREFIX_PROBES = ("What is a binary search tree?", "explain how Raft elects a leader", "2 + 2 = ?",
                 "Why is the sky blue?", "describe photosynthesis", "Is P equal to NP?")
PREFIX_CAPACITY = 64  # rows of the engine's prefix store (the template shares 16 tokens)


def prefix_candidate(tok, probes=PREFIX_PROBES) -> list[int]:
    """The longest common token prefix of ``build_prompt(q)`` over the probe queries: the prompt
    prefix a server sets on its engine.  The engine still matches per request, so a query whose
    tokenisation diverges earlier only loses the saving."""
    enc = [tok.encode(build_prompt(q)) for q in probes]
    n = 0
    while all(len(e) > n for e in enc) and len({e[n] for e in enc}) == 1:
        n += 1
    return enc[0][:n]


def enable_prefix_cache(engine, tok, max_len: int | None = None) -> list[int]:
    """Set the template's shared tokens as ``engine``'s prompt prefix (at most ``max_len`` of them,
    default what the engine takes) and return them; ``ValueError`` for an engine without a prefix
    store or a tokenizer that shares no leading token."""
    if not getattr(engine, "prefix_capacity", 0) or not hasattr(engine, "set_prompt_prefix"):
        raise ValueError("--prefix-cache on needs the GPU engine built with a prefix store (one GPU, bf16 weights)")
    cap = min(engine.prefix_capacity, engine.max_length - 2)
    prefix = prefix_candidate(tok)[: cap if max_len is None else min(cap, max_len)]
    if not prefix:
        raise ValueError("--prefix-cache on: the probe prompts share no leading token")
    engine.set_prompt_prefix(prefix)
    return prefix


@dataclass
class _Req:
    ids: list[int]
    fut: futures.Future
    t0: float


class Batcher:
    """Dynamic batching in front of an engine with ``generate(prompts, max_length, penalty)``."""

    def __init__(self, engine, gen: GenerationConfig, max_batch: int = 64, window_ms: float = 2.0, best_of: int = 1):
        """``best_of`` > 1 (a sampling ``gen`` with ``logprobs``): every batch runs as
        ``generate(..., n=best_of)`` and each query resolves to the completion ``pick_best`` chooses."""
        from ..engine.scheduler import GainMeter

        if best_of > 1 and not (gen.logprobs and gen.sampling() is not None):
            raise ValueError("best_of > 1 needs a sampling GenerationConfig with logprobs")
        self.best_of = best_of
        self.gain = GainMeter()
        self.engine = engine
        self.gen = gen
        self.batches = 0  # sampling: batch i draws under seed + i (a run is reproducible, its batches differ)
        self.max_batch = max_batch
        self.window = window_ms / 1e3
        self.q: queue.Queue = queue.Queue()
        self._stop = threading.Event()
        self._t = threading.Thread(target=self._loop, name="tutor-batcher", daemon=True)
        self._t.start()

    def submit(self, ids: list[int]) -> futures.Future:
        f: futures.Future = futures.Future()
        self.q.put(_Req(ids, f, time.perf_counter()))
        METRICS.set("tutor_queue_depth", self.q.qsize())
        return f

    def _loop(self):
        while not self._stop.is_set():
            try:
                first = self.q.get(timeout=0.1)
            except queue.Empty:
                continue
            batch = [first]
            deadline = time.perf_counter() + self.window
            while len(batch) < self.max_batch:
                rem = deadline - time.perf_counter()
                if rem <= 0:
                    break
                try:
                    batch.append(self.q.get(timeout=rem))
                except queue.Empty:
                    break
            self._run(batch)

    def _run(self, batch: list[_Req]):
        t0 = time.perf_counter()
        try:
            sp, ct = self.gen.sampling(), self.gen.controls()
            mode = {} if ct is None else {"controls": ct}  # (only when set: engines are called as before)
            if self.gen.logprobs:
                mode["logprobs"] = True
            if self.best_of > 1:  # (only then: engines without the argument are called as before)
                mode["n"] = self.best_of
            if sp is None:
                outs = self.engine.generate([r.ids for r in batch], self.gen.max_length, self.gen.repetition_penalty,
                                            **mode)
            else:
                sp = dataclasses.replace(sp, seed=(sp.seed + self.batches) % 2 ** 64)
                self.batches += 1
                outs = self.engine.generate([r.ids for r in batch], self.gen.max_length, self.gen.repetition_penalty,
                                            sampling=sp, **mode)
        except Exception as e:  # fail the whole batch, keep serving
            log.exception("generation failed")
            for r in batch:
                r.fut.set_exception(e)
            return
        lps = None
        if self.gen.logprobs:
            outs, lps = outs
        dt = time.perf_counter() - t0
        if self.best_of > 1:  # one answer per query: the group's best; every completion's tokens are counted
            from ..engine.scheduler import pick_best

            new = sum(len(o) - len(r.ids) for g, r in zip(outs, batch) for o in g)
            best = [pick_best(g) for g in lps]
            for g, b in zip(lps, best):
                self.gain.add(g, b)
            outs, lps = [g[b] for g, b in zip(outs, best)], [g[b] for g, b in zip(lps, best)]
        else:
            new = sum(len(o) - len(r.ids) for o, r in zip(outs, batch))
        METRICS.observe("tutor_batch_size", len(batch))
        METRICS.observe("tutor_batch_ms", dt * 1e3)
        METRICS.inc("tutor_tokens_generated", new)
        METRICS.set("tutor_tokens_per_s", new / dt if dt > 0 else 0.0)
        now = time.perf_counter()
        for i, (o, r) in enumerate(zip(outs, batch)):
            METRICS.observe("tutor_query_ms", (now - r.t0) * 1e3)
            r.fut.set_result(o if lps is None else (o, lps[i]))

    def stop(self):
        self._stop.set()
        self._t.join(timeout=2)


def trim_stop(out: list[int], prompt_len: int, stop) -> tuple[list[int], bool]:
    """``out`` without the stop sequence its generated part ends with (the longest one, when one is a
    suffix of another), and whether there was one (``models.gpt2.stop_hit``'s rule)."""
    m = max((len(s) for s in stop if len(s) and len(out) - len(s) >= prompt_len and
             list(out[len(out) - len(s):]) == list(s)), default=0)
    return (list(out[: len(out) - m]), True) if m else (out, False)


class StopTrimmer:
    """A batcher whose results come back without the stop sequence that ended them (the servers
    drop it before detokenising) and which counts those results; everything else is the batcher's.
    A ``(tokens, logprobs)`` result (a batcher with ``logprobs=True``) loses the stop tokens'
    log-probabilities with the tokens."""

    def __init__(self, batcher, stop):
        self._batcher = batcher
        self._stop_seqs = tuple(stop)
        self.stopped_by_sequence = 0

    def submit(self, ids: list[int]) -> futures.Future:
        inner = self._batcher.submit(ids)
        fut: futures.Future = futures.Future()
        n = max(1, len(ids))  # (an empty prompt is served as one EOS token)

        def done(f):
            try:
                res = f.result()
                if isinstance(res, tuple):
                    toks, lps = res
                    out, hit = trim_stop(toks, n, self._stop_seqs)
                    out = (out, list(lps[: len(lps) - (len(toks) - len(out))]))
                else:
                    out, hit = trim_stop(res, n, self._stop_seqs)
            except BaseException as e:
                fut.set_exception(e)
                return
            self.stopped_by_sequence += hit
            fut.set_result(out)

        inner.add_done_callback(done)
        return fut

    def __getattr__(self, name):
        return getattr(self._batcher, name)


class LogprobMeter:
    """In front of a batcher whose results are ``(tokens, logprobs)``: hands on the tokens alone (the
    answers and the wire format are those of a server without ``--logprobs``) and keeps the running
    mean, over the answered queries, of an answer's mean token log-probability; with ``threshold``
    also the count of answers whose mean lies below it.  Everything else is the batcher's."""

    def __init__(self, batcher, threshold: float | None = None):
        self._batcher = batcher
        self.threshold = threshold
        self._lock = threading.Lock()
        self.answers = 0
        self._sum = 0.0
        self.low_confidence_answers = 0

    @property
    def mean_token_logprob(self) -> float | None:
        with self._lock:
            return self._sum / self.answers if self.answers else None

    def submit(self, ids: list[int]) -> futures.Future:
        inner = self._batcher.submit(ids)
        fut: futures.Future = futures.Future()

        def done(f):
            try:
                toks, lps = f.result()
            except BaseException as e:
                fut.set_exception(e)
                return
            if lps:  # (an answer of no tokens has no mean)
                mean = sum(lps) / len(lps)
                with self._lock:
                    self.answers += 1
                    self._sum += mean
                    if self.threshold is not None and mean < self.threshold:
                        self.low_confidence_answers += 1
            fut.set_result(toks)

        inner.add_done_callback(done)
        return fut

    def __getattr__(self, name):
        return getattr(self._batcher, name)


def front_batcher(batcher, controls, logprobs: bool = False, min_mean_logprob: float | None = None):
    """What the servicers submit to: ``batcher``, behind a ``StopTrimmer`` when ``controls`` has stops,
    and a ``LogprobMeter`` when it returns log-probabilities."""
    front = StopTrimmer(batcher, controls.stop) if controls is not None and controls.stop else batcher
    return LogprobMeter(front, min_mean_logprob) if logprobs else front


class TutoringServicer:
    def __init__(self, batcher: Batcher, tokenizer: GPT2BPE, max_length: int, timeout: float = 300.0):
        self.batcher = batcher
        self.tok = tokenizer
        self.max_length = max_length
        self.timeout = timeout

    def GetLLMAnswer(self, request, context):
        # like generate(), a prompt already at max_length comes back unchanged (engines handle it)
        ids = self.tok.encode(build_prompt(request.query))
        try:
            out = self.batcher.submit(ids).result(timeout=self.timeout)
        except Overloaded as e:  # shed load now rather than queue past the client's deadline
            context.abort(grpc.StatusCode.RESOURCE_EXHAUSTED, str(e))
        except Exception as e:
            # a failed batcher (e.g. a tensor-parallel peer stalled in an xGMI collective) will not
            # serve again in this process: UNAVAILABLE makes the LMS's TutoringClient fail over to
            # a healthy replica (INTERNAL is not retried), and TutoringServer exits this process
            # for its supervisor to restart
            failed = getattr(self.batcher, "failed", None) is not None
            code = grpc.StatusCode.UNAVAILABLE if failed else grpc.StatusCode.INTERNAL
            context.abort(code, f"generation failed: {e}")
        return pb.QueryResponse(success=True, response=self.tok.decode(out, skip_special_tokens=True))


def make_engine(model: str, device: str, max_batch: int, max_length: int, weights: str | None = None, seed: int = 0,
                tp_group=None, weight_dtype: str = "bf16", kv_dtype: str = "bf16", latency_path: bool | None = None,
                prefix_capacity: int = 0):
    """GPU: the HIP engine (TP over ``tp_group`` when given).  CPU: the torch reference engine, or
    the sharded torch slot engine when a (gloo) TP group is given.  ``kv_dtype="fp8"``: the e4m3 KV
    cache (HIP engine) or its reference model (torch engine); not with a TP group.  ``latency_path``
    goes to the HIP engine as it is (None: its default; True also turns the low-batch paths on over
    an fp8 cache); the torch engines have no such paths and ignore it.  ``prefix_capacity > 0``: the
    HIP engine's prompt-prefix store (``set_prompt_prefix``); the torch engines have none
    (``ValueError``), nor has a TP group."""
    if prefix_capacity:
        from ..engine.gpt2_engine import prefix_unsupported

        why = prefix_unsupported(2 if tp_group is not None else 1, weight_dtype == "fp8")
        if why:
            raise ValueError(why)
    if kv_dtype == "fp8" and tp_group is not None:
        from ..engine.gpt2_engine import kv_fp8_unsupported

        raise ValueError(kv_fp8_unsupported(2, weight_dtype == "fp8"))
    cfg = gpt2_config(model)
    w = load_safetensors_weights(weights) if weights else init_gpt2_weights(cfg, seed=seed)
    if device == "auto":
        device = "cuda" if torch.cuda.is_available() else "cpu"
    if device.startswith("cuda"):
        from ..engine.gpt2_engine import HipGPT2Engine

        return HipGPT2Engine(cfg, w, device=device, max_batch=max_batch, max_length=max_length, tp_group=tp_group,
                             weight_dtype=weight_dtype, kv_dtype=kv_dtype, latency_path=latency_path,
                             prefix_capacity=prefix_capacity)
    if prefix_capacity:
        raise ValueError("the prompt-prefix cache needs the GPU engine (device cuda)")
    if tp_group is not None:
        from ..parallel.tp import TorchSlotEngine

        return TorchSlotEngine(cfg, w, group=tp_group, max_batch=max_batch or 8, max_length=max_length)
    from ..engine.gpt2_engine import TorchGPT2Engine

    return TorchGPT2Engine(cfg, w, max_length=max_length, kv_dtype=kv_dtype)


def make_gate_worker(model: str, weights: str | None, device):
    """The relevance gate's encoder for ``--serve-gate`` (gate/service.py GateWorker): the HIP BERT
    on the tutor's GPU (its graphs captured now), or the torch reference on a CPU engine."""
    import torch

    from ..gate.service import GateWorker
    from ..models.bert import BertReference, init_bert_weights, load_bert_safetensors
    from ..models.config import bert_config

    cfg = bert_config(model)
    w = load_bert_safetensors(weights) if weights else init_bert_weights(cfg, seed=0)
    if str(device).startswith("cuda") and torch.cuda.is_available():
        from ..engine.bert_engine import HipBertEncoder

        enc = HipBertEncoder(cfg, w, device=device, graph_max_rows=8192, graph_max_seqs=256)
        enc.warm_graphs()
    else:
        enc = BertReference(cfg, w, device="cpu")
    log.info("relevance gate served on the tutoring port (%s on %s, passes between decode chunks)", model, device)
    # under load at most one pass per DLMS_GATE_MIN_GAP_MS (fuller passes, fewer stops of the decode
    # stream); idle, a query is scored at the next batcher iteration
    return GateWorker(enc, max_seqs=255 if str(device).startswith("cuda") else 127,
                      min_gap_s=float(os.environ.get("DLMS_GATE_MIN_GAP_MS", "10")) / 1e3)


class TutoringServer:
    def __init__(self, engine, port: int = 50054, host: str = "[::]", max_batch: int = 64, window_ms: float = 2.0,
                 max_length: int = 150, repetition_penalty: float = 1.2, tokenizer: GPT2BPE | None = None,
                 workers: int = 64, batching: str = "auto", chunk: int = 8, max_queue: int | None = None,
                 sampling=None, controls=None, logprobs: bool = False, min_mean_logprob: float | None = None,
                 best_of: int = 1):
        """``sampling`` (a ``SamplingParams``, every server class): answers are sampled, not greedy.
        ``controls`` (a ``GenerationControls``, every server class): n-gram blocking, a minimum length
        and stop sequences; a matched stop sequence is dropped from the answer.  ``logprobs`` (every
        server class): the engine returns the tokens' log-probabilities and the health record gains
        ``mean_token_logprob``; ``min_mean_logprob`` (implies it): also ``low_confidence_answers``.
        The answers are unchanged.  ``best_of`` > 1 (every server class; needs ``sampling``, implies
        ``logprobs``): every query runs as ``best_of`` sampled completions of one prefill and is answered
        with the one of the highest mean token log-probability (``engine/scheduler.py pick_best``); the
        health record gains ``best_of`` and ``best_of_gain``, and the log-probability fields describe
        the chosen answers."""
        logprobs = self._init_best_of(best_of, sampling, logprobs, min_mean_logprob)
        self.gen = generation_config(max_length, repetition_penalty, sampling, controls, logprobs)
        self.controls = controls
        self.tok = tokenizer or GPT2BPE(eos_token_id=getattr(getattr(engine, "cfg", None), "eos_token_id", 50256))
        if batching == "auto":
            batching = "continuous" if hasattr(engine, "admit") else "window"
        if batching == "continuous":
            from ..engine.scheduler import ContinuousBatcher

            if engine.max_length != max_length:
                raise ValueError("continuous batching: engine max_length differs from the server's")
            self.batcher = ContinuousBatcher(engine, repetition_penalty, chunk=chunk,
                                             max_queue=default_max_queue(engine, max_queue), sampling=sampling,
                                             **_controls_kw(controls), **_logprobs_kw(logprobs),
                                             **_best_of_kw(best_of))
        else:
            self.batcher = Batcher(engine, self.gen, max_batch=max_batch, window_ms=window_ms, best_of=best_of)
        self.batching = batching
        self.server = grpc.server(futures.ThreadPoolExecutor(max_workers=workers),
                                  options=[("grpc.max_send_message_length", wire.DEFAULT_MAX_MESSAGE),
                                           ("grpc.max_receive_message_length", wire.DEFAULT_MAX_MESSAGE)])
        self.front = front_batcher(self.batcher, controls, logprobs, min_mean_logprob)
        wire.register(self.server, "Tutoring", TutoringServicer(self.front, self.tok, max_length))
        self.engine = engine
        self._stopping = threading.Event()
        self.server.add_generic_rpc_handlers((debug_handler(health=self._health),))
        self.port = self.server.add_insecure_port(f"{host}:{port}")
        if self.port == 0:
            raise RuntimeError(f"could not bind {host}:{port}")

    def _init_best_of(self, best_of: int, sampling, logprobs, min_mean_logprob) -> bool:
        """Check and keep ``best_of``; returns whether the engine is to return log-probabilities."""
        if isinstance(best_of, bool) or not isinstance(best_of, int) or best_of < 1:
            raise ValueError(f"best_of: a positive integer, got {best_of!r}")
        if best_of > 1 and sampling is None:
            raise ValueError("best_of > 1 needs sampling: greedy completions of one prompt are all equal")
        self.best_of = best_of
        return bool(logprobs) or min_mean_logprob is not None or best_of > 1

    def _health(self) -> dict:
        b = self.batcher
        out = {"batching": self.batching, "engine": type(getattr(self.engine, "engine", self.engine)).__name__,
               "max_length": self.gen.max_length}
        eng = getattr(self.engine, "engine", self.engine)
        if getattr(eng, "device", None) is not None and eng.device.type == "cuda":
            free, total = torch.cuda.mem_get_info(eng.device)
            out.update(hbm_used_gb=round((total - free) / 2**30, 2), hbm_total_gb=round(total / 2**30, 2),
                       kv_cache_gb=round(eng.kv_cache_bytes() / 2**30, 3), slots=eng.max_batch)
            METRICS.set("tutor_hbm_used_gb", out["hbm_used_gb"])
        if getattr(eng, "prompt_prefix", None):  # --prefix-cache on: how many admissions shared the prefix
            n = eng.prefix_prompts
            out.update(prefix_tokens=len(eng.prompt_prefix), prefix_hits=eng.prefix_hits,
                       prefix_rows_skipped=eng.prefix_rows_skipped, prefix_decode_launches=eng.prefix_decode_launches,
                       prefix_hit_rate=round(eng.prefix_hits / n, 4) if n else None)
            METRICS.set("tutor_prefix_hit_rate", eng.prefix_hits / n if n else 0.0)
        if getattr(self, "controls", None) is not None and self.controls.stop:
            out.update(stopped_by_sequence=self.front.stopped_by_sequence)
        if isinstance(self.front, LogprobMeter):
            out.update(logprob_stats(self.front))
        if getattr(self, "best_of", 1) > 1:
            out.update(best_of_stats(self))
        if self.batching == "continuous":
            out.update(active=b.active, completed=b.completed, ok=b._error is None and b._thread.is_alive())
        else:
            out.update(queued=b.q.qsize(), ok=b._t.is_alive())
        gw = getattr(getattr(self, "pool", None), "gate_worker", None)
        if gw is not None:  # --serve-gate: the relevance gate's passes between decode chunks
            out.update(gate=True, scored=gw.scored, passes=gw.passes, batched_queries=gw.scored,
                       device=str(getattr(gw.enc, "device", "cpu")))
        return out

    def start(self, on_fatal=None, poll_s: float = 0.25):
        """``on_fatal(error)``: called once if the batcher fails for good (a stalled TP peer, a
        device error): the CLI exits the process non-zero so a supervisor starts a fresh one --
        never a re-exec of a process that initialised the GPU."""
        self.server.start()
        log.info("tutoring server on port %d", self.port)
        self._arm_fatal(on_fatal, poll_s)
        return self

    def _arm_fatal(self, on_fatal, poll_s: float):
        if on_fatal is not None:
            def watch():
                while not self._stopping.is_set():
                    err = getattr(self.batcher, "failed", None)
                    if err is not None:
                        log.error("batcher failed (%s): this replica stops serving", err)
                        METRICS.inc("tutor_fatal_total")
                        on_fatal(err)
                        return
                    self._stopping.wait(poll_s)

            threading.Thread(target=watch, name="tutor-fatal-watch", daemon=True).start()

    def stop(self):
        self._stopping.set()
        self.server.stop(0.5).wait()
        self.batcher.stop()


class AioTutoringServicer:
    """``Tutoring.GetLLMAnswer`` as a coroutine: a query holds no thread while it decodes (the
    threaded servicer parks one worker per query, capping a replica at ``workers`` queries in
    flight -- far below the 1024-query operating point)."""

    def __init__(self, batcher, tokenizer: GPT2BPE, timeout: float = 300.0):
        self.batcher = batcher
        self.tok = tokenizer
        self.timeout = timeout

    async def GetLLMAnswer(self, request, context):
        import asyncio

        ids = self.tok.encode(build_prompt(request.query))
        try:
            out = await asyncio.wait_for(asyncio.wrap_future(self.batcher.submit(ids)), self.timeout)
        except Overloaded as e:
            await context.abort(grpc.StatusCode.RESOURCE_EXHAUSTED, str(e))
        except Exception as e:
            failed = getattr(self.batcher, "failed", None) is not None
            code = grpc.StatusCode.UNAVAILABLE if failed else grpc.StatusCode.INTERNAL
            await context.abort(code, f"generation failed: {e}")
        return pb.QueryResponse(success=True, response=self.tok.decode(out, skip_special_tokens=True))


class AioTutoringServer(TutoringServer):
    """The continuous-batching tutoring server with a ``grpc.aio`` front end on its own event-loop
    thread: thousands of queries in flight per replica (the reference's tutoring
    server is a 10-thread synchronous gRPC server).  Same engine, batcher, health/debug RPCs,
    fatal hook and stop() as ``TutoringServer``."""

    def __init__(self, engine, port: int = 50054, host: str = "[::]", max_length: int = 150,
                 repetition_penalty: float = 1.2, tokenizer: GPT2BPE | None = None, chunk: int = 8,
                 max_queue: int | None = None, sampling=None, controls=None, logprobs: bool = False,
                 min_mean_logprob: float | None = None, best_of: int = 1):
        import asyncio

        from ..engine.scheduler import ContinuousBatcher

        if not hasattr(engine, "admit"):
            raise ValueError("the aio front end needs a slot engine (continuous batching)")
        if engine.max_length != max_length:
            raise ValueError("continuous batching: engine max_length differs from the server's")
        logprobs = self._init_best_of(best_of, sampling, logprobs, min_mean_logprob)
        self.gen = generation_config(max_length, repetition_penalty, sampling, controls, logprobs)
        self.controls = controls
        self.tok = tokenizer or GPT2BPE(eos_token_id=getattr(getattr(engine, "cfg", None), "eos_token_id", 50256))
        self.batcher = ContinuousBatcher(engine, repetition_penalty, chunk=chunk,
                                         max_queue=default_max_queue(engine, max_queue), sampling=sampling,
                                         **_controls_kw(controls), **_logprobs_kw(logprobs), **_best_of_kw(best_of))
        self.front = front_batcher(self.batcher, controls, logprobs, min_mean_logprob)
        self.batching = "continuous"
        self.engine = engine
        self._stopping = threading.Event()
        self._loop = asyncio.new_event_loop()
        self._thread = threading.Thread(target=self._loop.run_forever, name="tutor-aio", daemon=True)
        self._thread.start()

        async def make():
            srv = grpc.aio.server(migration_thread_pool=futures.ThreadPoolExecutor(max_workers=4),
                                  options=[("grpc.max_send_message_length", wire.DEFAULT_MAX_MESSAGE),
                                           ("grpc.max_receive_message_length", wire.DEFAULT_MAX_MESSAGE)])
            wire.register(srv, "Tutoring", AioTutoringServicer(self.front, self.tok))
            srv.add_generic_rpc_handlers((debug_handler(health=self._health),))
            return srv, srv.add_insecure_port(f"{host}:{port}")

        self.server, self.port = asyncio.run_coroutine_threadsafe(make(), self._loop).result(30)
        if self.port == 0:
            raise RuntimeError(f"could not bind {host}:{port}")

    def start(self, on_fatal=None, poll_s: float = 0.25):
        import asyncio

        asyncio.run_coroutine_threadsafe(self.server.start(), self._loop).result(30)
        log.info("tutoring server (aio) on port %d", self.port)
        self._arm_fatal(on_fatal, poll_s)
        return self

    def stop(self):
        import asyncio

        self._stopping.set()
        try:
            asyncio.run_coroutine_threadsafe(self.server.stop(0.5), self._loop).result(10)
        finally:
            self.batcher.stop()
            self._loop.call_soon_threadsafe(self._loop.stop)
            self._thread.join(5)


class PooledTutoringServer(TutoringServer):
    """The continuous-batching engine behind ``n`` front-end processes (``tutor/frontend.py``):
    this process keeps the GPU and the scheduler; gRPC termination and (de)tokenization run in
    the front ends, which share the public port.  Same health/metrics surface, fatal hook and
    stop() as ``TutoringServer``."""

    def __init__(self, engine, pool, max_length: int = 150, repetition_penalty: float = 1.2, chunk: int = 8,
                 max_queue: int | None = None, sampling=None, controls=None, logprobs: bool = False,
                 min_mean_logprob: float | None = None, best_of: int = 1):
        from ..engine.scheduler import ContinuousBatcher

        if not hasattr(engine, "admit"):
            raise ValueError("the front-end pool needs a slot engine (continuous batching)")
        if engine.max_length != max_length:
            raise ValueError("continuous batching: engine max_length differs from the server's")
        logprobs = self._init_best_of(best_of, sampling, logprobs, min_mean_logprob)
        self.gen = generation_config(max_length, repetition_penalty, sampling, controls, logprobs)
        self.controls = controls
        self.batcher = ContinuousBatcher(engine, repetition_penalty, chunk=chunk,
                                         max_queue=default_max_queue(engine, max_queue), sampling=sampling,
                                         **_controls_kw(controls), **_logprobs_kw(logprobs), **_best_of_kw(best_of))
        self.front = front_batcher(self.batcher, controls, logprobs, min_mean_logprob)
        self.batching = "continuous"
        self.engine = engine
        self.pool = pool
        self.port = 0
        self._stopping = threading.Event()

    def start(self, on_fatal=None, poll_s: float = 0.25):
        self.pool.serve(self.front, health=self._health)
        self.port = self.pool.port
        log.info("tutoring server on port %d (%d front-end processes)", self.port, self.pool.n)
        self._arm_fatal(on_fatal, poll_s)
        return self

    def stop(self):
        self._stopping.set()
        try:
            self.pool.stop()
        finally:
            self.batcher.stop()


EXIT_FATAL = 75  # EX_TEMPFAIL: the supervisor restarts the replica


def generation_config(max_length: int, repetition_penalty: float, sampling=None, controls=None,
                      logprobs: bool = False) -> GenerationConfig:
    """The servers' ``GenerationConfig``: greedy, or carrying ``sampling``'s fields with ``do_sample``
    set; with ``controls``'s fields when given, and the ``logprobs`` flag."""
    ck = {} if controls is None else dict(no_repeat_ngram_size=controls.no_repeat_ngram_size,
                                          min_new_tokens=controls.min_new_tokens, stop=controls.stop)
    if logprobs:
        ck["logprobs"] = True
    if sampling is None:
        return GenerationConfig(max_length=max_length, repetition_penalty=repetition_penalty, **ck)
    return GenerationConfig(max_length=max_length, repetition_penalty=repetition_penalty, do_sample=True,
                            temperature=sampling.temperature, top_k=sampling.top_k, top_p=sampling.top_p,
                            seed=sampling.seed, **ck)


def _controls_kw(controls) -> dict:
    return {} if controls is None else {"controls": controls}


def _logprobs_kw(logprobs) -> dict:
    return {"logprobs": True} if logprobs else {}


def _best_of_kw(best_of: int) -> dict:
    return {"n": best_of, "select": "mean_logprob"} if best_of > 1 else {}


def best_of_stats(srv) -> dict:
    """The health record's (and the exit line's) best-of-n fields: N, and the running mean over the
    answered queries of the chosen answer's mean log-probability minus its group's average."""
    g = srv.batcher.gain.mean
    return {"best_of": srv.best_of, "best_of_gain": None if g is None else round(g, 4)}


def apply_best_of(args) -> None:
    """``--best-of N`` with N > 1 implies ``--sample`` and ``--logprobs`` (set on ``args``);
    ``ValueError`` for N < 1 or an explicit ``--max-batch`` smaller than N."""
    if args.best_of < 1:
        raise ValueError("--best-of: a positive integer")
    if args.best_of > 1:
        if args.max_batch and args.max_batch < args.best_of:
            raise ValueError(f"--best-of {args.best_of}: needs {args.best_of} decode slots per query, "
                             f"--max-batch is {args.max_batch}")
        args.sample = True
        args.logprobs = True


def logprob_stats(meter: "LogprobMeter") -> dict:
    """The health record's (and the exit line's) log-probability fields."""
    m = meter.mean_token_logprob
    out = {"mean_token_logprob": None if m is None else round(m, 4)}
    if meter.threshold is not None:
        out["low_confidence_answers"] = meter.low_confidence_answers
    return out


def decode_escapes(text: str) -> str:
    """``text`` with its backslash escapes decoded (``\\n`` -> a newline), other characters kept."""
    return text.encode("latin-1", "backslashreplace").decode("unicode_escape")


def controls_from_args(args, tok=None) -> "GenerationControls | None":
    """``--no-repeat-ngram-size / --min-new-tokens / --stop`` -> ``GenerationControls`` (None: none
    given).  Each ``--stop`` text has its backslash escapes decoded and is encoded once with ``tok``
    (the server's tokenizer)."""
    texts = list(args.stop or [])
    if not (args.no_repeat_ngram_size or args.min_new_tokens or texts):
        return None
    if texts and tok is None:
        raise ValueError("--stop: a tokenizer is needed to encode the stop texts")
    stop = []
    for t in texts:
        ids = tuple(int(i) for i in tok.encode(decode_escapes(t)))
        if not ids:
            raise ValueError(f"--stop {t!r}: encodes to no tokens")
        stop.append(ids)
    return GenerationControls(no_repeat_ngram_size=args.no_repeat_ngram_size, min_new_tokens=args.min_new_tokens,
                              stop=tuple(stop))


def sampling_from_args(args) -> "SamplingParams | None":
    """``--sample`` with ``--temperature / --top-k / --top-p / --seed`` -> ``SamplingParams`` (None: greedy)."""
    if not args.sample:
        return None
    return SamplingParams(temperature=args.temperature, top_k=args.top_k, top_p=args.top_p, seed=args.seed)


def arg_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="GPT-2 tutoring server (MI355X HIP engine)")
    ap.add_argument("--port", type=int, default=int(os.environ.get("DLMS_TUTOR_PORT", "50054")))
    ap.add_argument("--host", default="[::]")
    ap.add_argument("--model", default=os.environ.get("DLMS_MODEL", "gpt2"))
    ap.add_argument("--weights", default=None, help="local safetensors checkpoint (HF GPT-2 layout)")
    ap.add_argument("--vocab", default=None, help="GPT-2 vocab.json")
    ap.add_argument("--merges", default=None, help="GPT-2 merges.txt")
    ap.add_argument("--device", default=os.environ.get("DLMS_DEVICE", "auto"))
    ap.add_argument("--max-batch", type=int, default=0,
                    help="decode slots per engine; 0 (default) = as many as free HBM holds (engine/memory.py), "
                         "so one replica reaches the 1024-query operating point")
    ap.add_argument("--window-ms", type=float, default=2.0)
    ap.add_argument("--max-length", type=int, default=150)
    ap.add_argument("--repetition-penalty", type=float, default=1.2)
    ap.add_argument("--weight-dtype", choices=("bf16", "fp8"), default="bf16",
                    help="fp8: W8A8 e4m3 MFMA GEMMs for QKV / c_fc / LM head (GPU engine)")
    ap.add_argument("--kv-dtype", choices=("bf16", "fp8"), default="bf16",
                    help="fp8: the KV cache holds e4m3 bytes without scales -- half the bytes the decode attention "
                         "streams, twice the slots in the same HBM, reduced precision; one GPU per replica, bf16 weights")
    ap.add_argument("--prefix-cache", choices=("off", "on"), default="off",
                    help="on: compute the K/V of the prompt template's shared leading tokens once and keep them in "
                         "the engine's prefix store -- a query prefills only the rest of its prompt; the tokens "
                         "served are unchanged; one GPU per replica, bf16 weights")
    ap.add_argument("--latency-path", choices=("auto", "on", "off"), default="auto",
                    help="the GPU engine's low-batch decode paths (latency / mid-batch steps): auto = the engine's "
                         "default (on with the bf16 KV cache, off with --kv-dtype fp8), on / off force them -- on "
                         "also with --kv-dtype fp8")
    ap.add_argument("--tp", type=int, default=0, help="tensor-parallel degree under torchrun (default: world)")
    ap.add_argument("--batching", choices=("auto", "continuous", "window"), default="auto")
    ap.add_argument("--chunk", type=int, default=8, help="decode steps between scheduler polls")
    ap.add_argument("--max-queue", type=int, default=None,
                    help="queries that may wait for a KV slot before the replica answers RESOURCE_EXHAUSTED "
                         "(default: one batch of slots; 0 = unbounded)")
    ap.add_argument("--frontend", choices=("aio", "threads"), default="aio",
                    help="aio: asyncio gRPC front end (thousands of queries in flight); threads: a worker per query")
    ap.add_argument("--frontends", type=int, default=4,
                    help="gRPC front-end processes sharing the port (tutor/frontend.py); 0 = serve gRPC in "
                         "this process (--frontend)")
    ap.add_argument("--warm-batch", type=int, default=1024,
                    help="capture the decode graphs of every batch bucket up to this size before serving, so "
                         "the first burst of queries does not pay them (0 = capture on first use)")
    ap.add_argument("--serve-gate", action="store_true",
                    help="also serve the relevance gate (lmsinternal.Gate) on the tutoring port: the front ends "
                         "tokenize, this process runs the BERT encoder passes between decode chunks on the decode "
                         "stream (gate/service.py GateWorker) -- LMS nodes use it with --gate remote "
                         "--gate-addr <this address>")
    ap.add_argument("--gate-model", default="bert-base-uncased")
    ap.add_argument("--gate-vocab", default=None, help="BERT vocab.txt for the gate (synthetic if absent)")
    ap.add_argument("--gate-weights", default=None, help="local safetensors for the gate model")
    ap.add_argument("--log-level", default=os.environ.get("DLMS_LOG", "INFO"))
    ap.add_argument("--sample", action="store_true",
                    help="sample the answers (temperature / top-k / top-p, seeded) instead of greedy decoding; "
                         "bf16 weights on one GPU per replica")
    ap.add_argument("--temperature", type=float, default=0.7)
    ap.add_argument("--top-k", type=int, default=50)
    ap.add_argument("--top-p", type=float, default=0.9)
    ap.add_argument("--seed", type=int, default=0, help="sampling seed (the n-th request of a run draws from stream n)")
    ap.add_argument("--no-repeat-ngram-size", type=int, default=0, metavar="N",
                    help="no N-gram of tokens occurs twice in an answer's sequence, prompt included (0: off); with "
                         "--min-new-tokens and --stop: bf16 weights on one GPU per replica")
    ap.add_argument("--min-new-tokens", type=int, default=0, metavar="N",
                    help="the end-of-text token is banned until N tokens have been generated")
    ap.add_argument("--stop", action="append", default=None, metavar="TEXT",
                    help="stop sequence (repeatable, at most %d of at most %d tokens): an answer ends once its "
                         "generated tokens end with TEXT's tokens, which are dropped from it; backslash escapes are "
                         "decoded ('\\nQuestion:' starts with a newline).  TEXT is encoded once with the server's "
                         "tokenizer and matching is on tokens: a stop text that BPE merges with the characters "
                         "before it will not match" % (CONTROLS_MAX_STOP, CONTROLS_MAX_STOP_LEN))
    ap.add_argument("--logprobs", action="store_true",
                    help="have the engine return every generated token's log-probability: the health record and "
                         "the exit line gain mean_token_logprob, the running mean over the answered queries of an "
                         "answer's mean token log-probability; the answers are unchanged; bf16 weights on one GPU "
                         "per replica")
    ap.add_argument("--min-mean-logprob", type=float, default=None, metavar="X",
                    help="implies --logprobs: also count the answers whose mean token log-probability is below X "
                         "(low_confidence_answers)")
    ap.add_argument("--best-of", type=int, default=1, metavar="N",
                    help="implies --sample and --logprobs: run every query as N sampled completions of one prefill "
                         "(the prompt's K/V are forked into N decode slots) and answer with the one of the highest "
                         "mean token log-probability; one answer per query, the wire format is unchanged; the "
                         "health record and the exit line gain best_of and best_of_gain; --min-mean-logprob judges "
                         "the chosen answer; bf16 weights on one GPU per replica")
    return ap


def main(argv=None):
    ap = arg_parser()
    args, _ = parse_with_config(ap, argv)
    try:
        apply_best_of(args)
        sampling = sampling_from_args(args)
    except ValueError as e:
        ap.error(str(e))
    from ..engine import mode as engine_mode

    want_controls = bool(args.no_repeat_ngram_size or args.min_new_tokens or args.stop)
    logprobs = args.logprobs or args.min_mean_logprob is not None
    for wanted, option, unsupported in (
            (sampling is not None, "--best-of" if args.best_of > 1 else "--sample", engine_mode.sampling_unsupported),
            (args.kv_dtype == "fp8", "--kv-dtype fp8", engine_mode.kv_fp8_unsupported),
            (args.prefix_cache == "on", "--prefix-cache on", engine_mode.prefix_unsupported),
            (want_controls, "--no-repeat-ngram-size / --min-new-tokens / --stop", engine_mode.controls_unsupported),
            (logprobs, "--logprobs / --min-mean-logprob", engine_mode.logprobs_unsupported)):
        why = wanted and unsupported(args.tp or int(os.environ.get("WORLD_SIZE", "1")), args.weight_dtype == "fp8")
        if why:
            ap.error(f"{option}: {why}")
    controls = None
    if want_controls:
        try:  # (the stop texts are encoded here, once, with the tokenizer the server detokenises with)
            controls = controls_from_args(args, GPT2BPE(args.vocab, args.merges,
                                                        eos_token_id=gpt2_config(args.model).eos_token_id))
        except ValueError as e:
            ap.error(str(e))
    mode = {} if sampling is None else {"sampling": sampling}
    mode.update(_controls_kw(controls))
    mode.update(_logprobs_kw(logprobs))
    srv_mode = dict(mode, min_mean_logprob=args.min_mean_logprob) if logprobs else dict(mode)
    if args.best_of > 1:
        srv_mode["best_of"] = args.best_of
    logging.basicConfig(level=getattr(logging, args.log_level.upper(), logging.INFO),
                        format="%(asctime)s %(name)s %(levelname)s %(message)s")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    tp_group = proxy = pool = None
    if args.frontends > 0 and args.batching != "window":
        # spawned before anything here touches the GPU; only the rank that serves a TP group
        # (every --tp-th rank under torchrun) gets front ends, on its group's port
        tp = args.tp or world
        rank = int(os.environ.get("RANK", "0"))
        if rank % tp == 0:
            from ..models.config import bert_config
            from .frontend import FrontendPool

            gate_fe = None
            if args.serve_gate:
                bc = bert_config(args.gate_model)
                gate_fe = dict(vocab=args.gate_vocab, vocab_size=bc.vocab_size, max_length=bc.max_position)
            pool = FrontendPool(args.frontends, args.port + rank // tp, args.host, args.vocab, args.merges,
                                eos=gpt2_config(args.model).eos_token_id, gate=gate_fe)
    if world > 1:  # torchrun: TP groups of --tp consecutive ranks, one front end (port + group) each
        import torch.distributed as dist

        from ..engine.tp_serving import TPEngineProxy, serve_follower
        from ..parallel.tp import init_distributed, tp_groups

        rank, world, local = init_distributed("nccl" if args.device != "cpu" and torch.cuda.is_available()
                                              else "gloo")
        tp = args.tp or world
        tp_group, dp_idx, _ = tp_groups(tp)
        ctrl = None
        for g in range(world // tp):  # every rank creates every group, keeps its own
            grp = dist.new_group(list(range(g * tp, (g + 1) * tp)), backend="gloo")
            if g == dp_idx:
                ctrl = grp
        src = dp_idx * tp
        device = f"cuda:{local}" if args.device != "cpu" and torch.cuda.is_available() else "cpu"
        eng = make_engine(args.model, device, args.max_batch, args.max_length, args.weights, tp_group=tp_group,
                          weight_dtype=args.weight_dtype, kv_dtype=args.kv_dtype,
                          latency_path={"auto": None, "on": True, "off": False}[args.latency_path])
        if rank != src:
            n = serve_follower(eng, ctrl, src)
            log.info("TP follower rank %d done after %d commands", rank, n)
            if hasattr(eng, "close"):
                eng.close()
            return
        proxy = eng = TPEngineProxy(eng, ctrl, src)
        args.port += dp_idx
    else:
        eng = make_engine(args.model, args.device, args.max_batch, args.max_length, args.weights,
                          weight_dtype=args.weight_dtype, kv_dtype=args.kv_dtype,
                          latency_path={"auto": None, "on": True, "off": False}[args.latency_path],
                          prefix_capacity=PREFIX_CAPACITY if args.prefix_cache == "on" else 0)
    args.max_batch = getattr(eng, "max_batch", 0) or args.max_batch or 64
    if args.max_batch < args.best_of:  # (the slots planned from free HBM: engine/memory.py)
        if hasattr(eng, "close"):
            eng.close()
        raise SystemExit(f"--best-of {args.best_of}: the engine has {args.max_batch} decode slots, "
                         f"a query needs {args.best_of}")
    tok = GPT2BPE(args.vocab, args.merges, eos_token_id=eng.cfg.eos_token_id)
    if args.prefix_cache == "on":  # (ahead of the graph captures below)
        prefix = enable_prefix_cache(eng, tok)
        log.info("prompt-prefix cache on: the first %d tokens of every prompt come from the prefix store", len(prefix))
    if args.warm_batch > 0 and hasattr(eng, "warm_decode_graphs"):
        # (a TP proxy mirrors the call to every rank of its group: the captures' warm-up steps run
        # the group's collectives, engine/tp_serving.py)
        n, secs = eng.warm_decode_graphs(args.repetition_penalty, args.warm_batch, **mode)
        log.info("captured %d decode graphs (batch buckets <= %d) in %.1f s", n, args.warm_batch, secs)
    if pool is not None and hasattr(eng, "admit"):
        srv = PooledTutoringServer(eng, pool, args.max_length, args.repetition_penalty, chunk=args.chunk,
                                   max_queue=args.max_queue, **srv_mode)
        if args.serve_gate:
            pool.gate_worker = make_gate_worker(args.gate_model, args.gate_weights, getattr(eng, "device", "cpu"))
            pool.gate_worker.attach(srv.batcher)
    else:
        if pool is not None:  # not a slot engine (CPU window batching): serve in-process
            pool.stop(timeout=2)
            pool = None
    if pool is not None:
        pass
    elif args.frontend == "aio" and args.batching != "window" and hasattr(eng, "admit"):
        srv = AioTutoringServer(eng, args.port, args.host, args.max_length, args.repetition_penalty, tokenizer=tok,
                                chunk=args.chunk, max_queue=args.max_queue, **srv_mode)
    else:
        srv = TutoringServer(eng, args.port, args.host, args.max_batch, args.window_ms, args.max_length,
                             args.repetition_penalty, tokenizer=tok, batching=args.batching, chunk=args.chunk,
                             max_queue=args.max_queue, **srv_mode)
    done = threading.Event()
    fatal: list = []

    def on_fatal(err):
        fatal.append(err)
        done.set()

    srv.start(on_fatal=on_fatal)
    print(f"Tutoring Server started on port {srv.port}", flush=True)
    signal.signal(signal.SIGTERM, lambda *a: done.set())
    signal.signal(signal.SIGINT, lambda *a: done.set())
    done.wait()
    srv.stop()
    if getattr(eng, "prompt_prefix", None) and eng.prefix_prompts:
        log.info("prompt-prefix cache: %d of %d admitted prompts shared the prefix (%.1f %%), %d prefill rows skipped",
                 eng.prefix_hits, eng.prefix_prompts, 100.0 * eng.prefix_hits / eng.prefix_prompts,
                 eng.prefix_rows_skipped)
    if isinstance(getattr(srv, "front", None), LogprobMeter):
        log.info("log-probabilities: %s over %d answered queries",
                 ", ".join(f"{k} {v}" for k, v in logprob_stats(srv.front).items()), srv.front.answers)
    if args.best_of > 1:
        log.info("best of n: %s", ", ".join(f"{k} {v}" for k, v in best_of_stats(srv).items()))
    if proxy is not None:
        proxy.close()  # releases the followers, which close their engines (below, same order)
        eng = proxy.engine
    if hasattr(eng, "close"):
        eng.close()  # (TP: every rank of the group, the xGMI teardown is collective)
    if fatal:  # exit, never re-exec: a supervisor starts a fresh process on a clean device state
        log.error("exiting with status %d after a fatal serving error", EXIT_FATAL)
        os._exit(EXIT_FATAL)


if __name__ == "__main__":
    main()
