"""MI355X GPT-2 decode engine: hand-written HIP kernels + hipGraph-captured decode steps.

One engine instance owns one tensor-parallel group's share of the model (TP=1 on a single
MI355X, or one rank of a TP group; one process per GPU, RCCL over xGMI for the collectives).

Semantics are the reference's ``model.generate(max_length=150, repetition_penalty=1.2)``
greedy decode (``tutoring_server.py:21-29``): full sequences are returned (prompt echoed),
each ends at EOS (inclusive) or at ``max_length`` total tokens.

Per decode step (SURVEY.md §7.1 design choice 3), replayed as ONE hipGraph per batch bucket:

    for each layer:  LN1 -> QKV GEMM (+bias, q out, k/v scattered into the KV cache)
                     -> row attention over the cache -> out-proj GEMM (+bias +residual)
                     [-> RCCL all-reduce of the partial residual under TP]
                     -> LN2 -> c_fc GEMM (+bias, GELU-tanh) -> c_proj GEMM (+bias +residual)
                     [-> all-reduce]
    ln_f -> LM-head GEMM with repetition penalty + argmax fused in the epilogue
         [-> all-gather of the (value, index) keys across vocab shards]
    -> device-side update: token append, seen bitmap, stop flags, next embedding.

No host round trip happens inside a step; the host only checks the stop flags every few steps.
"""
from __future__ import annotations

import contextlib
import itertools
import logging
import math
import os
import time
from dataclasses import dataclass

import numpy as np
import torch

from .. import ops
from ..models.config import GenerationControls, GPT2Config, SamplingParams
from ..utils.metrics import METRICS
from .mode import (DecodeMode, controls_unsupported, kv_fp8_unsupported, logprobs_unsupported,  # noqa: F401
                   prefix_unsupported, sampling_unsupported)
from .weights import GPT2DeviceWeights, prepare_gpt2_weights

log = logging.getLogger(__name__)

# Streams of this process that run work beside the engine's decode (a co-located gate's encoder, a
# test's load generator).  An aborted dataflow launch records whether one of them was busy: the
# dataflow grid's workgroups wait on each other, so a kernel on another stream that holds CUs can
# leave part of the grid unscheduled until the bounded waits give up.
_SIDE_STREAMS: list = []


@contextlib.contextmanager
def capture_guard():
    """Around a hipGraph capture: collect garbage first, then keep Python's cyclic GC off until the
    capture ends.  An automatic collection DURING a capture runs the destructors of dead engines'
    graphs (hipGraphExecDestroy) in the middle of it -- in any thread, since the GC runs wherever
    an allocation triggers it -- which aborted the process (and, once, left a graph that
    segfaulted on replay) in the round-6 GPU tier."""
    import gc

    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


def register_side_stream(stream) -> None:
    """Declare a stream whose kernels may run beside the engine's decode (see ``_SIDE_STREAMS``)."""
    if all(s is not stream for s in _SIDE_STREAMS):
        _SIDE_STREAMS.append(stream)


def unregister_side_stream(stream) -> None:
    _SIDE_STREAMS[:] = [s for s in _SIDE_STREAMS if s is not stream]


@dataclass
class GenerateStats:
    batch: int = 0
    prompt_tokens: int = 0
    new_tokens: int = 0
    prefill_ms: float = 0.0
    decode_ms: float = 0.0
    steps: int = 0
    graph: bool = False

    @property
    def total_ms(self) -> float:
        return self.prefill_ms + self.decode_ms


def seen_bitmap(tokens, words: int) -> np.ndarray:
    """Repetition-penalty bitmap of a token list, as int32 words (bit t%32 of word t//32)."""
    bm = np.zeros(words, dtype=np.uint32)
    ids = np.asarray(sorted(set(int(t) for t in tokens)), dtype=np.int64)
    if ids.size:
        np.bitwise_or.at(bm, ids >> 5, (np.uint32(1) << (ids & 31).astype(np.uint32)))
    return bm.view(np.int32)


def passthrough(prompts, T: int, eos: int):
    """``generate()`` semantics for degenerate prompts: one already at/over ``max_length`` comes
    back unchanged (nothing is generated); an empty prompt starts from EOS (GPT-2's BOS).
    Returns (results with pass-through entries filled, indices of prompts that must run,
    normalised copies of all prompts)."""
    norm = [list(p) if len(p) else [eos] for p in prompts]
    out: list = [None] * len(prompts)
    run = []
    for i, p in enumerate(norm):
        if len(p) >= T:
            out[i] = p
        else:
            run.append(i)
    return out, run, norm


@dataclass
class _Rows:
    """Activation buffers of one contiguous range of batch rows (the whole batch, or one half of it
    in the overlapped decode step) plus the residual update still pending for the next LayerNorm."""
    x: torch.Tensor
    parts: torch.Tensor
    h: torch.Tensor
    q: torch.Tensor
    att: torch.Tensor
    ff: torch.Tensor
    row_slot: torch.Tensor
    row_pos: torch.Tensor
    row_kvlen: torch.Tensor
    M: int
    h8: torch.Tensor | None = None
    hsc: torch.Tensor | None = None
    ln_out: dict | None = None
    pend: tuple = (None, 0, None)
    tiles: "ops.AttnTiles | None" = None  # packed prompts: MFMA tile attention instead of per-row
    split_cap: int = 8  # split-K cap of the row-parallel projections (lower for concurrent row parts)
    split_fixed: int | None = None  # pinned split-K (M-independent arithmetic: prefill_split)
    persist_attn: bool = False  # decode attention as the low-occupancy persistent kernel
    pidx: int = 0  # index of the row part (timing-only experiments address parts by it)


class HostResult:
    """A device-to-host result in flight: ``result()`` waits on the event recorded right after the
    copies were enqueued -- not on work enqueued later on the stream."""

    def __init__(self, finish, keep=()):
        self._finish, self._keep = finish, keep
        self._ev = None
        if keep and torch.cuda.is_available():
            self._ev = torch.cuda.Event()
            self._ev.record()

    def result(self):
        if self._ev is not None:
            self._ev.synchronize()
        return self._finish()


def _to_device(a: np.ndarray, dev, dtype=np.int32) -> torch.Tensor:
    """Host array -> device through pinned memory, so the copy never blocks the host on the
    stream (a pageable-memory copy waits for the GPU to reach it: the work queued ahead)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).pin_memory().to(dev, non_blocking=True)


def _bucket(n: int) -> int:
    for b in (1, 2, 4, 8, 16, 32, 48, 64, 96, 128, 192, 256, 384, 512, 768, 1024):
        if n <= b:
            return b
    return (n + 255) // 256 * 256


def split_prefix(prompts, prefix) -> list[int]:
    """Per prompt, the number of leading tokens the prefix cache supplies: ``len(prefix)`` when the
    prompt starts with ``prefix`` and is longer than it (at least one suffix row has to run for the
    first token), else 0 -- a prompt equal to the prefix, a shorter one, or one differing in any
    prefix token is prefilled whole."""
    prefix = list(prefix) if prefix is not None else []
    P = len(prefix)
    if P == 0:
        return [0] * len(prompts)
    return [P if len(p) > P and list(p[:P]) == prefix else 0 for p in prompts]


def pack_prompts(prompts, slots, pfx=None):
    """The packed arrays of a prefill (numpy int64): the tokens, positions and slots of the rows
    that run -- prompt i without its first ``pfx[i]`` tokens (``split_prefix``; None: whole prompts),
    positions starting at ``pfx[i]`` -- then per prompt the index of its last row, its full length
    and the length of its suffix (what ``ops.AttnTiles`` is built from).
    Returns (tokens, positions, row slots, last rows, lengths, suffix lengths)."""
    lens_np = np.asarray([len(p) for p in prompts], dtype=np.int64)
    if pfx is None or not any(pfx):
        pfx_np = np.zeros(len(prompts), dtype=np.int64)
        rows = itertools.chain.from_iterable(prompts)
    else:
        pfx_np = np.asarray(pfx, dtype=np.int64)
        rows = itertools.chain.from_iterable(p[k:] for p, k in zip(prompts, pfx))
    sl_np = lens_np - pfx_np
    if sl_np.min() < 1:
        raise ValueError("prefill: every prompt needs at least one row past its cached prefix")
    R = int(sl_np.sum())
    ends = np.cumsum(sl_np)
    # (numpy, no per-prompt Python loops: a 1024-prompt admission used to spend ~20 ms of host time
    # here with the GPU idle)
    tok_np = np.fromiter(rows, dtype=np.int64, count=R)
    pos_np = np.arange(R, dtype=np.int64) - np.repeat(ends - sl_np - pfx_np, sl_np)
    slot_np = np.repeat(np.asarray(slots, dtype=np.int64), sl_np)
    return tok_np, pos_np, slot_np, ends - 1, lens_np, sl_np


class HipGPT2Engine:
    # (row, head) pairs up to which decode attention uses the split-K kernel (profiles/r2_skinny_bench.log:
    # at 32 rows x 12 heads, T=150: 7.9 us vs 12.3 us for one wave per pair)
    SPLIT_ATTN_MAX_PAIRS = 1024
    # fused attention + out-projection up to this many rows (its workgroups recompute a head's
    # attention per row): against the split attention + in-place skinny out-projection, batch 1
    # 36.8 vs 37.9 ms per query, batch 2 39.2 vs 38.7 (profiles/r2_attn_oproj_ab.txt)
    FUSE_AO_MAX_ROWS = 1
    # split-K of the row-parallel projections on the latency path (fixed: the fused add+LN
    # kernel sums exactly this many slabs)
    SMALL_SPLIT = 4
    PS_LM_MIN_ROWS = 256

    def __init__(self, cfg: GPT2Config, weights: dict[str, torch.Tensor] | GPT2DeviceWeights, device=None,
                 max_batch: int | str = 256, max_length: int = 150, tp_group=None, use_graph: bool = True,
                 check_every: int = 16, max_batch_cap: int = 4096, weight_dtype: str = "bf16",
                 overlap: bool | None = None, overlap_min_batch: int = 512, overlap_parts: int | None = None,
                 p2p: bool | None = None, latency_path: bool | None = None, prefill_split: int | None = None,
                 kv_dtype: str = "bf16", prefix_capacity: int = 0):
        """``prefix_capacity > 0``: an opt-in prompt-prefix cache of up to that many tokens
        (``set_prompt_prefix``): the K/V of a token prefix shared by the prompts are computed once and
        kept in a prefix store; a prompt that starts with it prefills only its suffix rows and gets
        the prefix's K/V copied into its slot (``ops.kv_prefix_fill``), after which every decode
        path runs unchanged.  bf16 weights on one GPU (``prefix_unsupported``: ``ValueError``); both
        KV dtypes.  0 (default): no store, and every launch is the one made without the feature.
        ``kv_dtype="fp8"``: the KV cache holds OCP e4m3 bytes without scales
        (``models.gpt2.quantize_kv_e4m3``: the bf16 cache's content, saturated and rounded to
        nearest-even e4m3) -- half the bytes the decode attention streams and twice the slots per
        GiB, at reduced precision (the oracle is ``GPT2Reference(kv_dtype="fp8")``).  By default
        every batch size then runs the tiled step (QKV GEMM scattering e4m3, the fp8 wave /
        persistent decode attention, the fp8 tile attention in the prefill) and the overlapped
        >= 512-row step is on.  An explicit ``latency_path=True`` turns on the latency, mid, fused
        attention-out-projection and fused-MLP paths on the fp8 cache under the rules of the bf16
        cache (their QKV epilogues scatter e4m3, their attention kernels read it); the one-row
        dataflow decode has no fp8-cache build and stays off.  Not with ``tp_group`` or
        ``weight_dtype="fp8"`` (out of scope: ``ValueError``).  The bf16 default is the
        reference-precision cache.
        ``weight_dtype="fp8"``: W8A8 OCP-e4m3 MFMA GEMMs for QKV, c_fc and the LM head (activation
        rows scaled by the fused LayerNorms); the bf16 default is the reference-precision path.
        ``overlap``: decode batches of >= ``overlap_min_batch`` rows run as ``overlap_parts`` row
        ranges on as many streams (attention of one beside the GEMMs of the others); default from
        ``DLMS_OVERLAP`` (on unless "0"; measured +1.7 % at 1024 queries, +7 % at 2048, 4 parts
        and the serialised-halves schedule slower -- profiles/r1_overlap_ab.jsonl; with the split-K
        cap below, +3-4 % at 512 and -11 % at 256 -- profiles/r1_split_cap_insitu.log, hence the
        512-row threshold, ``DLMS_OVERLAP_MIN_BATCH`` overrides).
        ``p2p`` (TP only): the row-parallel all-reduces and the argmax-key all-gather run as
        one-shot xGMI peer-memory kernels (``parallel/xgmi.py``) instead of RCCL calls; default
        on for an RCCL group unless ``DLMS_XGMI=0``.  Messages larger than the slab (big packed
        prefills) still go through RCCL.
        ``latency_path`` (default on unless ``DLMS_LATENCY_PATH=0``): decode buckets of at most
        ``ops.skinny_addln_max_rows(d)`` rows (8 for GPT-2 small/medium) run the latency-shaped step
        (``_decode_step_small``): fused add+LN+GEMM on pre-shuffled weights for LN1->QKV and
        LN2->c_fc, split-K flash-decode attention, no standalone LayerNorm kernels.
        ``prefill_split``: pin the split-K of the prefill's row-parallel projections (default: a
        heuristic of the packed row count) so a prompt's arithmetic does not depend on what else is
        admitted with it -- continuous batching is then bit-identical to serving it alone."""
        if kv_dtype not in ("bf16", "fp8"):
            raise ValueError(f"kv_dtype {kv_dtype!r}: bf16 or fp8")
        if kv_dtype == "fp8":
            w8 = weights.fp8 if isinstance(weights, GPT2DeviceWeights) else weight_dtype == "fp8"
            why = kv_fp8_unsupported(2 if tp_group is not None else 1, w8)
            if why:
                raise ValueError(why)
        prefix_capacity = int(prefix_capacity)
        if prefix_capacity < 0:
            raise ValueError("prefix_capacity: >= 0")
        if prefix_capacity:
            w8 = weights.fp8 if isinstance(weights, GPT2DeviceWeights) else weight_dtype == "fp8"
            why = prefix_unsupported(2 if tp_group is not None else 1, w8)
            if why:
                raise ValueError(why)
        if not max_length + 1 < cfg.vocab_size:  # (GenerationControls: a row can never be banned completely)
            raise ValueError(f"max_length {max_length}: must be below vocab_size - 1 = {cfg.vocab_size - 1}")
        if not torch.cuda.is_available():
            raise RuntimeError("HipGPT2Engine needs a GPU (use TorchGPT2Engine on CPU)")
        ops.lib()  # fail loudly if the kernel library is missing
        self.cfg = cfg
        self.kv_dtype = kv_dtype
        self.kv_fp8 = kv_dtype == "fp8"
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.index is None:  # pin "cuda" to a concrete ordinal (scheduler threads set it)
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.tp_group = tp_group
        if tp_group is not None:
            import torch.distributed as dist

            self.tp_rank, self.tp_size = dist.get_rank(tp_group), dist.get_world_size(tp_group)
        else:
            self.tp_rank, self.tp_size = 0, 1
        if isinstance(weights, GPT2DeviceWeights):
            self.w = weights
        else:
            if weight_dtype not in ("bf16", "fp8"):
                raise ValueError(f"weight_dtype {weight_dtype!r}: bf16 or fp8")
            self.w = prepare_gpt2_weights(cfg, weights, self.device, self.tp_rank, self.tp_size,
                                          fp8=weight_dtype == "fp8")
        if max_length > cfg.n_positions:
            raise ValueError("max_length exceeds n_positions")
        if not max_batch or max_batch == "auto":  # size the slot pool from free HBM (engine/memory.py)
            from .memory import plan_max_batch

            max_batch = plan_max_batch(cfg, max_length, self.tp_size, weights_resident=True, cap=max_batch_cap,
                                       device=self.device, kv_dtype=kv_dtype,
                                       prefix_capacity=min(prefix_capacity, max_length))
        self.max_batch = int(max_batch)
        self.max_length = max_length
        # prompt-prefix cache (set_prompt_prefix): rows of the store (more than max_length are no use)
        self.prefix_capacity = min(prefix_capacity, max_length)
        self._pfx_tokens: list[int] | None = None
        self.prefix_hits = 0  # prompts admitted with their prefix taken from the store
        self.prefix_rows_skipped = 0  # prefill rows those prompts did not run
        self.prefix_prompts = 0  # prompts admitted while a prefix was set (hit rate = hits / prompts)
        # decode attention launches, issued or captured, that read the shared keys from the store
        # (wave / persistent kernels on a bf16 cache; every other path reads the slots' copies)
        self.prefix_decode_launches = 0
        self.prefix_decode = os.environ.get("DLMS_PREFIX_DECODE", "1") != "0"
        self.use_graph = use_graph
        self.prefill_split = prefill_split
        self.check_every = check_every
        if overlap is None:
            overlap = os.environ.get("DLMS_OVERLAP", "1") != "0"
        self.overlap = bool(overlap)
        self.overlap_min_batch = max(2, int(os.environ.get("DLMS_OVERLAP_MIN_BATCH", overlap_min_batch)))
        # split-K cap of the row-parallel projections when row parts run concurrently: in situ at 1024
        # queries, cap 2 beats the isolated-kernel heuristic's 4-8 slices by 4-6 % (fewer partial
        # slabs for the add+LayerNorm to re-read while the other part streams its KV cache); single-
        # stream batches keep the heuristic (cap 2 costs 3 % at 256, 8 % at 64).
        # profiles/r1_split_cap_insitu.log; DLMS_OVERLAP_SPLIT_CAP overrides.
        self.overlap_split_cap = int(os.environ.get("DLMS_OVERLAP_SPLIT_CAP", "2"))
        self.gemm96 = os.environ.get("DLMS_GEMM96", "1") != "0"  # gemm.hip gemm96_on(): same switch
        # DLMS_TIMING_SKIP=attn|gemm|ln: TIMING-ONLY differential experiment (tokens are garbage): drop
        # the decode attention, the GEMM-side kernels (LN + GEMMs) or only the LayerNorms from every
        # decode step to see which side bounds it
        # per-part form "p0:attn+p1:gemm" (mode all = attention + GEMM side)
        self._timing_skip = os.environ.get("DLMS_TIMING_SKIP", "")
        self._timing_skip_part = {}
        for item in self._timing_skip.replace("+", ",").split(","):
            if item.startswith("p") and ":" in item:
                i, m = item[1:].split(":", 1)
                self._timing_skip_part[int(i)] = m
        self.overlap_parts = int(os.environ.get("DLMS_OVERLAP_PARTS", "2")) if overlap_parts is None else overlap_parts
        # decode steps per graph replay in the overlapped step: the row parts run that many steps each
        # on their own stream before joining (rows are independent sequences), so a part that gets
        # ahead is not held back at every step's join.  1024 queries, one box: 1 step 683 / 682 k
        # tok/s, 2 steps 697 k, 4 steps 698 / 696 k, 16 steps 698 k (profiles/r2_sweep_steps_per_graph.jsonl);
        # with the 768-block persistent attention 8 steps: decode 156.9 vs 157.9 ms at 4
        self.steps_per_graph = max(1, int(os.environ.get("DLMS_STEPS_PER_GRAPH", "8")))
        # the same for every other decode step shape (latency path, tiled single-stream step): one
        # replay per this many steps (fewer graph launches between dependent steps): batch 1
        # 32.6-32.8 -> 32.2 ms, batch 2 35.0 -> 34.5, batch 32 57.3 -> 55.5 (r2_sweep_steps_per_graph.jsonl)
        self.steps_per_graph_small = max(1, int(os.environ.get("DLMS_STEPS_PER_GRAPH_SMALL", "4")))
        # overlapped step's attention: persistent grid of this many 4-wave workgroups (0 = one wave
        # per (row, head) pair).  With one join per step it measured noise (profiles/r2_sweep_persist.jsonl);
        # with the row parts running 4 steps between joins, 512 blocks leave the other part's GEMMs
        # wave slots: 682.7 / 684.5 -> 691.5 / 691.1 k tok/s on one box; decode ms per generation over
        # three boxes: 256 blocks 169.2, 512 158.8, 768 157.9, 1024 160.1 (r2_sweep_persist_multistep.jsonl)
        self.persist_attn_blocks = int(os.environ.get("DLMS_PERSIST_ATTN_BLOCKS", "768"))
        # (measured and removed: a skinny MFMA LM head at B <= 8, neutral at batch 1, and ln_f fused
        # into it, 37.3 vs 35.9 ms per query -- profiles/r2_lm_head_b1.txt)
        # (measured and removed in round 5: the LayerNorms of the overlapped step folded into the GEMMs --
        # residual projections reducing their split-K slices in-kernel, QKV / c_fc applying the LN
        # algebraically -- 632-703 vs 718-721 k tok/s, profiles/r5_ln_fold_ab.jsonl; commit 9235466)
        # (measured and removed: 16-32 rows as latency-path parts on several HIP streams, slower than
        # the tiled step -- profiles/r2_sweep_small_overlap.jsonl)
        self.prefill_graphs = os.environ.get("DLMS_PREFILL_GRAPH", "1") != "0"
        self._pgraphs: dict[tuple[int, int], dict] = {}
        self._pseen: dict[tuple[int, int], int] = {}
        if self.overlap_parts not in (2, 3, 4):
            raise ValueError("overlap_parts: 2, 3 or 4 (one hardware queue each)")
        # fp8 cache: the latency-shaped kernels (skinny / mid QKV scatter, split attention, fused
        # attention + out-projection; the fused MLP never touches the cache) have e4m3-cache builds,
        # but only an explicit ``latency_path=True`` turns them on -- the default engine keeps
        # running the tiled step at every batch size
        self.kv_fp8_latency = self.kv_fp8 and latency_path is True
        if latency_path is None:
            latency_path = os.environ.get("DLMS_LATENCY_PATH", "1") != "0"
        if self.kv_fp8 and not self.kv_fp8_latency:
            latency_path = False
        # (fp8 engines too: the latency path runs the bf16 weights the fp8 engine keeps beside its e4m3
        # copies -- at <= 8 rows the decode is bound by launch and dependency latency, not weight bytes;
        # W8A8 serves the prefill and the larger batches, where the weight stream matters)
        self.small_max = ops.skinny_addln_max_rows(cfg.n_embd) if latency_path else 0
        # the mid path (below) serves 3+ rows faster than the fused add+LN latency path: batch 4
        # 35.9 vs 37.7 ms per query, batch 8 37.3 vs 41.0; batch 2 stays here (34.1 vs 35.2, the fused
        # MLP) -- profiles/r6_mid_sweep.jsonl.  DLMS_SMALL_MAX_ROWS moves the boundary.
        if latency_path and self.tp_size == 1 and ops.mid_max_rows(cfg.n_embd) and \
                os.environ.get("DLMS_MID_PATH", "1") != "0":
            self.small_max = min(self.small_max, int(os.environ.get("DLMS_SMALL_MAX_ROWS", "2")))
        inplace_ok = self.tp_size == 1 and os.environ.get("DLMS_SMALL_INPLACE", "1") != "0"
        if self.tp_size == 1 and not inplace_ok and \
                any((k // 64) % self.SMALL_SPLIT for k in (self.w.d_local, self.w.ffn_local)):
            # the fused add+LN kernel sums exactly SMALL_SPLIT slabs (tiny test models; GPT-2-XL's 25
            # heads) -- only without the in-place projections, which leave no slabs to sum
            self.small_max = 0
        if self.small_max:
            for lw in self.w.layers:  # MFMA-fragment-order copies of the QKV / c_fc weights
                if lw.w_qkv_sh is None:
                    lw.w_qkv_sh = ops.shuffle_weight(lw.w_qkv)
                    lw.w_fc_sh = ops.shuffle_weight(lw.w_fc)
        # latency path, TP=1: out-proj / c_proj as skinny MFMA GEMMs adding into the residual in
        # place (pre-shuffled W_o / W_proj copies)
        self.small_inplace = (self.small_max > 0 and self.tp_size == 1 and
                              os.environ.get("DLMS_SMALL_INPLACE", "1") != "0")
        if self.small_inplace:
            for lw in self.w.layers:
                if lw.w_p_sh is None:
                    lw.w_p_sh = ops.shuffle_weight(lw.w_p)
                if lw.w_o_sh is None:
                    lw.w_o_sh = ops.shuffle_weight(lw.w_o)
        # mid-batch path (TP=1): decode buckets of small_max < B <= mid_max rows (9-32 for GPT-2
        # small / medium: BASELINE config 2's 32 students) run five kernels per layer instead of the
        # tiled step's seven -- [LN1 + QKV] -> split attention -> out-projection adding into the
        # residual in place -> [LN2 + c_fc + GELU] -> c_proj in place (ops/csrc/mid.hip: the
        # residual is complete whenever a LayerNorm needs it, so it runs in the GEMM's prologue and
        # no add+LN kernels or split-K slabs remain).  DLMS_MID_PATH=0: off.
        # fp8 cache (latency_path=True): up to 32 rows by default.  The fp8 tiled step is faster than
        # the bf16 one, and at the 48- and 64-row buckets it beats the mid path: 48.24 vs 48.67 ms and
        # 49.40 vs 49.84 ms per 32 -> 150 generation (run-to-run spread 0.14 / 0.35 ms), against 47.77
        # vs 43.22 ms at 32 rows -- profiles/r11_kv_fp8_latency.jsonl.  DLMS_MID_MAX_ROWS overrides.
        self.mid_max = 0
        if self.small_inplace and os.environ.get("DLMS_MID_PATH", "1") != "0":
            self.mid_max = min(ops.mid_max_rows(cfg.n_embd),
                               int(os.environ.get("DLMS_MID_MAX_ROWS", "32" if self.kv_fp8 else "64")))
        # attention fused with the out-projection for <= 4 rows (one launch fewer per layer); its
        # workgroups recompute a head's attention, so only for short caches
        # (TP=1: its per-head slabs are summed by the next fused add+LN kernel, 12 or 16 of them)
        # (GPT-2-large / XL's 20 / 25 heads in groups of 5 -- 2 waves per head, 4 / 5 slabs for the fused
        # MLP -- measured slower than split attention + the in-place out-projection: large 131-135 vs
        # 128 ms, XL 226-228 vs 211-212 ms per query, profiles/r5_large_xl_hg5_tiles_ab.jsonl; removed)
        self.fuse_ao = (self.small_max > 0 and self.tp_size == 1 and self.max_length <= 512 and
                        self.w.n_heads_local in (12, 16) and cfg.n_embd <= 1024 and
                        os.environ.get("DLMS_FUSE_ATTN_OPROJ", "1") != "0")
        if self.fuse_ao:
            try:
                ops.attention_oproj_tiles(cfg.n_embd)
            except ValueError:
                self.fuse_ao = False
        self.ao_parts = None
        if self.fuse_ao:
            for lw in self.w.layers:
                if lw.w_o_sh is None:
                    lw.w_o_sh = ops.shuffle_weight(lw.w_o)
            self.ao_parts = torch.zeros(self.w.n_heads_local, 4, cfg.n_embd, dtype=torch.float32, device=self.device)
        # batch 1: head groups of H/4 (3 or 4 heads) -> 4 slabs, 3 W_o tiles per workgroup
        # (profiles/r2_attn_oproj_ab.txt: 36.6 vs 37.1 ms per query with one slab per head)
        Hl = self.w.n_heads_local
        self.ao_groups = Hl // 4 if (self.fuse_ao and Hl % 4 == 0 and Hl // 4 in (3, 4)) else 0
        self.ao_group_tiles = 3 if (cfg.n_embd // 16) % 3 == 0 else 1
        self.ao_slabs = Hl // self.ao_groups if self.ao_groups else 0
        # batch 1 (TP=1, head-grouped attention): LN2 -> c_fc -> GELU -> c_proj as ONE kernel whose
        # workgroups add their 16-column slices into an int64 fixed-point residual (order-independent
        # integer atomics; ops.skinny_mlp) -- one launch and one dependent round trip fewer per layer
        # (any width the kernel takes: batch 1 without head groups -- GPT-2-large/XL's 20 / 25 heads --
        # runs split attention + the in-place out-projection into the fixed-point residual first)
        self.fused_mlp = (self.small_inplace and cfg.n_embd in ops.SKINNY_MLP_WIDTHS and
                          self.w.ffn_local == 4 * cfg.n_embd and os.environ.get("DLMS_FUSED_MLP", "1") != "0")
        # ... and up to this many rows (2-8: split attention + in-place out-projection into the
        # fixed-point residual; each row adds 6 KB of atomics per MLP workgroup)
        self.fused_mlp_rows = int(os.environ.get("DLMS_FUSED_MLP_ROWS", "2")) if self.fused_mlp else 0
        if self.fused_mlp:
            for lw in self.w.layers:
                if lw.w_p_sl is None:
                    lw.w_p_sl = ops.slice_cproj(lw.w_p)
        # TP > 1, the latency path (<= tp_fused_rows rows): every rank runs a layer as six kernels --
        # [LN1 + QKV of its heads] -> attention -> [out-projection partial] -> xGMI all-reduce ->
        # [+ attention + b_o, LN2, c_fc shard, GELU, c_proj slice into an int64 fixed-point
        # accumulator; rank 0 also adds the residual + b_p] -> integer xGMI all-reduce, which IS the
        # next residual on every rank (exact, order-independent) -- against eight launch-per-op
        # kernels (separate c_fc and c_proj, two split partial slabs to sum).  DLMS_TP_FUSED=0: off.
        self.tp_fused = (self.tp_size > 1 and self.small_max > 0 and
                         cfg.n_embd in ops.SKINNY_MLP_WIDTHS and self.w.ffn_local % 16 == 0 and
                         os.environ.get("DLMS_TP_FUSED", "1") != "0")
        self.tp_fused_steps = 0
        self.tp_fused_rows = min(self.small_max, int(os.environ.get("DLMS_TP_FUSED_ROWS", "4"))) if self.tp_fused else 0
        if self.tp_fused:
            for lw in self.w.layers:
                if lw.w_o_sh is None:
                    lw.w_o_sh = ops.shuffle_weight(lw.w_o)
                if lw.w_p_sl is None:
                    lw.w_p_sl = ops.slice_cproj(lw.w_p)
        # LM head of the throughput path (>= PS_LM_MIN_ROWS rows): panel-resident gemm_ps on a
        # pre-shuffled copy of the (tied) LM-head shard: 67 vs 87 us at 512 rows, 114 vs 146 at 1024
        # (profiles/r2_gemm_ps_vs_tiled.log)
        self.lm_head_sh = None
        # (only where its 64-row panel fits in LDS, i.e. GPT-2-small: with 32-row panels GPT-2-medium
        # ran 254.8 k tok/s against 279.9 k on the tiled LM head; XL's K = 1600 is not a multiple of
        # its 128-deep register chunks either)
        ps_lm = (self.max_batch >= self.PS_LM_MIN_ROWS and cfg.n_embd % 128 == 0 and
                 64 * (2 * cfg.n_embd + 32) + 8 * 4096 <= ops.PS_LDS_BYTES and
                 os.environ.get("DLMS_PS_LMHEAD", "1") != "0")
        self.ps_lm = ps_lm and not self.w.fp8
        if self.ps_lm:
            self.lm_head_sh = ops.shuffle_weight(self.w.lm_head)
        # batch 1 (TP=1, bf16): the persistent dataflow decode -- one launch per chunk of decode steps
        # (ops/dataflow.py); built on first use (it packs a per-CU copy of the weights).  Default ON
        # at one row for the widths where it was measured faster: GPT-2-124M 29.9-30.3 vs 31.6 ms per
        # query launch-per-op (profiles/r3_df_sweep_grid200.jsonl), GPT-2-medium 73.5 vs 76.9 ms
        # (r3_df_medium_b1.jsonl, same tokens); at two rows it is slower (58.9 vs 34.9 ms,
        # r3_df_sweep_fine.jsonl).  DLMS_DATAFLOW=1 forces it on for every supported width,
        # DLMS_DATAFLOW_ROWS (1 or 2) the row counts it serves, DLMS_DATAFLOW=0 turns it off.
        df_env = os.environ.get("DLMS_DATAFLOW", "auto")
        self.dataflow_rows = max(1, min(2, int(os.environ.get("DLMS_DATAFLOW_ROWS", "1"))))
        self.dataflow = (df_env != "0" and tp_group is None and not self.w.fp8 and not self.kv_fp8 and
                         (df_env == "1" or cfg.n_embd in (768, 1024)) and self._df_supported())
        self._df = None
        self._df_status = None  # the last decode() launch's error words in flight (dataflow_status_async)
        self._df_off_until = 0.0  # after an aborted launch: launch-per-op until then (DLMS_DF_COOLDOWN_S)
        self.df_aborts = 0
        self.df_aborts_beside_side_work = 0  # of those, aborts while a registered side stream was busy
        self._side_streams: list[torch.cuda.Stream] = []
        self._flags: torch.Tensor | None = None
        self._graphs: dict[tuple, torch.cuda.CUDAGraph] = {}
        # the generation mode of the public call in progress (_mode_scope; the default: greedy), and
        # what the modes need, allocated on the first call that needs it (_alloc_for): the f32 logits
        # scratch of the sampled LM head, every slot's prompt length, the device tables of the stop
        # sequences seen, the chosen tokens' log-probabilities [slot][position]
        self._mode = DecodeMode()
        self._logits: torch.Tensor | None = None
        self.prompt_len: torch.Tensor | None = None
        self._stop_tables: dict[tuple, tuple[torch.Tensor, torch.Tensor]] = {}
        self.out_logprob: torch.Tensor | None = None
        self._rng_seed_host: int | None = None  # the seed in rng_seed (None: never set)
        self._rng_count = 0  # requests admitted since the seed was last set: the next stream id
        self._alloc_state()
        self.xgmi = None
        if self.tp_size > 1:
            import torch.distributed as dist

            if p2p is None:
                p2p = dist.get_backend(tp_group) == "nccl" and os.environ.get("DLMS_XGMI", "1") != "0"
            if p2p:
                from ..parallel.xgmi import XgmiComm

                # decode messages; big prefills: RCCL (DLMS_XGMI_SLAB_MB: a larger slab keeps packed
                # prefills on the one-shot kernels too -- the shared-GPU tests, whose group is gloo)
                slab = max(self.max_batch * cfg.n_embd * 4, int(float(os.environ.get("DLMS_XGMI_SLAB_MB", "1")) * (1 << 20)))
                self.xgmi = XgmiComm(tp_group, self.device, slab)

    # ------------------------------------------------------------------ state
    def _alloc_state(self):
        cfg, B, dev = self.cfg, self.max_batch, self.device
        D, Dl, Fl, Hl = cfg.n_embd, self.w.d_local, self.w.ffn_local, self.w.n_heads_local
        T = self.max_length
        i32, f32, bf = torch.int32, torch.float32, torch.bfloat16
        # KV cache [L][2][slots][H_local][T][64]: sized for the batch at full length.
        # (kv_dtype="fp8": the same shape in e4m3 bytes, 64-B key rows; zero bytes are +0.0)
        self.kv = torch.zeros(cfg.n_layer, 2, B, Hl, T, 64, dtype=ops.FP8 if self.kv_fp8 else bf, device=dev)
        self.x = torch.zeros(B, D, dtype=f32, device=dev)
        # second residual buffer: the latency path's fused add+LN kernels advance x by ping-pong
        self.x2 = torch.zeros(min(B, 64), D, dtype=f32, device=dev)
        # the fused MLP's ping-pong int64 fixed-point residual (batch 1)
        xr_rows = max(self.fused_mlp_rows, self.tp_fused_rows)
        self.xr = (torch.zeros(2, ops.fix_copies(), max(1, min(xr_rows, B)), D, dtype=torch.int64, device=dev)
                   if (self.fused_mlp or self.tp_fused) else None)
        # cross-workgroup split attention (few rows, long caches): partials + arrival counters
        self.attn_ws = ops.AttnSplitWorkspace(self.SPLIT_ATTN_MAX_PAIRS, 2, dev)
        self.parts = torch.zeros(8, B, D, dtype=f32, device=dev)  # split-K / TP partial slabs
        self.h = torch.zeros(B, D, dtype=bf, device=dev)
        self.q = torch.zeros(B, Dl, dtype=bf, device=dev)
        self.att = torch.zeros(B, Dl, dtype=bf, device=dev)
        self.ff = torch.zeros(B, Fl, dtype=bf, device=dev)
        self.h8 = self.hsc = None
        if self.w.fp8:  # row-scaled e4m3 LayerNorm outputs (K zero-padded to the fp8 ring step)
            self.h8 = torch.zeros(B, self.w.k_fp8, dtype=ops.FP8, device=dev)
            self.hsc = torch.ones(B, dtype=f32, device=dev)
        # LM-head argmax partial keys: one per (row, 64-column group) of this rank's vocab shard;
        # zero-initialised once (columns a 128-wide tile never writes stay at the minimum key)
        self.key_parts = torch.zeros(B, self.w.lm_head.shape[0] // 64, dtype=torch.int64, device=dev)
        self.local_keys = torch.zeros(B, dtype=torch.int64, device=dev)
        self.all_keys = torch.zeros(self.tp_size, B, dtype=torch.int64, device=dev)
        self.lens = torch.ones(B, dtype=i32, device=dev)  # every slot starts inert (see _reset_slots)
        self.finished = torch.ones(B, dtype=i32, device=dev)
        self.out_tokens = torch.zeros(B, T, dtype=i32, device=dev)
        self.seen_words = cfg.vocab_padded // 32
        self.seen = torch.zeros(B, self.seen_words, dtype=i32, device=dev)
        self.cur_tok = torch.zeros(B, dtype=i32, device=dev)
        self.cur_pos = torch.zeros(B, dtype=i32, device=dev)
        self.cur_kvlen = torch.ones(B, dtype=i32, device=dev)
        self.slots = torch.arange(B, dtype=i32, device=dev)
        # sampler RNG state, on the device so that graph replays do not bake it in: the seed word
        # and every slot's request stream id (written at admission)
        self.rng_seed = torch.zeros(1, dtype=torch.int64, device=dev)
        self.rng_stream = torch.zeros(B, dtype=torch.int64, device=dev)
        # prompt-prefix cache: the store [L][2][H_local][capacity][64] in the cache's dtype, every
        # slot's count of leading keys that came from it, and the prefix's tokens and seen-bitmap
        # row -- all at fixed addresses for the engine's life, so captured prefills stay valid when
        # the prefix is replaced
        self.pfx_store = self.slot_pfx = self._pfx_tok_d = self._pfx_seen = None
        if self.prefix_capacity:
            C = self.prefix_capacity
            self.pfx_store = torch.zeros(cfg.n_layer, 2, Hl, C, 64, dtype=self.kv.dtype, device=dev)
            self.slot_pfx = torch.zeros(B, dtype=i32, device=dev)
            self._pfx_tok_d = torch.zeros(C, dtype=i32, device=dev)
            self._pfx_seen = torch.zeros(self.seen_words, dtype=i32, device=dev)
        self._reset_slots(0, B)

    def kv_cache_bytes(self) -> int:
        n = self.kv.numel() * self.kv.element_size()
        if self.pfx_store is not None:
            n += self.pfx_store.numel() * self.pfx_store.element_size()
        return n

    # ------------------------------------------------------------------ collectives
    def _all_reduce(self, t: torch.Tensor):
        if self.tp_size > 1:
            import torch.distributed as dist

            if self.xgmi is not None and self.xgmi.fits(t):
                self.xgmi.all_reduce_(t)
            else:
                dist.all_reduce(t, group=self.tp_group)

    def _all_reduce_i64(self, t: torch.Tensor):
        """Integer all-reduce of a contiguous int64 tensor (the TP fused layer's fixed point)."""
        import torch.distributed as dist

        if self.xgmi is not None and self.xgmi.fits(t):
            self.xgmi.all_reduce_i64_(t)
        else:
            dist.all_reduce(t, group=self.tp_group)

    def _gather_keys(self, B: int, P: int) -> torch.Tensor:
        """Argmax keys as a [B, P] view: the LM head's per-tile partials (TP=1), or one reduced key
        per vocab shard after an all-gather of 8 B per row per rank (TP>1)."""
        if self.tp_size > 1:
            import torch.distributed as dist

            ops.argmax_reduce(self.key_parts[:B, :P], out=self.local_keys[:B])
            flat = self.all_keys.view(-1)[: self.tp_size * B]
            if self.xgmi is not None:
                self.xgmi.all_gather_u64(self.local_keys[:B], flat.view(self.tp_size, B))
            elif dist.get_backend(self.tp_group) == "nccl":
                dist.all_gather_into_tensor(flat, self.local_keys[:B], group=self.tp_group)
            else:  # gloo (functional TP tests on one GPU): list all-gather, eager only
                parts = list(flat.view(self.tp_size, B).unbind(0))
                dist.all_gather(parts, self.local_keys[:B].clone(), group=self.tp_group)
                for i, p in enumerate(parts):
                    flat.view(self.tp_size, B)[i].copy_(p)
            return flat.view(self.tp_size, B).t()
        return self.key_parts[:B, :P]

    # ------------------------------------------------------------------ transformer body
    def _split(self, M: int, N: int, K: int, cap: int = 8) -> int:
        """Split-K factor for a row-parallel projection (N = d): slice K until the grid covers the
        CUs (<= 1024 workgroups), keeping >= 3 K-steps per slice (>= 6 above M = 512, where the
        extra partial slabs the add+LayerNorm re-reads start to cost).  Fit to the cold-weight tile
        sweep (profiles/r1_gemm_tile_sweep_cold.jsonl): M=256 c_proj split 8 6.8 us vs unsplit
        15.9 us; M=1024 split 4 12.9 us vs 17.1 us."""
        if self.tp_size > 1:
            return 1
        bm = 32 if M <= 64 else 64
        tiles = -(-M // bm) * (N // 64)
        ksteps = K // 64
        min_steps = 3 if M <= 512 else 6
        best = 1
        for s in (2, 3, 4, 6, 8):
            if s > cap:
                break
            if ksteps % s == 0 and tiles * s <= 1024 and ksteps // s >= min_steps:
                best = s
        return best

    def _row_parallel(self, a: torch.Tensor, w: torch.Tensor, bias, parts: torch.Tensor, M: int, cap: int = 8,
                      fixed: int | None = None):
        """out-proj / c_proj: split-K (TP=1) or TP partial + all-reduce.  Returns the pending
        residual update (parts, nsplit, bias) that the next fused add+LayerNorm applies."""
        if self.tp_size > 1:
            ops.gemm(a, w, ops.EPI_PARTIAL, out=parts, split_k=1)
            self._all_reduce(parts[0, :M])
            return parts, 1, bias
        if fixed:
            s = max(d for d in range(1, fixed + 1) if (w.shape[1] // 64) % d == 0)
        elif M >= 16384 and w.shape[1] >= 3072 and w.shape[0] % 256 == 0 and parts.shape[0] >= 2:
            # packed-prefill c_proj: split 2 -> 768 256x256 tiles on the 8-phase GEMM, three full
            # rounds of workgroups instead of 1.5 (prefill 10.9-11.8 -> 10.7-11.4 ms per 1024-query
            # generation, profiles/r5_prefill_cproj_split2_ab.jsonl)
            s = 2
        elif self.gemm96 and 256 < M <= 512 and w.shape[1] >= 2048 and w.shape[0] % 96 == 0 and \
                (w.shape[1] // 64) % 4 == 0:
            # c_proj on a 512-row decode half: split 4 -> 64x96 tiles in one round of 256 workgroups
            # (the launcher's DLMS_GEMM96 rule): 10.5 -> 8.5 us alone, profiles/r3_kern_sweep_m512.jsonl
            s = 4
        else:
            s = self._split(M, w.shape[0], w.shape[1], cap)
        ops.gemm(a, w, ops.EPI_PARTIAL, out=parts, split_k=s)
        return parts, s, bias

    def _rows(self, x: torch.Tensor, parts: torch.Tensor, h, q, att, ff, row_slot, row_pos, row_kvlen, M: int,
              h8: torch.Tensor | None = None, hsc: torch.Tensor | None = None,
              tiles: "ops.AttnTiles | None" = None) -> "_Rows":
        """Bundle the activation buffers of one row range for the per-layer phase functions (fp8
        engines: the e4m3 LayerNorm outputs when ``h8`` is given -- the latency path runs bf16)."""
        fp8 = self.w.fp8 and h8 is not None
        r = _Rows(x=x[:M], parts=parts, h=h[:M], q=q[:M], att=att[:M], ff=ff[:M], row_slot=row_slot,
                  row_pos=row_pos, row_kvlen=row_kvlen, M=M, h8=h8[:M] if fp8 else None,
                  hsc=hsc[:M] if fp8 else None, tiles=tiles)
        r.ln_out = (dict(out_bf16=None, want_out=False, out_fp8=r.h8, out_fp8_scale=r.hsc) if fp8
                    else dict(out_bf16=r.h))
        return r

    def _attn_in(self, r: "_Rows", li: int, ln_done: bool = False):
        """LN1 (folding the pending residual update) -> QKV GEMM (+ K/V scattered into the cache).
        ``ln_done``: r.h already holds LN1 of the row (layer 0 after a fused ``decode_update``)."""
        if self._skip(r) in ("gemm", "ln", "all"):  # timing-only experiment: see __init__
            if self._skip(r) == "ln":
                self._attn_in_gemm_only(r, li)
            return
        lw, eps, pend = self.w.layers[li], self.cfg.layer_norm_epsilon, r.pend
        kc, vc = self.kv[li, 0], self.kv[li, 1]
        if not ln_done:
            ops.add_layernorm(r.x, lw.ln1_g, lw.ln1_b, eps, parts=pend[0], nsplit=pend[1], bias=pend[2], **r.ln_out)
        if self.w.fp8:
            ops.gemm(r.h8, lw.w_qkv8, ops.EPI_QKV, bias=lw.b_qkv, q_out=r.q, k_cache=kc, v_cache=vc,
                     row_slot=r.row_slot, row_pos=r.row_pos, a_scale=r.hsc, w_scale=lw.s_qkv)
        else:
            ops.gemm(r.h, lw.w_qkv, ops.EPI_QKV, bias=lw.b_qkv, q_out=r.q, k_cache=kc, v_cache=vc,
                     row_slot=r.row_slot, row_pos=r.row_pos)

    def _skip(self, r: "_Rows") -> str:
        """Timing-only skip mode for this row range (DLMS_TIMING_SKIP; never set in production)."""
        if not self._timing_skip or r.tiles is not None:
            return ""
        return self._timing_skip_part.get(r.pidx, "") if self._timing_skip_part else self._timing_skip

    def _attn_in_gemm_only(self, r: "_Rows", li: int):
        lw = self.w.layers[li]
        ops.gemm(r.h, lw.w_qkv, ops.EPI_QKV, bias=lw.b_qkv, q_out=r.q, k_cache=self.kv[li, 0], v_cache=self.kv[li, 1],
                 row_slot=r.row_slot, row_pos=r.row_pos)

    def _attn(self, r: "_Rows", li: int):
        if self._skip(r) in ("attn", "all"):  # timing-only experiment: see __init__
            return
        if r.tiles is not None:  # packed prompts (K6): 16-query MFMA tiles
            ops.tile_attention(r.q, self.kv[li, 0], self.kv[li, 1], r.row_slot, r.row_kvlen, r.tiles, out=r.att)
        elif r.M * self.w.n_heads_local <= self.SPLIT_ATTN_MAX_PAIRS and (not self.kv_fp8 or self.kv_fp8_latency):
            # decode with few (row, head) pairs: split-K flash-decode puts NW waves on each pair's keys
            nw, ns = ops.attention_split_geometry(r.M * self.w.n_heads_local, self.max_length)
            ops.attention_split(r.q, self.kv[li, 0], self.kv[li, 1], r.row_slot, r.row_kvlen, out=r.att,
                                waves=nw, splits=ns, workspace=self.attn_ws if ns > 1 else None)
        elif r.persist_attn:
            # overlapped step: a fixed low-occupancy grid leaves wave slots to the other half's GEMMs
            ops.row_attention(r.q, self.kv[li, 0], self.kv[li, 1], r.row_slot, r.row_kvlen, out=r.att,
                              impl="persist", blocks=self.persist_attn_blocks, prefix=self._attn_prefix(li))
        else:  # decode (K5): one query per sequence, a pure KV stream
            ops.row_attention(r.q, self.kv[li, 0], self.kv[li, 1], r.row_slot, r.row_kvlen, out=r.att,
                              prefix=self._attn_prefix(li))

    def _pfx_decode(self) -> bool:
        """The wave / persistent decode attention reads the slots' shared leading keys from the
        prefix store (a prefix is set, bf16 cache; ``DLMS_PREFIX_DECODE=0``: from the slots, which
        hold the same bytes -- the A/B switch of scripts/bench_prefix.py)."""
        return self._pfx_tokens is not None and not self.kv_fp8 and self.prefix_decode

    def _attn_prefix(self, li: int):
        if not self._pfx_decode():
            return None
        self.prefix_decode_launches += 1  # (issued or captured: a graph replay does not count again)
        return self.pfx_store[li, 0], self.pfx_store[li, 1], self.slot_pfx

    def _attn_out_mlp(self, r: "_Rows", li: int):
        """out-proj -> LN2 -> c_fc + GELU -> c_proj; leaves c_proj's residual update pending."""
        if self._skip(r) in ("gemm", "ln", "all"):  # timing-only experiment: see __init__
            if self._skip(r) == "ln":
                lw = self.w.layers[li]
                r.pend = self._row_parallel(r.att, lw.w_o, lw.b_o, r.parts, r.M, r.split_cap, r.split_fixed)
                ops.gemm(r.h, lw.w_fc, ops.EPI_GELU_TANH, bias=lw.b_fc, out=r.ff)
                r.pend = self._row_parallel(r.ff, lw.w_p, lw.b_p, r.parts, r.M, r.split_cap, r.split_fixed)
            return
        lw, eps = self.w.layers[li], self.cfg.layer_norm_epsilon
        pend = self._row_parallel(r.att, lw.w_o, lw.b_o, r.parts, r.M, r.split_cap, r.split_fixed)
        ops.add_layernorm(r.x, lw.ln2_g, lw.ln2_b, eps, parts=pend[0], nsplit=pend[1], bias=pend[2], **r.ln_out)
        if self.w.fp8:
            ops.gemm(r.h8, lw.w_fc8, ops.EPI_GELU_TANH, bias=lw.b_fc, out=r.ff, a_scale=r.hsc, w_scale=lw.s_fc)
        else:
            ops.gemm(r.h, lw.w_fc, ops.EPI_GELU_TANH, bias=lw.b_fc, out=r.ff)
        r.pend = self._row_parallel(r.ff, lw.w_p, lw.b_p, r.parts, r.M, r.split_cap, r.split_fixed)

    def _final_ln(self, r: "_Rows", final_h: torch.Tensor | None):
        w, eps, pend = self.w, self.cfg.layer_norm_epsilon, r.pend
        if w.fp8:
            fin = r.ln_out if final_h is not None else dict(want_out=False)
            ops.add_layernorm(r.x, w.lnf_g, w.lnf_b, eps, parts=pend[0], nsplit=pend[1], bias=pend[2], **fin)
        else:
            ops.add_layernorm(r.x, w.lnf_g, w.lnf_b, eps, parts=pend[0], nsplit=pend[1], bias=pend[2],
                              out_bf16=final_h, want_out=final_h is not None)

    def _layers(self, x: torch.Tensor, parts: torch.Tensor, h, q, att, ff, row_slot, row_pos, row_kvlen, M: int,
                final_h: torch.Tensor | None, h8: torch.Tensor | None = None, hsc: torch.Tensor | None = None,
                tiles: "ops.AttnTiles | None" = None, ln0_done: bool = False):
        """All blocks on rows [0, M) of the residual ``x`` (updated in place), then ln_f into
        ``final_h`` (or only the last residual update when ``final_h`` is None).  fp8 weights: the
        LayerNorms emit row-scaled e4m3 into ``h8``/``hsc`` for the W8A8 QKV / c_fc GEMMs, and the
        ln_f output goes there too (``final_h`` then only says whether it is wanted).  ``ln0_done``:
        h already holds layer 0's LN1 (fused ``decode_update``)."""
        r = self._rows(x, parts, h, q, att, ff, row_slot, row_pos, row_kvlen, M, h8, hsc, tiles)
        if tiles is not None:
            r.split_fixed = self.prefill_split
        for li in range(len(self.w.layers)):
            self._attn_in(r, li, ln_done=li == 0 and ln0_done)
            self._attn(r, li)
            self._attn_out_mlp(r, li)
        self._final_ln(r, final_h)

    def _lm_head_and_update(self, hidden: torch.Tensor | None, B: int, penalty: float, seen: torch.Tensor | None = None,
                            hscale: torch.Tensor | None = None, slot_map: torch.Tensor | None = None, lo: int = 0,
                            ln1_out: torch.Tensor | None = None):
        """LM head with the fused penalty + argmax on ``hidden`` (bf16, or e4m3 with ``hscale``) --
        in a mode with a ``sampler``: f32 logits, the bans, the device sampler and the chosen token's
        log-probability instead -- then the bookkeeping of the chosen token.  Rows map to slots
        [lo, lo + B) or through ``slot_map``.  ``ln1_out`` (rows [lo, lo + B), never with a slot
        map): the update also writes layer 0's LN1 of the new rows there."""
        cfg, mode = self.cfg, self._mode
        hi = lo + B

        def rows(t):  # per-slot state as the kernels take it: the rows' slots, or all of them under a slot map
            return t[lo:hi] if slot_map is None else t

        seen_rows = self.seen[lo:hi] if seen is None else seen
        kp = self.key_parts[lo:hi]
        P = self.key_parts.shape[1]  # partial keys per row the LM head writes (and the consumer reads)
        sp = mode.sampler
        if sp is not None:
            # raw f32 logits (the GEMMs' plain f32 epilogues; the penalty moves into the sampler),
            # then one drawn key per row in the first key column
            if hidden.dtype == ops.FP8 or self._logits is None:
                raise ValueError("sampled LM head: bf16 hidden rows inside a _mode_scope")
            z = self._logits[lo:hi]
            if self.ps_lm and B >= self.PS_LM_MIN_ROWS:
                ops.gemm_ps(hidden, self.lm_head_sh, ops.EPI_PARTIAL, out=z.unsqueeze(0), split_k=1)
            else:
                ops.gemm(hidden, self.w.lm_head, ops.EPI_F32, out=z)
            P = 1
            if mode.bans:
                # -inf at the banned tokens of every live row, between the logits and the sampler
                ops.logit_bans(z, rows(self.lens), rows(self.finished), rows(self.prompt_len), rows(self.out_tokens),
                               mode.bans.no_repeat_ngram_size, mode.bans.min_new_tokens, cfg.eos_token_id,
                               cfg.vocab_size, slot_map=slot_map)
            ops.sample_topk_topp(z, seen_rows, rows(self.lens), rows(self.rng_stream), self.rng_seed, penalty,
                                 sp.temperature, sp.top_k, sp.top_p, cfg.vocab_size, kp, slot_map=slot_map)
            if mode.logprobs:
                # the chosen token's log-probability into out_logprob[slot][lens[slot]]: behind the
                # sampler, which chose it, and ahead of the update, which advances lens
                ops.token_logprob(z, cfg.vocab_size, rows(self.out_logprob), keys=kp, seen=seen_rows,
                                  lens=rows(self.lens), finished=rows(self.finished), penalty=penalty,
                                  slot_map=slot_map)
        elif hidden.dtype != ops.FP8 and self.ps_lm and B >= self.PS_LM_MIN_ROWS:
            P = ops.gemm_ps_key_slots(B, self.lm_head_sh.shape[0] * 16, self.lm_head_sh.shape[1] * 32)
            ops.gemm_ps(hidden, self.lm_head_sh, ops.EPI_ARGMAX, argmax_out=kp, seen=seen_rows,
                        vocab=cfg.vocab_size, col_offset=self.w.vocab_range[0], penalty=penalty)
        elif hidden.dtype == ops.FP8:
            ops.gemm(hidden, self.w.lm_head8, ops.EPI_ARGMAX, argmax_out=kp, seen=seen_rows,
                     vocab=cfg.vocab_size, col_offset=self.w.vocab_range[0], penalty=penalty, a_scale=hscale,
                     w_scale=self.w.s_lm)
        else:
            ops.gemm(hidden, self.w.lm_head, ops.EPI_ARGMAX, argmax_out=kp, seen=seen_rows,
                     vocab=cfg.vocab_size, col_offset=self.w.vocab_range[0], penalty=penalty)
        if lo:
            if self.tp_size > 1:
                raise ValueError("row-offset LM head is TP=1 only")
            keys = kp[:, :P]
        else:
            keys = self._gather_keys(B, P)
        update, stop_args = ops.decode_update, ()
        if mode.stop:  # the same update, which also finishes a row at a match
            update, stop_args = ops.decode_update_stop, (rows(self.prompt_len), *self._stop_tables[mode.stop])
        l0 = self.w.layers[0]
        update(keys, rows(self.lens), rows(self.finished), rows(self.out_tokens), rows(self.seen), rows(self.cur_tok),
               rows(self.cur_pos), rows(self.cur_kvlen), self.w.wte, self.w.wpe, rows(self.x), cfg.eos_token_id,
               self.max_length, *stop_args, slot_map=slot_map,
               ln=(l0.ln1_g, l0.ln1_b, cfg.layer_norm_epsilon) if ln1_out is not None else None, h=ln1_out)

    # ------------------------------------------------------------------ generation mode
    @contextlib.contextmanager
    def _mode_scope(self, mode: DecodeMode):
        """The generation mode of one public call: every LM head, update and prefill issued (or
        captured) inside runs in it, and graphs are keyed by it.  The default mode: exactly the
        calls made before there were any."""
        mode.check(self.tp_size, self.w.fp8)
        self._alloc_for(mode)
        prev, self._mode = self._mode, mode
        try:
            yield
        finally:
            self._mode = prev

    def _alloc_for(self, mode: DecodeMode):
        """The buffers ``mode`` needs, on their first use and for the engine's life (outside any
        capture: graph pools must not own them)."""
        if mode.sampler is not None:
            self._logits_scratch()
        if mode.records_prompt_len and self.prompt_len is None:
            self.prompt_len = torch.zeros(self.max_batch, dtype=torch.int32, device=self.device)
        if mode.logprobs and self.out_logprob is None:
            self.out_logprob = torch.full((self.max_batch, self.max_length), float("nan"), dtype=torch.float32,
                                          device=self.device)
        if mode.stop and mode.stop not in self._stop_tables:
            self._stop_tables[mode.stop] = ops.stop_table(mode.stop, self.device)

    def _logits_scratch(self) -> torch.Tensor:
        """The f32 logits rows of the sampled LM head and of ``score``."""
        if self._logits is None:
            self._logits = torch.empty(self.max_batch, self.w.lm_head.shape[0], dtype=torch.float32,
                                       device=self.device)
        return self._logits

    def reseed(self, seed: int):
        """Set the sampler's seed word and restart the request count: the next request admitted
        draws from stream 0."""
        seed = int(seed)
        if not 0 <= seed < 2 ** 64:
            raise ValueError("seed: an integer in [0, 2^64)")
        self.rng_seed.fill_(seed - 2 ** 64 if seed >= 2 ** 63 else seed)  # (the int64 with the same bits)
        self._rng_seed_host, self._rng_count = seed, 0

    def _next_streams(self, n: int, sampling: "SamplingParams | None") -> list[int] | None:
        """Stream ids of the next ``n`` requests under ``sampling`` (None: greedy, no ids)."""
        if sampling is None:
            return None
        if self._rng_seed_host != sampling.seed:
            self.reseed(sampling.seed)
        first = self._rng_count
        self._rng_count += n
        return list(range(first, first + n))

    def _skey(self) -> tuple:
        """What the captured graphs depend on beyond their shapes: the generation mode, and whether
        the decode attention reads the prefix store."""
        key = self._mode.graph_key
        return key + ("pfx",) if self._pfx_decode() else key

    def _overlap_ok(self, B: int) -> bool:
        k = self.overlap_parts
        return self.overlap and self.tp_size == 1 and B >= self.overlap_min_batch and B % k == 0

    def _part_rows(self, lo: int, hi: int) -> "_Rows":
        fp8 = self.w.fp8
        r = self._rows(self.x[lo:hi], self.parts[:, lo:hi], self.h[lo:hi], self.q[lo:hi], self.att[lo:hi],
                          self.ff[lo:hi], self.slots[lo:hi], self.cur_pos[lo:hi], self.cur_kvlen[lo:hi], hi - lo,
                          self.h8[lo:hi] if fp8 else None, self.hsc[lo:hi] if fp8 else None)
        r.split_cap = self.overlap_split_cap
        r.persist_attn = self.persist_attn_blocks > 0
        r.pidx = lo // max(1, hi - lo)
        return r

    def _part_step(self, r: "_Rows", lo: int, penalty: float, h_ready: bool = False):
        """The whole decode step for one row range (rows are independent sequences).  bf16: the
        step's ``decode_update`` also writes layer 0's LN1 of the new rows into r.h, so a step that
        follows one in the same graph replay (``h_ready``) skips that launch."""
        # (decode per 1024-query generation 152.9 / 153.1 ms against 154.3 / 154.4 with the launch,
        # profiles/r5_fused_ln1_ab.jsonl; tokens bit-identical: test_kernels_gpu.py::
        # test_decode_update_fused_ln1_is_bit_identical, test_engine_gpu.py multi-step tests)
        fuse = not self.w.fp8 and not self._timing_skip
        for li in range(len(self.w.layers)):
            self._attn_in(r, li, ln_done=li == 0 and h_ready and fuse)
            self._attn(r, li)
            self._attn_out_mlp(r, li)
        self._final_ln(r, r.h)
        if self.w.fp8:
            self._lm_head_and_update(r.h8, r.M, penalty, hscale=r.hsc, lo=lo)
        else:
            self._lm_head_and_update(r.h, r.M, penalty, lo=lo, ln1_out=r.h if fuse else None)

    def _decode_step_overlap(self, B: int, penalty: float, nsteps: int = 1):
        """Decode step as ``overlap_parts`` row ranges on as many HIP streams (one hardware queue
        each), free-running: the decode GEMMs are latency-bound (a near-constant ~12 us per launch
        whatever M, profiles/r1_gemm_lab) and attention is HBM-bound, so independent row ranges
        fill each other's bubbles -- the GEMMs of one part run beside the KV stream and the GEMMs
        of the others.  Captured as one hipGraph with ``overlap_parts`` independent branches (fork
        at the start, join at the end).  (Measured and removed: the halves' GEMM phases serialised
        so attention of one always pairs with the GEMMs of the other, and the attentions forced to
        alternate on HBM -- both slower, profiles/r2_sweep_alt_attn.jsonl.)"""
        k = self.overlap_parts
        cur = torch.cuda.current_stream(self.device)
        while len(self._side_streams) < k - 1:
            self._side_streams.append(torch.cuda.Stream(device=self.device))
        streams = [cur] + self._side_streams[: k - 1]
        for s in streams[1:]:
            s.wait_stream(cur)
        step = B // k
        parts = [(i * step, self._part_rows(i * step, (i + 1) * step)) for i in range(k)]
        for (lo, r), s in zip(parts, streams):
            with torch.cuda.stream(s):
                for i in range(nsteps):
                    # (fresh row state per step: _Rows carries the residual update pending
                    # between layers, which the last layer of a step leaves set)
                    self._part_step(r if i == 0 else self._part_rows(lo, lo + step), lo, penalty, h_ready=i > 0)
        for s in streams[1:]:
            cur.wait_stream(s)

    def _df_supported(self) -> bool:
        from ..ops.dataflow import DataflowDecoder

        return DataflowDecoder.supported(self)

    def _df_ok(self, B: int) -> bool:
        from ..ops.dataflow import MAX_ROWS

        # (the launch-per-op path serves row counts whose stream window outgrows the LDS ring, and
        # every mode but the default: DecodeMode.dataflow_ok)
        return (self.dataflow and self._mode.dataflow_ok and 1 <= B <= min(MAX_ROWS, self.max_batch, self.dataflow_rows)
                and time.monotonic() >= self._df_off_until and self._df_decoder().fits(B))

    def _df_run(self, B: int, steps: int, penalty: float) -> bool:
        """Launch the dataflow decode for ``steps`` steps of rows [0, B); False (nothing ran) when
        the device cannot hold its grid at once -- the dataflow path is then off for good."""
        from ..ops.dataflow import DataflowUnavailable

        try:
            self._df_decoder().run(B, steps, penalty)
        except DataflowUnavailable as e:
            log.warning("%s: serving launch-per-op", e)
            self.dataflow = False
            return False
        return True

    def _df_note(self, st):
        """An aborted dataflow launch (error words ``st``): count it and serve launch-per-op for
        DLMS_DF_COOLDOWN_S seconds (default 30).  Nothing to repair: an aborted launch commits no
        row state (ops/csrc/dataflow.hip, commit), so whatever runs next redoes those steps."""
        from ..ops.dataflow import DataflowDecoder

        self.df_aborts += 1
        METRICS.inc("engine_dataflow_aborts")
        beside = any(not st_.query() for st_ in _SIDE_STREAMS)
        if beside:
            self.df_aborts_beside_side_work += 1
            METRICS.inc("engine_dataflow_aborts_beside_side_work")
        self._df_off_until = time.monotonic() + float(os.environ.get("DLMS_DF_COOLDOWN_S", "30"))
        log.warning("%s (committed %d steps%s); launch-per-op for a while", DataflowDecoder.describe(st), st[4],
                    ", a side stream busy" if beside else "")

    def dataflow_status_async(self) -> "HostResult | None":
        """Whether the last ``decode()`` chunk ran the dataflow kernel and it ABORTED before
        committing (``.result()`` True: that chunk made no progress, the row state is unchanged);
        None if the chunk ran launch-per-op.  A copy in flight, like ``flags_async``."""
        h, self._df_status = self._df_status, None
        if h is None:
            return None

        def finish():
            st = h.result()
            if st[0]:
                self._df_note(st)
            return bool(st[0]) and not st[4]

        return HostResult(finish)

    def _df_decoder(self):
        if self._df is None:
            from ..ops.dataflow import DataflowDecoder

            self._df = DataflowDecoder(self)
        return self._df

    def _small_ok(self, B: int) -> bool:
        return 0 < B <= self.small_max

    def _mid_ok(self, B: int) -> bool:
        return self.small_max < B <= self.mid_max

    def _mid_layers(self, lo: int, hi: int):
        """The mid path's 12 layers on rows [lo, hi): per layer [LN1 + QKV + K/V scatter] -> split-K
        attention -> out-projection, x += in place -> [LN2 + c_fc + GELU] -> c_proj, x += in place."""
        eps = self.cfg.layer_norm_epsilon
        x = self.x[lo:hi]
        r = self._rows(self.x[lo:hi], self.parts, self.h[lo:hi], self.q[lo:hi], self.att[lo:hi], self.ff[lo:hi],
                       self.slots[lo:hi], self.cur_pos[lo:hi], self.cur_kvlen[lo:hi], hi - lo)
        for li, lw in enumerate(self.w.layers):
            ops.mid_ln_gemm(x, lw.w_qkv_sh, ops.EPI_QKV, lw.ln1_g, lw.ln1_b, eps, bias=lw.b_qkv, q_out=r.q,
                            k_cache=self.kv[li, 0], v_cache=self.kv[li, 1], row_slot=r.row_slot, row_pos=r.row_pos)
            self._attn(r, li)
            ops.mid_proj(r.att, lw.w_o_sh, x, bias=lw.b_o)
            ops.mid_ln_gemm(x, lw.w_fc_sh, ops.EPI_GELU_TANH, lw.ln2_g, lw.ln2_b, eps, bias=lw.b_fc, out=r.ff)
            ops.mid_proj(r.ff, lw.w_p_sh, x, bias=lw.b_p)

    def _decode_step_mid(self, B: int, penalty: float):
        """Mid-batch decode step (``mid_max`` in __init__): the layers (``_mid_layers``), then ln_f,
        the LM head with the fused penalty / argmax, and the bookkeeping.  (Measured and removed: the
        two row halves' layers on two HIP streams joined for one LM head -- batch 32 50.4 vs 44.1 ms,
        batch 64 53.8 vs 51.9, profiles/r6_mid_sweep.jsonl: the row-blocked kernels already fill the
        chip.)"""
        eps = self.cfg.layer_norm_epsilon
        self._mid_layers(0, B)
        ops.layernorm(self.x[:B], self.w.lnf_g, self.w.lnf_b, eps, out_bf16=self.h[:B])
        self._lm_head_and_update(self.h[:B], B, penalty)

    def _decode_step_small(self, B: int, penalty: float, lo: int = 0):
        """Latency-shaped decode step for B <= ``small_max`` rows: per layer
        [add+LN1+QKV] -> split-K attention -> out-proj (split-K partials) -> [add+LN2+c_fc+GELU]
        -> c_proj (partials); the residual ping-pongs between ``x`` and ``x2`` (every workgroup of a
        fused add+LN kernel re-reads its input rows, so the updated rows go to the other buffer).
        Under TP the partial is all-reduced first and summed as one slab.  ``lo``: run on rows
        [lo, lo + B) only (one part of the multi-stream small step, TP=1)."""
        eps = self.cfg.layer_norm_epsilon
        hi = lo + B
        r = self._rows(self.x[lo:hi], self.parts[:, lo:hi], self.h[lo:hi], self.q[lo:hi], self.att[lo:hi],
                       self.ff[lo:hi], self.slots[lo:hi], self.cur_pos[lo:hi], self.cur_kvlen[lo:hi], B)
        bufs = (self.x[lo:hi], self.x2[lo:hi])
        cur = 0
        pend = None  # (nsplit, residual bias) still to be added into x
        tp = self.tp_size > 1
        split = 1 if tp else self.SMALL_SPLIT
        parts = self.parts[:, lo:hi]
        if lo and (tp or not self.small_inplace):
            raise ValueError("row-offset small step is TP=1 / in-place only")
        # TP=1: the row-parallel projections add straight into the residual (skinny MFMA, column-
        # owning, x += a W^T + b in place: no split-K slabs for the next kernel to sum)
        inplace = not tp and self.small_inplace

        def row_parallel(a, w):
            ops.gemm(a, w, ops.EPI_PARTIAL, out=self.parts, split_k=split)
            if tp:
                self._all_reduce(self.parts[0, :B])
            return split

        if inplace and self.fused_mlp and B <= max(1, self.fused_mlp_rows):
            self._decode_layers_fused_mlp(r, B)
            ops.ln_fix(self.xr[(len(self.w.layers) - 1) % 2, :, :B], self.w.lnf_g, self.w.lnf_b, eps, self.h[:B])
            self._lm_head_and_update(self.h[:B], B, penalty)
            return
        if tp and self.tp_fused and B <= self.tp_fused_rows and ops.skinny_mlp_cg(self.cfg.n_embd, B) > 0:
            self._decode_layers_tp_fused(r, B)
            ops.ln_fix(self.xr[(len(self.w.layers) - 1) % 2, :, :B], self.w.lnf_g, self.w.lnf_b, eps, self.h[:B])
            self._lm_head_and_update(self.h[:B], B, penalty)
            return
        for li, lw in enumerate(self.w.layers):
            kc, vc = self.kv[li, 0], self.kv[li, 1]
            if pend is None:
                ops.skinny_addln_gemm(bufs[cur], lw.w_qkv_sh, ops.EPI_QKV, lw.ln1_g, lw.ln1_b, eps, bias=lw.b_qkv,
                                      q_out=r.q, k_cache=kc, v_cache=vc, row_slot=r.row_slot, row_pos=r.row_pos)
            else:
                ops.skinny_addln_gemm(bufs[cur], lw.w_qkv_sh, ops.EPI_QKV, lw.ln1_g, lw.ln1_b, eps, x_out=bufs[1 - cur],
                                      parts=parts, nsplit=pend[0], res_bias=pend[1], bias=lw.b_qkv, q_out=r.q,
                                      k_cache=kc, v_cache=vc, row_slot=r.row_slot, row_pos=r.row_pos)
                cur = 1 - cur
            if self.fuse_ao and B == 1 and self.ao_groups and self.ao_slabs == 4:
                # heads in groups of H/4: exactly the 4 slabs the fused add+LN sums cheaply
                ops.attention_oproj_grouped(self.q[:1], kc, vc, r.row_slot, r.row_kvlen, lw.w_o_sh, self.ao_parts,
                                            self.ao_groups, tiles=self.ao_group_tiles)
                mlp_parts, ns, rb = self.ao_parts[:4, :1], 4, lw.b_o
            elif self.fuse_ao and B <= self.FUSE_AO_MAX_ROWS and self.w.n_heads_local in (12, 16):
                ops.attention_oproj(self.q[:B], kc, vc, r.row_slot, r.row_kvlen, lw.w_o_sh, self.ao_parts)
                mlp_parts, ns, rb = self.ao_parts[:, :B], self.w.n_heads_local, lw.b_o
            elif inplace:
                self._attn(r, li)
                ops.skinny_gemm(self.att[lo:hi], lw.w_o_sh, ops.EPI_F32, bias=lw.b_o, out=bufs[cur])
                mlp_parts, ns, rb = None, 0, None
            else:
                self._attn(r, li)
                mlp_parts, ns, rb = parts, row_parallel(r.att, lw.w_o), lw.b_o
            if ns:
                ops.skinny_addln_gemm(bufs[cur], lw.w_fc_sh, ops.EPI_GELU_TANH, lw.ln2_g, lw.ln2_b, eps,
                                      x_out=bufs[1 - cur], parts=mlp_parts, nsplit=ns, res_bias=rb, bias=lw.b_fc,
                                      out=r.ff)
                cur = 1 - cur
            else:  # residual already complete: LN2 only
                ops.skinny_addln_gemm(bufs[cur], lw.w_fc_sh, ops.EPI_GELU_TANH, lw.ln2_g, lw.ln2_b, eps,
                                      bias=lw.b_fc, out=r.ff)
            if inplace:
                ops.skinny_gemm(self.ff[lo:hi], lw.w_p_sh, ops.EPI_F32, bias=lw.b_p, out=bufs[cur])
                pend = None
            else:
                pend = (row_parallel(r.ff, lw.w_p), lw.b_p)
        if pend is None:
            ops.add_layernorm(bufs[cur], self.w.lnf_g, self.w.lnf_b, eps, out_bf16=self.h[lo:hi])
        else:
            ops.add_layernorm(bufs[cur], self.w.lnf_g, self.w.lnf_b, eps, parts=self.parts, nsplit=pend[0],
                              bias=pend[1], out_bf16=self.h[:B])
        self._lm_head_and_update(self.h[lo:hi], B, penalty, lo=lo)

    def _decode_layers_fused_mlp(self, r, B: int):
        """Layers as [LN1 + QKV (+ clear the MLP's accumulator)] -> attention + out-projection ->
        [add + LN2 + c_fc + GELU + c_proj, added into the int64 fixed-point residual xr[l % 2]].
        Batch 1 with head groups (12 / 16 heads): attention fused with the out-projection (4 head-group
        slabs the MLP sums); otherwise split attention, then the skinny out-projection adding into the residual in place (the
        f32 embedding rows x in layer 0, copy 0 of the fixed-point residual after that).  The final
        residual is xr[(L - 1) % 2]."""
        eps = self.cfg.layer_norm_epsilon
        xin = self.x[:B]
        for li, lw in enumerate(self.w.layers):
            kc, vc = self.kv[li, 0], self.kv[li, 1]
            acc = self.xr[li % 2, :, :B]
            ops.skinny_addln_gemm(xin, lw.w_qkv_sh, ops.EPI_QKV, lw.ln1_g, lw.ln1_b, eps, bias=lw.b_qkv, q_out=r.q,
                                  k_cache=kc, v_cache=vc, row_slot=r.row_slot, row_pos=r.row_pos,
                                  zero=self.xr[li % 2])  # (all of its rows: a contiguous clear)
            if B == 1 and self.ao_groups:
                ops.attention_oproj_grouped(self.q[:1], kc, vc, r.row_slot, r.row_kvlen, lw.w_o_sh, self.ao_parts,
                                            self.ao_groups, tiles=self.ao_group_tiles)
                ns = self.ao_slabs
                ops.skinny_mlp(xin, lw.ln2_g, lw.ln2_b, eps, lw.w_fc_sh, lw.b_fc, lw.w_p_sl, lw.b_p, acc,
                               parts=self.ao_parts[:ns, :1], nsplit=ns, res_bias=lw.b_o)
            else:
                self._attn(r, li)
                ops.skinny_gemm(self.att[:B], lw.w_o_sh, ops.EPI_F32, bias=lw.b_o, out=xin if li == 0 else xin[0])
                ops.skinny_mlp(xin, lw.ln2_g, lw.ln2_b, eps, lw.w_fc_sh, lw.b_fc, lw.w_p_sl, lw.b_p, acc)
            xin = acc

    def _decode_layers_tp_fused(self, r, B: int):
        """TP > 1 latency path, six kernels per layer on every rank (see ``tp_fused`` in __init__):
        the replicated residual enters as the f32 embedding rows (layer 0) or the all-reduced
        fixed-point accumulator of the previous layer; the final residual is xr[(L - 1) % 2]."""
        eps = self.cfg.layer_norm_epsilon
        xin = self.x[:B]
        base = self.tp_rank == 0
        self.tp_fused_steps += 1  # (host-side count of steps issued on this path: tests assert it)
        for li, lw in enumerate(self.w.layers):
            kc, vc = self.kv[li, 0], self.kv[li, 1]
            acc_all = self.xr[li % 2]  # [copies, rows, d], contiguous: the integer all-reduce's message
            ops.skinny_addln_gemm(xin, lw.w_qkv_sh, ops.EPI_QKV, lw.ln1_g, lw.ln1_b, eps, bias=lw.b_qkv, q_out=r.q,
                                  k_cache=kc, v_cache=vc, row_slot=r.row_slot, row_pos=r.row_pos, zero=acc_all)
            self._attn(r, li)
            ops.skinny_gemm(self.att[:B], lw.w_o_sh, ops.EPI_PARTIAL, out=self.parts[0, :B])
            self._all_reduce(self.parts[0, :B])
            ops.skinny_mlp(xin, lw.ln2_g, lw.ln2_b, eps, lw.w_fc_sh, lw.b_fc, lw.w_p_sl, lw.b_p, acc_all[:, :B],
                           parts=self.parts[:1, :B], nsplit=1, res_bias=lw.b_o, base=base)
            self._all_reduce_i64(acc_all)
            xin = acc_all[:, :B]

    def _decode_step(self, B: int, penalty: float, nsteps: int = 1, h_ready: bool = False):
        """One decode step (``nsteps`` back to back).  ``h_ready``: the previous step of the same
        graph replay ran the tiled path below, whose ``decode_update`` left layer 0's LN1 in h."""
        if nsteps > 1:
            if self._overlap_ok(B) and not self._small_ok(B):
                return self._decode_step_overlap(B, penalty, nsteps)
            for i in range(nsteps):
                self._decode_step(B, penalty, h_ready=i > 0)
            return
        if self._small_ok(B):
            return self._decode_step_small(B, penalty)
        if self._mid_ok(B):
            return self._decode_step_mid(B, penalty)
        if self._overlap_ok(B):
            return self._decode_step_overlap(B, penalty)
        # (batch 256: 84.9 / 84.9 ms per query against 85.8 / 86.4 with the launch; batch 32 within
        # box noise -- profiles/r5_fused_ln1_tiled_ab.jsonl)
        fuse = not self.w.fp8 and not self._timing_skip
        self._layers(self.x, self.parts, self.h, self.q, self.att, self.ff, self.slots[:B], self.cur_pos[:B],
                     self.cur_kvlen[:B], B, final_h=self.h[:B], h8=self.h8, hsc=self.hsc, ln0_done=h_ready and fuse)
        if self.w.fp8:
            self._lm_head_and_update(self.h8[:B], B, penalty, hscale=self.hsc[:B])
        else:
            self._lm_head_and_update(self.h[:B], B, penalty, ln1_out=self.h[:B] if fuse else None)

    def _graph_for(self, B: int, penalty: float, nsteps: int = 1) -> torch.cuda.CUDAGraph:
        key = (B, float(penalty), nsteps) + self._skey()  # (the seed is a device word: not in the key)
        g = self._graphs.get(key)
        if g is None:
            # warm up on a side stream (kernel code objects loaded, RCCL comm initialised).  The
            # snapshot is enqueued BEFORE the side stream's wait, so the warm-up step is ordered
            # after it: the other order let the warm-up advance the rows before the snapshot copied
            # them, and the restore then left them one step ahead (the first generation after a
            # capture deviated -- TP=8 on a shared GPU showed it, profiles/r6_tp124m_tests.txt)
            saved = self._snapshot_state(B)
            s = torch.cuda.Stream(device=self.device)
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                self._decode_step(B, penalty, nsteps)
            torch.cuda.current_stream().wait_stream(s)
            self._restore_state(B, saved)
            # (one graph per row part replayed on its own stream measured identical to this one
            # forked graph: 668.07 vs 668.08 k tok/s, profiles/r2_sweep_split_graphs.jsonl)
            g = torch.cuda.CUDAGraph()
            with capture_guard(), torch.cuda.graph(g):
                self._decode_step(B, penalty, nsteps)
            self._restore_state(B, saved)
            self._graphs[key] = g
        return g

    def _stop_flags(self) -> torch.Tensor:
        """Two pinned int32 host words for the lagged all-finished check in ``generate``."""
        if self._flags is None:
            self._flags = torch.zeros(2, dtype=torch.int32, pin_memory=True)
        return self._flags

    def _snapshot_state(self, B: int):
        return [t[:B].clone() for t in (self.lens, self.finished, self.out_tokens, self.seen, self.cur_tok,
                                        self.cur_pos, self.cur_kvlen, self.x)]

    def _restore_state(self, B: int, saved):
        for t, s in zip((self.lens, self.finished, self.out_tokens, self.seen, self.cur_tok, self.cur_pos,
                         self.cur_kvlen, self.x), saved):
            t[:B].copy_(s)

    # ------------------------------------------------------------------ prefill
    def _reset_slots(self, lo: int, hi: int):
        """Make slots [lo, hi) inert: finished, one EOS token, position 0 (decode replays over a
        bucket touch them harmlessly and decode_update leaves them alone)."""
        if hi <= lo:
            return
        self.lens[lo:hi].fill_(1)
        self.finished[lo:hi].fill_(1)
        self.out_tokens[lo:hi, 0].fill_(self.cfg.eos_token_id)
        self.cur_tok[lo:hi].fill_(self.cfg.eos_token_id)
        self.cur_pos[lo:hi].zero_()
        self.cur_kvlen[lo:hi].fill_(1)
        if self.slot_pfx is not None:
            self.slot_pfx[lo:hi].zero_()

    # ------------------------------------------------------------------ prompt-prefix cache
    @torch.no_grad()
    def set_prompt_prefix(self, tokens):
        """Set (``tokens``: 1 .. min(prefix_capacity, max_length - 2) ids), replace or clear (None)
        the shared prompt prefix.  Its K/V are computed once, by the ordinary packed prefill of
        ``tokens`` as one prompt into slot 0 (the layers only: no LM head, no first token, no
        bookkeeping), and copied into the prefix store; from then on a prompt that starts with
        ``tokens`` and is longer (``split_prefix``) prefills only its suffix.  The engine matches per
        prompt, so any other prompt is served as before.  ``RuntimeError`` while any slot is
        unfinished: its decode may be reading the store."""
        if not self.prefix_capacity:
            raise ValueError("set_prompt_prefix: the engine was built with prefix_capacity=0")
        if int(self.finished.min().item()) == 0:
            raise RuntimeError("set_prompt_prefix: a slot is unfinished; change the prefix between batches")
        self.slot_pfx.zero_()  # (every slot is finished: none counts on the old store any more)
        if tokens is None:
            self._pfx_tokens = None
            return
        toks = [int(t) for t in tokens]
        P, cap = len(toks), min(self.prefix_capacity, self.max_length - 2)
        if not 1 <= P <= cap:
            raise ValueError(f"set_prompt_prefix: 1 .. {cap} tokens (prefix_capacity, max_length - 2), got {P}")
        if min(toks) < 0 or max(toks) >= self.cfg.vocab_size:
            raise ValueError("set_prompt_prefix: token id out of range")
        self._pfx_tokens = None  # (not valid until the store is written)
        dev = self.device
        tok_np, pos_np, slot_np, _, _, sl_np = pack_prompts([toks], [0])
        tokens_d, pos_d, slot_d = (_to_device(a, dev) for a in (tok_np, pos_np, slot_np))
        self._prefill_layers(tokens_d, pos_d, slot_d, ops.AttnTiles(sl_np.tolist(), dev))
        self.pfx_store[:, :, :, :P].copy_(self.kv[:, :, 0, :, :P])
        self._pfx_tok_d.zero_()
        self._pfx_tok_d[:P].copy_(tokens_d)
        self._pfx_seen.copy_(_to_device(seen_bitmap(toks, self.seen_words), dev))
        self._pfx_tokens = toks

    @property
    def prompt_prefix(self) -> list[int] | None:
        """The tokens of the prefix in the store (None: no prefix set)."""
        return None if self._pfx_tokens is None else list(self._pfx_tokens)

    def _check_completions(self, k: int) -> int:
        """``n`` of a public call: an integer in [1, max_batch]; more than one only in a sampling mode
        (n equal greedy answers is a mistake, not a feature)."""
        if isinstance(k, bool) or not isinstance(k, int) or k < 1:
            raise ValueError(f"n: a positive integer, got {k!r}")
        if k > self.max_batch:
            raise ValueError(f"n = {k} completions per prompt do not fit max_batch = {self.max_batch} slots")
        if k > 1 and self._mode.sampling is None:
            raise ValueError("n > 1 needs sampling=: greedy completions of one prompt are all equal")
        return k

    def _prefill_into(self, prompts: list[list[int]], slots: list[int], penalty: float,
                      streams: list[int] | None = None, k: int = 1):
        """Packed variable-length prefill of ``prompts`` into KV-cache slots ``slots`` (any free
        slots of a running batch), then the first token of each (greedy, or drawn in a sampling
        mode, then with the requests' stream ids ``streams``): the LM head's key rows map back to
        their slots through decode_update's slot map.  ``k`` > 1 (best of n): ``slots`` lists k per
        prompt, prompt i owning ``slots[i * k: (i + 1) * k]``; the prompt is prefilled once, into the
        first of them (its parent), whose K/V and bookkeeping are forked into the other k - 1 before
        the LM head draws k first tokens, one per slot and stream."""
        if k > 1:
            return self._prefill_forked(prompts, slots, penalty, streams, k)
        cfg, dev = self.cfg, self.device
        n = len(prompts)
        if n != len(slots) or n == 0:
            raise ValueError("prefill: one slot per prompt")
        if min(slots) < 0 or max(slots) >= self.max_batch or len(set(slots)) != n:
            raise ValueError(f"prefill: slots must be distinct and in [0, {self.max_batch})")
        pfx, pfx_np = self._split_prompts(prompts)
        # packed token / position / slot arrays built with numpy (pack_prompts)
        tok_np, pos_np, slot_np, last_np, lens_np, sl_np = pack_prompts(prompts, slots, pfx)
        R = tok_np.size
        if tok_np.min() < 0 or tok_np.max() >= cfg.vocab_size:
            raise ValueError("prefill: token id out of range")
        if self._mode.sampling is not None:
            # the slots' stream ids, ahead of (and outside) a replayed prefill graph
            if streams is None or len(streams) != n:
                raise ValueError("prefill: one stream id per sampled prompt")
            self.rng_stream.index_copy_(0, _to_device(np.asarray(slots), dev, np.int64),
                                        _to_device(np.asarray(streams, dtype=np.uint64).view(np.int64), dev, np.int64))
        if self._prefill_graph_ok(R, n):
            return self._prefill_graphed(tok_np, pos_np, slot_np, last_np, np.asarray(slots), lens_np, penalty, pfx_np)
        tokens_d, pos_d, slot_d, last_d, slots_d, lens_d = (
            _to_device(a, dev) for a in (tok_np, pos_np, slot_np, last_np, np.asarray(slots), lens_np))
        pfx_d = None if pfx_np is None else _to_device(pfx_np, dev)
        self._prefill_core(tokens_d, pos_d, slot_d, last_d, slots_d, lens_d, ops.AttnTiles(sl_np.tolist(), dev),
                           penalty, pfx_d)

    def _split_prompts(self, prompts: list[list[int]]):
        """Length check, then the prompt-prefix split of a prefill: the prompts that start with the
        stored prefix run their suffix rows only (one packed prefill with the others).  Counts
        prompts (not completions) into the prefix-hit counters.  Returns (pfx list, pfx int64 array),
        both None on an engine without a store."""
        n = len(prompts)
        lens = [len(p) for p in prompts]
        if min(lens) < 1 or max(lens) > self.max_length:
            raise ValueError("prefill: prompt lengths must be in [1, max_length]")
        pfx = pfx_np = None
        if self.prefix_capacity:
            pfx = split_prefix(prompts, self._pfx_tokens)
            pfx_np = np.asarray(pfx, dtype=np.int64)
            if self._pfx_tokens is not None:
                hits, rows = sum(1 for k in pfx if k), sum(pfx)
                self.prefix_prompts += n
                self.prefix_hits += hits
                self.prefix_rows_skipped += rows
                METRICS.inc("engine_prefix_prompts", n)
                METRICS.inc("engine_prefix_hits", hits)
                METRICS.inc("engine_prefix_rows_skipped", rows)
        return pfx, pfx_np

    def _prefill_forked(self, prompts: list[list[int]], slots: list[int], penalty: float,
                        streams: list[int] | None, k: int):
        """``_prefill_into`` for k > 1 completions per prompt: the packed arrays and the prefix split
        see the parents only; the per-slot arrays (last row, slot, length, prefix) repeat each
        prompt's words k times, and the fork table lists (parent, child, prompt length) per child."""
        cfg, dev = self.cfg, self.device
        n = len(prompts)
        N = n * k
        if n == 0 or len(slots) != N:
            raise ValueError(f"prefill: {k} slots per prompt")
        if min(slots) < 0 or max(slots) >= self.max_batch or len(set(slots)) != N:
            raise ValueError(f"prefill: slots must be distinct and in [0, {self.max_batch})")
        if self._mode.sampling is None or streams is None or len(streams) != N:
            raise ValueError("prefill: one stream id per sampled completion")
        slots_np = np.asarray(slots, dtype=np.int64)
        groups = slots_np.reshape(n, k)
        pfx, pfx_np = self._split_prompts(prompts)
        tok_np, pos_np, slot_np, last_np, lens_np, sl_np = pack_prompts(prompts, groups[:, 0].tolist(), pfx)
        R = tok_np.size
        if tok_np.min() < 0 or tok_np.max() >= cfg.vocab_size:
            raise ValueError("prefill: token id out of range")
        self.rng_stream.index_copy_(0, _to_device(slots_np, dev, np.int64),
                                    _to_device(np.asarray(streams, dtype=np.uint64).view(np.int64), dev, np.int64))
        fork_np = (np.repeat(groups[:, 0], k - 1), groups[:, 1:].reshape(-1), np.repeat(lens_np, k - 1))
        ops.check_fork_pairs(*fork_np, self.max_batch)
        if self._prefill_graph_ok(R, n, k):
            return self._prefill_graphed(tok_np, pos_np, slot_np, last_np, slots_np, lens_np, penalty, pfx_np, fork_np)
        tokens_d, pos_d, slot_d, last_d, slots_d, lens_d = (
            _to_device(a, dev) for a in (tok_np, pos_np, slot_np, np.repeat(last_np, k), slots_np,
                                         np.repeat(lens_np, k)))
        pfx_d = None if pfx_np is None else _to_device(np.repeat(pfx_np, k), dev)
        self._prefill_core(tokens_d, pos_d, slot_d, last_d, slots_d, lens_d, ops.AttnTiles(sl_np.tolist(), dev),
                           penalty, pfx_d, tuple(_to_device(a, dev) for a in fork_np))

    def _prefill_core(self, tokens_d, pos_d, slot_d, last_d, slots_d, lens_d, tiles, penalty: float, pfx_d=None,
                      fork=None):
        """Device side of a packed prefill (no host synchronisation: also captured as a graph).
        ``pfx_d`` (engines with a prefix store): per prompt the number of leading tokens whose K/V
        come from the store -- the packed rows are then the suffixes (positions from ``pfx``), the
        bookkeeping still sees whole prompts, and the store's rows are copied into the slots.
        ``fork`` (best of n: ``(src, dst, lens)`` per child): ``last_d`` / ``slots_d`` / ``lens_d`` /
        ``pfx_d`` then hold one word per slot, parents and children, while the packed rows are the
        parents' alone (``_prefill_core_forked``)."""
        if fork is not None:
            return self._prefill_core_forked(tokens_d, pos_d, slot_d, last_d, slots_d, lens_d, tiles, penalty, pfx_d,
                                             fork)
        cfg = self.cfg
        T = self.max_length
        n = slots_d.numel()
        fin_d = (lens_d >= T).to(torch.int32)
        # per-sequence state scattered into the chosen slots on the device
        idx = slots_d.long()
        if pfx_d is None:
            self.out_tokens.index_fill_(0, idx, 0)
            self.out_tokens.index_put_((slot_d.long(), pos_d.long()), tokens_d)
            self.seen.index_fill_(0, idx, 0)
        else:
            # the prefix's tokens and seen-bitmap row for the prompts that share it, zeros for the
            # others; the store's K/V into the slots in one launch, ahead of layer 0
            C = self.prefix_capacity
            share = pfx_d[:, None] > torch.arange(C, dtype=torch.int32, device=self.device)[None, :]
            self.out_tokens.index_fill_(0, idx, 0)
            self.out_tokens[:, :C].index_copy_(0, idx, self._pfx_tok_d[None, :] * share)
            self.seen.index_copy_(0, idx, self._pfx_seen[None, :] * (pfx_d[:, None] > 0))
            self.slot_pfx.index_copy_(0, idx, pfx_d)
            ops.kv_prefix_fill(self.kv, self.pfx_store, slots_d, pfx_d)
            self.out_tokens.index_put_((slot_d.long(), pos_d.long()), tokens_d)
        ops.seen_set(self.seen, slot_d, tokens_d)
        self.lens.index_copy_(0, idx, lens_d)
        if self._mode.records_prompt_len:
            self.prompt_len.index_copy_(0, idx, lens_d)
        if self._mode.logprobs:  # (a position the decode never reaches stays NaN)
            self.out_logprob.index_fill_(0, idx, float("nan"))
        self.finished.index_copy_(0, idx, fin_d)
        # the LM head of the first token reads the prompts' bitmaps as rows [0, n)
        seen_d = self.seen.index_select(0, idx)
        x = self._prefill_layers(tokens_d, pos_d, slot_d, tiles)
        hl = ops.layernorm_gather(x, last_d, self.w.lnf_g, self.w.lnf_b, cfg.layer_norm_epsilon)
        hsc_l = None
        if self.w.fp8:
            hl8 = torch.zeros(n, self.w.k_fp8, dtype=ops.FP8, device=self.device)  # K padding stays zero
            _, hsc_l = ops.quantize_fp8_rows(hl, out=hl8)
            hl = hl8
        # first token: argmax rows are prompts (seen rows gathered), updates land in their slots
        self._lm_head_and_update(hl, n, penalty, seen=seen_d, hscale=hsc_l, slot_map=slots_d)

    def _prefill_core_forked(self, tokens_d, pos_d, slot_d, last_d, slots_d, lens_d, tiles, penalty: float, pfx_d,
                             fork):
        """``_prefill_core`` for k completions per prompt.  The per-slot bookkeeping is written for all
        the slots (the children get their parents' ``out_tokens`` and ``seen`` rows), the layers run
        the parents' packed rows, one ``ops.kv_fork`` copies each parent's prompt keys -- the store's
        rows included, so a child's ``slot_pfx`` equals its parent's -- into its children, and the LM
        head draws one first token per slot from k equal rows per prompt."""
        cfg = self.cfg
        src_d, dst_d, flens_d = fork
        N = slots_d.numel()
        n = N - dst_d.numel()  # prompts
        idx = slots_d.long()
        src_l, dst_l = src_d.long(), dst_d.long()
        self.out_tokens.index_fill_(0, idx, 0)
        if pfx_d is None:
            self.seen.index_fill_(0, idx, 0)
        else:
            C = self.prefix_capacity
            share = pfx_d[:, None] > torch.arange(C, dtype=torch.int32, device=self.device)[None, :]
            self.out_tokens[:, :C].index_copy_(0, idx, self._pfx_tok_d[None, :] * share)
            self.seen.index_copy_(0, idx, self._pfx_seen[None, :] * (pfx_d[:, None] > 0))
            self.slot_pfx.index_copy_(0, idx, pfx_d)
            k = N // n
            ops.kv_prefix_fill(self.kv, self.pfx_store, slots_d.view(n, k)[:, 0].contiguous(),
                               pfx_d.view(n, k)[:, 0].contiguous())
        self.out_tokens.index_put_((slot_d.long(), pos_d.long()), tokens_d)
        ops.seen_set(self.seen, slot_d, tokens_d)
        self.out_tokens.index_copy_(0, dst_l, self.out_tokens.index_select(0, src_l))
        self.seen.index_copy_(0, dst_l, self.seen.index_select(0, src_l))
        self.lens.index_copy_(0, idx, lens_d)
        if self._mode.records_prompt_len:
            self.prompt_len.index_copy_(0, idx, lens_d)
        if self._mode.logprobs:
            self.out_logprob.index_fill_(0, idx, float("nan"))
        self.finished.index_copy_(0, idx, (lens_d >= self.max_length).to(torch.int32))
        seen_d = self.seen.index_select(0, idx)
        x = self._prefill_layers(tokens_d, pos_d, slot_d, tiles)
        ops.kv_fork(self.kv, src_d, dst_d, flens_d, host_checked=True)  # (_prefill_forked checked the table)
        hl = ops.layernorm_gather(x, last_d, self.w.lnf_g, self.w.lnf_b, cfg.layer_norm_epsilon)
        self._lm_head_and_update(hl, N, penalty, seen=seen_d, slot_map=slots_d)

    def _prefill_layers(self, tokens_d, pos_d, slot_d, tiles) -> torch.Tensor:
        """Embedding and every block of a packed prefill (K/V scattered into the rows' slots at
        their positions); returns the final residual rows, ahead of ln_f."""
        cfg, dev = self.cfg, self.device
        R = tokens_d.numel()
        D, Dl, Fl = cfg.n_embd, self.w.d_local, self.w.ffn_local
        f32, bf = torch.float32, torch.bfloat16
        x = ops.embed(tokens_d, pos_d, self.w.wte, self.w.wpe)
        nsplit = max(self._split(R, D, Fl), self._split(R, D, Dl), self.prefill_split or 1,
                     2 if R >= 16384 else 1)  # (c_proj's split 2 at this size: _row_parallel)
        parts = torch.empty(nsplit, R, D, dtype=f32, device=dev)
        h = torch.empty(R, D, dtype=bf, device=dev)
        q = torch.empty(R, Dl, dtype=bf, device=dev)
        att = torch.empty(R, Dl, dtype=bf, device=dev)
        ff = torch.empty(R, Fl, dtype=bf, device=dev)
        h8 = hsc = None
        if self.w.fp8:
            h8 = torch.zeros(R, self.w.k_fp8, dtype=ops.FP8, device=dev)  # K padding stays zero
            hsc = torch.empty(R, dtype=f32, device=dev)
        self._layers(x, parts, h, q, att, ff, slot_d, pos_d, pos_d + 1, R, final_h=None, h8=h8, hsc=hsc, tiles=tiles)
        return x

    # hipGraph-replayed prefill, keyed by (packed rows, prompts): a (rows, prompts) shape seen
    # twice is captured (inputs go through one static pinned -> device buffer, the tile table is
    # padded by repeating its last tile); single-GPU engines only, small shapes only
    PREFILL_GRAPH_MAX_ROWS = 4096
    PREFILL_GRAPH_CACHE = 32

    def _pkey(self, R: int, n: int, k: int = 1) -> tuple:
        """The key of a prefill graph: (packed rows, prompts), the completions per prompt where there
        are more than one, then the mode key."""
        return ((R, n) if k == 1 else (R, n, k)) + self._skey()

    def _prefill_graph_ok(self, R: int, n: int, k: int = 1) -> bool:
        if not (self.use_graph and self.prefill_graphs and R <= self.PREFILL_GRAPH_MAX_ROWS):
            return False
        if self.tp_size > 1 and not self._tp_capturable(R):
            return False
        key = self._pkey(R, n, k)
        if key in self._pgraphs:
            return True
        if len(self._pseen) > 8192:  # shapes seen once: a bounded memory of candidates
            self._pseen.clear()
        self._pseen[key] = self._pseen.get(key, 0) + 1
        return self._pseen[key] >= 2 and len(self._pgraphs) < self.PREFILL_GRAPH_CACHE

    def _tp_capturable(self, R: int) -> bool:
        """A TP prefill of R packed rows can be captured: every collective in it is an xGMI kernel
        (its messages fit the slab) or the group is RCCL (capturable); gloo calls are eager-only."""
        import torch.distributed as dist

        if self.xgmi is None:
            return False
        return R * self.cfg.n_embd * 4 <= self.xgmi.slab_bytes or dist.get_backend(self.tp_group) == "nccl"

    def _prefill_graphed(self, tok, pos, slot, last, slots, lens, penalty: float, pfx=None, fork=None):
        """``pfx`` (engines with a prefix store): per prompt the leading tokens taken from the store;
        the packed rows and the tiles are then those of the suffixes, and ``pfx`` is staged with the
        other per-prompt words (one graph serves every mix of sharing and other prompts of its
        (rows, prompts) shape).  ``fork`` (best of n: the ``(src, dst, lens)`` arrays of the children):
        ``slots`` then lists every slot, k per prompt, while ``last`` / ``lens`` / ``pfx`` stay per prompt;
        the per-slot words are staged k times over and the fork table behind the tiles."""
        if fork is not None:
            P, k = lens.size, slots.size // lens.size
            tile_lens, tile_pfx = lens, pfx
            last, lens = np.repeat(last, k), np.repeat(lens, k)
            pfx = None if pfx is None else np.repeat(pfx, k)
        else:
            P, k, tile_lens, tile_pfx = slots.size, 1, lens, pfx
        R, n = tok.size, slots.size
        key = self._pkey(R, P, k)
        TB = R // 16 + P  # >= the tile count of any R rows in P prompts
        npp = 3 if pfx is None else 4  # staged words per slot
        nf = 0 if fork is None else fork[0].size  # children
        st = self._pgraphs.get(key)
        if st is None:
            words = 3 * R + npp * n + 2 * TB + 3 * nf
            st = dict(host=torch.empty(words, dtype=torch.int32).pin_memory(),
                      dev=torch.empty(words, dtype=torch.int32, device=self.device), copied=torch.cuda.Event(),
                      graph=None, penalty=penalty)
            self._pgraphs[key] = st
        st["copied"].synchronize()  # the previous upload has left the staging buffer
        hbuf = st["host"].numpy()
        hbuf[:R], hbuf[R:2 * R], hbuf[2 * R:3 * R] = tok, pos, slot
        o = 3 * R
        hbuf[o:o + n], hbuf[o + n:o + 2 * n], hbuf[o + 2 * n:o + 3 * n] = last, slots, lens
        if pfx is not None:
            hbuf[o + 3 * n:o + 4 * n] = pfx
        of = o + npp * n + 2 * TB  # the fork table, behind the tiles
        if fork is not None:
            hbuf[of:of + nf], hbuf[of + nf:of + 2 * nf], hbuf[of + 2 * nf:] = fork
        rl = tile_lens if tile_pfx is None else tile_lens - tile_pfx  # rows each prompt runs: its suffix
        nt = (rl + 15) // 16
        seq = np.repeat(np.arange(P), nt)
        k = np.arange(int(nt.sum())) - np.repeat(np.cumsum(nt) - nt, nt)
        starts = np.cumsum(rl) - rl
        tt = np.empty((TB, 2), dtype=np.int64)
        tt[: len(seq), 0] = starts[seq] + 16 * k
        tt[: len(seq), 1] = np.minimum(16, rl[seq] - 16 * k)
        tt[len(seq):] = tt[len(seq) - 1]  # padding tiles repeat the last one (identical writes)
        hbuf[o + npp * n:of] = tt.reshape(-1)
        st["dev"].copy_(st["host"], non_blocking=True)
        st["copied"].record()
        if st["graph"] is None or st["penalty"] != penalty:
            d = st["dev"]
            tiles = ops.AttnTiles.__new__(ops.AttnTiles)
            tiles.rows, tiles.n, tiles.t = R, TB, d[o + npp * n:of].view(TB, 2)
            args = (d[:R], d[R:2 * R], d[2 * R:3 * R], d[o:o + n], d[o + n:o + 2 * n], d[o + 2 * n:o + 3 * n], tiles,
                    penalty, None if pfx is None else d[o + 3 * n:o + 4 * n])
            if fork is not None:
                args += ((d[of:of + nf], d[of + nf:of + 2 * nf], d[of + 2 * nf:]),)
            g = torch.cuda.CUDAGraph()
            with capture_guard(), torch.cuda.graph(g):
                self._prefill_core(*args)
            st["graph"], st["penalty"] = g, penalty
        st["graph"].replay()

    def _prefill(self, prompts: list[list[int]], B: int, penalty: float, streams: list[int] | None = None,
                 k: int = 1):
        """Static batch: prompts (``k`` completions each) into slots [0, n * k), the rest of [0, B) inert."""
        self._reset_slots(len(prompts) * k, B)
        self._prefill_into(prompts, list(range(len(prompts) * k)), penalty, streams, k)

    @torch.no_grad()
    def prefill_last_hidden(self, prompts: list[list[int]]) -> torch.Tensor:
        """ln_f(hidden) of each prompt's last token after a packed prefill (bf16 -> f32); test hook."""
        cfg, dev = self.cfg, self.device
        lens = [len(p) for p in prompts]
        R = sum(lens)
        tokens = torch.tensor([t for p in prompts for t in p], dtype=torch.int32, device=dev)
        pos = torch.tensor([i for L in lens for i in range(L)], dtype=torch.int32, device=dev)
        slot = torch.tensor([b for b, L in enumerate(lens) for _ in range(L)], dtype=torch.int32, device=dev)
        last = torch.tensor([sum(lens[: b + 1]) - 1 for b in range(len(prompts))], dtype=torch.int32, device=dev)
        D, Dl, Fl = cfg.n_embd, self.w.d_local, self.w.ffn_local
        x = ops.embed(tokens, pos, self.w.wte, self.w.wpe)
        nsplit = max(self._split(R, D, Fl), self._split(R, D, Dl), self.prefill_split or 1, 2 if R >= 16384 else 1)
        parts = torch.empty(nsplit, R, D, device=dev)
        bf = torch.bfloat16
        h, q, att, ff = (torch.empty(R, n, dtype=bf, device=dev) for n in (D, Dl, Dl, Fl))
        h8 = hsc = None
        if self.w.fp8:
            h8 = torch.zeros(R, self.w.k_fp8, dtype=ops.FP8, device=dev)
            hsc = torch.empty(R, device=dev)
        self._layers(x, parts, h, q, att, ff, slot, pos, pos + 1, R, final_h=None, h8=h8, hsc=hsc,
                     tiles=ops.AttnTiles(lens, dev))
        return ops.layernorm_gather(x, last, self.w.lnf_g, self.w.lnf_b, cfg.layer_norm_epsilon).float()

    # ------------------------------------------------------------------ slot API (continuous batching)
    @torch.no_grad()
    def admit(self, prompts: list[list[int]], slots: list[int], repetition_penalty: float = 1.2,
              sampling: SamplingParams | None = None, controls: GenerationControls | None = None,
              logprobs: bool = False, n: int = 1):
        """Prefill new sequences into free ``slots`` of the running batch (first token included).
        ``sampling``: draw their tokens instead; each takes the next stream id (the count of requests
        admitted since the seed was last set: ``reseed``, or a ``sampling.seed`` other than the
        current one).  ``controls``: the slots' generation controls; every later call that serves
        these slots passes the same.  ``logprobs``: record the chosen tokens' log-probabilities
        (``collect(..., logprobs=True)`` returns them); every later call passes the same too.
        ``n`` > 1 (needs ``sampling``): n completions per prompt from one prefill.  ``slots`` lists
        ``n * len(prompts)`` distinct slots, prompt i owning ``slots[i * n: (i + 1) * n]``, the first of
        them its parent: the prompt is prefilled into the parent and forked into the others
        (``ops.kv_fork``); completion j of the i-th prompt draws on stream ``first + i * n + j``.  The
        decode does not know about groups: every slot is an ordinary sequence from here on."""
        with self._mode_scope(DecodeMode(sampling, controls, bool(logprobs))):
            n = self._check_completions(n)
            self._prefill_into([list(p) for p in prompts], list(slots), repetition_penalty,
                               self._next_streams(n * len(prompts), sampling), n)

    @torch.no_grad()
    def decode(self, B: int, steps: int, repetition_penalty: float = 1.2, sampling: SamplingParams | None = None,
               controls: GenerationControls | None = None, logprobs: bool = False):
        """``steps`` decode steps over slots [0, B) (finished/inert slots are no-ops): greedy, or
        sampled with ``sampling`` under the slots' stream ids (``admit``); under ``controls``, the
        ones the slots were admitted with; with ``logprobs``, recording the chosen tokens'
        log-probabilities, as the slots were admitted."""
        with self._mode_scope(DecodeMode(sampling, controls, bool(logprobs))):
            self._decode(B, steps, repetition_penalty)

    def _decode(self, B: int, steps: int, repetition_penalty: float):
        if B > self.max_batch or B not in (_bucket(B), self.max_batch):
            raise ValueError(f"decode: batch bucket {B} invalid")
        self._df_status = None
        if steps > 0 and self._df_ok(B) and self._df_run(B, steps, repetition_penalty):
            self._df_status = self._df.status_async()
            return
        graph = self._graph_for(B, repetition_penalty) if self.use_graph else None
        kg = self._steps_per_graph_for(B) if graph is not None else 1
        graph_k = self._graph_for(B, repetition_penalty, kg) if steps >= kg > 1 else None
        self._replay(B, steps, repetition_penalty, graph, graph_k, kg)

    def _replay(self, B: int, steps: int, penalty: float, graph, graph_k, kg: int):
        """``steps`` decode steps: replays of the ``kg``-step graph ``graph_k`` (None: none) where
        they fit, then the one-step ``graph`` (None: eager steps) for the rest."""
        n_k = steps // kg if graph_k is not None else 0
        for _ in range(n_k):
            graph_k.replay()
        for _ in range(steps - n_k * kg):
            if graph is not None:
                graph.replay()
            else:
                self._decode_step(B, penalty)

    @torch.no_grad()
    def warm_decode_graphs(self, repetition_penalty: float = 1.2, max_batch: int | None = None,
                           sampling: SamplingParams | None = None,
                           controls: GenerationControls | None = None, logprobs: bool = False) -> tuple[int, float]:
        """Capture the decode-step graphs ``decode()`` would capture on first use (one step and one
        replay's worth of steps per batch bucket up to ``max_batch``; the dataflow buckets need none)
        so a server's first burst of queries does not pay the captures.  ``sampling``: the graphs of
        that sampling mode; ``controls``: of those generation controls; ``logprobs``: the graphs that
        record log-probabilities.  Returns (graphs, seconds)."""
        with self._mode_scope(DecodeMode(sampling, controls, bool(logprobs))):
            return self._warm_decode_graphs(repetition_penalty, max_batch)

    def _warm_decode_graphs(self, repetition_penalty: float, max_batch: int | None) -> tuple[int, float]:
        if not self.use_graph:
            return 0, 0.0
        t0 = time.perf_counter()
        cap = min(self.max_batch, max_batch or self.max_batch)
        n, B = 0, 1
        while True:
            B = min(_bucket(B), self.max_batch)
            if B > cap:
                break
            if not self._df_ok(B):
                self._graph_for(B, repetition_penalty)
                n += 1
                kg = self._steps_per_graph_for(B)
                if kg > 1:
                    self._graph_for(B, repetition_penalty, kg)
                    n += 1
            if B >= self.max_batch:
                break
            B += 1
        torch.cuda.synchronize(self.device)
        return n, time.perf_counter() - t0

    def _steps_per_graph_for(self, B: int) -> int:
        """Decode steps per graph replay for a batch bucket (DLMS_STEPS_PER_GRAPH[_SMALL])."""
        overlapped = self._overlap_ok(B) and not self._small_ok(B)
        return self.steps_per_graph if overlapped else self.steps_per_graph_small

    def close(self):
        """Release the engine's device-side objects in a defined order while the HIP runtime is
        still fully up: drain the device, destroy the captured decode / prefill graphs, the dataflow
        decoder's buffers and the xGMI peer mappings (IPC handles).  Idempotent.  Leaving them to
        interpreter teardown puts hipGraphExecDestroy / hipIpcCloseMemHandle behind the runtime's
        (and a profiler's) own exit handlers -- the order behind round 4's one SIGSEGV inside exit()
        under rocprofv3."""
        if getattr(self, "_closed", False):
            return
        self._closed = True
        torch.cuda.synchronize(self.device)
        self._graphs.clear()
        self._pgraphs.clear()
        self._df = None
        # the prefix store and the slots' prefix counts (after the graphs that captured their addresses)
        self._pfx_tokens = None
        self.pfx_store = self.slot_pfx = self._pfx_tok_d = self._pfx_seen = None
        self.prefix_capacity = 0
        if self.xgmi is not None:
            self.xgmi.close()
            self.xgmi = None
        import gc

        gc.collect()
        torch.cuda.synchronize(self.device)

    def health_async(self) -> "HostResult | None":
        """Non-zero ``.result()`` when a TP collective gave up waiting for a peer (the xGMI
        barrier's error word): the tokens of that chunk are garbage.  None without xGMI."""
        return self.xgmi.error_async() if self.xgmi is not None else None

    def finished_flags(self, B: int) -> list[int]:
        return self.finished[:B].cpu().tolist()

    def flags_async(self, B: int) -> "HostResult":
        """``finished_flags`` as a copy in flight: enqueued behind the work issued so far, read
        by ``result()`` without waiting for anything enqueued later (the pipelined scheduler reads
        chunk k's flags while chunk k+1 runs)."""
        h = torch.empty(B, dtype=torch.int32, pin_memory=True)
        h.copy_(self.finished[:B], non_blocking=True)
        return HostResult(lambda: h.tolist(), keep=(h,))

    def collect_async(self, slots: list[int], logprobs: bool = False) -> "HostResult":
        """``collect`` as a copy in flight (finished sequences never change, so the tokens can be
        gathered behind a later decode chunk; a slot may be re-admitted right after, the admission
        is stream-ordered behind this copy)."""
        if logprobs and self.out_logprob is None:
            raise ValueError("collect: no slot was admitted with logprobs=True")
        if not slots:
            return HostResult(lambda: ([], []) if logprobs else [])
        idx = _to_device(np.asarray(slots, dtype=np.int64), self.device)
        lens_h = torch.empty(len(slots), dtype=torch.int32, pin_memory=True)
        toks_h = torch.empty(len(slots), self.max_length, dtype=torch.int32, pin_memory=True)
        lens_h.copy_(self.lens.index_select(0, idx), non_blocking=True)
        toks_h.copy_(self.out_tokens.index_select(0, idx), non_blocking=True)
        if not logprobs:
            def finish():
                lens, toks = lens_h.tolist(), toks_h.tolist()
                return [toks[i][: lens[i]] for i in range(len(slots))]

            return HostResult(finish, keep=(lens_h, toks_h, idx))
        plen_h = torch.empty(len(slots), dtype=torch.int32, pin_memory=True)
        lp_h = torch.empty(len(slots), self.max_length, dtype=torch.float32, pin_memory=True)
        plen_h.copy_(self.prompt_len.index_select(0, idx), non_blocking=True)
        lp_h.copy_(self.out_logprob.index_select(0, idx), non_blocking=True)

        def finish_lp():
            lens, toks, plen, lp = lens_h.tolist(), toks_h.tolist(), plen_h.tolist(), lp_h.tolist()
            return ([toks[i][: lens[i]] for i in range(len(slots))],
                    [lp[i][plen[i]: lens[i]] for i in range(len(slots))])

        return HostResult(finish_lp, keep=(lens_h, toks_h, plen_h, lp_h, idx))

    def collect(self, slots: list[int], logprobs: bool = False):
        """Token sequences (prompt + generated) of ``slots``; with ``logprobs`` (slots admitted with
        it): ``(tokens, logprobs)``, one float per generated token."""
        if logprobs:
            return self.collect_async(slots, logprobs=True).result()
        if not slots:
            return []
        idx = torch.tensor(slots, dtype=torch.long, device=self.device)
        lens = self.lens.index_select(0, idx).cpu().tolist()
        toks = self.out_tokens.index_select(0, idx).cpu().tolist()
        return [toks[i][: lens[i]] for i in range(len(slots))]

    # ------------------------------------------------------------------ public API
    @torch.no_grad()
    def generate(self, prompts: list[list[int]], max_length: int | None = None, repetition_penalty: float = 1.2,
                 stats: GenerateStats | None = None, sampling: SamplingParams | None = None,
                 controls: GenerationControls | None = None, logprobs: bool = False, n: int = 1):
        """Full sequences (prompt echoed) of ``prompts``: greedy, or with ``sampling`` drawn under
        ``sampling.seed`` with prompt i on stream i -- set anew on every call, so equal calls return
        equal outputs.  ``controls`` (a ``GenerationControls``): n-gram blocking, a minimum length and
        stop sequences, applied on the device inside the decode loop.  ``logprobs``: returns
        ``(tokens, logprobs)``; ``logprobs[i]`` holds one float per generated token of prompt i, its
        log-probability under the distribution the repetition penalty and the bans leave
        (``ops/csrc/logprob.hip``: at temperature 1, ahead of top-k / top-p).
        ``n`` > 1 (needs ``sampling``; at most ``max_batch``): per prompt a list of n sequences from one
        prefill, completion j of prompt i drawn on stream ``i * n + j`` (``tokens`` and ``logprobs``
        nested the same way); a prompt that only passes through yields n copies; more than
        ``max_batch`` completions run in chunks of whole groups."""
        with self._mode_scope(DecodeMode(sampling, controls, bool(logprobs))):
            n = self._check_completions(n)
            streams = None
            if sampling is not None:
                self.reseed(sampling.seed)
                self._rng_count = n * len(prompts)
                streams = list(range(n * len(prompts)))
            if n == 1:
                toks, lps = self._generate(prompts, max_length, repetition_penalty, stats, streams)
            else:
                toks, lps = self._generate_groups(prompts, max_length, repetition_penalty, stats, n)
        return (toks, lps) if logprobs else toks

    def _generate_groups(self, prompts: list[list[int]], max_length: int | None, repetition_penalty: float,
                         stats: GenerateStats | None, k: int):
        """``_generate`` with k > 1 completions per prompt, nested per prompt: the prompts that run go
        through ``_generate`` in chunks of ``max_batch // k`` whole groups, completion j of prompt i on
        stream ``i * k + j``; a prompt that only passes through yields k copies."""
        T = self.max_length if max_length is None else max_length
        if T != self.max_length:
            raise ValueError(f"engine built for max_length={self.max_length}, got {T}")
        done, run_idx, norm = passthrough(prompts, T, self.cfg.eos_token_id)
        toks = [None if o is None else [list(o) for _ in range(k)] for o in done]
        lps = [[[] for _ in range(k)] for _ in done]
        per = self.max_batch // k
        for c in range(0, len(run_idx), per):
            idx = run_idx[c: c + per]
            sub = self._generate([norm[i] for i in idx], max_length, repetition_penalty, stats,
                                 [i * k + j for i in idx for j in range(k)], k)
            for m, i in enumerate(idx):
                toks[i], lps[i] = sub[0][m * k: (m + 1) * k], sub[1][m * k: (m + 1) * k]
        return toks, lps

    def _generate(self, prompts: list[list[int]], max_length: int | None, repetition_penalty: float,
                  stats: GenerateStats | None, streams: list[int] | None,
                  k: int = 1) -> tuple[list[list[int]], list[list[float]]]:
        """(tokens, log-probabilities) per prompt in the mode of the scope around it; a prompt that
        only passes through, or a mode without log-probabilities, gives ``[]`` for the second.
        ``k`` > 1 (``_generate_groups``: no pass-through prompt, at most ``max_batch`` completions): k
        completions per prompt from one forked prefill, returned flat, prompt i's at [i * k, (i + 1) * k)."""
        T = self.max_length if max_length is None else max_length
        if T != self.max_length:
            raise ValueError(f"engine built for max_length={self.max_length}, got {T}")
        if k > 1:  # from here on a row per completion; only the prefill knows about groups
            groups, prompts = prompts, [p for p in prompts for _ in range(k)]
        n = len(prompts)
        if n == 0:
            return [], []

        def pick(idx):
            return None if streams is None else [streams[i] for i in idx]

        done, run_idx, prompts = passthrough(prompts, T, self.cfg.eos_token_id)
        if len(run_idx) < n:
            lps: list[list[float]] = [[] for _ in prompts]
            if run_idx:
                sub = self._generate([prompts[i] for i in run_idx], max_length, repetition_penalty, stats, pick(run_idx))
                for i, o, lp in zip(run_idx, *sub):
                    done[i], lps[i] = o, lp
            return done, lps
        if n > self.max_batch:
            out, lps = [], []
            for i in range(0, n, self.max_batch):
                sub = self._generate(prompts[i: i + self.max_batch], max_length, repetition_penalty, stats,
                                     pick(range(i, min(n, i + self.max_batch))))
                out += sub[0]
                lps += sub[1]
            return out, lps
        B = min(_bucket(n), self.max_batch)  # (prompts are passthrough()'s normalised copies)
        ev0 = torch.cuda.Event(enable_timing=True)
        ev1 = torch.cuda.Event(enable_timing=True)
        ev2 = torch.cuda.Event(enable_timing=True)
        ev0.record()
        self._prefill(prompts if k == 1 else groups, B, repetition_penalty, streams, k)
        ev1.record()
        steps_max = T - min(len(p) for p in prompts) - 1
        if steps_max > 0 and self._df_ok(B) and self._df_run(B, steps_max, repetition_penalty):
            # one persistent launch for every decode step (it stops on device once all rows finish)
            ev2.record()
            st = tuple(self._df.err[:5].cpu().tolist())
            if st[0]:
                self._df_note(st)
            if st[4]:  # committed (an error after the commit -- a straggler CU -- changes nothing)
                lens = self.lens[:n].cpu().tolist()
                toks = self.out_tokens[:n].cpu().numpy()
                res = [toks[b, : lens[b]].tolist() for b in range(n)]
                self._add_stats(stats, prompts, lens, (ev0, ev1, ev2), st[4], False)
                return res, [[] for _ in res]  # (the dataflow decode serves the default mode only)
            # aborted before its commit: the rows are exactly as the prefill left them -- decode
            # them launch-per-op below
        graph = self._graph_for(B, repetition_penalty) if (self.use_graph and steps_max > 0) else None
        kg = self._steps_per_graph_for(B)
        if graph is None or self.check_every % kg:
            kg = 1
        graph_k = self._graph_for(B, repetition_penalty, kg) if kg > 1 and steps_max >= kg else None
        steps = 0
        # Stop check one chunk behind: the all-finished flag of chunk k is copied to pinned host
        # memory asynchronously and read after chunk k+1 has been enqueued, so the GPU never idles
        # on the host round trip (at most one extra chunk of no-op steps once every row is done).
        flags = self._stop_flags()
        pending = None
        while steps < steps_max:
            chunk = min(self.check_every, steps_max - steps)
            self._replay(B, chunk, repetition_penalty, graph, graph_k, kg)
            steps += chunk
            if steps >= steps_max:
                break
            slot = (steps // self.check_every) & 1
            flags[slot].copy_(self.finished[:n].min(), non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            if pending is not None:
                pending[0].synchronize()
                if int(flags[pending[1]]):
                    break
            pending = (ev, slot)
        ev2.record()
        lens = self.lens[:n].cpu().tolist()
        # one device->host copy, then ONE numpy list conversion of the whole block and each row cut
        # to its length in place (1024 x 150 ids: 40 % less host time than a conversion per row,
        # which was itself about half of Tensor.tolist's)
        toks = self.out_tokens[:n].cpu().numpy()
        if self.xgmi is not None:
            self.xgmi.check()  # a timed-out peer barrier means these tokens are garbage
        res = toks.tolist()
        for row, ln in zip(res, lens):
            del row[ln:]
        if self._mode.logprobs:
            lp = self.out_logprob[:n].cpu().numpy().tolist()
            lps = [lp[b][len(prompts[b]): lens[b]] for b in range(n)]
        else:
            lps = [[] for _ in res]
        self._add_stats(stats, prompts, lens, (ev0, ev1, ev2), steps, graph is not None)
        return res, lps

    @staticmethod
    def _add_stats(stats: GenerateStats | None, prompts, lens, events, steps: int, graph: bool):
        """One batch of ``_generate`` into ``stats`` (None: nothing): ``events`` are the ones
        recorded ahead of the prefill, between it and the decode, and behind the decode."""
        if stats is None:
            return
        ev0, ev1, ev2 = events
        ev2.synchronize()
        stats.batch += len(prompts)
        stats.prompt_tokens += sum(len(p) for p in prompts)
        stats.new_tokens += sum(ln - len(p) for ln, p in zip(lens, prompts))
        stats.prefill_ms += ev0.elapsed_time(ev1)
        stats.decode_ms += ev1.elapsed_time(ev2)
        stats.steps += steps
        stats.graph = graph

    @torch.no_grad()
    def score(self, sequences: list[list[int]]) -> list[list[float]]:
        """Teacher-forced scoring: per sequence, the log-probabilities of its tokens 1 .. len - 1
        given their prefixes under the model's raw distribution (no penalty, no bans, temperature
        1: ``ops/csrc/logprob.hip`` teacher-forced mode); a one-token sequence gives ``[]``.
        One packed prefill of the whole sequences into slots [0, n) (``n <= max_batch``, lengths
        ``<= max_length``), ln_f of the rows that have a next token, then the f32 LM head and the
        log-probability kernel over chunks of at most ``max_batch`` rows.  ``RuntimeError`` while any
        slot is unfinished (the prefill overwrites the slots' K/V).  The prefix store is ignored:
        every sequence is prefilled whole.  bf16 weights on one GPU (``logprobs_unsupported``)."""
        cfg, dev = self.cfg, self.device
        why = logprobs_unsupported(self.tp_size, self.w.fp8)
        if why:
            raise ValueError(why)
        seqs = [[int(t) for t in s] for s in sequences]
        n = len(seqs)
        if n == 0:
            return []
        if n > self.max_batch:
            raise ValueError(f"score: at most max_batch = {self.max_batch} sequences")
        if min(len(s) for s in seqs) < 1 or max(len(s) for s in seqs) > self.max_length:
            raise ValueError("score: sequence lengths must be in [1, max_length]")
        if min(min(s) for s in seqs) < 0 or max(max(s) for s in seqs) >= cfg.vocab_size:
            raise ValueError("score: token id out of range")
        if int(self.finished.min().item()) == 0:
            raise RuntimeError("score: a slot is unfinished; score between batches")
        logits = self._logits_scratch()
        tok_np, pos_np, slot_np, last_np, lens_np, sl_np = pack_prompts(seqs, list(range(n)))
        # the packed rows that have a next token (all but each sequence's last), and that token
        has_next = np.ones(tok_np.size, dtype=bool)
        has_next[last_np] = False
        rows_np = np.nonzero(has_next)[0]
        R = rows_np.size
        if R == 0:
            return [[] for _ in seqs]
        tgt_np = tok_np[rows_np + 1]
        tokens_d, pos_d, slot_d, rows_d, tgt_d = (_to_device(a, dev) for a in (tok_np, pos_np, slot_np, rows_np, tgt_np))
        x = self._prefill_layers(tokens_d, pos_d, slot_d, ops.AttnTiles(sl_np.tolist(), dev))
        h = ops.layernorm_gather(x, rows_d, self.w.lnf_g, self.w.lnf_b, cfg.layer_norm_epsilon)
        out = torch.empty(R, dtype=torch.float32, device=dev)
        for c0 in range(0, R, self.max_batch):
            m = min(self.max_batch, R - c0)
            z = logits[:m]
            if self.ps_lm and m >= self.PS_LM_MIN_ROWS:
                ops.gemm_ps(h[c0:c0 + m], self.lm_head_sh, ops.EPI_PARTIAL, out=z.unsqueeze(0), split_k=1)
            else:
                ops.gemm(h[c0:c0 + m], self.w.lm_head, ops.EPI_F32, out=z)
            ops.token_logprob(z, cfg.vocab_size, out[c0:c0 + m], targets=tgt_d[c0:c0 + m])
        lp = out.cpu().tolist()
        res, o = [], 0
        for s in seqs:
            res.append(lp[o: o + len(s) - 1])
            o += len(s) - 1
        return res


class TorchGPT2Engine:
    """CPU (or any-device) engine on the plain-torch reference model: BASELINE config 1."""

    def __init__(self, cfg: GPT2Config, weights: dict[str, torch.Tensor], device="cpu", max_length: int = 150,
                 dtype=torch.float32, kv_dtype: str = "bf16"):
        """``kv_dtype="fp8"``: the reference model of the fp8 (e4m3) KV cache
        (``GPT2Reference(kv_dtype="fp8")``)."""
        from ..models.gpt2 import GPT2Reference

        self.cfg = cfg
        self.max_length = max_length
        self.kv_dtype = kv_dtype
        self.model = GPT2Reference(cfg, weights, device=device, dtype=dtype, kv_dtype=kv_dtype)

    @torch.no_grad()
    def generate(self, prompts: list[list[int]], max_length: int | None = None, repetition_penalty: float = 1.2,
                 stats: GenerateStats | None = None, sampling: SamplingParams | None = None,
                 controls: GenerationControls | None = None, logprobs: bool = False, n: int = 1):
        """``sampling``: tokens drawn by ``models.gpt2.reference_sample`` under ``sampling.seed``,
        prompt i on stream i (the HIP engine's rule).  ``controls``: the bans and stops of
        ``models.gpt2.banned_tokens`` / ``stop_hit``.  ``logprobs``: returns ``(tokens, logprobs)``,
        the second from ``models.gpt2.teacher_forced_logprobs`` on the generated sequences.
        ``n`` > 1 (needs ``sampling``): the definition of n completions per prompt -- every prompt
        repeated n times, so completion j of prompt i runs on stream ``i * n + j``, regrouped per prompt."""
        from ..models.gpt2 import reference_generate, teacher_forced_logprobs

        if isinstance(n, bool) or not isinstance(n, int) or n < 1:
            raise ValueError(f"n: a positive integer, got {n!r}")
        if n > 1:
            if sampling is None:
                raise ValueError("n > 1 needs sampling=: greedy completions of one prompt are all equal")
            flat = self.generate([p for p in prompts for _ in range(n)], max_length, repetition_penalty, stats,
                                 sampling, controls, logprobs)

            def group(rows):
                return [rows[i: i + n] for i in range(0, len(rows), n)]

            return (group(flat[0]), group(flat[1])) if logprobs else group(flat)
        if logprobs:
            norm = passthrough(prompts, self.max_length if max_length is None else max_length,
                               self.cfg.eos_token_id)[2]
            outs = self.generate(prompts, max_length, repetition_penalty, stats, sampling, controls)
            return outs, [teacher_forced_logprobs(self.model, o, len(p), repetition_penalty, controls).tolist()
                          for o, p in zip(outs, norm)]

        T = self.max_length if max_length is None else max_length
        out, run_idx, norm = passthrough(prompts, T, self.cfg.eos_token_id)
        prompts = [norm[i] for i in run_idx]
        t0 = time.perf_counter()
        if prompts:
            gen = reference_generate(self.model, prompts, max_length=T, repetition_penalty=repetition_penalty,
                                     sampling=sampling, streams=list(run_idx), controls=controls)
            for i, o in zip(run_idx, gen):
                out[i] = o
        out_run = [out[i] for i in run_idx]
        if stats is not None:
            stats.batch += len(prompts)
            stats.prompt_tokens += sum(map(len, prompts))
            stats.new_tokens += sum(len(o) - len(p) for o, p in zip(out_run, prompts))
            stats.decode_ms += (time.perf_counter() - t0) * 1e3
        return out

    @torch.no_grad()
    def score(self, sequences: list[list[int]]) -> list[list[float]]:
        """``HipGPT2Engine.score`` on the reference model: ``models.gpt2.reference_logprob`` (no
        penalty, no seen set) of tokens 1 .. len - 1 of each sequence, one forward per sequence."""
        from ..models.gpt2 import teacher_forced_logprobs

        return [teacher_forced_logprobs(self.model, [int(t) for t in s], 1, 1.0).tolist() for s in sequences]
