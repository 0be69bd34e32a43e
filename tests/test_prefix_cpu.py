"""Prompt-prefix cache, the parts that need no GPU: which prompts share the prefix
(``split_prefix``), the packed arrays of a mixed suffix-only prefill (``pack_prompts``), the
server's prefix candidate, the planner's accounting, and -- from ``GPT2Reference`` alone -- that the
engine tests' prompts (prefix_cases.py) keep at least 70 % of their positions decisive at the
project's eps = 0.05, so the floor the GPU tests assert is one the reference itself clears."""
import functools

import numpy as np
import pytest
import torch

import kv_fp8_cases as kc
import prefix_cases as pc

from distributed_lms_raft_llm_amd.engine.gpt2_engine import (pack_prompts, prefix_unsupported, sampling_unsupported,
                                                             split_prefix)


def test_split_prefix_cases():
    prefix = [7, 8, 9]
    assert split_prefix([[7, 8, 9, 1], [1]], []) == [0, 0]  # an empty prefix
    assert split_prefix([[7, 8, 9, 1]], None) == [0]
    assert split_prefix([[7, 8, 9]], prefix) == [0]  # equal to the prefix: no row left for the first token
    assert split_prefix([[7, 8], [7], []], prefix) == [0, 0, 0]  # shorter
    assert split_prefix([[7, 8, 5, 1, 2]], prefix) == [0]  # differs in the last prefix token
    assert split_prefix([[5, 8, 9, 1, 2]], prefix) == [0]  # ... in the first
    assert split_prefix([[7, 8, 9, 1], [7, 8, 9, 9, 9, 9]], prefix) == [3, 3]  # a match
    assert split_prefix([(7, 8, 9, 1)], (7, 8, 9)) == [3]  # tuples as well
    mixed = [[7, 8, 9, 4], [1, 2], [7, 8, 9], [7, 8, 9, 7, 8, 9]]
    assert split_prefix(mixed, prefix) == [3, 0, 0, 3]


def test_packed_arrays_of_a_mixed_batch():
    """pos starts at P for the sharing prompts and at 0 for the others, the tiles follow the suffix
    lengths, the row count is the sum of the suffixes, the bookkeeping lengths are the full ones."""
    from distributed_lms_raft_llm_amd import ops

    P = 16
    prefix = list(range(100, 100 + P))
    prompts = [prefix + [1, 2, 3], [9] * 20, prefix + list(range(200, 217)), list(prefix), prefix + [5]]
    slots = [4, 0, 7, 2, 5]
    pfx = split_prefix(prompts, prefix)
    assert pfx == [P, 0, P, 0, P]
    tok, pos, slot, last, lens, sl = pack_prompts(prompts, slots, pfx)
    assert sl.tolist() == [3, 20, 17, 16, 1] and lens.tolist() == [19, 20, 33, 16, 17]
    assert tok.size == pos.size == slot.size == sum(sl) == 57
    want_tok, want_pos, want_slot = [], [], []
    for p, s, k in zip(prompts, slots, pfx):
        want_tok += p[k:]
        want_pos += list(range(k, len(p)))
        want_slot += [s] * (len(p) - k)
    assert tok.tolist() == want_tok and pos.tolist() == want_pos and slot.tolist() == want_slot
    assert last.tolist() == (np.cumsum(sl) - 1).tolist() == [2, 22, 39, 55, 56]
    assert [int(pos[i]) + 1 for i in last] == lens.tolist()  # the last row of a prompt sees all its keys
    tiles = ops.AttnTiles(sl.tolist(), "cpu")
    # (row0, rows) per 16-query tile: the 17-row suffix takes two tiles, the others one or two by their own length
    assert tiles.rows == 57 and tiles.t.tolist() == [[0, 3], [3, 16], [19, 4], [23, 16], [39, 1], [40, 16], [56, 1]]
    # without a prefix the arrays are those of whole prompts
    tok0, pos0, slot0, last0, lens0, sl0 = pack_prompts(prompts, slots)
    assert tok0.tolist() == [t for p in prompts for t in p] and sl0.tolist() == lens0.tolist() == lens.tolist()
    assert pos0.tolist() == [i for p in prompts for i in range(len(p))] and last0.tolist() == (np.cumsum(lens) - 1).tolist()
    for a, b in zip(pack_prompts(prompts, slots, [0] * 5), (tok0, pos0, slot0, last0, lens0, sl0)):
        assert a.tolist() == b.tolist()
    with pytest.raises(ValueError):  # a prompt with no row left
        pack_prompts([list(prefix)], [0], [P])


def test_prefix_unsupported_shapes():
    assert prefix_unsupported(1, False) is None
    assert "tensor parallelism" in prefix_unsupported(2, False)
    assert "fp8 weights" in prefix_unsupported(1, True)
    assert sampling_unsupported(1, False) is None  # (sampling and the prefix cache share an engine shape)


def test_server_prefix_candidate_and_flag():
    from distributed_lms_raft_llm_amd.tokenizer import GPT2BPE
    from distributed_lms_raft_llm_amd.tutor import server

    tok = GPT2BPE()
    cand = server.prefix_candidate(tok)
    assert len(cand) >= 1
    encs = [tok.encode(server.build_prompt(q)) for q in server.PREFIX_PROBES]
    assert all(e[: len(cand)] == cand and len(e) > len(cand) for e in encs)
    assert len({e[len(cand)] for e in encs}) > 1  # the longest one: the next token differs somewhere
    assert split_prefix(encs, cand) == [len(cand)] * len(encs)
    assert len(cand) <= server.PREFIX_CAPACITY
    # a query the probes do not cover still shares it
    other = tok.encode(server.build_prompt("zebra crossings: who invented them?"))
    assert other[: len(cand)] == cand
    ap = server.arg_parser()
    assert ap.parse_args([]).prefix_cache == "off" and ap.parse_args(["--prefix-cache", "on"]).prefix_cache == "on"
    with pytest.raises(ValueError):  # the torch reference engine has no prefix store
        server.make_engine("gpt2-tiny", "cpu", 2, 32, prefix_capacity=8)
    with pytest.raises(ValueError, match="tensor parallelism"):
        server.make_engine("gpt2-tiny", "cpu", 2, 32, prefix_capacity=8, tp_group=object())
    with pytest.raises(ValueError):
        server.enable_prefix_cache(server.make_engine("gpt2-tiny", "cpu", 2, 32), tok)


def test_planner_counts_the_prefix_store():
    from distributed_lms_raft_llm_amd.engine.memory import (GIB, kv_bytes, plan_max_batch, prefix_store_bytes,
                                                            slot_bytes)
    from distributed_lms_raft_llm_amd.models.config import gpt2_config

    cfg = gpt2_config("gpt2")
    assert prefix_store_bytes(cfg, 0) == 0
    assert prefix_store_bytes(cfg, 64) == 12 * 2 * 12 * 64 * 64 * 2 == kv_bytes(cfg, 64)
    assert prefix_store_bytes(cfg, 64, kv_dtype="fp8") * 2 == prefix_store_bytes(cfg, 64)
    # a budget that holds exactly 8 slots loses the eighth to the store
    fixed = 32768 * (cfg.n_embd * 4 * 9 + cfg.n_inner * 2 + cfg.n_embd * 6)
    free = 8 * slot_bytes(cfg, 150) + fixed + 1024
    kw = dict(weights_resident=True, reserve_frac=0.0, reserve_bytes=0)
    assert plan_max_batch(cfg, 150, free_bytes=free, **kw) == 8
    assert plan_max_batch(cfg, 150, free_bytes=free, prefix_capacity=64, **kw) == 4
    assert plan_max_batch(cfg, 150, free_bytes=free + prefix_store_bytes(cfg, 64) + 8 * 4, prefix_capacity=64, **kw) == 8
    assert plan_max_batch(cfg, 150, free_bytes=64 * GIB, prefix_capacity=64, weights_resident=True) == \
        plan_max_batch(cfg, 150, free_bytes=64 * GIB, weights_resident=True)  # a few MiB: the same bucket


@functools.lru_cache(maxsize=None)
def _reference(name, kv_dtype="bf16"):
    from distributed_lms_raft_llm_amd.models.gpt2 import GPT2Reference

    cfg, w = kc.setup(name)
    return cfg, GPT2Reference(cfg, w, device="cpu", kv_dtype=kv_dtype)


def test_fp8_reference_alone_clears_the_decisive_floor():
    """The fp8-cache engine test's floor: ``GPT2Reference(kv_dtype="fp8")`` on the same prompts at
    kv_fp8_cases.KV_FP8_EPS keeps 489 / 504 = 97.0 % of its positions decisive (P = 16)."""
    from distributed_lms_raft_llm_amd.models.gpt2 import reference_generate, teacher_forced_check_batch

    cfg, model = _reference("gpt2", "fp8")
    _, prompts = pc.prefix_and_prompts(cfg, 16)
    outs = reference_generate(model, prompts, max_length=pc.T, repetition_penalty=1.2)
    res = teacher_forced_check_batch(model, outs, [len(p) for p in prompts], 1.2, kc.KV_FP8_EPS["gpt2"])
    total, decisive = sum(r["positions"] for r in res), sum(r["decisive"] for r in res)
    print(f"fp8 reference: {decisive} / {total} positions decisive at eps {kc.KV_FP8_EPS['gpt2']}")
    assert not any(r["mismatches"] for r in res)
    assert decisive >= kc.MIN_DECISIVE["gpt2"] * total, (decisive, total)


@pytest.mark.parametrize("name", ["gpt2-tiny", "gpt2"])
@pytest.mark.parametrize("P", pc.P_VALUES)
def test_reference_alone_clears_the_decisive_floor(name, P):
    """The reference's own generations of the engine-test prompts, teacher-forced against itself:
    no mismatch, and at least 70 % of the positions decisive at eps = 0.05.
    Measured: gpt2-tiny P=16 / 13, GPT-2-124M P=16 / 13 -- see prefix_cases.py."""
    from distributed_lms_raft_llm_amd.models.gpt2 import reference_generate, teacher_forced_check_batch

    cfg, model = _reference(name)
    prefix, prompts = pc.prefix_and_prompts(cfg, P)
    assert len(prefix) == P and len(prompts) == 13 and max(map(len, prompts)) < pc.T
    assert split_prefix(prompts, prefix) == [P] * 8 + [0] * 5
    outs = reference_generate(model, prompts, max_length=pc.T, repetition_penalty=1.2)
    res = teacher_forced_check_batch(model, outs, [len(p) for p in prompts], 1.2, pc.EPS)
    total, decisive = sum(r["positions"] for r in res), sum(r["decisive"] for r in res)
    mism = sum(len(r["mismatches"]) for r in res)
    print(f"{name} P={P}: {decisive} / {total} positions decisive at eps {pc.EPS} ({100.0 * decisive / total:.1f} %), "
          f"{mism} mismatches")
    assert mism == 0
    assert total > 0 and decisive >= pc.MIN_DECISIVE * total, (decisive, total)
