"""CPU proof that the cases of tests/gemm_cases.py bite: for every family of case, every K and row
count tests/test_gemm_exact_gpu.py runs and every fault model that applies to the family, the exact
comparison (the one-ulp GELU rule, the key comparison) REJECTS the faulty result in every affected
(row, 16-column group) block and accepts the reference; and what the randn / atol 3e-2 / rtol 2e-2
comparison of test_skinny_gpu.py / test_mid_gpu.py makes of the same faults at K = 768.

A fault can be invisible at single outputs (a zero weight, a bf16 output past 256 whose ulp is 2, an
e4m3 byte with 3 mantissa bits); a case counts as detecting it only when at least one output of
EVERY affected block differs.  That is asserted here for the seeds gemm_cases.py uses, so a later
change of seed or shape cannot hollow the GPU tests out."""
import pytest
import torch

import gemm_cases as gc

PRODUCT_FAULTS = ["drop_k", "double_k", "shift_slice", "swap_kblocks"]
OUTPUT_FAULTS = ["swap_groups", "tile_alias"]


def _ln(R, K, N=gc.N_LN, wdiv=1):
    return gc.addln_case(R, N, K, wdiv) if R == gc.ADDLN_R else gc.ln_case(R, N, K, wdiv)


def _family_cases():
    """(id, family, case, waves): family in bf16 / f32 / qkv_bf16 / qkv_fp8 / gelu."""
    out = []
    for R, K, waves in gc.ln_shapes():
        if R != gc.ADDLN_R:  # (skinny_addln_gemm has no plain bf16 epilogue)
            out.append((f"ln-bf16-R{R}-K{K}", "bf16", _ln(R, K), waves))
        out.append((f"ln-gelu-R{R}-K{K}", "gelu", _ln(R, K, wdiv=16), waves))
        for N in gc.N_QKV:
            for kind in ("bf16", "fp8"):
                out.append((f"ln-qkv-{kind}-R{R}-N{N}-K{K}", "qkv_" + kind, _ln(R, K, N), waves))
    for R, N, K, waves in gc.plain_shapes():
        c = gc.plain_case(R, N, K)
        out.append((f"plain-bf16-R{R}-K{K}", "bf16", c, waves))
        out.append((f"plain-f32-R{R}-K{K}", "f32", c, waves))  # in place, fixed point and partial slabs
        if R == gc.PS_R:
            out.append((f"plain-gelu-R{R}-K{K}", "gelu", gc.plain_case(R, N, K, 16), waves))
            out.append((f"plain-qkv-R{R}-K{K}", "qkv_bf16", gc.plain_case(R, gc.N_PS_QKV, K), waves))
    return out


FAMILY_CASES = _family_cases()


def _flags(family, case, v):
    """bool [M, N]: where the comparator of ``family`` rejects a kernel that stored round(v) (v: the
    pre-rounding output it computed, bias included) against the case's reference."""
    want = case.ref + case.bias
    if family == "bf16":
        return gc.bits(gc.rne_bf16(v)) != gc.bits(gc.rne_bf16(want))
    if family == "f32":
        return v.float() != want.float()
    if family.startswith("qkv_"):
        return gc.qkv_codes(v, family[4:]) != gc.qkv_codes(want, family[4:])
    assert family == "gelu"
    return gc.gelu_bad(gc.gelu_ref(v).to(torch.bfloat16), want)


@pytest.mark.parametrize("cid,family,case,waves", FAMILY_CASES, ids=[c[0] for c in FAMILY_CASES])
def test_reference_passes_and_every_fault_is_caught_in_every_block(cid, family, case, waves):
    assert not _flags(family, case, case.ref + case.bias).any()
    nkb = case.K // 32
    for fault in PRODUCT_FAULTS:
        if fault == "swap_kblocks" and nkb < 2:
            continue  # one k-block: nothing to swap
        prod, blocks = gc.mutate_product(fault, case.a, case.w, waves=max(1, waves))
        hits = gc.block_hits(_flags(family, case, prod + case.bias))
        assert blocks.any() and bool(hits[blocks].all()), (fault, int((blocks & ~hits).sum()), int(blocks.sum()))
        assert not hits[~blocks].any()
    for fault in OUTPUT_FAULTS:
        if fault == "tile_alias" and case.R <= 16:
            continue  # skinny_addln_gemm holds one row tile
        v, blocks = gc.mutate_output(fault, case.ref + case.bias)
        hits = gc.block_hits(_flags(family, case, v))
        assert bool(hits[blocks].all()), (fault, int((blocks & ~hits).sum()))
    if family == "gelu":  # gelu applied to the accumulator without the bias
        groups = (case.bias.reshape(-1, 16) != 0).any(1)
        assert groups.all()
        hits = gc.block_hits(_flags(family, case, case.ref))
        assert bool(hits.all()), int((~hits).sum())


@pytest.mark.parametrize("Kc,split", gc.PS_SPLITS)
def test_every_split_k_slab_catches_every_fault(Kc, split):
    """gemm_ps's partial slabs: slab s is compared with the product over ITS K slice of the K = Kc *
    split case; every product fault inside a slice is caught in every block of that slab."""
    full = gc.plain_case(gc.PS_R, gc.N_PS, Kc * split)
    for s_ in range(split):
        ks = slice(s_ * Kc, (s_ + 1) * Kc)
        a, w = full.a[:, ks], full.w[:, ks]
        slab = gc.Case(a=a, w=w, bias=torch.zeros(full.N, dtype=torch.float64), ref=a @ w.t(), R=full.R, N=full.N, K=Kc)
        assert not _flags("f32", slab, slab.ref).any()
        for fault in PRODUCT_FAULTS:
            prod, blocks = gc.mutate_product(fault, a, w, waves=1)
            hits = gc.block_hits(_flags("f32", slab, prod))
            assert bool(hits[blocks].all()) and not hits[~blocks].any(), (s_, fault)
        for fault in OUTPUT_FAULTS:
            v, blocks = gc.mutate_output(fault, slab.ref)
            assert bool(gc.block_hits(_flags("f32", slab, v))[blocks].all()), (s_, fault)


QKV_CASES = [c for c in FAMILY_CASES if c[1].startswith("qkv_")]


@pytest.mark.parametrize("cid,family,case,waves", QKV_CASES, ids=[c[0] for c in QKV_CASES])
def test_a_row_scattered_to_the_next_position_is_caught(cid, family, case, waves):
    kind = family[4:]
    M, S, T = case.R, case.R + 3, 11
    slot, pos = gc.scatter_plan(M, S, T)
    v = case.ref + case.bias
    want = gc.qkv_expected(v, slot, pos, S, T, kind)
    again = gc.qkv_expected(v, slot, pos, S, T, kind)
    assert all(gc.same(a, b) for a, b in zip(want, again))
    for r in range(M):
        if int(pos[r]) + 1 >= T:
            continue
        wrong = pos.clone()
        wrong[r] += 1
        got = gc.qkv_expected(v, slot, wrong, S, T, kind)
        assert not gc.same(got[1], want[1]) and not gc.same(got[2], want[2])
        # ... at both places: the intended position keeps its sentinel, the next one loses it
        s = int(slot[r])
        assert not gc.same(got[1][s, :, int(pos[r])], want[1][s, :, int(pos[r])])
        assert not gc.same(got[1][s, :, int(pos[r]) + 1], want[1][s, :, int(pos[r]) + 1])


ARGMAX_CASES = gc.argmax_shapes()


@pytest.mark.parametrize("R,N,K,vocab,ln", ARGMAX_CASES, ids=[f"R{r}-N{n}-K{k}-ln{int(l)}" for r, n, k, _, l in ARGMAX_CASES])
def test_argmax_cases_catch_tie_vocab_and_logit_faults(R, N, K, vocab, ln):
    case = gc.argmax_case(R, N, K, vocab, ln)
    tok, val = gc.argmax_expected(case.logits, case.seen, vocab)
    # the kinds of tie the builder promises: inside a 16-column group, inside a 64-column key
    # group, across key groups (rows r % 4 == 0, 1 / 2, 3)
    for r in range(min(R, 8)):
        a, b = case.cands[r % 4], case.cands[r % 4 + 1]
        assert int(tok[r]) == a
        assert (a // 16 == b // 16) == (r % 4 == 0) and (a // 64 == b // 64) == (r % 4 < 3)
    # some rows' unpenalised maximum is seen
    raw = case.logits[:, :vocab].argmax(1)
    assert bool(case.seen[torch.arange(R), raw].any()) and not bool(case.seen[torch.arange(R), raw].all())
    # faults: every row has a tie to break the wrong way and a larger padding column to fall for
    hi_tok, _ = gc.argmax_expected(case.logits, case.seen, vocab, highest=True)
    assert bool((hi_tok != tok).all())
    nv_tok, _ = gc.argmax_expected(case.logits, case.seen, vocab, use_vocab=False)
    assert bool((nv_tok != tok).all()) and bool((nv_tok >= vocab).all())
    no_pen, _ = gc.argmax_expected(case.logits, torch.zeros_like(case.seen), vocab)
    assert bool((no_pen != tok)[torch.arange(R) % 4 != 0].all())
    keys = gc.make_keys(val, tok)
    assert torch.equal(gc.key_token(keys), tok) and torch.equal(gc.key_high(keys), gc.f32_ordered(val))


def _groupings(R, N):
    """The column sets per key of every launch test_gemm_exact_gpu.py makes at this shape."""
    if R == gc.SKINNY_R:
        return [gc.key_groups64(N)]
    return [gc.ps_slot_groups(N, nt, cw) for nt in (1, 2) for cw in (1, 3)]


@pytest.mark.parametrize("R,N,K,vocab,ln", ARGMAX_CASES, ids=[f"R{r}-N{n}-K{k}-ln{int(l)}" for r, n, k, _, l in ARGMAX_CASES])
def test_argmax_keys_catch_every_product_and_output_fault(R, N, K, vocab, ln):
    """The logits are a GEMM: every fault of the product and of the store must change the KEYS the
    kernels write -- per (row, key column set), wherever the set's expected winner sits in an affected
    16-column block -- and every row's reduced key.  (A key is (value, column) of the set's maximum: it
    survives a fault only if the winner's logit is computed right, so 'affected' is decided from the
    fault's blocks, and the construction -- a candidate in every 64-column group, k-blocks of different
    weight -- must make the wrong logit differ: that is what a seed could hollow out.)"""
    case = gc.argmax_case(R, N, K, vocab, ln)
    tok, val = gc.argmax_expected(case.logits, case.seen, vocab)
    reduced = gc.make_keys(val, tok)
    cand_blocks = sorted({c // 16 for c in case.cands})
    faults = [("drop_k", b) for b in cand_blocks] + [("double_k", b) for b in cand_blocks] + [("shift_slice", 0)]
    if K >= 64:
        faults.append(("swap_kblocks", 0))
    faults += [("swap_groups", 0), ("tile_alias", 0)]
    bit = {}
    for fault, blk in faults:
        if fault in ("swap_groups", "tile_alias"):
            logits, blocks = gc.mutate_output(fault, case.logits)
        else:
            logits, blocks = gc.mutate_product(fault, case.a, case.w, waves=4 if R == gc.SKINNY_R else 1, group=blk)
        wrong = gc.block_hits(logits != case.logits)
        assert not wrong[~blocks].any()
        # every row whose winner sits in an affected block: the reduced key changes
        t2, v2 = gc.argmax_expected(logits, case.seen, vocab)
        hit_rows = blocks[torch.arange(R), tok // 16]
        if fault in ("shift_slice", "swap_kblocks", "tile_alias"):
            assert bool(hit_rows.all() if fault != "tile_alias" else hit_rows[16:].all())
        assert bool((gc.make_keys(v2, t2) != reduced)[hit_rows].all()), (fault, blk)
        if fault in ("drop_k", "double_k") and blk == 0:
            assert bool(hit_rows[torch.arange(R) % 4 < 2].all())
        # ... and per key: every (row, column set) whose expected winner sits in an affected block
        for groups in _groupings(R, N):
            want = gc.group_keys(case.logits, case.seen, vocab, groups)
            got = gc.group_keys(logits, case.seen, vocab, groups)
            wcol = gc.key_token(want)
            live = want != 0
            hit = live & blocks[torch.arange(R)[:, None].expand_as(wcol), (wcol // 16).clamp(max=N // 16 - 1)]
            bit[fault] = bit.get(fault, False) or bool(hit.any())  # (a block such as 97's never holds a winner)
            # sets won by a candidate: always.  A set without one (gemm_ps slots of 16 or 32 columns) is won
            # by a random column whose logit moves by a random integer, which may be 0: nearly always.
            cand = torch.isin(wcol, torch.tensor(case.cands))
            assert bool((got != want)[hit & cand].all()), (fault, blk, int(((got == want) & hit & cand).sum()))
            assert not hit.any() or float((got != want)[hit].float().mean()) > 0.95, (fault, blk)
            if fault in ("shift_slice", "swap_kblocks"):  # every key of every row that has a valid column
                assert bool(hit[live].all())
    assert all(bit[f] for f, _ in faults), bit


def test_f32_ordered_is_monotone():
    v = torch.tensor([-3e38, -7.0, -1.5, -1e-30, 0.0, 1e-30, 0.5, 2.0, 65536.0, 3e38])
    o = gc.f32_ordered(v)
    assert bool((o[1:] > o[:-1]).all()) and int(o.min()) >= 0 and int(o.max()) < 2 ** 32


def test_gelu_rule_accepts_fp32_evaluations_and_the_limits():
    """The kernels' formula evaluated in fp32 by torch is within the rule on the grid v = -10 ... 25
    step 1/16 (0 ulp from the fp64 sigmoid form); fp64 tanh-form cancels to -0.0 far below zero, which
    the rule accepts only below -8."""
    v = torch.arange(-160, 401, dtype=torch.float64)[None, :] / 16
    x = v.float()
    u = torch.tensor(gc.K0, dtype=torch.float32) * (x + torch.tensor(gc.K1, dtype=torch.float32) * x * x * x)
    out = (x / (1.0 + torch.exp(-2.0 * u))).to(torch.bfloat16)
    assert not gc.gelu_bad(out, v).any()
    assert int((gc._ordered(out) - gc._ordered(gc.gelu_ref(v).to(torch.bfloat16))).abs().max()) == 0
    assert not gc.gelu_bad(torch.full_like(out, -0.0), v)[v < -8].any()
    assert gc.gelu_bad(torch.full_like(out, -0.0), v)[(v >= -8) & (v != 0)].all()


# ------------------------------------------------------------------------------------------------
# what the old comparison makes of the same faults
# ------------------------------------------------------------------------------------------------
def _randn_case(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).to(torch.bfloat16).double()
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16).double()
    return a, w


def _old_passes(out64, ref64):
    out, ref = out64.float().to(torch.bfloat16).float(), ref64.float()
    return bool(((out - ref).abs() <= 3e-2 + 2e-2 * ref.abs()).all())


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("fault", ["drop_k", "double_k"])
def test_old_tolerance_passes_a_lost_or_doubled_element(fault, seed):
    """K = 768, randn A, W of scale 0.05, one row (the batch-1 decode shape every old test runs): in
    EVERY k-block there is a k-element whose loss / doubling for a whole 16-column group passes the
    old comparison entirely (the smallest |a_k| of the block: the fault moves the outputs by
    |a_k w_nk|, the allowance is 0.03 + 0.02 |out|), and at 17 rows four out of five affected
    outputs pass.  The integer case of the same shape flags every k-element of every block."""
    K, N = 768, 96
    a, w = _randn_case(1, N, K, seed)
    ref = a @ w.t()
    cols = slice(16, 32)
    for kb in range(K // 32):
        k = 32 * kb + int(a[0, 32 * kb:32 * kb + 32].abs().argmin())
        out = ref.clone()
        out[:, cols] += (1 if fault == "double_k" else -1) * a[:, k:k + 1] * w[cols, k][None, :]
        assert _old_passes(out, ref), kb
    a17, w17 = _randn_case(17, N, K, seed)
    prod, blocks = gc.mutate_product(fault, a17, w17)
    out, ref17 = prod.float().to(torch.bfloat16).float(), (a17 @ w17.t()).float()
    passed = ((out - ref17).abs() <= 3e-2 + 2e-2 * ref17.abs())[:, cols]
    assert float(passed.float().mean()) > 0.7
    c = gc.ln_case(gc.SKINNY_R, gc.N_LN, K).rows(1)
    want = gc.rne_bf16(c.ref + c.bias)
    sign = 1 if fault == "double_k" else -1
    for k in range(K):
        v = c.ref + c.bias
        v[:, cols] = v[:, cols] + sign * c.a[:, k:k + 1] * c.w[cols, k][None, :]
        assert not gc.same(gc.rne_bf16(v), want), k


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_old_tolerance_against_a_shifted_k_slice(seed):
    """A wave's K slice shifted by one k-block replaces 32 products by 32 others: on randn data that
    moves an output by about sqrt(64) * 0.05 = 0.4, several times the old allowance, so the old
    comparison does reject it at 17 rows -- but one output in five still passes (|delta| below
    0.03 + 0.02 |out|), where the exact comparison flags every block."""
    a, w = _randn_case(17, 96, 768, seed)
    prod, _ = gc.mutate_product("shift_slice", a, w, waves=4)
    ref = a @ w.t()
    assert not _old_passes(prod, ref)
    out = prod.float().to(torch.bfloat16).float()
    passed = (out - ref.float()).abs() <= 3e-2 + 2e-2 * ref.float().abs()
    assert 0.02 < float(passed.float().mean()) < 0.5
