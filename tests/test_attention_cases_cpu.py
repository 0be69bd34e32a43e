"""The attention structure tests bite: on the CPU, a pure-torch online softmax (attention_cases.emulate)
passes the comparators of attention_cases.py, and with ONE key dropped, doubled or read past kvlen,
one rescale skipped or two q chunks swapped it is rejected by the count or the comb family -- at
700 and 1024 cached keys, where atol = rtol = 2e-2 against randn data lets all of that through.
Also the builders' exactness claims and the measured constant of the random family."""
import pytest
import torch

import attention_cases as ac

H = 2
LENS = (700, 1024)
T = 1088  # one 64-key period past 1024, so that "one key past kvlen" exists at 1024 too


def _count(code, lens=LENS):
    return ac.count_case(H, code, T, lens)


def _comb(lens=LENS):
    return ac.comb_case(H, T, lens)


def _comb_bad(c, out):
    ref, _ = ac.reference(c.q, c.k, c.v, c.row_slot, c.row_kvlen)
    return ac.close_mismatches(out, ref)


def _rejected_by(fault):
    hits = []
    for code in "AB":
        c = _count(code)
        if ac.count_mismatches(ac.emulate(c, fault), c):
            hits.append("count " + code)
    c = _comb()
    if _comb_bad(c, ac.emulate(c, fault)):
        hits.append("comb")
    return hits


def test_existing_tolerance_misses_a_dropped_key():
    """The gap itself: on randn data, the fp32 reference with the last of 700 / 1024 keys dropped is
    within atol = rtol = 2e-2 of the true result in most heads (a head notices only when the
    dropped key happens to carry a large weight)."""
    c = ac.random_case(12, kvlens=LENS, rows_per_slot=1)
    ref, _ = ac.reference(c.q, c.k, c.v, c.row_slot, c.row_kvlen, torch.float32)
    got, _ = ac.reference(c.q, c.k, c.v, c.row_slot, c.row_kvlen - 1, torch.float32)
    unnoticed = ((got - ref).abs() <= 2e-2 + 2e-2 * ref.abs()).view(2, 12, 64).all(-1)
    print("heads whose dropped key goes unnoticed:", int(unnoticed.sum()), "of", unnoticed.numel())
    assert not torch.equal(got, ref) and int(unnoticed.sum()) > unnoticed.numel() // 2


@pytest.mark.parametrize("block", [8, 32, 96, 128])
def test_unfaulted_emulation_passes(block):
    for code in "AB":
        c = _count(code)
        assert ac.count_mismatches(ac.emulate(c, block=block), c) == []
    c = _comb()
    assert _comb_bad(c, ac.emulate(c, block=block)) == []
    c = ac.random_case(H)
    ref, _ = ac.reference(c.q, c.k, c.v, c.row_slot, c.row_kvlen)
    assert ac.close_mismatches(ac.emulate(c, block=block), ref, atol=ac.RANDOM_ATOL) == []


@pytest.mark.parametrize("fault", ac.FAULTS)
def test_fault_is_rejected(fault):
    hits = _rejected_by(fault)
    print(fault, "rejected by", hits)
    assert hits
    # the key-set faults change a count: the count family alone must see them
    if fault in ("drop_last", "drop_first", "drop_last8", "read_past", "double_at_span"):
        assert "count A" in hits
    else:  # q = 0 hides the score path: that is the comb family's
        assert hits == ["comb"]


@pytest.mark.parametrize("fault", ["drop_last", "drop_first", "drop_last8", "read_past", "double_at_span"])
@pytest.mark.parametrize("L", LENS)
def test_key_set_faults_are_rejected_at_each_length(fault, L):
    for code in "AB":
        c = _count(code, (L,))
        assert ac.count_mismatches(ac.emulate(c, fault), c), (fault, L, code)
    c = _comb((L,))
    assert _comb_bad(c, ac.emulate(c, fault)), (fault, L)


def test_one_ulp_is_the_count_familys_whole_allowance():
    c = _count("A")
    exp = ac.count_expected(c)
    assert ac.count_mismatches(exp, c) == []
    bits = exp.view(torch.int16)
    up = (bits + 1).view(torch.bfloat16)
    assert ac.count_mismatches(up, c) == []
    two = (bits + 2).view(torch.bfloat16)
    assert len(ac.count_mismatches(two, c)) > 0
    nan = exp.clone()
    nan[0, 0] = float("nan")
    assert ac.count_mismatches(nan, c)[0] == (0, 0)
    # code B's exact zeros (blocks past kvlen) must stay exactly zero
    cb = _count("B")
    eb = ac.count_expected(cb)
    assert bool((eb[0].float() == 0).any())
    eb = eb.clone()
    z = (eb[0].float() == 0).nonzero()[0, 0]
    eb[0, z] = 1e-30
    assert ac.count_mismatches(eb, cb) == [(0, int(z))]


def test_reciprocal_multiply_rounds_like_the_division():
    """For every L in 1..2048 and both codes, bf16(f32(count) * f32(1 / L)) == bf16(count / L): a
    kernel that multiplies by the f32 reciprocal hits the expected value bit for bit (the one-ulp
    allowance is for other summation / division choices)."""
    L = torch.arange(1, 2049)
    for code in (ac.code_a, ac.code_b):
        counts = torch.cumsum(code(2048).double(), 0)  # [L - 1, d]
        exact = (counts / L.double()[:, None]).to(torch.bfloat16)
        inv = (1.0 / L.float())
        mul = (counts.float() * inv[:, None]).to(torch.bfloat16)
        assert torch.equal(mul, exact)
        assert int(counts.max()) == 32


def test_values_are_exact_in_bf16_and_e4m3():
    cases = [ac.count_case(H, "A"), ac.count_case(H, "B"), _count("A"), _comb(), ac.random_case(H),
             ac.tile_count_case(H, "A"), ac.tile_comb_case(H, 1, -1.0), ac.tile_random_case(H),
             ac.comb_case(H, ac.LONG_T, tuple(ac.LONG_KVLENS), (0, 63))]
    for c in cases:
        assert torch.equal(c.q.to(torch.bfloat16).float(), c.q)
        for x in (c.k, c.v):
            assert bool(torch.isfinite(x).all())
            assert torch.equal(x.to(torch.bfloat16).float(), x)
            assert torch.equal(x.to(torch.float8_e4m3fn).float(), x)
            for kind in ("bf16", "fp8"):  # the NaN tail, and nothing but the tail
                cc = ac.cache(x, kind, c.slot_kvlen).float()
                if c.slot_kvlen is None:
                    assert torch.equal(cc, x)
                else:
                    for s, n in enumerate(c.slot_kvlen):
                        assert torch.equal(cc[s, :, :n], x[s, :, :n]) and bool(torch.isnan(cc[s, :, n:]).all())
    assert ac.KVLENS_FUSED == [1, 7, 9, 32, 63, 65, 128, 255, 257, 700, 1023, 1024]


def test_comb_scores_are_exactly_0_or_4():
    c = _comb()
    for dtype in (torch.float32, torch.float64):
        s = torch.einsum("rhd,htd->rht", c.q.view(-1, H, 64).to(dtype), c.k[0].to(dtype)) * ac.SCALE
        for r, (L, j, sign) in enumerate(c.rows):
            want = torch.zeros(c.T, dtype=dtype)
            want[j::64] = sign * ac.COMB_S
            assert torch.equal(s[r, 0], want) and torch.equal(s[r, H - 1], want)
    # the tile comb: row i (kvlen i + 1) carries residue (i + off) % 64
    t = ac.tile_comb_case(H, 1, 1.0)
    # the second sequence starts at packed row 1: row 1 + 16 has kvlen 17
    assert int(t.row_kvlen[1 + 16]) == 17 and t.q[1 + 16].view(H, 64)[0].nonzero().item() == (16 + 1) % 64


def test_random_atol_covers_the_measured_reference_error():
    worst = 0.0
    for c in (ac.random_case(5), ac.random_case(12), ac.random_case(5, ac.LONG_T, tuple(ac.LONG_KVLENS)),
              ac.tile_random_case(5)):
        a, _ = ac.reference(c.q, c.k, c.v, c.row_slot, c.row_kvlen, torch.float32)
        b, _ = ac.reference(c.q, c.k, c.v, c.row_slot, c.row_kvlen, torch.float64)
        d = float((a.double() - b).abs().max())
        print(c.H, c.T, tuple(c.q.shape), "max |f32 - f64|", d)
        worst = max(worst, d)
    assert ac.RANDOM_ATOL >= max(1e-5, 8 * worst)
    assert ac.RANDOM_ATOL <= 2 * max(1e-5, 8 * worst)  # and not padded beyond the measurement


def test_tile_rows_are_causal_packed_sequences():
    row_slot, row_kvlen, slot_kvlen = ac.tile_rows()
    assert row_slot.numel() == sum(ac.TILE_SEQ_LENS) and int(row_kvlen.max()) == 1024
    r = 0
    for L in ac.TILE_SEQ_LENS:
        assert row_kvlen[r:r + L].tolist() == list(range(1, L + 1)) and len(set(row_slot[r:r + L].tolist())) == 1
        assert slot_kvlen[int(row_slot[r])] == L
        r += L
