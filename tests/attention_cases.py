"""Shared by tests/test_attention_cases_cpu.py and tests/test_attention_structure_gpu.py: inputs, an
fp64 reference and comparators for the attention kernels that notice ONE missing, doubled or extra
key at any cache length.  Plain torch only; every function runs where its inputs live.

Why: the other attention tests compare randn inputs against an fp32 softmax with atol = rtol = 2e-2.
At 700 cached keys a dropped key moves a randn output by 0.003 and a dropped group of 8 by 0.02:
both pass.  The three families below leave the kernels (almost) no rounding, so the bounds can be
a few bf16 ulps.

All K / V values are exactly representable in bf16 AND in OCP e4m3 (``cache`` asserts it), so one
builder serves the bf16 cache and the fp8 byte cache and one reference serves both.

count   q = 0: every score is exactly 0, every weight exactly 1 / L.  K is arbitrary finite data.  V is
        position-coded: code "A" V[t, d] = [t % 64 == d], code "B" V[t, d] = [t // 32 == d] (T <= 2048).
        Every partial sum in a kernel (l, acc, the merges: exp2(0) = 1) is then a small integer in f32
        and the output is count_d / L, rounded once (reciprocal, product, bf16 store).  A dropped,
        doubled or extra key moves one output of code A by >= 1/32 relative (count_d <= 32); code B
        says which 32-key block it belonged to.
comb    K[t, d] = [t % 64 == d].  Row (L, j, +-) has q = +-8 S e_j (S = 4) in every head: under the
        scale 1/8 its scores are exactly +-4 on keys t = j (mod 64) and exactly 0 elsewhere.  V is code
        B.  All rows share one slot.  Over j = 0..63 the key that lifts the running maximum sits at
        every position of every unroll block, wave span and workgroup span: the dot product's
        dimension indexing, the rescale of the partial sums at every merge level, the masking at kvlen.
random  randn q, K, V (V doubled), one kvlen per slot, NaN in every K / V element past it.

Tolerances (relative to the fp64 softmax of the same tensors), derived, not fitted:
  * A bf16 store is one round-to-nearest: relative error <= 2^-8 (half an ulp of a value just above
    a power of two).  exp2f, the f32 reciprocal and the f32 sums add relative errors near 1e-6
    (positive terms only in the count and comb families: no cancellation).
  * count: the output must lie within ONE bf16 ulp of bf16(count_d / L) (bit distance <= 1): the
    single rounding can fall on either side of the correctly rounded quotient when a kernel
    multiplies by the rounded reciprocal instead of dividing.  (For L <= 2048 and both codes
    bf16(f32(count) * f32(1 / L)) == bf16(count / L) bit for bit: test_attention_cases_cpu.py.)
  * comb, random: |out - ref| <= 2^-7 |ref|  ("two bf16 ulps": 2^-8 for the store, the rest
    headroom for exp2f and the reciprocal) -- REL below.
  * tile_attention rounds P to bf16 (relative 2^-8 per weight) ahead of the P.V product while l
    sums the unrounded weights: + 2^-8 (P . |V|), P.|V| from the same reference -- TILE_P_REL.
  * the fused attention + out-projection kernels round the head output to bf16 and pass it through
    an MFMA with W_o = I: one more bf16 ulp, i.e. bit distance <= 2 (count), + 2^-8 |ref| -- ULP_REL.
  * random only: + RANDOM_ATOL, the cancellation floor, measured on the reference alone (below).
"""
import functools
import math

import torch

KVLENS = [1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 700, 1023, 1024]
T_MAX = 1024
# the fused attention + out-projection kernels take 1..4 rows per call: every second kvlen, and
# always 700, 1023 and 1024; comb residues around the 8-key groups and the 32-key blocks
KVLENS_FUSED = sorted(set(KVLENS[::2]) | {700, 1023, 1024})
RESIDUES_FUSED = [0, 7, 8, 31, 32, 63]
TILE_SEQ_LENS = [1, 17, 33, 257, 1024]
LONG_T, LONG_KVLENS = 2048, [2047, 2048]  # the LDS kernel's limit
COMB_S = 4.0
SCALE = 1.0 / 8.0

NAN_BYTE = 0x7F    # e4m3fn NaN
NAN_BF16 = 0x7FC0  # bf16 quiet NaN

REL = 2.0 ** -7
ULP_REL = 2.0 ** -8
TILE_P_REL = 2.0 ** -8

# The random family's absolute term: 8 x the largest |fp32 reference - fp64 reference| over the
# random cases below (the factor 8: a kernel sums the same products in another order, in blocks, and
# merges partials), floored at 1e-5.  Measured on the CPU, reference against reference:
#   random_case(5)  (20 slots, T 1024, 40 rows)      max |f32 - f64| = 5.6e-07
#   random_case(12) (20 slots, T 1024, 40 rows)      max |f32 - f64| = 7.6e-07
#   random_case(5, LONG_T, LONG_KVLENS) (4 rows)     max |f32 - f64| = 2.3e-07
#   tile_random_case(5) (1332 causal rows)           max |f32 - f64| = 9.1e-07
# 8 x 9.1e-07 = 7.3e-06 -> the floor.  test_attention_cases_cpu.py recomputes these and asserts the
# constant is not smaller.
RANDOM_ATOL = 1e-5


# ------------------------------------------------------------------------------------------------
# builders
# ------------------------------------------------------------------------------------------------
class Case(dict):
    """q fp32 [R, H*64] (bf16-exact); k, v fp32 [S, H, T, 64] (bf16- and e4m3-exact, finite
    everywhere); row_slot, row_kvlen int32 [R]; slot_kvlen (list, or None): the valid keys per slot,
    past which ``cache`` puts NaN; H, T; and what the family needs (code, rows)."""

    __getattr__ = dict.__getitem__


def code_a(T):
    t = torch.arange(T)
    return (t[:, None] % 64 == torch.arange(64)[None, :]).float()


def code_b(T):
    assert T <= 2048
    t = torch.arange(T)
    return (t[:, None] // 32 == torch.arange(64)[None, :]).float()


def _finite_e4m3(shape, g):
    """Arbitrary finite e4m3 values (every byte but the two NaNs), as fp32."""
    b = torch.randint(0, 256, shape, generator=g, dtype=torch.int32)
    b = torch.where((b & 0x7F) == 0x7F, b - 1, b)  # 0x7F / 0xFF are NaN: +-448 instead
    return b.to(torch.uint8).view(torch.float8_e4m3fn).float()


def _quant(x):
    """randn values onto the e4m3 grid (through bf16, saturated: the fp8 cache's own quantiser)."""
    return x.to(torch.bfloat16).float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float()


@functools.lru_cache(maxsize=None)
def count_case(H, code, T=T_MAX, kvlens=tuple(KVLENS), seed=0):
    """One row per kvlen, all on slot 1 of 2 (slot 0 holds other data: a kernel that ignores row_slot
    fails)."""
    g = torch.Generator().manual_seed(1000 + seed + H)
    k = _finite_e4m3((2, H, T, 64), g)
    pos = code_a(T) if code == "A" else code_b(T)
    v = torch.empty(2, H, T, 64)
    v[1] = pos
    v[0] = 1.0 - pos
    R = len(kvlens)
    return Case(q=torch.zeros(R, H * 64), k=k, v=v, row_slot=torch.ones(R, dtype=torch.int32),
                row_kvlen=torch.tensor(kvlens, dtype=torch.int32), slot_kvlen=None, H=H, T=T, code=code)


def comb_rows(kvlens, residues):
    return [(L, j, s) for L in kvlens for j in residues for s in (1.0, -1.0)]


def comb_kv(H, T):
    return code_a(T).expand(1, H, T, 64).contiguous(), code_b(T).expand(1, H, T, 64).contiguous()


def comb_q(H, js, signs):
    q = torch.zeros(len(js), H, 64)
    r = torch.arange(len(js))
    q[r, :, torch.as_tensor(js)] = (8.0 * COMB_S * torch.as_tensor(signs, dtype=torch.float32))[:, None]
    return q.reshape(len(js), H * 64)


@functools.lru_cache(maxsize=None)
def comb_case(H, T=T_MAX, kvlens=tuple(KVLENS), residues=tuple(range(64))):
    rows = comb_rows(kvlens, residues)
    k, v = comb_kv(H, T)
    return Case(q=comb_q(H, [j for _, j, _ in rows], [s for _, _, s in rows]), k=k, v=v,
                row_slot=torch.zeros(len(rows), dtype=torch.int32),
                row_kvlen=torch.tensor([L for L, _, _ in rows], dtype=torch.int32), slot_kvlen=None, H=H, T=T,
                rows=rows)


@functools.lru_cache(maxsize=None)
def random_case(H, T=T_MAX, kvlens=tuple(KVLENS), rows_per_slot=2, seed=0):
    """Slot s holds kvlens[s] keys (NaN beyond, once through ``cache``); rows visit the slots in a
    permuted order, ``rows_per_slot`` times."""
    g = torch.Generator().manual_seed(2000 + seed + H + T)
    S = len(kvlens)
    k = _quant(torch.randn(S, H, T, 64, generator=g))
    v = _quant(torch.randn(S, H, T, 64, generator=g) * 2)
    R = S * rows_per_slot
    q = torch.randn(R, H * 64, generator=g).to(torch.bfloat16).float()
    slot = torch.cat([torch.randperm(S, generator=g) for _ in range(rows_per_slot)]).to(torch.int32)
    return Case(q=q, k=k, v=v, row_slot=slot, row_kvlen=torch.tensor(kvlens, dtype=torch.int32)[slot.long()],
                slot_kvlen=list(kvlens), H=H, T=T)


def tile_rows(lens=tuple(TILE_SEQ_LENS)):
    """Packed causal sequences, sequence b in slot (3 b + 1) % (n + 2): row_slot, row_kvlen (row i of
    a sequence attends i + 1 keys) and the valid keys per slot."""
    n = len(lens)
    slots = [(3 * b + 1) % (n + 2) for b in range(n)]
    assert len(set(slots)) == n
    row_slot = torch.tensor([slots[b] for b, L in enumerate(lens) for _ in range(L)], dtype=torch.int32)
    row_kvlen = torch.tensor([i + 1 for L in lens for i in range(L)], dtype=torch.int32)
    slot_kvlen = [1] * (n + 2)
    for b, L in enumerate(lens):
        slot_kvlen[slots[b]] = L
    return row_slot, row_kvlen, slot_kvlen


@functools.lru_cache(maxsize=None)
def tile_count_case(H, code, T=T_MAX, lens=tuple(TILE_SEQ_LENS), seed=0):
    g = torch.Generator().manual_seed(3000 + seed + H)
    row_slot, row_kvlen, slot_kvlen = tile_rows(lens)
    S = len(slot_kvlen)
    pos = code_a(T) if code == "A" else code_b(T)
    return Case(q=torch.zeros(row_slot.numel(), H * 64), k=_finite_e4m3((S, H, T, 64), g),
                v=pos.expand(S, H, T, 64).contiguous(), row_slot=row_slot, row_kvlen=row_kvlen, slot_kvlen=None, H=H,
                T=T, code=code, lens=list(lens))


# residue of row i (kvlen i + 1) is (i + off) % 64: off 0 puts the comb on the row's LAST key, 63 on
# the one before, 1 on the first MASKED key (a kernel that reads one key too many meets a +-4 there),
# 33 half a period away
TILE_COMB_OFFSETS = [0, 1, 33, 63]


@functools.lru_cache(maxsize=None)
def tile_comb_case(H, off, sign, T=T_MAX, lens=tuple(TILE_SEQ_LENS)):
    row_slot, row_kvlen, slot_kvlen = tile_rows(lens)
    S = len(slot_kvlen)
    k, v = comb_kv(H, T)
    js = ((row_kvlen - 1 + off) % 64).tolist()
    return Case(q=comb_q(H, js, [sign] * len(js)), k=k.expand(S, H, T, 64).contiguous(),
                v=v.expand(S, H, T, 64).contiguous(), row_slot=row_slot, row_kvlen=row_kvlen, slot_kvlen=None, H=H, T=T,
                lens=list(lens))


@functools.lru_cache(maxsize=None)
def tile_random_case(H, T=T_MAX, lens=tuple(TILE_SEQ_LENS), seed=0):
    g = torch.Generator().manual_seed(4000 + seed + H)
    row_slot, row_kvlen, slot_kvlen = tile_rows(lens)
    S = len(slot_kvlen)
    k = _quant(torch.randn(S, H, T, 64, generator=g))
    v = _quant(torch.randn(S, H, T, 64, generator=g) * 2)
    q = torch.randn(row_slot.numel(), H * 64, generator=g).to(torch.bfloat16).float()
    return Case(q=q, k=k, v=v, row_slot=row_slot, row_kvlen=row_kvlen, slot_kvlen=slot_kvlen, H=H, T=T,
                lens=list(lens))


def cache(values, kind, slot_kvlen=None):
    """The cache tensor a kernel reads: bf16, or the e4m3 byte cache -- the exact conversion of
    ``values`` (asserted) -- with NaN in every element at positions >= slot_kvlen[slot]."""
    dt = {"bf16": torch.bfloat16, "fp8": torch.float8_e4m3fn}[kind]
    c = values.to(dt)
    assert torch.equal(c.float(), values), "values must be exact in " + kind
    if slot_kvlen is not None:
        tail = torch.arange(values.shape[2])[None, :] >= torch.tensor(slot_kvlen)[:, None]  # [S, T]
        tail = tail[:, None, :, None].expand_as(values)
        if kind == "bf16":
            c.view(torch.int16)[tail] = NAN_BF16
        else:
            c.view(torch.uint8)[tail] = NAN_BYTE
        assert bool(torch.isnan(c.float()[tail]).all())
    return c


# ------------------------------------------------------------------------------------------------
# reference
# ------------------------------------------------------------------------------------------------
def reference(q, k, v, row_slot, row_kvlen, dtype=torch.float64, scale=SCALE):
    """Plain softmax attention of row r over keys [0, row_kvlen[r]) of slot row_slot[r], evaluated
    in ``dtype``.  Returns (out, P . |V|), both [R, H*64]."""
    S, H, T, _ = k.shape
    R = q.shape[0]
    out = torch.zeros(R, H * 64, dtype=dtype, device=q.device)
    pav = torch.zeros_like(out)
    t = torch.arange(T, device=q.device)
    for s in row_slot.unique().tolist():
        rows = (row_slot == s).nonzero()[:, 0]
        for r0 in range(0, rows.numel(), 512):  # bound the [rows, H, T] score tensor
            rr = rows[r0:r0 + 512]
            L = int(row_kvlen[rr].max())
            K, V = k[s, :, :L].to(dtype), v[s, :, :L].to(dtype)
            sc = torch.einsum("rhd,htd->rht", q[rr].to(dtype).view(-1, H, 64), K) * scale
            sc = sc.masked_fill(t[None, None, :L] >= row_kvlen[rr][:, None, None], float("-inf"))
            p = torch.softmax(sc, -1)
            out[rr] = torch.einsum("rht,htd->rhd", p, V).reshape(-1, H * 64)
            pav[rr] = torch.einsum("rht,htd->rhd", p, V.abs()).reshape(-1, H * 64)
    return out, pav


def count_expected(case):
    """bf16(count_d / L) per row, [R, H*64] bf16: count_d = the valid keys whose code hits dim d."""
    v = case.v[case.row_slot.long()[0], 0].double()  # [T, 64], the same in every head
    counts = torch.cumsum(v, 0)[case.row_kvlen.long() - 1]  # [R, 64]
    exp = (counts / case.row_kvlen.double()[:, None]).to(torch.bfloat16)
    return exp.repeat(1, case.H)


# ------------------------------------------------------------------------------------------------
# comparators: each returns the list of failing (row, column) pairs, worst first (empty: pass)
# ------------------------------------------------------------------------------------------------
def _ordered(x_bf16):
    """bf16 bit patterns as integers ordered like the values (+0 and -0 both 0)."""
    i = x_bf16.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def _report(bad, score):
    idx = bad.nonzero()
    order = score[bad].argsort(descending=True)
    return [tuple(i) for i in idx[order][:8].tolist()]


def count_mismatches(out, case, ulps=1):
    """``out`` [R, H*64] bf16 against bf16(count_d / L): bit distance <= ulps, exact zeros stay
    exactly zero, everything finite."""
    out = out.detach().cpu()
    assert out.dtype == torch.bfloat16
    exp = count_expected(case)
    dist = (_ordered(out) - _ordered(exp)).abs()
    bad = ~torch.isfinite(out.float()) | (dist > ulps) | ((exp.float() == 0) & (out.float() != 0))
    return _report(bad, dist.float() + 1e6 * (~torch.isfinite(out.float())).float())


def close_mismatches(out, ref, pav=None, rel=REL, p_rel=0.0, atol=0.0):
    """|out - ref| <= rel |ref| + p_rel (P . |V|) + atol, everything finite.  ``ref`` / ``pav``: the
    fp64 ``reference``."""
    out = out.detach().double().cpu()
    ref = ref.cpu()
    tol = rel * ref.abs() + atol
    if p_rel:
        tol = tol + p_rel * pav.cpu()
    err = (out - ref).abs()
    bad = ~torch.isfinite(out) | (err > tol)
    return _report(bad, torch.where(torch.isfinite(err), err / (tol + 1e-300), torch.full_like(err, math.inf)))


# ------------------------------------------------------------------------------------------------
# a pure-torch online softmax with fault switches: what the comparators must reject
# ------------------------------------------------------------------------------------------------
FAULTS = ["drop_last", "drop_first", "drop_last8", "read_past", "double_at_span", "skip_rescale", "swap_q_chunks"]


def emulate(case, fault=None, block=32, waves=4):
    """The kernels' scheme in fp32: q * scale * log2(e), keys in blocks of ``block`` with one
    running (m, l, acc) rescaled per block, exp2, one reciprocal, one bf16 store.  The keys past
    kvlen are whatever ``case.k`` / ``case.v`` hold (finite), as in an un-NaN'd cache.

    fault: drop_last / drop_first / drop_last8 -- keys [0, L-1) / [1, L) / [0, L-8);
    read_past -- keys [0, L+1); double_at_span -- the first key of the second of ``waves`` spans
    (rounded to 8, as attn_split_kernel's) is accumulated twice; skip_rescale -- acc misses its
    ``*= corr`` the first time the maximum rises; swap_q_chunks -- dims 24..31 and 32..39 of q swapped."""
    assert fault is None or fault in FAULTS
    out = torch.empty(case.q.shape[0], case.H * 64, dtype=torch.bfloat16)
    for s in case.row_slot.unique().tolist():
        rows = (case.row_slot == s).nonzero()[:, 0]
        out[rows] = _emulate_slot(case.q[rows], case.k[s], case.v[s], case.row_kvlen[rows].long(), fault, block, waves)
    return out


def _emulate_slot(q, k, v, L, fault, block, waves):
    H, T, _ = k.shape
    q = q.view(-1, H, 8, 8).clone()
    if fault == "swap_q_chunks":
        q[:, :, [3, 4]] = q[:, :, [4, 3]]
    q = q.reshape(-1, H, 64) * torch.tensor(SCALE * 1.4426950408889634, dtype=torch.float32)
    R = q.shape[0]
    lo = torch.zeros_like(L)
    hi = L.clone()
    if fault == "drop_last":
        hi = (L - 1).clamp(min=1)
    elif fault == "drop_first":
        lo = torch.where(L > 1, 1, 0)
    elif fault == "drop_last8":
        hi = torch.where(L > 8, L - 8, L)
    elif fault == "read_past":
        hi = (L + 1).clamp(max=T)
    span = ((L + waves - 1) // waves + 7) & ~7
    m = torch.full((R, H), -math.inf)
    l = torch.zeros(R, H)
    acc = torch.zeros(R, H, 64)
    skipped = torch.zeros(R, H, dtype=torch.bool)
    for t0 in range(0, int(hi.max()), block):
        t = torch.arange(t0, min(t0 + block, T))
        K, V = k[:, t], v[:, t]  # [H, b, 64]
        s = torch.einsum("rhd,hbd->rhb", q, K)
        valid = (t[None, :] >= lo[:, None]) & (t[None, :] < hi[:, None])  # [R, b]
        s = s.masked_fill(~valid[:, None, :], -math.inf)
        m_new = torch.maximum(m, s.max(-1).values)
        live = m_new > -math.inf
        m_safe = torch.where(live, m_new, torch.zeros_like(m_new))
        corr = torch.where(live, torch.exp2(m - m_safe), torch.ones_like(m))
        p = torch.exp2(s - m_safe[..., None])
        if fault == "double_at_span":
            p = p * torch.where((t[None, :] == span[:, None]) & valid, 2.0, 1.0)[:, None, :]
        acc_corr = corr
        if fault == "skip_rescale":
            rises = (m_new > m) & (m > -math.inf) & ~skipped
            acc_corr = torch.where(rises, torch.ones_like(corr), corr)
            skipped |= rises
        acc = acc * acc_corr[..., None] + torch.einsum("rhb,hbd->rhd", p, V)
        l = l * corr + p.sum(-1)
        m = m_new
    return (acc * (1.0 / l)[..., None]).reshape(R, H * 64).to(torch.bfloat16)
