"""Shared by tests/test_gemm_cases_cpu.py and tests/test_gemm_exact_gpu.py: inputs, fp64 references,
comparators and fault models for the skinny (skinny.hip), mid-batch (mid.hip) and persistent
(gemm_ps.hip) decode GEMMs that notice ONE wrong k-element.  Plain torch / numpy only.

Why: the other tests of these kernels compare randn data with atol = 3e-2, rtol = 2e-2.  At K = 768
and weights of scale 0.05 one dropped or doubled k-element moves an output by about 0.05 and the
allowance at a typical output (|out| ~ 1.4) is 0.03 + 0.02 * 1.4 = 0.06: four of five outputs of a
kernel that loses one element of one wave's K slice pass (test_gemm_cases_cpu.py shows it).  The
families below leave the kernels no rounding at all ahead of the final store, so the comparison can
be equality.

Operands.  A, W and every bias are integers: W in [-3, 3], a plain bf16 A in [-4, 4] without 0 (a
zero factor would hide a lost element from a whole output row), biases in [-3, 3].  Every product is
an integer of magnitude <= 12 and for K <= 6400 every partial sum is an integer below
12 * 6400 + 3 < 2^24 (each builder asserts |ref|max + |bias|max < 2^24 on its own data), exact in
fp32 in ANY summation order: the kernel's split of K over waves, its MFMA order and its LDS
reduction cannot matter.  The reference is the fp64 product, rounded ONCE to nearest-even for a
bf16 output (``rne_bf16``) and not at all for fp32 outputs.  Cases are built once at the largest row
count a kernel takes and sliced (``Case.rows``), so the row-block checks of the CPU proof hold for
every M the GPU tests use.

Through a LayerNorm.  Residual row m is x[m] = d_m + c_m * s[m] with s[m] in {-1, +1}^K holding
exactly K/2 of each sign, c_m in {0.5, 1, 2, 4} and an integer d_m in [-5, 5].  Every x is a multiple
of 0.5 below 10: sums of them are exact in fp32, the mean is exactly d_m and the variance exactly
c_m^2, so LN(x) * gamma + beta = +-gamma_k * c_m / sqrt(c_m^2 + eps) + beta_k = +-gamma_k (1 - O(eps))
+ beta_k.  With integer gamma_k in {2, 3} and beta_k in {-1, 0, 1} that lies within 2e-5 of an integer
in +-[1, 4] (never near 0), and bf16's half ulp there is >= 2^-9: every correct fp32 LayerNorm --
whatever its reduction order, rsqrt or 1/K rounding -- stores the same bf16 integer h = s * gamma +
beta.  (gamma = 1 with beta = -+1 is excluded: the sum cancels to ~-5e-6, which bf16 keeps.)
``ln_case`` asserts bf16(LN(x)) == h for an fp64 LayerNorm and for an fp32 one written like the
kernels' prologue.  For ``skinny_addln_gemm`` that pattern is the SUM v = x_in + res_bias + sum(parts):
parts and res_bias are free small integers and x_in = v - res_bias - sum(parts) (multiples of 0.5
below 2^8: exact in any order); x_out must equal v.  A fixed-point residual is v * 2^32 in int64.

GELU.  W / 16 (still exact in bf16) keeps the pre-activation v = integer / 16 exact and most of it
inside |v| <= 6 where gelu bends.  Reference: fp64 v / (1 + exp(-2u)), u = 0.79788456 (v + 0.044715
v^3) -- the sigmoid form; fp64 0.5 v (1 + tanh u) cancels to -0.0 below v ~ -7 where the true value
is -2e-16.  Rule, from fp32 against bf16 precision and not from any kernel: an fp32 evaluation with
relative error under 2^-10 lands on one of the two bf16 neighbours of the true value, so for
v >= -8 the output is within ONE bf16 ulp of bf16(ref) (distance of the sign-magnitude bit patterns,
+-0 equal); below -8, where |gelu| < 4e-21 and exp overflows in some evaluations, the output lies
in [-2^-60, 0].  No other tolerance.

fp8 KV cache: the expected byte is models.gpt2.quantize_kv_e4m3 of the exact bf16 value.

Argmax.  Logits are exact integers and penalty = 2.0, so penalised logits are exact.  A and (through
the LayerNorm) h share their first 3K/4 elements over all rows; the candidate columns ``ARGMAX_CANDS``
all hold ONE weight row aligned with that part (m_k * sign, m_k in {1, 2} at random, so that the
k-blocks weigh differently and a shifted or swapped block moves the tied logits), so they tie in every
row at a high value; the padding columns >= vocab hold (m_k + 1) * sign on it and the same tail:
strictly the largest logits of every row (asserted), so a kernel that ignores ``vocab`` picks one.
Every 64-column key group below ``vocab`` holds a candidate.  The seen bits of row r cover the
first r % 4 candidates (the unpenalised maximum's column whenever r % 4 > 0) and a random eighth of
the other columns: the surviving top tie is (3, 9) inside a 16-column group, (9, 20) / (20, 40) inside
a 64-column key group, (40, 70) across key groups -- and the candidates further up (70, 75, 97, 130,
200, 260, 299) tie across wave slots and persistent passes of gemm_ps.  Expected token: arg max of the
penalised fp64 logits below ``vocab``, LOWEST column on ties; expected key = (f32_ordered(logit) <<
32) | ~column, where f32_ordered is the monotone map of fp32 bits onto unsigned integers.

Faults: ``mutate_product`` (a lost or doubled k-element, a K slice shifted by one k-block, two
k-blocks of W swapped) and ``mutate_output`` (two column groups swapped, a row tile aliased) take
exact operands and return what a kernel with that defect would store; a K / V row at pos + 1 is
``qkv_expected`` with that position, a tie broken upwards and an ignored vocab are flags of
``argmax_expected``, GELU without the bias is the comparator applied to the bias-free product.
test_gemm_cases_cpu.py proves, for every family, K and row count the GPU file uses, that the
comparators here reject each of them in EVERY affected (row, 16-column group) block, and what the
old tolerance makes of the first three."""
import functools
import zlib

import numpy as np
import torch

PENALTY = 2.0
ARGMAX_CANDS = (3, 9, 20, 40, 70, 75, 97, 130, 200, 260, 299)
K0 = 0.7978845608028654
K1 = 0.044715


class Case(dict):
    """Read-only bundle of CPU tensors; ``rows(M)`` slices every per-row tensor to the first M rows."""

    __getattr__ = dict.__getitem__

    def rows(self, M):
        R = self["R"]
        assert M <= R
        out = Case(self)
        for k, v in self.items():
            if isinstance(v, torch.Tensor) and k in self["per_row"]:
                out[k] = v[..., :M, :] if k == "parts" else v[:M]
        out["R"] = M
        return out


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _ints(shape, lo, hi, g, nonzero=False):
    x = torch.randint(lo, hi + 1, shape, generator=g)
    if nonzero:
        x = torch.where(x == 0, torch.where(torch.rand(shape, generator=g) < 0.5, torch.tensor(lo), torch.tensor(hi)), x)
    return x.double()


def rne_bf16(x64):
    """Integers (or multiples of 1/16) below 2^24: fp64 -> fp32 is exact, then one RNE to bf16."""
    f = x64.float()
    assert torch.equal(f.double(), x64)
    return f.to(torch.bfloat16)


def _check_exact(ref, bias):
    assert float(ref.abs().max()) + float(bias.abs().max()) < 2 ** 24


# ------------------------------------------------------------------------------------------------
# builders
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plain_case(R, N, K, wdiv=1, seed=0):
    """a [R, K] (bf16-exact nonzero integers), w [N, K] = integers / wdiv, bias [N], ref = a @ w.T
    (fp64, no bias)."""
    g = _gen("plain", R, N, K, wdiv, seed)
    a, w, bias = _ints((R, K), -4, 4, g, nonzero=True), _ints((N, K), -3, 3, g) / wdiv, _ints((N,), -3, 3, g)
    ref = a @ w.t()
    _check_exact(ref * wdiv, bias * wdiv)
    return Case(a=a, w=w, bias=bias, ref=ref, R=R, N=N, K=K, per_row=("a", "ref"))


def ln_fp64(x, gamma, beta, eps):
    x = x.double()
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()


def ln_fp32(x, gamma, beta, eps):
    """Two-pass fp32 LayerNorm in the kernels' operation order (mean, centred squares, rsqrt)."""
    x = x.float()
    K = x.shape[1]
    mean = x.sum(1, keepdim=True) / K
    c = x - mean
    rstd = torch.rsqrt((c * c).sum(1, keepdim=True) / K + torch.tensor(eps, dtype=torch.float32))
    return c * rstd * gamma.float() + beta.float()


def _signs(R, K, g, common=0):
    """[R, K] of +-1, K/2 of each per row; the first ``common`` columns (balanced) equal in all rows."""
    assert K % 8 == 0 and common % 2 == 0 and (K - common) % 2 == 0
    s = torch.empty(R, K, dtype=torch.float64)
    head = torch.cat([torch.ones(common // 2), -torch.ones(common // 2)])[torch.randperm(common, generator=g)]
    tail = torch.cat([torch.ones((K - common) // 2), -torch.ones((K - common) // 2)])
    for r in range(R):
        s[r, :common] = head
        s[r, common:] = tail[torch.randperm(K - common, generator=g)]
    return s


def _ln_rows(R, K, g, eps, common=0):
    s = _signs(R, K, g, common)
    c = torch.tensor([0.5, 1.0, 2.0, 4.0], dtype=torch.float64)[torch.randint(0, 4, (R,), generator=g)]
    d = _ints((R,), -5, 5, g)
    x = (d[:, None] + c[:, None] * s).float()
    gamma = _ints((K,), 2, 3, g).float()
    beta = _ints((K,), -1, 1, g).float()
    h = s * gamma.double() + beta.double()
    assert float(h.abs().min()) >= 1 and float(h.abs().max()) <= 4
    for e in (eps, 1e-12):
        assert torch.equal(ln_fp64(x, gamma, beta, e).to(torch.bfloat16).double(), h)
        assert torch.equal(ln_fp32(x, gamma, beta, e).to(torch.bfloat16).double(), h)
    return x, gamma, beta, h


@functools.lru_cache(maxsize=None)
def ln_case(R, N, K, wdiv=1, seed=0, eps=1e-5):
    """x fp32 [R, K] whose LayerNorm is the integer matrix a (= h) in bf16; w = integers / wdiv."""
    g = _gen("ln", R, N, K, wdiv, seed)
    x, gamma, beta, h = _ln_rows(R, K, g, eps)
    w, bias = _ints((N, K), -3, 3, g) / wdiv, _ints((N,), -3, 3, g)
    ref = h @ w.t()
    _check_exact(ref * wdiv, bias * wdiv)
    return Case(x=x, gamma=gamma, beta=beta, eps=eps, a=h, w=w, bias=bias, ref=ref, R=R, N=N, K=K,
                per_row=("x", "a", "ref"))


@functools.lru_cache(maxsize=None)
def addln_case(R, N, K, wdiv=1, seed=0):
    """ln_case whose x is the sum v = x_in + res_bias + sum(parts[:nsplit]): ``addln_x_in`` gives x_in."""
    c = Case(ln_case(R, N, K, wdiv, seed))
    g = _gen("addln", R, N, K, seed)
    c["parts"] = _ints((16, R, K), -3, 3, g).float()
    c["res_bias"] = _ints((K,), -3, 3, g).float()
    c["per_row"] = c["per_row"] + ("parts",)
    return c


def addln_x_in(case, nsplit, with_res_bias):
    x = case.x.double() - case.parts[:nsplit].double().sum(0)
    if with_res_bias:
        x = x - case.res_bias.double()
    assert float(x.abs().max()) < 2 ** 8
    return x.float()


def to_fix(x, copies):
    """fp32 [M, K] -> int64 [copies, M, K] fixed point (value * 2^32), spread unevenly over the copies."""
    total = (x.double() * 2.0 ** 32).to(torch.int64)
    assert torch.equal(total.double() / 2.0 ** 32, x.double())
    out = torch.zeros(copies, *x.shape, dtype=torch.int64)
    for c in range(1, copies):
        out[c] = (c * 12345) << 20
    out[0] = total - out[1:].sum(0)
    return out


@functools.lru_cache(maxsize=None)
def argmax_case(R, N, K, vocab, ln, eps=1e-5):
    """See the module docstring.  a [R, K] integers (plain A, or the LayerNorm of x), w [N, K], seen
    bool [R, N], logits fp64 [R, N] (unpenalised, all columns).  The first seed whose data meets the
    construction's asserts (at K = 32 the 8-element tails can lift another column over the candidates)."""
    for seed in range(64):
        try:
            return _argmax_case(R, N, K, vocab, ln, seed, eps)
        except AssertionError:
            continue
    raise AssertionError("no seed gives the argmax construction")


def _argmax_case(R, N, K, vocab, ln, seed, eps):
    g = _gen("argmax", R, N, K, vocab, ln, seed)
    C = K - K // 4
    cands = [c for c in ARGMAX_CANDS if c < vocab]
    if ln:
        x, gamma, beta, a = _ln_rows(R, K, g, eps, common=C)
    else:
        a = _ints((R, K), -4, 4, g, nonzero=True)
        a[:, :C] = a[0, :C]
    sign = torch.sign(a[0, :C])
    w = _ints((N, K), -3, 3, g)
    w[:, :C] = _ints((N, C), -1, 1, g)  # the other columns pull less on the common part: the candidates lead
    w_top = w[cands[0]].clone()
    mag = torch.randint(1, 3, (C,), generator=g).double()
    w_top[:C] = mag * sign
    w[cands] = w_top
    w[vocab:] = w_top
    w[vocab:, :C] = (mag + 1) * sign
    logits = a @ w.t()
    _check_exact(logits, torch.zeros(1))
    assert bool((logits[:, vocab:].min(1).values > logits[:, :vocab].max(1).values).all())
    seen = torch.rand(R, N, generator=g) < 0.125
    seen[:, cands] = False
    for r in range(R):
        seen[r, cands[:r % 4]] = True
    # every row's maxima below vocab are exactly its unseen candidates (>= 2 of them: a tie to break)
    p = penalised(logits, seen)[:, :vocab]
    for r in range(R):
        tops = (p[r] == p[r].max()).nonzero()[:, 0].tolist()
        assert tops == cands[r % 4:] and len(tops) >= 2, (r, tops)
    # rows 16 apart (one row tile) differ in their winning value: an aliased row tile shows in the keys
    top = p.max(1).values
    assert bool((top[16:] != top[:-16]).all())
    case = Case(a=a, w=w, seen=seen, logits=logits, vocab=vocab, cands=cands, R=R, N=N, K=K,
                per_row=("a", "seen", "logits", "x"))
    if ln:
        case.update(x=x, gamma=gamma, beta=beta, eps=eps)
    return case


# ------------------------------------------------------------------------------------------------
# references and comparators
# ------------------------------------------------------------------------------------------------
def gelu_ref(v64):
    u = K0 * (v64 + K1 * v64 ** 3)
    return v64 / (1.0 + torch.exp(-2.0 * u))


def _ordered(x_bf16):
    """bf16 bit patterns as integers ordered like the values (+0 and -0 both 0)."""
    i = x_bf16.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def gelu_bad(out, v64):
    """bool [M, N]: where the bf16 ``out`` breaks the GELU rule for the exact pre-activation v64."""
    out = out.detach().cpu()
    assert out.dtype == torch.bfloat16
    o = out.double()
    exp = gelu_ref(v64).to(torch.bfloat16)
    near = (_ordered(out) - _ordered(exp)).abs() <= 1
    tiny = (o <= 0) & (o >= -(2.0 ** -60))
    return ~torch.isfinite(o) | torch.where(v64 >= -8, ~near, ~tiny)


def scatter_plan(M, S, T, seed=0):
    """Permuted slots and scattered positions for M rows of a [S, H, T, 64] cache (S >= M)."""
    g = _gen("scatter", M, S, T, seed)
    return torch.randperm(S, generator=g)[:M].to(torch.int32), ((torch.arange(M) * 7 + 3) % T).to(torch.int32)


def cache_sentinel(S, H, T, kind):
    """A cache full of known, position-dependent values (bf16 integers 1..13 / bytes 1..13)."""
    pat = (torch.arange(S * H * T * 64) % 13 + 1).reshape(S, H, T, 64)
    if kind == "bf16":
        return pat.to(torch.bfloat16)
    return pat.to(torch.uint8).view(torch.float8_e4m3fn)


def kv_values(v64, kind):
    """What a cache of ``kind`` holds for the exact values v64."""
    if kind == "bf16":
        return rne_bf16(v64)
    from distributed_lms_raft_llm_amd.models.gpt2 import quantize_kv_e4m3

    return quantize_kv_e4m3(rne_bf16(v64))


def qkv_expected(v64, slot, pos, S, T, kind):
    """(q bf16 [M, D], k_cache, v_cache) after the QKV epilogue ran on sentinel caches."""
    M, D = v64.shape[0], v64.shape[1] // 3
    H = D // 64
    kc, vc = cache_sentinel(S, H, T, kind), cache_sentinel(S, H, T, kind)
    kc[slot.long(), :, pos.long()] = kv_values(v64[:, D:2 * D], kind).reshape(M, H, 64)
    vc[slot.long(), :, pos.long()] = kv_values(v64[:, 2 * D:], kind).reshape(M, H, 64)
    return rne_bf16(v64[:, :D]), kc, vc


def qkv_codes(v64, kind):
    """int32 [M, 3D]: the bits the epilogue stores per element (bf16 q; bf16 or e4m3 K / V)."""
    D = v64.shape[1] // 3
    q = rne_bf16(v64[:, :D]).view(torch.int16).to(torch.int32)
    kv = kv_values(v64[:, D:], kind)
    kv = kv.view(torch.int16).to(torch.int32) if kind == "bf16" else kv.view(torch.uint8).to(torch.int32)
    return torch.cat([q, kv], 1)


def bits(x):
    """Bit-exact view for comparisons (bf16 / fp8 tensors: NaN sentinels must compare equal)."""
    if x.dtype == torch.bfloat16:
        return x.contiguous().view(torch.int16)
    if x.dtype == torch.float32:
        return x.contiguous().view(torch.int32)
    if x.dtype == torch.float8_e4m3fn:
        return x.contiguous().view(torch.uint8)
    return x


def same(got, want):
    got, want = got.detach().cpu(), want.detach().cpu()
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(bits(got), bits(want))


def penalised(logits, seen, penalty=PENALTY):
    return torch.where(seen, torch.where(logits < 0, logits * penalty, logits / penalty), logits)


def f32_ordered(v):
    """fp32 values -> uint32 (as int64) ordered like the values: negative floats complement all
    bits, the others set the sign bit."""
    u = v.float().contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return torch.where(u >= 2 ** 31, (~u) & 0xFFFFFFFF, u | 0x80000000)


def make_keys(value, col):
    """int64 keys (f32_ordered(value) << 32) | ~col (two's-complement view of the uint64)."""
    hi = f32_ordered(value).numpy().astype(np.uint64)
    lo = (~col.numpy().astype(np.int64)).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    return torch.from_numpy(((hi << np.uint64(32)) | lo).view(np.int64))


def argmax_expected(logits, seen, vocab, penalty=PENALTY, highest=False, use_vocab=True):
    """(token [M], penalised logit of the token [M]); ``highest`` / ``use_vocab=False`` are the faults."""
    p = penalised(logits, seen, penalty)
    if use_vocab:
        p = p[:, :vocab]
    top = p.max(1, keepdim=True).values
    hit = (p == top)
    n = p.shape[1]
    tok = (n - 1 - hit.flip(1).float().argmax(1)) if highest else hit.float().argmax(1)
    return tok, top[:, 0]


def group_keys(logits, seen, vocab, groups, penalty=PENALTY):
    """Expected key per (row, column set): ``groups`` is a list of column-index lists (a 64-column
    key group of the skinny LM head, or the tiles of one gemm_ps wave slot); 0 where no column of
    the set is below vocab."""
    p = penalised(logits, seen, penalty)
    M = p.shape[0]
    out = torch.zeros(M, len(groups), dtype=torch.int64)
    for j, cols in enumerate(groups):
        cols = torch.tensor([c for c in cols if c < vocab], dtype=torch.long)
        if cols.numel() == 0:
            continue
        sub = p[:, cols]
        top = sub.max(1, keepdim=True).values
        first = (sub == top).float().argmax(1)
        out[:, j] = make_keys(top[:, 0], cols[first])
    return out


def key_token(keys):
    return (~keys) & 0xFFFFFFFF


def key_high(keys):
    return (keys >> 32) & 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------
# fault models
# ------------------------------------------------------------------------------------------------
def _pick_k(a, w, cols, kb):
    """A k of k-block kb where every row of a and some column of the group is nonzero."""
    for k in range(32 * kb, 32 * kb + 32):
        if bool((a[:, k] != 0).all()) and bool((w[cols, k] != 0).any()):
            return k
    raise AssertionError("no usable k-element in the block")


def mutate_product(name, a, w, waves=4, group=1):
    """The product a @ w.T (fp64) as a kernel with the fault ``name`` computes it, and the affected
    (row, 16-column group) blocks (bool [M, N/16]).  ``waves``: the waves that split K."""
    M, K = a.shape
    N = w.shape[0]
    nkb = K // 32
    prod = a @ w.t()
    blocks = torch.zeros(M, N // 16, dtype=torch.bool)
    cols = slice(16 * group, 16 * group + 16)
    if name in ("drop_k", "double_k"):
        k = _pick_k(a, w, cols, nkb // 2)
        term = a[:, k:k + 1] * w[cols, k][None, :]
        prod[:, cols] += term if name == "double_k" else -term
        blocks[:, group] = True
    elif name == "shift_slice":
        # wave 0's slice [0, per) read as [1, per + 1): block 0 is lost and the block after the slice
        # counted again; past the end of K the kernel's clamp re-reads A's last block against the next
        # column group's first block of W (the shuffled layout's neighbour)
        per = -(-nkb // waves)
        lo, hi = slice(0, 32), slice(32 * per, 32 * per + 32)
        prod -= a[:, lo] @ w[:, lo].t()
        if per < nkb:
            prod += a[:, hi] @ w[:, hi].t()
        else:
            last = slice(K - 32, K)
            prod += a[:, last] @ torch.roll(w, -16, 0)[:, lo].t()
        blocks[:] = True
    elif name == "swap_kblocks":
        assert nkb >= 2
        ws = w.clone()
        ws[:, :32], ws[:, K - 32:] = w[:, K - 32:], w[:, :32]
        prod = a @ ws.t()
        blocks[:] = True
    else:
        raise ValueError(name)
    return prod, blocks


def mutate_output(name, v):
    """Faults of the store: v [M, N] is the exact pre-rounding output (bias included)."""
    M, N = v.shape
    out = v.clone()
    blocks = torch.zeros(M, N // 16, dtype=torch.bool)
    if name == "swap_groups":
        out[:, 0:16], out[:, 16:32] = v[:, 16:32], v[:, 0:16]
        blocks[:, :2] = True
    elif name == "tile_alias":
        assert M > 16
        out[16:] = v[:M - 16]
        blocks[16:] = True
    else:
        raise ValueError(name)
    return out, blocks


def block_hits(diff):
    """bool [M, N] element differences -> bool [M, N/16]: blocks with at least one difference."""
    M, N = diff.shape
    return diff.reshape(M, N // 16, 16).any(-1)


# ------------------------------------------------------------------------------------------------
# the shapes test_gemm_exact_gpu.py runs (and test_gemm_cases_cpu.py proves): K per kernel family,
# the rows every case is built with, and the waves that split K (for the shift_slice fault)
# ------------------------------------------------------------------------------------------------
SKINNY_R, ADDLN_R, MID_R, PS_R = 32, 8, 64, 129
SKINNY_LN_KS = (32, 160, 512, 544, 768, 1280, 1600, 2048)
SKINNY_PLAIN_KS = (32, 224, 2048, 2080, 3072, 5120, 6400)
SKINNY_ARGMAX_KS = (32, 160, 768)
ADDLN_KS = (32, 256, 768, 1024, 1280, 1600)
MID_LN_KS = (544, 768, 1024)
MID_PROJ_KS = (768, 1024, 3072, 4096)
PS_KS = (128, 256, 384, 768)  # K / split
PS_SPLITS = ((128, 1), (256, 1), (384, 1), (768, 1), (128, 2), (384, 2), (128, 4), (256, 4))  # (K / split, split)
ARGMAX_NV = ((128, 100), (320, 300))
N_LN, N_QKV, N_PLAIN, N_PS, N_PS_QKV = 96, (192, 384), 96, 320, 384


def ln_shapes():
    """(R, K, waves) of every LayerNorm-fed case."""
    return ([(SKINNY_R, K, 4) for K in SKINNY_LN_KS] + [(ADDLN_R, K, 4) for K in ADDLN_KS] +
            [(MID_R, K, 8) for K in MID_LN_KS])


def plain_shapes():
    """(R, N, K, waves) of every bf16-A case."""
    return ([(SKINNY_R, N_PLAIN, K, 16 if K > 2048 else 8) for K in SKINNY_PLAIN_KS] +
            [(MID_R, N_PLAIN, K, 8) for K in MID_PROJ_KS] + [(PS_R, N_PS, K, 1) for K in PS_KS])


def argmax_shapes():
    """(R, N, K, vocab, ln) of every argmax case."""
    out = [(SKINNY_R, N, K, V, ln) for K in SKINNY_ARGMAX_KS for N, V in ARGMAX_NV for ln in (False, True)]
    return out + [(PS_R, 320, K, 300, False) for K in PS_KS]


def pack_seen(seen):
    """bool [M, N] -> the kernels' int32 bitmap [M, N / 32] (bit c % 32 of word c // 32)."""
    M, N = seen.shape
    w = (seen.reshape(M, N // 32, 32).to(torch.int64) << torch.arange(32)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def key_groups64(N):
    """Column sets of the skinny LM head's keys: one per 64 columns."""
    return [list(range(64 * j, 64 * j + 64)) for j in range(N // 64)]


def ps_slot_groups(N, nt, col_wgs):
    """Column sets of gemm_ps's keys: wave slot s owns the 16 nt-column tiles s, s + slots, ..."""
    slots, tiles = 8 * col_wgs, N // (16 * nt)
    return [[col for t in range(s, tiles, slots) for col in range(16 * nt * t, 16 * nt * (t + 1))] for s in range(slots)]
