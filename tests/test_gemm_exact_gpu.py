"""Exact checks of the skinny (skinny.hip: skinny_gemm, skinny_addln_gemm), mid-batch (mid.hip:
mid_ln_gemm, mid_proj) and persistent (gemm_ps.hip) decode GEMMs on the integer cases of
tests/gemm_cases.py (derivations there; tests/test_gemm_cases_cpu.py proves they catch one lost
k-element).  Every kernel must EQUAL the fp64 product rounded once -- bit for bit, the GELU epilogue
within one bf16 ulp, argmax keys column and value -- at the smallest shapes that reach each path:
empty and short K slices of a wave, every KBW register budget, the 8 | 16-wave switch, the row-tile
boundaries, FULL / guarded instantiations, row blocks on grid.y, the persistent column loop.

Every output buffer is larger than needed (rows past M, columns past N where the binding takes a
strided view) and pre-filled with a sentinel -- NaN for bf16 / fp32 outputs, known integers for
in-place residuals, caches and key buffers -- and the WHOLE buffer is compared: nothing outside the
intended outputs may change.  Every launch runs twice on fresh sentinels; both results must agree."""
import pytest
import torch

import gemm_cases as gc

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
T_CACHE = 11
KEY_SENTINEL = 0x5A5A5A5A5A5A5A5A


def _ops():
    from distributed_lms_raft_llm_amd import ops

    ops.lib()
    return ops


def _wsh(case):
    return _ops().shuffle_weight(case.w.to(torch.bfloat16).to(DEV))


def _bf16(x):
    return x.to(torch.bfloat16).to(DEV)


def _f32(x):
    return x.float().to(DEV)


def _twice(make, launch):
    """make() -> dict of fresh sentinel-filled buffers; launch(bufs) runs the kernel.  Twice; the two
    results must be bit-identical.  Returns the first, on the CPU."""
    res = []
    for _ in range(2):
        bufs = make()
        launch(bufs)
        res.append({k: v.cpu() for k, v in bufs.items()})
    for k in res[0]:
        assert gc.same(res[0][k], res[1][k]), f"{k}: second launch differs from the first"
    return res[0]


def _check(got, want, what=""):
    for k, w in want.items():
        assert gc.same(got[k], w), f"{what}: {k} differs in {int((gc.bits(got[k]) != gc.bits(w)).sum())} elements"


def _pad(want, rows=3, cols=16, fill=NAN):
    """``want`` [M, N] inside a sentinel frame of ``rows`` more rows and ``cols`` more columns."""
    big = torch.full((want.shape[0] + rows, want.shape[1] + cols), fill, dtype=want.dtype)
    big[:want.shape[0], :want.shape[1]] = want
    return big


def _frame(M, N, dtype, rows=3, cols=16, fill=NAN):
    return torch.full((M + rows, N + cols), fill, dtype=dtype, device=DEV)


def _ints_frame(M, N, dtype, rows=3, cols=16):
    """Known integers (-8 .. 8) for an in-place residual and its frame."""
    n = (M + rows) * (N + cols)
    return ((torch.arange(n) * 7) % 17 - 8).reshape(M + rows, N + cols).to(dtype)


class _Qkv:
    """Sentinel q / K / V buffers for M rows of width 3 D, permuted slots, scattered positions."""

    def __init__(self, M, D, kind):
        self.M, self.D, self.kind, self.S, self.H = M, D, kind, M + 3, D // 64
        self.slot, self.pos = gc.scatter_plan(M, self.S, T_CACHE)
        self.slot_d, self.pos_d = self.slot.to(DEV), self.pos.to(DEV)

    def make(self):
        return dict(q=_frame(self.M, self.D, torch.bfloat16),
                    k=gc.cache_sentinel(self.S, self.H, T_CACHE, self.kind).to(DEV),
                    v=gc.cache_sentinel(self.S, self.H, T_CACHE, self.kind).to(DEV))

    def args(self, b):
        return dict(q_out=b["q"][:self.M, :self.D], k_cache=b["k"], v_cache=b["v"], row_slot=self.slot_d,
                    row_pos=self.pos_d)

    def want(self, v64):
        q, k, v = gc.qkv_expected(v64, self.slot, self.pos, self.S, T_CACHE, self.kind)
        return dict(q=_pad(q), k=k, v=v)


def _key_frame(M, cols):
    return torch.full((M + 3, cols + 5), KEY_SENTINEL, dtype=torch.int64, device=DEV)


def _key_want(keys, M, cols):
    big = torch.full((M + 3, cols + 5), KEY_SENTINEL, dtype=torch.int64)
    big[:M, :keys.shape[1]] = keys
    return big


def _check_reduced(ops, keybuf, ncols, case):
    """argmax_reduce of the kernel's keys: EVERY row's token (lowest column on ties) and the key's high
    word, the ordered fp32 bits of the expected penalised logit."""
    M = case.R
    red = ops.argmax_reduce(keybuf.to(DEV)[:M, :ncols].contiguous()).cpu()
    tok, val = gc.argmax_expected(case.logits, case.seen, case.vocab)
    assert torch.equal(gc.key_token(red), tok)
    assert torch.equal(gc.key_high(red), gc.f32_ordered(val))


SKINNY_MS = [1, 15, 16, 17, 32]  # one row; a ragged / full first row tile; second row tile of 1 / 16 rows
LN_K_IDS = {32: "K=32: slices 1,0,0,0", 160: "K=160: slices 2,2,1,0", 512: "K=512: per 4, KBW 4",
            544: "K=544: slices 5,5,5,2, KBW 8", 768: "K=768: per 6", 1280: "K=1280: per 10, KBW 12", 1600: "K=1600: slices 13,13,13,11, KBW 16",
            2048: "K=2048: the LN limit, per 16"}
PLAIN_K_IDS = {32: "K=32: 8 waves, 7 empty", 224: "K=224: 8 waves 1,1,1,1,1,1,1,0",
               2048: "K=2048: 8 waves, per 8", 2080: "K=2080: 16-wave switch, slices 5 x13, 0, 0, 0",
               3072: "K=3072: 16 waves, per 6", 5120: "K=5120: 16 waves, per 10, KBW 12", 6400: "K=6400: 16 waves, per 13, KBW 16"}


# ------------------------------------------------------------------------------------------------
# skinny_gemm
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", ["bf16", "gelu"])
@pytest.mark.parametrize("K", gc.SKINNY_LN_KS, ids=[LN_K_IDS[k] for k in gc.SKINNY_LN_KS])
def test_skinny_ln_bf16_gelu(K, epi):
    """LN prologue, 4 waves per column group; M = 1, 15, 16 | 17, 32: MT 1 | 2 row tiles."""
    ops = _ops()
    full = gc.ln_case(gc.SKINNY_R, gc.N_LN, K, 16 if epi == "gelu" else 1)
    wsh, g, b, bias = _wsh(full), _f32(full.gamma), _f32(full.beta), _f32(full.bias)
    for M in SKINNY_MS:
        c = full.rows(M)
        x = _f32(c.x)
        got = _twice(lambda: dict(out=_frame(M, c.N, torch.bfloat16)),
                     lambda bf: ops.skinny_gemm(x, wsh, ops.EPI_GELU_TANH if epi == "gelu" else ops.EPI_BF16,
                                                ln=(g, b, c.eps), bias=bias, out=bf["out"][:M, :c.N]))
        v = c.ref + c.bias
        if epi == "bf16":
            _check(got, dict(out=_pad(gc.rne_bf16(v))), f"M={M}")
        else:
            bad = gc.gelu_bad(got["out"][:M, :c.N], v)
            assert not bad.any(), (M, bad.nonzero()[:8].tolist())
            frame = got["out"].clone()
            frame[:M, :c.N] = NAN
            assert bool(torch.isnan(frame.float()).all()), f"M={M}: written outside the output"


@pytest.mark.parametrize("kind", ["bf16", "fp8"])
@pytest.mark.parametrize("K", gc.SKINNY_LN_KS, ids=[LN_K_IDS[k] for k in gc.SKINNY_LN_KS])
def test_skinny_ln_qkv(K, kind):
    """LN prologue -> q rows + K / V rows scattered to permuted slots; whole caches compared."""
    ops = _ops()
    N = gc.N_QKV[1] if K in (160, 768) else gc.N_QKV[0]
    full = gc.ln_case(gc.SKINNY_R, N, K)
    wsh, g, b, bias = _wsh(full), _f32(full.gamma), _f32(full.beta), _f32(full.bias)
    for M in SKINNY_MS:
        c = full.rows(M)
        x, io = _f32(c.x), _Qkv(M, N // 3, kind)
        got = _twice(io.make, lambda bf: ops.skinny_gemm(x, wsh, ops.EPI_QKV, ln=(g, b, c.eps), bias=bias, **io.args(bf)))
        _check(got, io.want(c.ref + c.bias), f"M={M}")


@pytest.mark.parametrize("ln", [False, True], ids=["plain", "ln"])
@pytest.mark.parametrize("N,vocab", gc.ARGMAX_NV, ids=["N128-vocab100", "N320-vocab300"])
@pytest.mark.parametrize("K", gc.SKINNY_ARGMAX_KS, ids=["K=32: 4 waves per group, 3 empty", "K=160: slices 2,2,1,0",
                                                         "K=768: per 6"])
def test_skinny_argmax(K, N, vocab, ln):
    """16 waves, 4 column groups of 4 waves: one key per (row, 64 columns); ties at the top of every
    row inside a 16-column group, inside a key group and across key groups, the padding columns
    >= vocab the largest of the row, seen bits on the unpenalised maximum: every key of every row."""
    ops = _ops()
    full = gc.argmax_case(gc.SKINNY_R, N, K, vocab, ln)
    wsh = _wsh(full)
    groups = gc.key_groups64(N)
    for M in SKINNY_MS:
        c = full.rows(M)
        seen = gc.pack_seen(c.seen).to(DEV)
        a = _f32(c.x) if ln else _bf16(c.a)
        lnp = (_f32(c.gamma), _f32(c.beta), c.eps) if ln else None
        got = _twice(lambda: dict(keys=_key_frame(M, N // 64)),
                     lambda bf: ops.skinny_gemm(a, wsh, ops.EPI_ARGMAX, ln=lnp, argmax_out=bf["keys"][:M], seen=seen,
                                                vocab=vocab, penalty=gc.PENALTY))
        _check(got, dict(keys=_key_want(gc.group_keys(c.logits, c.seen, vocab, groups), M, N // 64)), f"M={M}")
        _check_reduced(ops, got["keys"], N // 64, c)


@pytest.mark.parametrize("epi", ["bf16", "f32", "fix", "partial"])
@pytest.mark.parametrize("K", gc.SKINNY_PLAIN_KS, ids=[PLAIN_K_IDS[k] for k in gc.SKINNY_PLAIN_KS])
def test_skinny_plain(K, epi):
    """bf16 A read as fragments from global memory.  bf16: 4 waves (K = 32: 3 empty; 224: 2,2,2,1;
    2048: per 16; past 2048 no register budget: refused, nothing written); in place (f32 residual of known
    integers, int64 fixed point: out += (acc + bias) << 32) and partial slabs: 8 waves, 16 past
    K = 2048.  M = 1, 15, 16 | 17, 32."""
    ops = _ops()
    full = gc.plain_case(gc.SKINNY_R, gc.N_PLAIN, K)
    wsh, bias = _wsh(full), _f32(full.bias)
    N = full.N
    for M in SKINNY_MS:
        c = full.rows(M)
        a, v = _bf16(c.a), c.ref + c.bias
        if epi == "bf16":
            make, want = (lambda: dict(out=_frame(M, N, torch.bfloat16))), _pad(gc.rne_bf16(v))
            run = lambda bf: ops.skinny_gemm(a, wsh, ops.EPI_BF16, bias=bias, out=bf["out"][:M, :N])
        elif epi == "partial":
            make, want = (lambda: dict(out=_frame(M, N, torch.float32))), _pad(c.ref.float())
            run = lambda bf: ops.skinny_gemm(a, wsh, ops.EPI_PARTIAL, out=bf["out"][:M, :N])
        else:
            dt = torch.float32 if epi == "f32" else torch.int64
            old = _ints_frame(M, N, dt)
            want = old.clone()
            want[:M, :N] += v.to(dt) if epi == "f32" else (v.to(torch.int64) << 32)
            make = lambda: dict(out=old.to(DEV))
            run = lambda bf: ops.skinny_gemm(a, wsh, ops.EPI_F32, bias=bias, out=bf["out"][:M, :N])
        if epi == "bf16" and -(-(K // 32) // 4) > 16:
            # the bf16 epilogue's 4 waves hold at most 16 k-blocks each: refused on the host
            bufs = make()
            with pytest.raises(RuntimeError):
                run(bufs)
            torch.cuda.synchronize()
            assert bool(torch.isnan(bufs["out"].float()).all())
            continue
        _check(_twice(make, run), dict(out=want), f"M={M}")


# ------------------------------------------------------------------------------------------------
# skinny_addln_gemm
# ------------------------------------------------------------------------------------------------
ADDLN_K_IDS = {32: "K=32: nv4 1, slices 1,0,0,0", 256: "K=256: nv4 1, per 2", 768: "K=768: nv4 3", 1024: "K=1024: nv4 4",
               1280: "K=1280: nv4 5, KBW 12, M <= 4", 1600: "K=1600: nv4 7, KBW 16, M <= 4"}


def _addln_common(c, nsplit, with_rb):
    """x_in inside a sentinel frame (and a copy to compare afterwards), slabs and residual bias."""
    x_in = gc.addln_x_in(c, nsplit, with_rb)
    xin_big = _pad(x_in, 2, 32, 5.0).to(DEV)
    keep = xin_big.clone()
    kw = dict(parts=_f32(c.parts[:max(nsplit, 1)]) if nsplit else None, nsplit=nsplit,
              res_bias=_f32(c.res_bias) if with_rb else None)
    return xin_big, keep, kw


ADDLN_SLABS = [(K, ns) for K in gc.ADDLN_KS for ns in (0, 1, 4)] + [(K, ns) for K in (768, 1024) for ns in (12, 16)]


@pytest.mark.parametrize("K,nsplit", ADDLN_SLABS, ids=[f"{ADDLN_K_IDS[k]}-nsplit{ns}" for k, ns in ADDLN_SLABS])
def test_addln_gelu(K, nsplit):
    """v = x_in + res_bias + sum(parts) (exact), x_out = v, out = gelu(LN(v) W^T + b): RPW 1 | 2 at
    M = 4 | 5, with and without res_bias and x_out; x_in unchanged.  12 / 16 slabs: K 768 / 1024, M <= 4."""
    ops = _ops()
    full = gc.addln_case(gc.ADDLN_R, gc.N_LN, K, 16)
    wsh, g, b, bias = _wsh(full), _f32(full.gamma), _f32(full.beta), _f32(full.bias)
    N = full.N
    limit = 4 if nsplit > 4 else ops.skinny_addln_max_rows(K)
    assert limit == (4 if (K > 1024 or nsplit > 4) else 8)
    for M in [m for m in (1, 4, 5, 8) if m <= limit]:
        c = full.rows(M)
        for with_rb, with_xout in ((True, True), (False, True), (True, False), (False, False)):
            xin_big, keep, kw = _addln_common(c, nsplit, with_rb)
            make = lambda: dict(out=_frame(M, N, torch.bfloat16), x_out=torch.full_like(xin_big, NAN))
            run = lambda bf: ops.skinny_addln_gemm(xin_big[:M, :K], wsh, ops.EPI_GELU_TANH, g, b, c.eps, bias=bias,
                                                   out=bf["out"][:M, :N],
                                                   x_out=bf["x_out"][:M, :K] if with_xout else None, **kw)
            got = _twice(make, run)
            what = f"M={M} res_bias={with_rb} x_out={with_xout}"
            assert gc.same(xin_big, keep), what + ": x_in changed"
            xo = torch.full(tuple(xin_big.shape), NAN)
            if with_xout:
                xo[:M, :K] = c.x
            _check(got, dict(x_out=xo), what)
            bad = gc.gelu_bad(got["out"][:M, :N], c.ref + c.bias)
            assert not bad.any(), (what, bad.nonzero()[:8].tolist())
            frame = got["out"].clone()
            frame[:M, :N] = NAN
            assert bool(torch.isnan(frame.float()).all()), what + ": written outside the output"


@pytest.mark.parametrize("kind", ["bf16", "fp8"])
@pytest.mark.parametrize("K", gc.ADDLN_KS, ids=[ADDLN_K_IDS[k] for k in gc.ADDLN_KS])
def test_addln_qkv(K, kind):
    """The QKV epilogue behind the fused add + LN (4 slabs, res_bias, x_out), both cache types."""
    ops = _ops()
    full = gc.addln_case(gc.ADDLN_R, gc.N_QKV[0], K)
    wsh, g, b, bias = _wsh(full), _f32(full.gamma), _f32(full.beta), _f32(full.bias)
    for M in [m for m in (1, 4, 5, 8) if m <= ops.skinny_addln_max_rows(K)]:
        c = full.rows(M)
        io = _Qkv(M, full.N // 3, kind)
        xin_big, keep, kw = _addln_common(c, 4, True)
        make = lambda: dict(io.make(), x_out=torch.full_like(xin_big, NAN))
        run = lambda bf: ops.skinny_addln_gemm(xin_big[:M, :K], wsh, ops.EPI_QKV, g, b, c.eps, bias=bias,
                                               x_out=bf["x_out"][:M, :K], **io.args(bf), **kw)
        got = _twice(make, run)
        assert gc.same(xin_big, keep)
        _check(got, dict(io.want(c.ref + c.bias), x_out=_pad(c.x, 2, 32)), f"M={M}")


@pytest.mark.parametrize("kind", ["bf16", "fp8"])
@pytest.mark.parametrize("K", [768, 1024, 1280, 1600], ids=["K=768: nv4 3", "K=1024: nv4 4", "K=1280: nv4 5",
                                                            "K=1600: nv4 7, late gamma / beta loads"])
def test_addln_fixed_point_input_and_zero(K, kind):
    """x_in = v * 2^32 in int64, spread over the copies (the kernel sums them); ``zero``: a buffer of
    non-zero bytes is all zero afterwards and the guard words around it are unchanged."""
    ops = _ops()
    full = gc.addln_case(gc.ADDLN_R, gc.N_QKV[0], K)
    wsh, g, b, bias = _wsh(full), _f32(full.gamma), _f32(full.beta), _f32(full.bias)
    for M in [m for m in (1, 3, 4, 8) if m <= ops.skinny_addln_max_rows(K)]:
        c = full.rows(M)
        io = _Qkv(M, full.N // 3, kind)
        xf = gc.to_fix(c.x, ops.fix_copies()).to(DEV)
        keep = xf.clone()
        make = lambda: dict(io.make(), zero=torch.full((72,), KEY_SENTINEL, dtype=torch.int64, device=DEV))
        run = lambda bf: ops.skinny_addln_gemm(xf, wsh, ops.EPI_QKV, g, b, c.eps, bias=bias, zero=bf["zero"][4:-4],
                                               **io.args(bf))
        got = _twice(make, run)
        assert gc.same(xf, keep), "x_in changed"
        z = torch.zeros_like(got["zero"])
        z[:4], z[-4:] = KEY_SENTINEL, KEY_SENTINEL
        _check(got, dict(io.want(c.ref + c.bias), zero=z), f"M={M}")


def test_addln_refuses_a_width_without_a_kernel():
    """nv4 = 6 (K = 1536) has no instantiation: refused on the host, nothing launched or written."""
    ops = _ops()
    K, N = 1536, 96
    assert ops.skinny_addln_max_rows(K) == 0
    wsh = ops.shuffle_weight(torch.ones(N, K, dtype=torch.bfloat16, device=DEV))
    x, g = torch.ones(1, K, device=DEV), torch.ones(K, device=DEV)
    out = _frame(1, N, torch.bfloat16)
    with pytest.raises(ValueError):
        ops.skinny_addln_gemm(x, wsh, ops.EPI_GELU_TANH, g, g, 1e-5, out=out[:1, :N])
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.float()).all())


# ------------------------------------------------------------------------------------------------
# mid_ln_gemm
# ------------------------------------------------------------------------------------------------
MID_MS = [1, 16, 17, 32, 33, 48, 49, 64]  # row tiles 1 | 2 | 3 | 4 full and holding one row
MID_K_IDS = {544: "K=544: 17 k-blocks, 8 waves 3,3,3,3,3,2,0,0, 4 waves 5,5,5,2", 768: "K=768: nv4 3",
             1024: "K=1024: nv4 4"}
MID_GEO_IDS = ["geo0: 16-row blocks on grid.y, 8 | 4 waves", "geo1: all rows in one block, 8 waves",
               "geo2: all rows, 4 waves, M <= 32 only", "geo3: 8 waves over 2 column groups", "geo4: 16-row blocks, 8 waves",
               "geo5: 16-row blocks, 4 waves", "geo6: 32-row blocks, 8 waves", "geo7: 16-row blocks, 16 waves"]


def _mid_accepts(geo, M):
    """mid::pick_geometry builds every geometry for every row count but geo 2 past 32 rows."""
    return not (geo == 2 and M > 32)


@pytest.mark.parametrize("epi", ["bf16", "gelu"])
@pytest.mark.parametrize("geo", range(8), ids=MID_GEO_IDS)
@pytest.mark.parametrize("K", gc.MID_LN_KS, ids=[MID_K_IDS[k] for k in gc.MID_LN_KS])
def test_mid_ln_bf16_gelu(K, geo, epi):
    """Strided x rows (ldx = K + 32); M over the row-tile and row-block boundaries; a refused
    (geo, M) raises and writes nothing."""
    ops = _ops()
    full = gc.ln_case(gc.MID_R, gc.N_LN, K, 16 if epi == "gelu" else 1)
    wsh, g, b, bias = _wsh(full), _f32(full.gamma), _f32(full.beta), _f32(full.bias)
    N = full.N
    for M in MID_MS:
        c = full.rows(M)
        x = _pad(c.x, 1, 32, 9.0).to(DEV)[:M, :K]
        run = lambda bf: ops.mid_ln_gemm(x, wsh, ops.EPI_GELU_TANH if epi == "gelu" else ops.EPI_BF16, g, b, c.eps,
                                         bias=bias, out=bf["out"][:M, :N], geo=geo)
        make = lambda: dict(out=_frame(M, N, torch.bfloat16))
        if not _mid_accepts(geo, M):
            bufs = make()
            with pytest.raises(RuntimeError):
                run(bufs)
            torch.cuda.synchronize()
            assert bool(torch.isnan(bufs["out"].float()).all())
            continue
        got = _twice(make, run)
        v = c.ref + c.bias
        if epi == "bf16":
            _check(got, dict(out=_pad(gc.rne_bf16(v))), f"M={M}")
        else:
            bad = gc.gelu_bad(got["out"][:M, :N], v)
            assert not bad.any(), (M, bad.nonzero()[:8].tolist())
            frame = got["out"].clone()
            frame[:M, :N] = NAN
            assert bool(torch.isnan(frame.float()).all()), f"M={M}: written outside the output"


@pytest.mark.parametrize("kind", ["bf16", "fp8"])
@pytest.mark.parametrize("geo", range(8), ids=MID_GEO_IDS)
@pytest.mark.parametrize("K", gc.MID_LN_KS, ids=[MID_K_IDS[k] for k in gc.MID_LN_KS])
def test_mid_ln_qkv(K, geo, kind):
    """The row0 offsets of grid.y row blocks in the scatter: permuted slots, whole caches compared."""
    ops = _ops()
    N = gc.N_QKV[1] if K == 768 else gc.N_QKV[0]
    full = gc.ln_case(gc.MID_R, N, K)
    wsh, g, b, bias = _wsh(full), _f32(full.gamma), _f32(full.beta), _f32(full.bias)
    for M in MID_MS:
        c = full.rows(M)
        x, io = _f32(c.x), _Qkv(M, N // 3, kind)
        run = lambda bf: ops.mid_ln_gemm(x, wsh, ops.EPI_QKV, g, b, c.eps, bias=bias, geo=geo, **io.args(bf))
        if not _mid_accepts(geo, M):
            bufs = io.make()
            keep = {k: v.clone() for k, v in bufs.items()}
            with pytest.raises(RuntimeError):
                run(bufs)
            torch.cuda.synchronize()
            assert all(gc.same(bufs[k], keep[k]) for k in bufs)
            continue
        _check(_twice(io.make, run), io.want(c.ref + c.bias), f"M={M}")


# ------------------------------------------------------------------------------------------------
# mid_proj
# ------------------------------------------------------------------------------------------------
PROJ_MS = [1, 16, 17, 32, 33, 64]  # FULL (M % 16 MT == 0) and guarded instantiations of 1, 2 and 4 row tiles


def _proj_accepts(geo, K, M):
    """mid::proj_shape / proj_geo: K/32 must split exactly over the geometry's waves within its
    register budget.  geo 0 / 4 / 5: 16-row blocks; 6: 32-row blocks; 1-3: all rows in one block."""
    mt = 1 if M <= 16 else (2 if M <= 32 else 4)
    return {0: True,
            1: K != 4096 or mt <= 2,                       # 8 waves: 3, 4, 12 k-blocks, 16 up to 32 rows
            2: K in (768, 1024) or (K == 3072 and mt == 1),  # 4 waves: 6, 8, 24 (16 rows)
            3: K in (3072, 4096) and mt == 1,              # 16 waves: 6, 8 (16 rows)
            4: K != 4096,                                  # 16-row blocks, 4 waves
            5: K in (3072, 4096),                          # 16-row blocks, 16 waves
            6: True}[geo]                                  # 32-row blocks, 8 waves


PROJ_GEO_IDS = ["geo0: 16-row blocks, 4 waves (16 where K/32 splits into 6 or 8 each)", "geo1: all rows, 8 waves",
                "geo2: all rows, 4 waves", "geo3: all rows, 16 waves, M <= 16", "geo4: 16-row blocks, 4 waves",
                "geo5: 16-row blocks, 16 waves", "geo6: 32-row blocks, 8 waves"]


@pytest.mark.parametrize("geo", range(7), ids=PROJ_GEO_IDS)
@pytest.mark.parametrize("K", gc.MID_PROJ_KS, ids=["K=768: 24 k-blocks", "K=1024: 32", "K=3072: 96", "K=4096: 128"])
def test_mid_proj(K, geo):
    """x += a W^T + b on an integer fp32 residual, in place, exact; with and without the bias; rows
    past M and columns past N (ldx = N + 16) unchanged; a refused (geo, K, M) raises and writes nothing."""
    ops = _ops()
    full = gc.plain_case(gc.MID_R, gc.N_PLAIN, K)
    wsh, bias = _wsh(full), _f32(full.bias)
    N = full.N
    for M in PROJ_MS:
        c = full.rows(M)
        a = _bf16(c.a)
        old = _ints_frame(M, N, torch.float32)
        for with_bias in (True, False):
            make = lambda: dict(x=old.to(DEV))
            run = lambda bf: ops.mid_proj(a, wsh, bf["x"][:M, :N], bias=bias if with_bias else None, geo=geo)
            if not _proj_accepts(geo, K, M):
                bufs = make()
                with pytest.raises(RuntimeError):
                    run(bufs)
                torch.cuda.synchronize()
                assert gc.same(bufs["x"], old), (M, "refused launch wrote")
                continue
            want = old.clone()
            want[:M, :N] += (c.ref + (c.bias if with_bias else 0)).float()
            _check(_twice(make, run), dict(x=want), f"M={M} bias={with_bias}")


# ------------------------------------------------------------------------------------------------
# gemm_ps
# ------------------------------------------------------------------------------------------------
PS_MS = [1, 31, 32, 33, 63, 64, 65, 129]  # ragged / full 32- and 64-row blocks, a third and fifth block of one row
PS_K_IDS = ["Kc=128: 1 chunk of 4 k-blocks", "Kc=256: 2 chunks (one of 8)", "Kc=384: 3 chunks", "Kc=768: 6 chunks (3 of 8)"]
# (mt, nt, col_wgs): the four of test_gemm_ps_bf16_gelu, the default, and one column workgroup whose
# 8 wave slots take 10 tiles (a persistent loop with a ragged second pass)
PS_GEOS = [(2, 1, None), (2, 2, None), (4, 2, None), (4, 1, 3), None, (2, 2, 1)]
PS_GEO_IDS = ["mt2-nt1", "mt2-nt2", "mt4-nt2", "mt4-nt1-cw3", "default", "mt2-nt2-cw1: 10 tiles on 8 slots"]


def _ps_geo(geo, N):
    if geo is None:
        return None
    mt, nt, cw = geo
    return mt, nt, cw or -(-(N // (16 * nt)) // 8)


@pytest.mark.parametrize("epi", ["bf16", "gelu"])
@pytest.mark.parametrize("geo", PS_GEOS, ids=PS_GEO_IDS)
@pytest.mark.parametrize("K", gc.PS_KS, ids=PS_K_IDS)
def test_gemm_ps_bf16_gelu(K, geo, epi):
    ops = _ops()
    full = gc.plain_case(gc.PS_R, gc.N_PS, K, 16 if epi == "gelu" else 1)
    wsh, bias = _wsh(full), _f32(full.bias)
    N = full.N
    for M in PS_MS:
        c = full.rows(M)
        a = _bf16(c.a)
        got = _twice(lambda: dict(out=_frame(M, N, torch.bfloat16)),
                     lambda bf: ops.gemm_ps(a, wsh, ops.EPI_GELU_TANH if epi == "gelu" else ops.EPI_BF16, bias=bias,
                                            out=bf["out"][:M, :N], geometry=_ps_geo(geo, N)))
        v = c.ref + c.bias
        if epi == "bf16":
            _check(got, dict(out=_pad(gc.rne_bf16(v))), f"M={M}")
        else:
            bad = gc.gelu_bad(got["out"][:M, :N], v)
            assert not bad.any(), (M, bad.nonzero()[:8].tolist())
            frame = got["out"].clone()
            frame[:M, :N] = NAN
            assert bool(torch.isnan(frame.float()).all()), f"M={M}: written outside the output"


@pytest.mark.parametrize("geo", PS_GEOS, ids=PS_GEO_IDS)
@pytest.mark.parametrize("Kc,split", gc.PS_SPLITS)
def test_gemm_ps_partial_slabs(Kc, split, geo):
    """EPI_PARTIAL: every fp32 slab equals ITS K slice's product (not only the sum)."""
    ops = _ops()
    full = gc.plain_case(gc.PS_R, gc.N_PS, Kc * split)
    wsh = _wsh(full)
    N = full.N
    for M in PS_MS:
        c = full.rows(M)
        a = _bf16(c.a)
        want = torch.full((split, M + 3, N + 16), NAN)
        for s in range(split):
            ks = slice(s * Kc, (s + 1) * Kc)
            want[s, :M, :N] = (c.a[:, ks] @ c.w[:, ks].t()).float()
        got = _twice(lambda: dict(out=torch.full((split, M + 3, N + 16), NAN, device=DEV)),
                     lambda bf: ops.gemm_ps(a, wsh, ops.EPI_PARTIAL, out=bf["out"][:, :M, :N], split_k=split,
                                            geometry=_ps_geo(geo, N)))
        _check(got, dict(out=want), f"M={M}")


@pytest.mark.parametrize("geo", PS_GEOS, ids=PS_GEO_IDS)
@pytest.mark.parametrize("K", gc.PS_KS, ids=PS_K_IDS)
def test_gemm_ps_qkv(K, geo):
    ops = _ops()
    full = gc.plain_case(gc.PS_R, gc.N_PS_QKV, K)
    wsh, bias = _wsh(full), _f32(full.bias)
    N = full.N
    for M in PS_MS:
        c = full.rows(M)
        a, io = _bf16(c.a), _Qkv(M, N // 3, "bf16")
        got = _twice(io.make, lambda bf: ops.gemm_ps(a, wsh, ops.EPI_QKV, bias=bias, geometry=_ps_geo(geo, N), **io.args(bf)))
        _check(got, io.want(c.ref + c.bias), f"M={M}")


@pytest.mark.parametrize("mt,nt", [(4, 2), (2, 2), (2, 1)], ids=["mt4-nt2 (8-k-block chunks where Kc % 256 == 0)", "mt2-nt2",
                                                                  "mt2-nt1"])
@pytest.mark.parametrize("col_wgs", [1, 3], ids=["cw1: 8 slots, ragged last pass", "cw3: 24 slots, some without a tile"])
@pytest.mark.parametrize("K", gc.PS_KS, ids=PS_K_IDS)
def test_gemm_ps_argmax(K, col_wgs, mt, nt):
    """N = 320: 10 (nt 2) or 20 (nt 1) column tiles on 8 or 24 wave slots -- the persistent loop's
    last pass is ragged and some slots own no tile (key 0).  One key per (row, wave slot): every key,
    the key columns past the slots untouched, every row's reduced token and value."""
    ops = _ops()
    N, vocab = 320, 300
    full = gc.argmax_case(gc.PS_R, N, K, vocab, False)
    wsh = _wsh(full)
    slots, tiles = 8 * col_wgs, N // (16 * nt)
    groups = gc.ps_slot_groups(N, nt, col_wgs)
    assert tiles % slots != 0
    for M in PS_MS:
        c = full.rows(M)
        a, seen = _bf16(c.a), gc.pack_seen(c.seen).to(DEV)
        got = _twice(lambda: dict(keys=_key_frame(M, slots)),
                     lambda bf: ops.gemm_ps(a, wsh, ops.EPI_ARGMAX, argmax_out=bf["keys"][:M], seen=seen, vocab=vocab,
                                            penalty=gc.PENALTY, geometry=(mt, nt, col_wgs)))
        _check(got, dict(keys=_key_want(gc.group_keys(c.logits, c.seen, vocab, groups), M, slots)), f"M={M}")
        _check_reduced(ops, got["keys"], slots, c)


def test_gemm_ps_default_argmax_geometry_key_slots():
    """The default LM-head geometry: keys past gemm_ps_key_slots columns are untouched."""
    ops = _ops()
    N, vocab, K, M = 320, 300, 768, 65
    c = gc.argmax_case(gc.PS_R, N, K, vocab, False).rows(M)
    mt, nt, cw = ops.gemm_ps_geometry(M, N, ops.EPI_ARGMAX, K=K)
    slots = ops.gemm_ps_key_slots(M, N, K)
    assert slots == 8 * cw
    groups = gc.ps_slot_groups(N, nt, cw)
    a, seen, wsh = _bf16(c.a), gc.pack_seen(c.seen).to(DEV), _wsh(c)
    got = _twice(lambda: dict(keys=_key_frame(M, slots)),
                 lambda bf: ops.gemm_ps(a, wsh, ops.EPI_ARGMAX, argmax_out=bf["keys"][:M], seen=seen, vocab=vocab,
                                        penalty=gc.PENALTY))
    _check(got, dict(keys=_key_want(gc.group_keys(c.logits, c.seen, vocab, groups), M, slots)))
    _check_reduced(ops, got["keys"], slots, c)
