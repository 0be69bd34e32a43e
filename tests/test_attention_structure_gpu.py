"""Every attention kernel against the count, comb and random families of attention_cases.py: one
missing, doubled or extra key, a skipped rescale or a wrong dimension index fails these at every
cache length, which atol = rtol = 2e-2 on randn data does not (tests/test_attention_cases_cpu.py
shows both on the CPU).  Bounds and their derivation: attention_cases.py.

Kernels: row_attention wave / lds / persist on the bf16 cache, wave / persist on the fp8 cache;
tile_attention (causal) on both; attention_split in six geometries, attention_oproj and
attention_oproj_grouped on both.  The persistent fp8 kernel's unroll 6 and 8 run in child processes
(the override is read once per process): ``python -m test_attention_structure_gpu <unroll>``."""
import collections
import os
import subprocess
import sys

import pytest
import torch

import attention_cases as ac

pytestmark = pytest.mark.gpu

DEV = "cuda"
TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
H_ROW, H_FUSED = 5, 12  # 5: a partial last group of four heads
Q_SENTINEL, OUT_SENTINEL = float("nan"), -55.0


def _ops():
    from distributed_lms_raft_llm_amd import ops

    ops.lib()
    return ops


# ------------------------------------------------------------------------------------------------
# device copies and references, one per case (never modified)
# ------------------------------------------------------------------------------------------------
_gpu_cache, _ref_cache = {}, {}


def _gpu(case, kind, nan_tail=True):
    """``case`` (one of attention_cases' cached builders' results) on the device; nan_tail False:
    the caches keep their ordinary values past kvlen."""
    key = (id(case), kind, nan_tail)
    if key not in _gpu_cache:
        tail = case.slot_kvlen if nan_tail else None
        _gpu_cache[key] = ac.Case(q=case.q.to(torch.bfloat16).to(DEV), k=ac.cache(case.k, kind, tail).to(DEV),
                                  v=ac.cache(case.v, kind, tail).to(DEV), slot=case.row_slot.to(DEV),
                                  kvlen=case.row_kvlen.to(DEV))
    return _gpu_cache[key]


def _ref(case):
    """The fp64 reference (out, P.|V|), evaluated on the GPU by torch, kept on the CPU."""
    if id(case) not in _ref_cache:
        out, pav = ac.reference(case.q.to(DEV), case.k.to(DEV), case.v.to(DEV), case.row_slot.to(DEV),
                                case.row_kvlen.to(DEV))
        _ref_cache[id(case)] = (out.cpu(), pav.cpu())
    return _ref_cache[id(case)]


# ------------------------------------------------------------------------------------------------
# the kernels: run(ops, case, q, k, v, slot, kvlen, out) -> bf16 [R, H*64]
# ------------------------------------------------------------------------------------------------
def _row(impl):
    def run(ops, case, q, k, v, slot, kvlen, out):
        return ops.row_attention(q, k, v, slot, kvlen, out=out, impl=impl, blocks=64)

    return run


def _tile(ops, case, q, k, v, slot, kvlen, out):
    return ops.tile_attention(q, k, v, slot, kvlen, ops.AttnTiles(case.lens, DEV), out=out)


_split_ws = []


def _split_workspace(ops):
    """One workspace for every attention_split call of this module: the largest call is the comb
    family's 2560 rows x 5 heads over 64 workgroups."""
    if not _split_ws:
        _split_ws.append(ops.AttnSplitWorkspace(len(ac.KVLENS) * 128 * H_ROW, 64, DEV))
    return _split_ws[0]


def _split(waves, splits):
    def run(ops, case, q, k, v, slot, kvlen, out):
        ws = _split_workspace(ops)
        if waves:
            out = ops.attention_split(q, k, v, slot, kvlen, out=out, waves=waves, splits=splits, workspace=ws)
        else:  # the engine's geometry, per cache length (a call's rows share kv_len_max there)
            if out is None:
                out = torch.empty(q.shape[0], case.H * 64, dtype=torch.bfloat16, device=DEV)
            lens = case.row_kvlen
            for L in lens.unique().tolist():
                idx = (lens == L).nonzero()[:, 0].to(DEV)
                nw, ns = ops.attention_split_geometry(idx.numel() * case.H, L)
                out[idx] = ops.attention_split(q[idx], k, v, slot[idx], kvlen[idx], waves=nw, splits=ns, workspace=ws)
        assert int(ws.counters.abs().sum()) == 0  # re-armed by the last workgroup of every pair
        return out

    return run


_wo = {}


def _identity_wo(ops, n):
    if n not in _wo:
        _wo[n] = ops.shuffle_weight(torch.eye(n, device=DEV).to(torch.bfloat16))
    return _wo[n]


def _from_slabs(parts):
    """parts [calls, G, rows, H*64] fp32, written through W_o = I: slab g must hold the bf16 outputs
    of its heads in their own columns and exact zeros elsewhere.  -> [calls, rows, H*64] bf16."""
    n, G, rows, N = parts.shape
    p = parts.view(n, G, rows, G, N // G)
    own = torch.diagonal(p, dim1=1, dim2=3).permute(0, 1, 3, 2).reshape(n, rows, N)  # slab g's own columns, g-major
    off = p.clone()
    torch.diagonal(off, dim1=1, dim2=3).zero_()
    assert bool((off == 0).all()), "a slab holds something outside its heads' columns"
    out = own.to(torch.bfloat16)
    same = (out.float() == own) | torch.isnan(own)
    assert bool(same.all()), "a slab value is not a bf16 number"
    return out


def _oproj(M):
    def run(ops, case, q, k, v, slot, kvlen, out):
        H, N, R = case.H, case.H * 64, q.shape[0]
        wo = _identity_wo(ops, N)
        calls = [(r0, min(M, R - r0)) for r0 in range(0, R, M)]
        parts = torch.full((len(calls), H, 4, N), 7.0, device=DEV)
        for i, (r0, m) in enumerate(calls):
            ops.attention_oproj(q[r0:r0 + m], k, v, slot[r0:r0 + m], kvlen[r0:r0 + m], wo, parts[i])
        for i, (r0, m) in enumerate(calls):
            if m < 4:
                assert bool((parts[i, :, m:] == 7.0).all()), "rows >= M of the slabs were written"
                parts[i, :, m:] = 0
        res = _from_slabs(parts)
        return torch.cat([res[i, :m] for i, (r0, m) in enumerate(calls)])

    return run


def _grouped(hg, tiles):
    def run(ops, case, q, k, v, slot, kvlen, out):
        H, N, R = case.H, case.H * 64, q.shape[0]
        wo = _identity_wo(ops, N)
        parts = torch.full((R, H // hg, 2, N), 7.0, device=DEV)
        for r in range(R):
            ops.attention_oproj_grouped(q[r:r + 1], k, v, slot[r:r + 1], kvlen[r:r + 1], wo, parts[r], hg, tiles=tiles)
        assert bool((parts[:, :, 1] == 7.0).all()), "row 1 of the slabs was written"
        return _from_slabs(parts[:, :, :1].contiguous())[:, 0]

    return run


Target = collections.namedtuple("Target", "name kind run H shape ulps rel p_rel")


def _targets():
    t = []
    for kind in ("bf16", "fp8"):
        for impl in ("wave", "lds", "persist"):
            if kind == "fp8" and impl == "lds":
                continue  # no fp8 build of the LDS kernel
            t.append(Target(f"row-{impl}-{kind}", kind, _row(impl), H_ROW, "row", 1, ac.REL, 0.0))
            if impl != "persist":
                t.append(Target(f"row-{impl}-{kind}-t2048", kind, _row(impl), H_ROW, "long", 1, ac.REL, 0.0))
        t.append(Target(f"tile-{kind}", kind, _tile, H_ROW, "tile", 1, ac.REL, ac.TILE_P_REL))
        for waves, splits in [(2, 1), (16, 1), (4, 3), (8, 4), (8, 64), (0, 0)]:
            name = f"split-w{waves}s{splits}-{kind}" if waves else f"split-engine-geometry-{kind}"
            t.append(Target(name, kind, _split(waves, splits), H_ROW, "row", 1, ac.REL, 0.0))
        for M in (4, 2, 1):  # 1 / 2 / 4 waves per row
            t.append(Target(f"oproj-m{M}-{kind}", kind, _oproj(M), H_FUSED, "fused", 2, ac.REL + ac.ULP_REL, 0.0))
        for hg, tiles in [(3, 3), (4, 1)]:
            t.append(Target(f"oproj-grouped-hg{hg}t{tiles}-{kind}", kind, _grouped(hg, tiles), H_FUSED, "fused", 2,
                            ac.REL + ac.ULP_REL, 0.0))
    return t


TARGETS = _targets()
target = pytest.mark.parametrize("tg", TARGETS, ids=[t.name for t in TARGETS])


def _count_cases(tg):
    if tg.shape == "tile":
        return [ac.tile_count_case(tg.H, code) for code in "AB"]
    if tg.shape == "long":
        return [ac.count_case(tg.H, code, ac.LONG_T, tuple(ac.LONG_KVLENS)) for code in "AB"]
    return [ac.count_case(tg.H, code) for code in "AB"]


def _comb_cases(tg):
    if tg.shape == "tile":
        return [ac.tile_comb_case(tg.H, off, sign) for off in ac.TILE_COMB_OFFSETS for sign in (1.0, -1.0)]
    if tg.shape == "long":
        return [ac.comb_case(tg.H, ac.LONG_T, tuple(ac.LONG_KVLENS))]
    if tg.shape == "fused":
        return [ac.comb_case(tg.H, ac.T_MAX, tuple(ac.KVLENS_FUSED), tuple(ac.RESIDUES_FUSED))]
    return [ac.comb_case(tg.H)]


def _random_case(tg):
    if tg.shape == "tile":
        return ac.tile_random_case(tg.H)
    if tg.shape == "long":
        return ac.random_case(tg.H, ac.LONG_T, tuple(ac.LONG_KVLENS))
    return ac.random_case(tg.H)


def _run(ops, tg, case, q=None, out=None):
    d = _gpu(case, tg.kind)
    return tg.run(ops, case, d.q if q is None else q, d.k, d.v, d.slot, d.kvlen, out)


def _explain(case, bad, out, want):
    out, want = out.detach().cpu().double(), want.cpu().double()
    lines = []
    for r, c in bad:
        row = f"row {r} kvlen {int(case.row_kvlen[r])}" + (f" (L, j, sign) {case.rows[r]}" if "rows" in case else "")
        lines.append(f"{row} head {c // 64} dim {c % 64}: got {out[r, c]:.9g} want {want[r, c]:.9g}")
    return "\n".join(lines)


def _count_failures(ops, tg):
    fails = []
    for case in _count_cases(tg):
        out = _run(ops, tg, case)
        bad = ac.count_mismatches(out, case, ulps=tg.ulps)
        if bad:
            fails.append(f"count code {case.code}:\n" + _explain(case, bad, out, ac.count_expected(case)))
    return fails


def _comb_failures(ops, tg):
    fails = []
    for case in _comb_cases(tg):
        out = _run(ops, tg, case)
        ref, pav = _ref(case)
        bad = ac.close_mismatches(out, ref, pav, rel=tg.rel, p_rel=tg.p_rel)
        if bad:
            fails.append("comb:\n" + _explain(case, bad, out, ref))
    return fails


@target
def test_count(tg):
    """q = 0, position-coded V: the output is count_d / kvlen to one bf16 ulp (two behind the fused
    out-projection), for both codes."""
    fails = _count_failures(_ops(), tg)
    assert not fails, "\n".join(fails)


@target
def test_comb(tg):
    """Scores exactly +-4 on the keys t = j (mod 64), 0 elsewhere, against the fp64 softmax."""
    fails = _comb_failures(_ops(), tg)
    assert not fails, "\n".join(fails)


@target
def test_random(tg):
    """randn data, one kvlen per slot, NaN in every K / V element past it; q and out are views of
    wider buffers (row stride H*64 + 64) filled with sentinels: the result is finite and tight
    against fp64, and nothing outside the R x H*64 output was written."""
    ops = _ops()
    case = _random_case(tg)
    d = _gpu(case, tg.kind)
    R, W = d.q.shape
    qbuf = torch.full((R + 3, W + 64), Q_SENTINEL, dtype=torch.bfloat16, device=DEV)
    qbuf[:R, :W] = d.q
    q0 = qbuf.clone()
    obuf = torch.full((R + 3, W + 64), OUT_SENTINEL, dtype=torch.bfloat16, device=DEV)
    out = _run(ops, tg, case, q=qbuf[:R, :W], out=None if tg.shape == "fused" else obuf[:R, :W])
    assert torch.equal(qbuf.view(torch.int16), q0.view(torch.int16))
    if tg.shape != "fused":
        assert out.data_ptr() == obuf.data_ptr() and out.stride(0) == W + 64
        assert bool((obuf[:, W:] == OUT_SENTINEL).all()) and bool((obuf[R:] == OUT_SENTINEL).all())
    assert bool(torch.isfinite(out.float()).all())
    ref, pav = _ref(case)
    bad = ac.close_mismatches(out, ref, pav, rel=tg.rel, p_rel=tg.p_rel, atol=ac.RANDOM_ATOL)
    assert not bad, _explain(case, bad, out, ref)
    # the content past kvlen is never used: the same bits over ordinary values there
    dp = _gpu(case, tg.kind, nan_tail=False)
    again = tg.run(ops, case, d.q, dp.k, dp.v, d.slot, d.kvlen, None)
    assert torch.equal(again, out.contiguous())


def test_persist_fp8_unroll_6_and_8_in_fresh_processes():
    """DLMS_ATTN_FP8_UNROLL is read once per process, so 6 and 8 (96- and 128-key blocks) each get
    a child of their own, one after the other; a child runs the count and comb families on
    row_attention(impl="persist") over the fp8 cache and exits non-zero on a mismatch."""
    for unroll in (6, 8):
        path = os.pathsep.join([TESTS, ROOT] + ([os.environ["PYTHONPATH"]] if os.environ.get("PYTHONPATH") else []))
        env = dict(os.environ, DLMS_ATTN_FP8_UNROLL=str(unroll), PYTHONPATH=path)
        p = subprocess.run([sys.executable, "-m", "test_attention_structure_gpu", str(unroll)], env=env, cwd=ROOT,
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, f"unroll {unroll}: exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
        assert f"persist-fp8 unroll {unroll}: ok" in p.stdout


def _child(unroll):
    assert os.environ.get("DLMS_ATTN_FP8_UNROLL") == str(unroll)
    ops = _ops()
    tg = next(t for t in TARGETS if t.name == "row-persist-fp8")
    fails = _count_failures(ops, tg) + _comb_failures(ops, tg)
    if fails:
        print("\n".join(fails))
        return 1
    print(f"persist-fp8 unroll {unroll}: ok")
    return 0


if __name__ == "__main__":
    sys.exit(_child(int(sys.argv[1])))
