"""tests/batched_ref.py without a GPU: pack_ref against the obvious torch statement, the float32 restatements of the reductions against
the float64 ones within gamma(n - 1) * sum |terms|, every case on its declared side of the kernels' shape predicates with both sides of each
predicate present, and the tile counts the job tables are built from (the address predicates are asserted from real pointers in
tests/test_gpu_batched_direct.py)."""
import numpy as np
import pytest
import torch

from tests import batched_ref as R


# ---- pack ---------------------------------------------------------------------------------------------------------------------------

DENSE = [(c, it) for c in R.PACK_CASES for it in c.items if R.is_dense(it)]


@pytest.mark.parametrize("case,it", DENSE, ids=[c.name for c, _ in DENSE])
def test_pack_ref_dense_is_the_permuted_parameter(case, it):
    src = R.pack_params(case, 1)[it.src]
    pre = R.sentinel(case.dst_len)
    got = R.pack_ref(pre, src, it)
    w = torch.from_numpy(src).reshape(it.I, it.J, it.T, 1)
    p = w.permute(2, 3, 1, 0) if it.mode else w.permute(2, 3, 0, 1)
    exp = torch.zeros((it.T, it.rows, it.cols))
    exp[:, :p.shape[2], :p.shape[3]] = p.reshape(it.T, p.shape[2], p.shape[3])
    n = it.T * it.rows * it.cols
    assert np.array_equal(R.bits(got[it.dst_off:it.dst_off + n]), R.bits(exp.numpy().reshape(-1)))
    rest = np.ones(case.dst_len, dtype=bool)
    rest[it.dst_off:it.dst_off + n] = False
    assert np.array_equal(R.bits(got[rest]), R.bits(pre[rest]))


def test_pack_ref_leaves_everything_outside_the_block():
    """strided items: exactly the T x rows x cols block changes; side-by-side neighbours keep their columns"""
    for case in R.PACK_CASES:
        srcs = R.pack_params(case, 2)
        pre = R.sentinel(case.dst_len)
        touched = np.zeros(case.dst_len, dtype=bool)
        for it in case.items:
            dld, ts = R.strides(it)
            t, r, c = np.ogrid[:it.T, :it.rows, :it.cols]
            idx = it.dst_off + t * ts + r * dld + c
            assert not touched[idx].any(), f"{case.name}: items overlap"
            touched[idx] = True
            one = R.pack_ref(pre, srcs[it.src], it)
            assert np.array_equal(R.bits(one) != R.bits(pre), _mask(case.dst_len, idx)), case.name
        allof = R.pack_ref_all(pre, srcs, case.items)
        assert np.array_equal(R.bits(allof) != R.bits(pre), touched), case.name
        assert touched[:64].sum() == 0 and touched[-64:].sum() == 0, f"{case.name}: no guard band"


def _mask(n, idx):
    m = np.zeros(n, dtype=bool)
    m[idx] = True
    return m


def test_rgb_pack_ref():
    for name, mode, I, J, T, rows, cols in R.RGB_PACK_CASES:
        src = R.values(R.rng(3), (I, J, T))
        it = R.item(mode, I, J, T, rows, cols, dst_off=64)
        got = R.pack_ref(R.sentinel(64 + rows * cols + 64), src, it)[64:64 + rows * cols].reshape(rows, cols)
        exp = torch.zeros((rows, cols))
        w = torch.from_numpy(src)
        for t in range(T):
            if mode == 2:
                exp[:I, 4 * t:4 * t + J] = w[:, :, t]
            else:
                exp[4 * t:4 * t + J, :I] = w[:, :, t].T
        assert np.array_equal(R.bits(got), R.bits(exp.numpy())), name
        assert (rows >= I and cols >= 4 * T) if mode == 2 else (rows >= 4 * T and cols >= I)
    rc = [(m, r, c, I, T) for _, m, I, _, T, r, c in R.RGB_PACK_CASES]
    assert any(m == 2 and r > I and c > 4 * T for m, r, c, I, T in rc) and any(m == 3 and r > 4 * T and c > I for m, r, c, I, T in rc)
    assert {J for _, _, _, J, _, _, _ in R.RGB_PACK_CASES} == {1, 3, 4} and {T for _, _, _, _, T, _, _ in R.RGB_PACK_CASES} == {9, 25, 121}


def test_pack_cases_cover_the_branches():
    items = [it for c in R.PACK_CASES for it in c.items]
    for it in items:
        assert it.T <= R.PACK_MAX_T and it.rows % 8 == 0 and it.cols % 32 == 0 and it.mode in (0, 1)
        pr, pc = (it.J, it.I) if it.mode else (it.I, it.J)
        dld, ts = R.strides(it)
        assert it.rows >= pr and it.cols >= pc and dld >= it.cols and ts >= (it.rows - 1) * dld + it.cols and it.j0 + it.J <= it.sJ
    preds = [(it, R.pack_predicates(it)) for it in items]
    for key in ("sjt4", "dld4", "ts4", "src16", "dst16", "al", "vec", "novec"):
        for mode in (0, 1):
            sides = {p[key] for it, p in preds if it.mode == mode}
            assert sides == {True, False}, f"mode {mode}: only {sides} of {key}"
    # each term of `al` decides it ALONE somewhere: al is false with only that term false
    for key in ("sjt4", "dld4", "ts4", "src16", "dst16"):
        assert any(not p[key] and all(p[k] for k in ("sjt4", "dld4", "ts4", "src16", "dst16") if k != key) for _, p in preds), key
    terms = ("sjt4", "dld4", "ts4", "src16", "dst16")
    for name, key in R.PACK_NOT_AL_BY.items():
        (it,) = R.PACK_CASES[R.PACK_IDS.index(name)].items
        assert [k for k in terms if not R.pack_predicates(it)[k]] == [key], name
    assert set(R.PACK_NOT_AL_BY.values()) == set(terms)
    # an item whose first tile takes whole-run loads and whose last does not, in both modes (J = 33 / J = 12)
    assert any(it.mode == 0 and it.J == 33 and p["vec"] and p["novec"] for it, p in preds)
    assert any(it.mode == 1 and it.J == 12 and p["vec"] and p["novec"] for it, p in preds)
    assert {it.T for it in items} >= {1, 4, 9, 25, 32}
    assert {it.I for it in items} | {it.J for it in items} >= {1, 3, 5, 31, 32, 33, 40, 64, 70}
    assert any(it.rows > -(-((it.J, it.I)[it.mode == 0]) // 8) * 8 and it.cols > -(-((it.I, it.J)[it.mode == 0]) // 32) * 32 for it in items)
    assert any(it.dld > it.cols for it in items) and any(it.tstride > it.rows * (it.dld or it.cols) for it in items)
    assert any(it.dst_off % 4 == 0 and it.dst_off != 64 for it in items) and any(it.dst_off % 4 for it in items)
    assert any(it.j0 and (it.j0 * it.T) % 4 == 0 for it in items) and any((it.j0 * it.T) % 4 for it in items)
    assert any((it.sJ * it.T) % 4 and (it.J, it.T) == (3, 9) for it in items)
    assert sum(len(c.items) > 1 for c in R.PACK_CASES) >= 2
    # every case runs the access path it declares
    assert set(R.PACK_PATH) == set(R.PACK_IDS) and set(R.PACK_PATH.values()) == {"al", "scalar", "mixed"}
    for c in R.PACK_CASES:
        al = [R.pack_predicates(it)["al"] for it in c.items]
        assert R.PACK_PATH[c.name] == ("al" if all(al) else "mixed" if any(al) else "scalar"), c.name


@pytest.mark.parametrize("n", R.MANY_PACK)
def test_many_pack_items(n):
    case = R.many_pack_case(n)
    assert len(case.items) == n and (n + 1 <= R.PREFIX_CACHE) == (n == 1023)
    tiles = [R.pack_tiles(it) for it in case.items]
    assert sum(tiles) > R.PACK_GRID and len(set(tiles)) > 3 and min(tiles) == 1 and max(tiles) == 1024
    assert tiles.count(1024) == 2 and all(it.T <= R.PACK_MAX_T for it in case.items)
    assert {R.pack_predicates(it)["al"] for it in case.items} == {True, False}
    assert 4 * case.dst_len < 8 << 20


def test_pack_tile_formula_is_the_tables():
    """(rows // 8) * (cols // 32): what packs.PackTable hands to JobTable.upload, read from its source"""
    import inspect
    from crdr_amd.hip import packs
    assert "(it.rows // 8) * (it.cols // 32)" in inspect.getsource(packs.PackTable._refresh)
    assert packs.PackTable.CAP == 4096 > max(R.MANY_PACK) + 1 > R.PREFIX_CACHE
    for c in R.PACK_CASES:
        for it in c.items:
            assert R.pack_tiles(it) == len([(r, cc) for r in range(0, it.rows, 8) for cc in range(0, it.cols, 32)])


# ---- weight-gradient reduce -------------------------------------------------------------------------------------------------------------

def _job(c):
    from crdr_amd.hip import lib as L
    return L.WgradJob(slab=0, g=0, PC=c.PC, QC=c.QC, gI=c.gI, gJ=c.gJ, T=c.T, nsplit=c.nsplit, smallj=c.smallj, accumulate=c.acc,
                      gJtot=c.gJtot if c.gJtot != c.gJ else 0, reserved=0)


@pytest.mark.parametrize("c", R.REDUCE_CASES, ids=R.REDUCE_IDS)
def test_reduce_ref32_within_gamma_of_ref64(c):
    slab, g = R.reduce_inputs(c, 11)
    r32 = R.reduce_ref32(slab, c, g)
    r64, bound = R.reduce_ref64(slab, c, g)
    assert r32.dtype == np.float32 and r32.shape == g.shape and np.isfinite(r32).all()
    assert np.all(np.abs(r32.astype(np.float64) - r64) <= bound)
    out = np.ones(g.shape, dtype=bool)
    out[:, c.j0:c.j0 + c.gJ] = False
    assert np.array_equal(R.bits(r32[out]), R.bits(g[out])) and np.all(bound[out] == 0)
    assert (bound[~out] > 0).all() == (c.nsplit + c.acc > 1)


def test_reduce_ref32_order_is_the_promised_one():
    """the restatement against a scalar, one-output-at-a-time evaluation of the same promise; and the order matters (another grouping differs)"""
    c = next(x for x in R.REDUCE_CASES if x.name == "v_s9_j64_t9_wide")
    slab, g = R.reduce_inputs(c, 12)
    r32 = R.reduce_ref32(slab, c, g)
    f = np.float32
    differs = 0
    for (i, j, t) in [(0, 0, 0), (2, 63, 8), (1, 17, 4), (2, 5, 3)]:
        x = [f(slab[s, t, i, j]) for s in range(9)]
        v0 = f(f(f(f(0) + x[0]) + x[4]) + x[8])
        v1, v2, v3 = f(f(f(0) + x[1]) + x[5]), f(f(f(0) + x[2]) + x[6]), f(f(f(0) + x[3]) + x[7])
        exp = f(g[i, c.j0 + j, t] + f(f(v0 + v1) + f(v2 + v3)))
        assert R.bits(r32[i, c.j0 + j, t]) == R.bits(exp)
    seq = np.zeros((c.gI, c.gJ, c.T), dtype=f)
    for s in range(9):
        seq = seq + R.reduce_terms(slab, c)[s]
    differs = int((R.bits(g[:, c.j0:c.j0 + c.gJ] + seq) != R.bits(r32[:, c.j0:c.j0 + c.gJ])).sum())
    assert differs > 0, "the inputs cannot tell the promised order from the sequential one"


def test_reduce_cases_cover_the_branches():
    from crdr_amd.hip import ops
    preds = {c.name: R.reduce_predicates(c) for c in R.REDUCE_CASES}
    for c in R.REDUCE_CASES:
        p = preds[c.name]
        assert c.gJ <= c.QC or c.smallj
        assert c.PC >= c.gI and c.j0 + c.gJ <= c.gJtot and (not c.smallj or (c.gJ <= 4 and c.T > 1))
        # the declared side: the name's first letter
        kind = c.name.split("_")[0]
        assert {"v": p["vector"], "s": not p["flat"] and not p["vector"], "f": p["flat"] and not p["smallj"], "sj": p["smallj"]}[kind], c.name
        assert ops._wgrad_job_tiles(_job(c)) == R.reduce_tiles(c) == (-(-c.gI * c.gJ * c.T // 256) if (c.smallj or c.T > 32) else c.gI * -(-c.gJ // 64))
    assert set(R.REDUCE_SCALAR_BY) == {c.name for c in R.REDUCE_CASES if c.name.startswith("s_")}
    for name, key in R.REDUCE_SCALAR_BY.items():
        assert [k for k in ("qc4", "slab16") if not preds[name][k]] == [key], name
    for key in ("flat", "smallj", "t_le_32", "qc4", "slab16", "vector"):
        assert {p[key] for p in preds.values()} == {True, False}, key
    reg = [c for c in R.REDUCE_CASES if not R.reduce_flat(c)]
    # scalar by QC alone and by the address alone
    assert any(c.QC % 4 and c.off == 0 for c in reg) and any(c.QC % 4 == 0 and c.off for c in reg)
    for form in (True, False):
        mine = [c for c in reg if preds[c.name]["vector"] == form]
        assert len({c.nsplit % 4 for c in mine}) == 4   # no, one, two and three leftover splits
        assert any(c.nsplit >= 8 for c in mine) and any(c.gJ % 64 for c in mine) and any(c.acc for c in mine) and any(not c.acc for c in mine)
        assert any(c.gJtot > c.gJ for c in mine) and any(c.PC > c.gI for c in mine)
    assert {c.nsplit for c in R.REDUCE_CASES} >= {1, 2, 3, 4, 5, 8, 9} and {c.T for c in R.REDUCE_CASES} >= {1, 9, 25, 32, 49}
    assert {c.gJ for c in reg} >= {1, 63, 64, 65, 130} and {c.off for c in R.REDUCE_CASES} >= {0, 1, 2}
    assert any(c.QC == c.gJ for c in reg) and any(c.QC == -(-c.gJ // 4) * 4 != c.gJ for c in reg) and any(c.QC == -(-c.gJ // 64) * 64 != -(-c.gJ // 4) * 4 for c in reg)
    sj = [c for c in R.REDUCE_CASES if c.smallj]
    assert {c.gJ for c in sj} >= {1, 3, 4} and {c.T for c in sj} == {25, 121}
    assert any(c.T > 32 and not c.smallj and c.nsplit >= 5 for c in R.REDUCE_CASES)


def test_many_reduce_jobs():
    from crdr_amd.hip import ops
    cases = R.many_reduce_cases(1200)
    assert len(cases) + 1 > R.PREFIX_CACHE and ops.DeferredWgrad.CAP >= len(cases)
    tiles = [R.reduce_tiles(c) for c in cases]
    assert tiles == [ops._wgrad_job_tiles(_job(c)) for c in cases] and len(set(tiles)) >= 4 and min(tiles) >= 1
    ps = [R.reduce_predicates(c) for c in cases]
    assert all({p[k] for p in ps} == {True, False} for k in ("flat", "smallj", "vector", "qc4", "slab16"))
    assert sum(int(np.prod(R.slab_shape(c))) for c in cases) * 4 < 8 << 20
    b = R.BIG_REDUCE
    assert R.reduce_tiles(b) == ops._wgrad_job_tiles(_job(b)) == 20480 > R.REDUCE_GRID and (b.gI, b.gJ, b.T, b.nsplit) == (4096, 320, 1, 1)


# ---- column-sum finish -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", R.COLSUM_CASES, ids=R.COLSUM_IDS)
def test_colsum_ref32_within_gamma_of_ref64(c):
    cs, pre, post = R.colsum_inputs(c, 21)
    r32 = R.colsum_finish_ref32(cs, c, pre, post)
    r64, bounds = R.colsum_finish_ref64(cs, c, pre, post)
    for k, (have, before) in enumerate(((c.pre, pre), (c.post, post))):
        assert r32[k].dtype == np.float32 and np.isfinite(r32[k]).all()
        assert np.all(np.abs(r32[k].astype(np.float64) - r64[k]) <= bounds[k])
        if not have:
            assert np.array_equal(R.bits(r32[k]), R.bits(before))
        else:
            assert (bounds[k] > 0).all() == (c.rows + c.acc > 1)


def test_colsum_ref32_order_is_the_promised_one():
    """one column, one output at a time: rows 0, 4, 8, ... into lane 0 and so on, slabs 0, 4, 8 into pass-B lane 0"""
    c = next(x for x in R.COLSUM_CASES if x.name == "r1025_c63_acc")
    cs, pre, post = R.colsum_inputs(c, 22)
    got = R.colsum_finish_ref32(cs, c, pre, post)
    f = np.float32

    def four(xs):
        lane = [f(0)] * 4
        for k, x in enumerate(xs):
            lane[k & 3] = f(lane[k & 3] + x)
        return f(f(f(lane[0] + lane[1]) + lane[2]) + lane[3])
    for k, col in ((0, 0), (1, 62), (0, 31)):
        slabs = [four([f(v) for v in cs[r0:r0 + 128, k, col]]) for r0 in range(0, c.rows, 128)]
        exp = f((pre, post)[k][col] + four(slabs))
        assert R.bits(got[k][col]) == R.bits(exp)
    seq = np.zeros((2, c.C), dtype=f)
    for r in range(c.rows):
        seq = seq + cs[r, :, :c.C]
    assert (R.bits(R.colsum_sums32(cs, c.C)) != R.bits(seq)).any(), "the inputs cannot tell the promised order from the sequential one"


def test_colsum_cases_cover_the_branches():
    from crdr_amd.hip import ops
    cs = R.COLSUM_CASES
    assert {c.rows for c in cs} >= {1, 3, 127, 128, 129, 600} and {c.C for c in cs} >= {1, 63, 64, 65, 200}
    assert any(c.rows % 128 and c.rows > 128 for c in cs) and any(c.rows % 4 for c in cs) and any(c.rows % 128 == 0 for c in cs)
    assert any(c.C % 64 for c in cs) and any(c.C % 64 == 0 for c in cs) and any(c.ld > c.C for c in cs) and any(c.ld == c.C for c in cs)
    assert all(c.ld >= c.C and (c.pre or c.post) for c in cs)
    assert {(c.pre, c.post) for c in cs} == {(1, 1), (0, 1), (1, 0)} and {c.acc for c in cs} == {0, 1}
    assert {(c.pre, c.post, c.acc) for c in cs} >= {(0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1)}
    assert {R.colsum_geometry(c)[0] % 4 for c in cs} == {0, 1, 2, 3} and len(cs) >= 20 <= ops.ColsumQueue.CAP
    for c in cs:
        nslab, cpad, tiles = R.colsum_geometry(c)
        assert tiles == ((cpad // 64) * nslab, cpad // 64) and (nslab - 1) * 128 < c.rows <= nslab * 128 and cpad - 64 < c.C <= cpad
    n, C, rows, _ = R.MANY_COLSUM
    big = R.ColsumCase("many", "", rows, C, C, 1, 1, 0)
    ta, tb = R.colsum_geometry(big)[2]
    assert (n * ta, n * tb) == (4200, 600) and n * ta > R.COLSUM_A_GRID and n * tb > R.COLSUM_B_GRID and n <= ops.ColsumQueue.CAP
    import inspect
    assert "((j.cpad // 64) * j.nslab, j.cpad // 64)" in inspect.getsource(ops.ColsumQueue.flush)


def test_gamma():
    assert R.gamma(0) == 0.0 and R.gamma(1) == R.U / (1 - R.U) and abs(R.gamma(1024) - 1024 * R.U) < 1e-8
