"""crdr_pack_weights_batched, crdr_wgrad_reduce_batched and crdr_colsum_finish_batched launched through their C ABI over hand-made job
tables, against the plain restatements of tests/batched_ref.py (proved against each other on the CPU by tests/test_batched_ref_host.py).  No conv
runs here.

  * A pack is BIT-EQUAL to plain indexing, over the whole destination buffer: every buffer is prefilled with a position-dependent sentinel, so
    a write outside the item's block (guard bands, the gaps between rows and taps, a neighbour's columns) fails the comparison.
  * A reduction is BIT-EQUAL to the float32 restatement that adds in the order the kernel's comments promise, and within
    gamma(n - 1) * sum |terms| of the float64 sum -- for every element, none excluded.  What the kernels may read but must never emit (slab
    columns gJ .. QC, slab rows gI .. PC, partial-row columns C .. ld) is NaN.
  * The address terms of the kernels' alignment predicates are asserted from the real data_ptr() values, so the access path each case is
    there for is known to have run.
Every test prints its worst error as a fraction of its bound (profiles/batched_direct_test_margins.txt)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import batched_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64


def dev():
    return torch.device("cuda:0")


def hip():
    from crdr_amd.hip import lib as L
    return L, L.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev())


def down(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def same_bits(got, exp, what):
    bad = np.flatnonzero(R.bits(got).reshape(-1) != R.bits(exp).reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} floats differ, first at {bad[:8].tolist()}: got {got.reshape(-1)[bad[:4]]}, expected {exp.reshape(-1)[bad[:4]]}"


def within(got, r64, bound, what):
    """|got - r64| <= bound for every element; -> the worst error as a fraction of its bound (elements with bound 0 must be equal)"""
    err = np.abs(got.astype(np.float64) - r64)
    assert np.all(err <= bound), f"{what}: {int((err > bound).sum())} elements beyond gamma(n - 1) * sum |terms|, worst {float((err / np.maximum(bound, 1e-300)).max()):.3g} of it"
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


# ================================================================================================================================ pack

def c_items(L, case, d_srcs, dst):
    """the crdr_pack_item rows of a case over real buffers, and each item's `al` predicate from the real addresses"""
    out, al = [], []
    for it in case.items:
        src_p, dst_p = d_srcs[it.src].data_ptr() + 4 * it.j0 * it.T, dst.data_ptr() + 4 * it.dst_off
        out.append(L.PackItem(src=src_p, dst=dst_p, I=it.I, J=it.J, T=it.T, rows=it.rows, cols=it.cols, mode=it.mode,
                              srcJ=it.sJ if it.sJ != it.J else 0, dld=it.dld, tstride=it.tstride))
        dld, ts = R.strides(it)
        al.append((it.sJ * it.T) % 4 == 0 and src_p % 16 == 0 and dst_p % 16 == 0 and dld % 4 == 0 and ts % 4 == 0)
    return out, al


def launch_batched_pack(L, lib, items, cap=None):
    from crdr_amd.hip.batched import JobTable
    tb = JobTable(dev(), L.PackItem, cap or max(16, len(items)), name="test").upload(items, lambda it: (it.rows // 8) * (it.cols // 32))
    L.check(lib.crdr_pack_weights_batched(*tb.operands, stream()), "pack_weights_batched")
    torch.cuda.synchronize()
    return tb


@pytest.mark.parametrize("case", R.PACK_CASES, ids=R.PACK_IDS)
def test_pack_batched_item_and_reference(case):
    L, lib = hip()
    srcs = R.pack_params(case, 100 + R.PACK_IDS.index(case.name))
    d_srcs = [up(s) for s in srcs]
    pre = R.sentinel(case.dst_len)
    exp = R.pack_ref(pre, srcs[0], case.items[0]) if len(case.items) == 1 else R.pack_ref_all(pre, srcs, case.items)
    # one launch of the batched kernel over all items of the case
    dst = up(pre)
    items, al = c_items(L, case, d_srcs, dst)
    assert al == [R.pack_predicates(it)["al"] for it in case.items], "the buffers are not aligned as the case assumes"
    assert R.PACK_PATH[case.name] == ("al" if all(al) else "mixed" if any(al) else "scalar")
    launch_batched_pack(L, lib, items)
    same_bits(down(dst), exp, f"{case.name} batched")
    # the single-item kernel, item after item
    dst1 = up(pre)
    for it in c_items(L, case, d_srcs, dst1)[0]:
        L.check(lib.crdr_pack_weight_item(C.byref(it), stream()), "pack_weight_item")
    same_bits(down(dst1), exp, f"{case.name} crdr_pack_weight_item")
    # dense items: the plain kernel too
    n_dense = 0
    if all(R.is_dense(it) for it in case.items):
        dst2 = up(pre)
        for it in case.items:
            L.check(lib.crdr_pack_weight(d_srcs[it.src].data_ptr(), dst2.data_ptr() + 4 * it.dst_off, it.I, it.J, it.T, it.rows, it.cols, it.mode,
                                         stream()), "pack_weight")
            n_dense += 1
        same_bits(down(dst2), exp, f"{case.name} crdr_pack_weight transpose={case.items[0].mode}")
    wrote = int((R.bits(exp) != R.bits(pre)).sum())
    print(f"pack {case.name} [{R.PACK_PATH[case.name]}]: batched = item{' = plain' if n_dense else ''} = pack_ref, {case.dst_len} floats bit-equal ({wrote} written)")


@pytest.mark.parametrize("name,mode,I,J,T,rows,cols", R.RGB_PACK_CASES, ids=[c[0] for c in R.RGB_PACK_CASES])
def test_pack_tapmajor_and_scatter(name, mode, I, J, T, rows, cols):
    L, lib = hip()
    src = R.values(R.rng(300 + T + J), (I, J, T))
    it = R.item(mode, I, J, T, rows, cols, dst_off=GUARD)
    pre = R.sentinel(GUARD + rows * cols + GUARD)
    dst, d_src = up(pre), up(src)
    L.check(lib.crdr_pack_weight(d_src.data_ptr(), dst.data_ptr() + 4 * GUARD, I, J, T, rows, cols, mode, stream()), "pack_weight")
    same_bits(down(dst), R.pack_ref(pre, src, it), name)
    print(f"pack {name} [mode {mode}]: crdr_pack_weight = pack_ref, {pre.size} floats bit-equal")


@pytest.mark.parametrize("n", R.MANY_PACK)
def test_pack_many_items(n):
    """n + 1 prefix entries on either side of the LDS cache, more tiles than workgroups; every item has its own content, all are compared"""
    from crdr_amd.hip import packs
    L, lib = hip()
    case = R.many_pack_case(n)
    srcs = R.pack_params(case, 400 + n)
    flat = up(np.concatenate([s.reshape(-1) for s in srcs] + [np.zeros(4, np.float32)]))
    offs = np.concatenate([[0], np.cumsum([s.size for s in srcs])])
    d_srcs = [flat[offs[k]:offs[k + 1]] for k in range(len(srcs))]
    pre = R.sentinel(case.dst_len)
    dst = up(pre)
    items, al = c_items(L, case, d_srcs, dst)
    assert 0 < sum(al) < n, "the launch should mix 16-byte and scalar items"
    tb = launch_batched_pack(L, lib, items, cap=packs.PackTable.CAP)
    meta = tb.meta.cpu().tolist()
    assert meta[0] == n and meta[1] == sum(R.pack_tiles(it) for it in case.items) > R.PACK_GRID and (n + 1 > R.PREFIX_CACHE) == (n == 1200)
    same_bits(down(dst), R.pack_ref_all(pre, srcs, case.items), case.name)
    print(f"pack {case.name}: {n} items, {meta[1]} tiles on {R.PACK_GRID} workgroups, prefix search in {'LDS' if n + 1 <= R.PREFIX_CACHE else 'global memory'}, "
          f"{sum(al)} items 16-byte: {case.dst_len} floats bit-equal")


def test_pack_table_routing():
    """PackTable over an address range holding a 3 x 3, a 7 x 7 (T = 49) and a tap-major RGB entry: one batched launch for the first, single
    launches for the others, all three packs == pack_ref"""
    from crdr_amd.hip import packs
    shapes = [(40, 24, 3, 3), (8, 5, 7, 7), (33, 3, 3, 3)]
    sizes = [int(np.prod(s)) for s in shapes]
    host = R.values(R.rng(500), (sum(sizes),))
    flat = up(host)
    ws, o = [], 0
    for s, n in zip(shapes, sizes):
        ws.append(flat[o:o + n].view(s))
        o += n
    its = [R.item(0, 40, 24, 9, 40, 32, dst_off=GUARD), R.item(1, 8, 5, 49, 8, 32, dst_off=GUARD), R.item(2, 33, 3, 9, 64, 64, dst_off=GUARD)]
    pres = [R.sentinel(GUARD + (it.T if it.mode < 2 else 1) * it.rows * it.cols + GUARD, k) for k, it in enumerate(its)]
    wholes = [up(p) for p in pres]
    ents = [packs._PackEntry(w, whole[GUARD:whole.numel() - GUARD], it.mode, it.rows, it.cols) for w, whole, it in zip(ws, wholes, its)]

    class _Flat:  # an address range standing in for an optimiser's flat parameter buffer
        device = dev()

        def data_ptr(self):
            return flat.data_ptr()

        def numel(self):
            return flat.numel()
    tb = packs.PackTable(_Flat())
    tb.refill()
    assert [id(e) for e in tb.entries] == [id(ents[0])] and {id(e) for e in tb.singles} == {id(ents[1]), id(ents[2])}
    assert tb.table.meta.cpu().tolist() == [1, R.pack_tiles(its[0])]
    o = 0
    for it, pre, whole, n in zip(its, pres, wholes, sizes):
        same_bits(down(whole), R.pack_ref(pre, host[o:o + n], it), f"PackTable entry T = {it.T} mode {it.mode}")
        o += n
    print("pack PackTable: 3x3 batched, 7x7 (T = 49) and tap-major RGB single launches, all three bit-equal to pack_ref")


# ======================================================================================================================== wgrad reduce

def run_reduce(cases, seed):
    """One reduce_jobs_now call over `cases` (each its own slab and its own gradient inside one sentinel-filled buffer); every check of the
    module docstring on every job; -> [(worst fraction of the gamma bound, terms per output)]"""
    from crdr_amd.hip import ops
    L, _ = hip()
    inputs = [R.reduce_inputs(c, seed + k) for k, c in enumerate(cases)]
    # slabs: each `off` floats past a 16-byte boundary of one allocation, NaN between them
    s_off, pos = [], 0
    for c, (slab, _) in zip(cases, inputs):
        s_off.append(pos + c.off)
        pos += (c.off + slab.size + 3) // 4 * 4 + 4
    slabs = np.full(pos, np.nan, dtype=np.float32)
    for o, (slab, _) in zip(s_off, inputs):
        slabs[o:o + slab.size] = slab.reshape(-1)
    # gradients: GUARD sentinel floats in front, behind and between
    g_off, pos = [], GUARD
    for _, g in inputs:
        g_off.append(pos)
        pos += g.size + GUARD
    pre = R.sentinel(pos, seed)
    for o, (_, g) in zip(g_off, inputs):
        pre[o:o + g.size] = g.reshape(-1)
    d_slabs, d_g = up(slabs), up(pre)
    assert d_slabs.data_ptr() % 16 == 0
    jobs = []
    for c, so, go in zip(cases, s_off, g_off):
        sp = d_slabs.data_ptr() + 4 * so
        p = R.reduce_predicates(c)
        assert (sp % 16 == 0) == p["slab16"] and (not p["flat"] and c.QC % 4 == 0 and sp % 16 == 0) == p["vector"], c.name
        jobs.append(L.WgradJob(slab=sp, g=d_g.data_ptr() + 4 * (go + c.j0 * c.T), PC=c.PC, QC=c.QC, gI=c.gI, gJ=c.gJ, T=c.T, nsplit=c.nsplit,
                               smallj=c.smallj, accumulate=c.acc, gJtot=c.gJtot if c.gJtot != c.gJ else 0, reserved=0))
    ops.reduce_jobs_now(jobs, dev())
    got = down(d_g)
    exp = pre.copy()
    res = []
    for c, (slab, g), go in zip(cases, inputs, g_off):
        exp[go:go + g.size] = R.reduce_ref32(slab, c, g).reshape(-1)
        r64, bound = R.reduce_ref64(slab, c, g)
        res.append((within(got[go:go + g.size].reshape(g.shape), r64, bound, c.name), c.nsplit + c.acc))
    same_bits(got, exp, "+".join(c.name for c in cases[:3]))
    return res


@pytest.mark.parametrize("c", R.REDUCE_CASES, ids=R.REDUCE_IDS)
def test_reduce_case(c):
    p = R.reduce_predicates(c)
    (worst, n), = run_reduce([c], 600 + R.REDUCE_IDS.index(c.name))
    path = "smallj" if p["smallj"] else "flat" if p["flat"] else "vector" if p["vector"] else "scalar"
    print(f"reduce {c.name} [{path}]: bit-equal to the float32 restatement; {worst:.3f} of gamma({n - 1}) * sum|terms| at worst")


def test_reduce_many_jobs():
    """1200 jobs in one launch: the prefix search from global memory, every form of job mixed"""
    cases = R.many_reduce_cases(1200)
    res = run_reduce(cases, 700)
    print(f"reduce many_1200: {len(cases)} jobs, {sum(R.reduce_tiles(c) for c in cases)} tiles, all bit-equal; "
          f"{max(r[0] for r in res):.3f} of the gamma bound at worst")


def test_reduce_grid_stride():
    """a 4096 x 320 gradient (20480 tiles on 16384 workgroups) between small jobs of every form"""
    by = {c.name: c for c in R.REDUCE_CASES}
    cases = [by["v_s5_j130_qc192_t25"], by["sj_j3_t25_s4"], R.BIG_REDUCE, by["s_s3_j65_t9"], by["f_t49_s3_j65"]]
    assert sum(R.reduce_tiles(c) for c in cases) > R.REDUCE_GRID + R.reduce_tiles(cases[0]) + R.reduce_tiles(cases[1])
    res = run_reduce(cases, 800)
    print(f"reduce grid_stride: {sum(R.reduce_tiles(c) for c in cases)} tiles on {R.REDUCE_GRID} workgroups, all bit-equal; "
          f"{max(r[0] for r in res):.3f} of the gamma bound at worst")


# ======================================================================================================================= colsum finish

def run_colsum(cases, seed, shared=0):
    """One ColsumQueue flush over `cases` (shared > 0: the jobs read `shared` partial buffers in turn instead of one each); every check of
    the module docstring on every job; -> the worst fraction of the gamma bound"""
    from crdr_amd.hip import ops
    L, lib = hip()
    assert lib.crdr_colsum_slab_rows() == R.COLSUM_SLAB
    inputs = [R.colsum_inputs(c, seed + k) for k, c in enumerate(cases[:shared or len(cases)])]
    d_cs = [up(i[0]) for i in inputs]
    if shared:   # the outputs stay per job
        gen = R.rng(seed + 99)
        inputs = [(inputs[k % shared][0], *[R.values(gen, (c.C,)) if c.acc else R.sentinel(c.C, k + s) for s in range(2)]) for k, c in enumerate(cases)]
    o_off, pos = [], GUARD
    for c in cases:
        o_off.append((pos, pos + c.C + 8))
        pos += 2 * (c.C + 8) + GUARD
    pre = R.sentinel(pos, seed)
    for (op, oq), (_, a, b) in zip(o_off, inputs):
        pre[op:op + a.size], pre[oq:oq + b.size] = a, b
    d_out = up(pre)
    q = ops.ColsumQueue(dev(), arena_bytes=1 << 20)
    for k, (c, (op, oq)) in enumerate(zip(cases, o_off)):
        q.add(d_cs[k % shared if shared else k].data_ptr(), c.rows, c.ld, c.C, d_out.data_ptr() + 4 * op if c.pre else None,
              d_out.data_ptr() + 4 * oq if c.post else None, bool(c.acc))
    chain = 0
    for jb, c in zip(q.jobs, cases):   # the table rows the kernels will read
        nslab, cpad, _ = R.colsum_geometry(c)
        assert (jb.nslab, jb.cpad, jb.scratch_off) == (nslab, cpad, chain) and bool(jb.out_pre) == bool(c.pre) and bool(jb.out_post) == bool(c.post)
        chain += nslab * 2 * cpad
    q.flush(("test", seed))
    got = down(d_out)
    exp, worst, sums = pre.copy(), 0.0, {}
    for k, (c, (cs, a, b), (op, oq)) in enumerate(zip(cases, inputs, o_off)):
        key = k % shared if shared else k
        if key not in sums:
            sums[key] = R.colsum_sums32(cs, c.C)
        r32 = R.colsum_finish_ref32(cs, c, a, b, sums=sums[key])
        r64, bounds = R.colsum_finish_ref64(cs, c, a, b)
        exp[op:op + c.C], exp[oq:oq + c.C] = r32
        for o, r, bd, nm in ((op, r64[0], bounds[0], "pre"), (oq, r64[1], bounds[1], "post")):
            worst = max(worst, within(got[o:o + c.C], r, bd, f"{c.name} {nm}"))
    same_bits(got, exp, "+".join(c.name for c in cases[:3]))
    return worst


@pytest.mark.parametrize("c", R.COLSUM_CASES, ids=R.COLSUM_IDS)
def test_colsum_case(c):
    worst = run_colsum([c], 900 + R.COLSUM_IDS.index(c.name))
    print(f"colsum {c.name}: bit-equal to the float32 restatement; {worst:.3f} of gamma({c.rows + c.acc - 1}) * sum|terms| at worst")


def test_colsum_mixed_flush():
    """every case in ONE flush: the chained scratch offsets, both prefix rows"""
    worst = run_colsum(R.COLSUM_CASES, 1000)
    print(f"colsum mixed flush: {len(R.COLSUM_CASES)} jobs, all bit-equal; {worst:.3f} of the gamma bound at worst")


def test_colsum_grid_stride():
    """300 jobs of 800 rows x 128 columns over four shared partial buffers: 4200 pass-A tiles on 4096 workgroups, 600 pass-B tiles on 512"""
    n, Cc, rows, shared = R.MANY_COLSUM
    cases = [R.ColsumCase(f"g{k}", "", rows, Cc, Cc, int(k % 7 != 3), int(k % 7 != 5), (k // 4) & 1) for k in range(n)]
    tiles = [sum(R.colsum_geometry(c)[2][p] for c in cases) for p in range(2)]
    assert tiles[0] > R.COLSUM_A_GRID and tiles[1] > R.COLSUM_B_GRID and all(c.pre or c.post for c in cases)
    worst = run_colsum(cases, 1100, shared=shared)
    print(f"colsum grid_stride: {n} jobs, {tiles[0]} / {tiles[1]} tiles on {R.COLSUM_A_GRID} / {R.COLSUM_B_GRID} workgroups, all bit-equal; "
          f"{worst:.3f} of gamma({rows}) * sum|terms| at worst")
