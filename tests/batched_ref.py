"""Plain numpy restatements of the three batched launches that end every training step, and the cases their direct tests run.

  crdr_pack_weights_batched   (csrc/wgrad.hip)    pack_ref: plain indexing, to be matched bit for bit over the WHOLE destination buffer
  crdr_wgrad_reduce_batched   (csrc/wgrad.hip)    reduce_ref64 (float64 sum) and reduce_ref32 (float32, the order the kernel's comments promise)
  crdr_colsum_finish_batched  (csrc/eltwise.hip)  colsum_finish_ref64 / colsum_finish_ref32, the same pair for pass A + pass B

Nothing here is shaped like a kernel: no tiles, no staging, no thread mapping -- an index formula per output and, for the float32 restatements,
the ORDER of the additions and nothing else.  The kernels move data and add float32 in a fixed order, and the library is built without
fast-math, so the tests (tests/test_gpu_batched_direct.py) hold a pack to bit equality with pack_ref and a reduction to bit equality with
its float32 restatement AND to the textbook bound  |fl(sum) - sum| <= gamma(n - 1) * sum |terms|,  gamma(k) = k u / (1 - k u), u = 2^-24,
against the float64 sum; the bound holds for any order of n terms, so it rests on no measurement.  tests/test_batched_ref_host.py checks the
restatements against each other and the case lists against the branches they claim, without a GPU.

The case lists carry, beside every case, the branch it is there for; `*_predicates` evaluate the kernels' shape predicates from the shapes alone.
"""
import collections

import numpy as np

U = 2.0 ** -24
PREFIX_CACHE = 1024      # find_entry searches LDS while n + 1 <= this many prefix entries, global memory beyond
PACK_GRID, REDUCE_GRID, COLSUM_A_GRID, COLSUM_B_GRID = 2048, 16384, 4096, 512   # workgroups of the four launches (grid-stride beyond)
PACK_MAX_T = REDUCE_MAX_T = 32
COLSUM_SLAB = 128        # partial rows per pass-A slab (crdr_colsum_slab_rows)


def gamma(k):
    return k * U / (1.0 - k * U)


def rng(seed: int):
    return np.random.default_rng(seed)


def values(gen, shape):
    """seeded float32 of mixed sign and magnitude (cancellation in the sums, no zeros, no ties by construction of nothing: the
    restatements decide the order, so ties are harmless)"""
    return (gen.standard_normal(shape) * np.exp2(gen.integers(-3, 4, shape))).astype(np.float32)


def sentinel(n: int, salt: int = 0):
    """finite position-dependent float32 pattern far outside the data's range: a write that lands in the wrong place cannot reproduce it"""
    return (-(1024.0 + ((np.arange(n, dtype=np.int64) * 7 + salt) % 251))).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ======================================================================================================================== pack
# One pack item, as crdr_pack_item describes it (addresses as float offsets into the case's buffers):
#   src      index of the case's parameter [I][sJ][T] this item reads
#   j0       first input channel of the sub-block (J channels from there); sJ = second dim of the parameter
#   dst_off  floats into the destination buffer; dld / tstride: row / tap stride in floats (0 = dense: cols, rows * cols)
PackItem = collections.namedtuple("PackItem", "mode I J T rows cols src sJ j0 dst_off dld tstride")
PackCase = collections.namedtuple("PackCase", "name why params items dst_len")   # params: [(I, sJ, T)]


def item(mode, I, J, T, rows=None, cols=None, src=0, sJ=None, j0=0, dst_off=64, dld=0, tstride=0):
    pr, pc = (J, I) if mode == 1 else (I, J)
    return PackItem(mode, I, J, T, rows or -(-pr // 8) * 8, cols or -(-pc // 32) * 32, src, sJ or J, j0, dst_off, dld, tstride)


def is_dense(it) -> bool:
    return it.sJ == it.J and it.j0 == 0 and it.dld == 0 and it.tstride == 0


def strides(it):
    dld = it.dld or it.cols
    return dld, it.tstride or it.rows * it.cols


def span(it) -> int:
    """floats from the item's first destination element to one past its last"""
    dld, ts = strides(it)
    return (it.T - 1) * ts + (it.rows - 1) * dld + it.cols


def _case(name, why, items, params=None, tail=64):
    items = list(items)
    if params is None:
        params = [(it.I, it.sJ, it.T) for it in items]
        items = [it._replace(src=k) for k, it in enumerate(items)]
    return PackCase(name, why, params, items, max(it.dst_off + span(it) for it in items) + tail)


def _pack_into(dst, src, it):
    dld, ts = strides(it)
    blk = np.zeros((it.T, it.rows, it.cols), dtype=np.float32)
    sub = src[:it.I, it.j0:it.j0 + it.J, :]                   # [i][j][t]
    if it.mode == 0:
        blk[:, :it.I, :it.J] = sub.transpose(2, 0, 1)         # (r, c) = (i, j)
    else:
        blk[:, :it.J, :it.I] = sub.transpose(2, 1, 0)         # (r, c) = (j, i)
    t, r, c = np.ogrid[:it.T, :it.rows, :it.cols]
    dst[it.dst_off + t * ts + r * dld + c] = blk


def pack_ref(dst_prefill, src, it):
    """The whole destination buffer (flat float32) after one item.  Modes 0 / 1 (crdr_pack_item): dst[t*tstride + r*dld + c] =
    src[i][j0 + j][t] with (i, j) = (r, c) in mode 0 and (c, r) in mode 1, zero where i >= I or j >= J, everything outside the
    T x rows x cols block unchanged.  Mode 2 (tap-major, one `tap` of rows x cols): dst[i][4 t + j] = src[i][j][t].  Mode 3 (scatter):
    dst[4 t + j][i] = src[i][j][t].  Both zero elsewhere inside rows x cols.  src: the parameter [I][sJ][T]."""
    dst = np.array(dst_prefill, dtype=np.float32, copy=True)
    src = np.asarray(src, dtype=np.float32).reshape(it.I, it.sJ, it.T)
    if it.mode in (0, 1):
        _pack_into(dst, src, it)
        return dst
    assert is_dense(it) and it.J <= 4
    blk = np.zeros((it.rows, it.cols), dtype=np.float32)
    for t in range(it.T):
        for j in range(it.J):
            if it.mode == 2:
                blk[:it.I, 4 * t + j] = src[:, j, t]
            else:
                blk[4 * t + j, :it.I] = src[:, j, t]
    dst[it.dst_off:it.dst_off + it.rows * it.cols] = blk.reshape(-1)
    return dst


def pack_ref_all(dst_prefill, srcs, items):
    dst = np.array(dst_prefill, dtype=np.float32, copy=True)
    for it in items:
        _pack_into(dst, np.asarray(srcs[it.src], dtype=np.float32).reshape(it.I, it.sJ, it.T), it)
    return dst


def pack_tiles(it) -> int:
    return (it.rows // 8) * (it.cols // 32)


def pack_predicates(it):
    """The shape side of pack_weights_batched_kernel's predicates.  `src16` / `dst16` are what the address terms of `al` come to when the
    buffers themselves are 16-byte aligned (the GPU test asserts `al` again from the real addresses); vec / novec: whether some tile takes
    the whole-run loads and whether some tile does not."""
    dld, ts = strides(it)
    p = {"sjt4": (it.sJ * it.T) % 4 == 0, "dld4": dld % 4 == 0, "ts4": ts % 4 == 0, "src16": (it.j0 * it.T) % 4 == 0, "dst16": it.dst_off % 4 == 0}
    p["al"] = all(p.values())
    firsts = range(0, it.cols, 32) if it.mode == 0 else range(0, it.rows, 8)
    whole = [p["al"] and f + (32 if it.mode == 0 else 8) <= it.J for f in firsts]
    p["vec"], p["novec"] = any(whole), not all(whole)
    return p


def pack_params(case, seed: int):
    gen = rng(seed)
    return [values(gen, p) for p in case.params]


def _side_by_side(name, why, mode, widths, I, T, j_total, dst_off, gap=0):
    """items that share one destination [T][rows][sum of cols (+ gap)] side by side, each an input-channel range of its own parameter"""
    its, col = [], 0
    cols = [-(-(I if mode else w) // 32) * 32 for w in widths]
    rows = -(-(max(widths) if mode else I) // 8) * 8
    dld = sum(cols) + gap
    for k, w in enumerate(widths):
        its.append(item(mode, I, w, T, rows, cols[k], src=k, sJ=j_total, j0=k * 5 if k else 0, dst_off=dst_off + col, dld=dld, tstride=rows * dld))
        col += cols[k]
    return _case(name, why, its, params=[(I, j_total, T)] * len(widths))


PACK_CASES = [
    # ---- dense, aligned: the 16-byte path, whole-run loads where the tile lies inside the parameter
    _case("m0_32x32_t1", "mode 0, one tile, al, vec", [item(0, 32, 32, 1)]),
    _case("m1_32x32_t1", "mode 1, al, vec in every row tile", [item(1, 32, 32, 1)]),
    _case("m0_40x64_t9", "mode 0, T = 9 (odd LDS stride 32 T + 1), two vec column tiles, 5 row tiles", [item(0, 40, 64, 9)]),
    _case("m1_40x64_t9", "mode 1, T = 9 (LDS stride 8 T + 1), I = 40 spills into a second column tile", [item(1, 40, 64, 9)]),
    _case("m0_5x33_t4", "mode 0, J = 33: first column tile vec, second not (j >= J guard of the scalar load)", [item(0, 5, 33, 4)]),
    _case("m0_31x33_t32", "mode 0, the batched limit T = 32 (the LDS image exactly full), vec then not", [item(0, 31, 33, 32)]),
    _case("m1_33x12_t9", "mode 1, J = 12: first row tile vec, second not; I = 33 -> two column tiles", [item(1, 33, 12, 9)]),
    _case("m1_70x40_t32", "mode 1, T = 32 (LDS image exactly full in mode 1: 32 (8 T + 1)), I = 70", [item(1, 70, 40, 32)]),
    _case("m0_70x70_t25", "mode 0, T = 25, J = 70 (70 * 25 % 4 != 0): scalar both sides, three column tiles", [item(0, 70, 70, 25)]),
    _case("m1_64x31_t25", "mode 1, T = 25, J = 31: 31 * 25 % 4 != 0 -> scalar", [item(1, 64, 31, 25)]),
    # ---- the scalar path by sJ * T
    _case("m0_1x3_t9", "sJ * T = 27: not al; I = 1, J = 3", [item(0, 1, 3, 9)]),
    _case("m1_1x3_t9", "the same in mode 1", [item(1, 1, 3, 9)]),
    _case("m0_3x1_t1", "J = 1, T = 1: not al, one element per source row", [item(0, 3, 1, 1)]),
    _case("m1_5x5_t25", "mode 1, I = J = 5, T = 25 (odd everything)", [item(1, 5, 5, 25)]),
    # ---- rows / cols beyond the rounding
    _case("m0_31x40_t4_big", "rows = 48 > round8(31) = 32 and cols = 96 > round32(40) = 64: zero tiles beyond I and J", [item(0, 31, 40, 4, rows=48, cols=96)]),
    _case("m1_33x5_t1_big", "mode 1, rows = 24 > 8, cols = 96 > 64", [item(1, 33, 5, 1, rows=24, cols=96)]),
    # ---- destination strides and offsets
    _case("m0_32x64_t9_dld", "dld = 100 > cols = 64 (a multiple of 4: al), tstride = rows * dld", [item(0, 32, 64, 9, dld=100, tstride=32 * 100)]),
    _case("m0_32x64_t9_dld_odd", "dld = 67: not al by dld alone", [item(0, 32, 64, 9, dld=67, tstride=32 * 67)]),
    _case("m1_32x64_t4_ts", "tstride = rows * dld + 40 > rows * dld (al)", [item(1, 32, 64, 4, tstride=64 * 32 + 40)]),
    _case("m0_32x64_t4_ts_odd", "tstride = rows * cols + 2: not al by tstride alone", [item(0, 32, 64, 4, tstride=32 * 64 + 2)]),
    _case("m1_32x64_t9_ts_odd", "mode 1, tstride = rows * cols + 3: not al by tstride alone", [item(1, 32, 64, 9, tstride=64 * 32 + 3)]),
    _case("m0_32x32_t4_dst4", "dst offset 68 floats (a multiple of 4): al", [item(0, 32, 32, 4, dst_off=68)]),
    _case("m0_32x32_t4_dst_odd", "dst offset 67 floats: not al by the dst address alone", [item(0, 32, 32, 4, dst_off=67)]),
    _case("m1_32x32_t4_dst_odd", "the same in mode 1, offset 66", [item(1, 32, 32, 4, dst_off=66)]),
    # ---- sub-blocks of a wider parameter
    _case("m0_sub_j0_aligned", "channels [32, 64) of a 96-channel parameter, T = 9: j0 * T = 288 -> src aligned, al, srcJ != J",
          [item(0, 32, 32, 9, sJ=96, j0=32)]),
    _case("m0_sub_j0_odd", "channels [3, 36) of a 40-channel parameter, T = 9: j0 * T = 27 -> not al by the src address alone",
          [item(0, 32, 33, 9, sJ=40, j0=3)]),
    _case("m1_sub_j0_aligned", "mode 1, channels [8, 20) of 32, T = 4: al, vec then not", [item(1, 33, 12, 4, sJ=32, j0=8)]),
    _case("m1_sub_j0_odd", "mode 1, channels [1, 13) of 32, T = 25: j0 * T = 25 -> scalar", [item(1, 33, 12, 25, sJ=32, j0=1)]),
    _case("m0_sub_sjt_odd", "channels [4, 36) of a 37-channel parameter, T = 9: sJ * T = 333 -> scalar although J = 32", [item(0, 8, 32, 9, sJ=37, j0=4)]),
    # ---- several items in one destination
    _side_by_side("m0_side_by_side", "three sub-blocks side by side in one [T][rows][96 + 4] buffer (dld = 100, al): neighbours' columns must survive",
                  0, [32, 17, 5], 40, 9, 64, dst_off=64, gap=4),
    _side_by_side("m1_side_by_side_odd", "mode 1, two sub-blocks side by side, dst offset 65 and dld = 66: scalar", 1, [12, 7], 33, 4, 32, dst_off=65, gap=2),
    _case("m0_stacked_rows", "the Charm's hoisted layout: three 32 x 64 T = 9 blocks stacked along the rows of one [9][96][64] pack",
          [item(0, 32, 64, 9, src=g, sJ=64 + 32 * g, dst_off=64 + g * 32 * 64, dld=64, tstride=96 * 64) for g in range(3)],
          params=[(32, 64 + 32 * g, 9) for g in range(3)]),
]
PACK_IDS = [c.name for c in PACK_CASES]
# the access path each case is there for (the `al` predicate of every item): 16-byte accesses, scalar ones, or a launch with both
PACK_PATH = {
    "m0_32x32_t1": "al", "m1_32x32_t1": "al", "m0_40x64_t9": "al", "m1_40x64_t9": "al", "m0_5x33_t4": "al", "m0_31x33_t32": "al",
    "m1_33x12_t9": "al", "m1_70x40_t32": "al", "m0_70x70_t25": "scalar", "m1_64x31_t25": "scalar", "m0_1x3_t9": "scalar", "m1_1x3_t9": "scalar",
    "m0_3x1_t1": "scalar", "m1_5x5_t25": "scalar", "m0_31x40_t4_big": "al", "m1_33x5_t1_big": "scalar", "m0_32x64_t9_dld": "al",
    "m0_32x64_t9_dld_odd": "scalar", "m1_32x64_t4_ts": "al", "m0_32x64_t4_ts_odd": "scalar", "m1_32x64_t9_ts_odd": "scalar",
    "m0_32x32_t4_dst4": "al", "m0_32x32_t4_dst_odd": "scalar", "m1_32x32_t4_dst_odd": "scalar", "m0_sub_j0_aligned": "al",
    "m0_sub_j0_odd": "scalar", "m1_sub_j0_aligned": "al", "m1_sub_j0_odd": "scalar", "m0_sub_sjt_odd": "scalar", "m0_side_by_side": "mixed",
    "m1_side_by_side_odd": "scalar", "m0_stacked_rows": "al",
}

# the cases in which ONE term of `al` is false and every other true: the term
PACK_NOT_AL_BY = {
    "m0_70x70_t25": "sjt4", "m0_1x3_t9": "sjt4", "m0_sub_sjt_odd": "sjt4", "m0_32x64_t9_dld_odd": "dld4", "m0_32x64_t4_ts_odd": "ts4",
    "m1_32x64_t9_ts_odd": "ts4", "m0_32x32_t4_dst_odd": "dst16", "m1_32x32_t4_dst_odd": "dst16", "m0_sub_j0_odd": "src16", "m1_sub_j0_odd": "src16",
}

# crdr_pack_weight modes 2 (tap-major) and 3 (scatter): (name, mode, I, J, T, rows, cols)
RGB_PACK_CASES = [
    ("tap_j3_t9", 2, 40, 3, 9, 64, 64), ("tap_j1_t25", 2, 5, 1, 25, 32, 128), ("tap_j4_t121", 2, 33, 4, 121, 40, 512), ("tap_j4_t9_min", 2, 32, 4, 9, 32, 36),
    ("scat_j3_t9", 3, 40, 3, 9, 64, 64), ("scat_j1_t25", 3, 5, 1, 25, 128, 32), ("scat_j4_t121", 3, 33, 4, 121, 512, 40), ("scat_j3_t25_min", 3, 31, 3, 25, 100, 31),
]


def many_pack_case(n: int):
    """n items in one launch: mostly one-tile T = 1 items, every 61st a larger one (tiles per item vary), two 512 x 512 T = 1 items (1024 tiles
    each) that push the total past the 2048 workgroups; every item its own parameter and its own stretch of the destination, 16 sentinel
    floats between neighbours."""
    gen = rng(1000 + n)
    its, off = [], 64
    for k in range(n):
        if k in (n // 3, n - 2):
            it = item(k & 1, 512, 512, 1, dst_off=off)
        elif k % 61 == 7:
            it = item(k & 1, int(gen.integers(9, 41)), int(gen.integers(33, 71)), (4, 9)[(k // 61) & 1], dst_off=off)
        else:
            I, J = int(gen.integers(1, 9)), int(gen.integers(1, 33))
            it = item(0, I, J, 1, dst_off=off) if k & 1 else item(1, J, I, 1, dst_off=off)
        its.append(it)
        off += span(it) + 16
    return _case(f"many_{n}", f"{n} items: n + 1 {'<=' if n + 1 <= PREFIX_CACHE else '>'} {PREFIX_CACHE}, grid-stride", its)


MANY_PACK = (1023, 1200)


# ===================================================================================================================== wgrad reduce
# slab: regular [nsplit][T][PC][QC], smallj [nsplit][PC][T][4], `off` floats into its allocation; g: [gI][gJtot][T], the job writes
# channels [j0, j0 + gJ) of it.
ReduceCase = collections.namedtuple("ReduceCase", "name why gI gJ T nsplit QC PC off gJtot j0 acc smallj")


def _red(name, why, gI, gJ, T, nsplit, QC=None, PC=None, off=0, gJtot=None, j0=0, acc=0, smallj=0):
    return ReduceCase(name, why, gI, gJ, T, nsplit, 4 if smallj else (QC or gJ), PC or gI, off, gJtot or gJ, j0, acc, smallj)


REDUCE_CASES = [
    _red("v_s1_j64_t1", "vector form, one split (n = 1: exact), one full column tile", 3, 64, 1, 1),
    _red("v_s2_j64_t9_acc", "vector, two splits: leftovers only (both into v0), accumulate", 3, 64, 9, 2, acc=1),
    _red("v_s3_j63_qc64", "vector with QC = 64 > gJ = 63: the NaN column is loaded, never emitted; three leftovers", 2, 63, 9, 3, QC=64, PC=5),
    _red("v_s4_j65_qc68", "vector, one group of four, gJ = 65 -> second tile jn = 1, QC rounded up to 4", 3, 65, 9, 4, QC=68),
    _red("v_s5_j130_qc192_t25", "vector, four + one leftover, three column tiles (jn = 2), QC rounded up to 64, T = 25 > 16 taps per pass", 2, 130, 25, 5, QC=192, PC=3, acc=1),
    _red("v_s8_j1_qc4_t32", "vector, two groups of four, gJ = 1 in QC = 4, T = 32 (LDS tile exactly full)", 5, 1, 32, 8, QC=4, PC=8),
    _red("v_s9_j64_t9_wide", "vector, two groups + one leftover, g = channels [32, 96) of a 100-channel parameter: the others stay", 3, 64, 9, 9, gJtot=100, j0=32, acc=1),
    _red("s_s1_j63", "scalar form by QC = 63, one split", 3, 63, 1, 1, PC=4),
    _red("s_s3_j65_t9", "scalar by QC = 65, jn = 1 tail tile, three leftovers", 2, 65, 9, 3, acc=1),
    _red("s_s4_j130_t9", "scalar by QC = 130, one group of four", 2, 130, 9, 4, PC=3),
    _red("s_s5_j64_off1", "scalar by the slab address alone (QC = 64, slab 1 float into its allocation), 4 + 1", 3, 64, 9, 5, off=1, acc=1),
    _red("s_s9_j64_off2_t25", "scalar by the slab address alone (8-byte aligned), 8 + 1, T = 25", 2, 64, 25, 9, off=2, PC=4),
    _red("s_s8_j1_t32", "scalar, gJ = QC = 1, T = 32, two groups of four, wide parameter (gJtot = 3, j0 = 1)", 4, 1, 32, 8, gJtot=3, j0=1, acc=1),
    _red("s_s2_j63_qc64_off1_wide", "scalar by address with QC = 64 > gJ = 63 and PC > gI, wide parameter", 3, 63, 9, 2, QC=64, PC=6, off=1, gJtot=70, j0=7),
    _red("f_t49_s3_j65", "flat path by T = 49 > 32 (7 x 7 layer), splits in order", 3, 65, 49, 3, QC=68, PC=4, acc=1),
    _red("f_t49_s5_j64_wide", "flat by T = 49, five splits (the regular order would group four), wide parameter, no accumulate", 2, 64, 49, 5, gJtot=80, j0=16),
    _red("f_t49_s1_j1", "flat by T = 49, gJ = 1, one split, a tile with 49 * 3 < 256 outputs", 3, 1, 49, 1, QC=4),
    _red("sj_j3_t25_s4", "smallj, slab rows [T][4], gJ = 3, T = 25, four splits in order", 40, 3, 25, 4, PC=64, smallj=1, acc=1),
    _red("sj_j4_t121_s5", "smallj, gJ = 4, T = 121 (11 x 11), five splits", 5, 4, 121, 5, smallj=1),
    _red("sj_j1_t25_s9_off1", "smallj, gJ = 1, nine splits, slab 1 float into its allocation, accumulate", 33, 1, 25, 9, off=1, smallj=1, acc=1),
    _red("sj_j3_t121_s2_wide", "smallj writing channels [1, 4) of a 4-channel parameter", 6, 3, 121, 2, PC=8, gJtot=4, j0=1, smallj=1),
]
REDUCE_IDS = [c.name for c in REDUCE_CASES]
# name prefix = the declared path: v vector (16-byte) form, s scalar form, f flat by T > 32, sj smallj.  Why each scalar case is scalar:
REDUCE_SCALAR_BY = {"s_s1_j63": "qc4", "s_s3_j65_t9": "qc4", "s_s4_j130_t9": "qc4", "s_s8_j1_t32": "qc4", "s_s5_j64_off1": "slab16",
                    "s_s9_j64_off2_t25": "slab16", "s_s2_j63_qc64_off1_wide": "slab16"}


def reduce_flat(c) -> bool:
    return bool(c.smallj) or c.T > REDUCE_MAX_T


def reduce_tiles(c) -> int:
    """the formula in the comment above wgrad_reduce_batched_kernel, with its T > 32 jobs on the 256-outputs side"""
    return -(-(c.gI * c.gJ * c.T) // 256) if reduce_flat(c) else c.gI * -(-c.gJ // 64)


def reduce_predicates(c):
    p = {"flat": reduce_flat(c), "smallj": bool(c.smallj), "t_le_32": c.T <= REDUCE_MAX_T, "qc4": c.QC % 4 == 0, "slab16": c.off % 4 == 0}
    p["vector"] = not p["flat"] and p["qc4"] and p["slab16"]
    return p


def slab_shape(c):
    return (c.nsplit, c.PC, c.T, 4) if c.smallj else (c.nsplit, c.T, c.PC, c.QC)


def reduce_inputs(c, seed: int):
    """-> (slab with NaN in every element the kernel must not emit, g before the call)"""
    gen = rng(seed)
    slab = np.full(slab_shape(c), np.nan, dtype=np.float32)
    if c.smallj:
        slab[:, :c.gI, :, :c.gJ] = values(gen, (c.nsplit, c.gI, c.T, c.gJ))
    else:
        slab[:, :, :c.gI, :c.gJ] = values(gen, (c.nsplit, c.T, c.gI, c.gJ))
    g = values(gen, (c.gI, c.gJtot, c.T)) if c.acc else sentinel(c.gI * c.gJtot * c.T, seed).reshape(c.gI, c.gJtot, c.T)
    return slab, g


def reduce_terms(slab, c):
    """[nsplit][gI][gJ][T]: the terms of every output the job writes, in split order"""
    s = np.asarray(slab).reshape(slab_shape(c))
    return s[:, :c.gI, :, :c.gJ].transpose(0, 1, 3, 2) if c.smallj else s[:, :, :c.gI, :c.gJ].transpose(0, 2, 3, 1)


def reduce_ref64(slab, c, g_before):
    """-> (g after in float64, gamma(n - 1) * sum |terms| per element: 0 where the job writes nothing)"""
    terms = reduce_terms(slab, c).astype(np.float64)
    g = np.asarray(g_before, dtype=np.float64).copy()
    bound = np.zeros_like(g)
    cols = slice(c.j0, c.j0 + c.gJ)
    mag = np.abs(terms).sum(0) + (np.abs(g[:, cols]) if c.acc else 0.0)
    g[:, cols] = terms.sum(0) + (g[:, cols] if c.acc else 0.0)
    bound[:, cols] = gamma(c.nsplit + c.acc - 1) * mag
    return g, bound


def reduce_ref32(slab, c, g_before):
    """float32, in the order the kernel promises.  Regular jobs: four partial sums from zero, split s joins v[s & 3] while s < 4 (nsplit // 4),
    every later split joins v0; v = (v0 + v1) + (v2 + v3).  Flat jobs (smallj or T > 32): v from zero, the splits in order.  Then d + v if
    accumulating, else v."""
    terms = reduce_terms(slab, c).astype(np.float32)
    zero = np.zeros(terms.shape[1:], dtype=np.float32)
    if reduce_flat(c):
        v = zero.copy()
        for s in range(c.nsplit):
            v = v + terms[s]
    else:
        part = [zero.copy() for _ in range(4)]
        full = 4 * (c.nsplit // 4)
        for s in range(c.nsplit):
            k = s & 3 if s < full else 0
            part[k] = part[k] + terms[s]
        v = (part[0] + part[1]) + (part[2] + part[3])
    assert v.dtype == np.float32
    g = np.array(g_before, dtype=np.float32, copy=True)
    cols = slice(c.j0, c.j0 + c.gJ)
    g[:, cols] = g[:, cols] + v if c.acc else v
    return g


def many_reduce_cases(n: int):
    """n small jobs of mixed shapes (1 to ~12 tiles each; regular vector / scalar, flat and smallj mixed): the uncached prefix search"""
    gen = rng(77)
    out = []
    for k in range(n):
        kind = k % 6
        ns, acc = int(gen.integers(1, 7)), int(gen.integers(0, 2))
        if kind == 4:
            out.append(_red(f"m{k}", "", int(gen.integers(1, 9)), int(gen.integers(1, 5)), 25, ns, smallj=1, acc=acc))
        elif kind == 5:
            out.append(_red(f"m{k}", "", 2, int(gen.integers(1, 9)), 49, ns, acc=acc))
        else:
            gJ = int(gen.integers(1, 71))
            QC = (gJ, -(-gJ // 4) * 4, -(-gJ // 64) * 64)[kind % 3]
            out.append(_red(f"m{k}", "", int(gen.integers(1, 4)), gJ, (1, 9)[k & 1], ns, QC=QC, off=(0, 1)[kind == 3], acc=acc))
    return out


BIG_REDUCE = _red("big_4096x320", "20480 tiles against 16384 workgroups: the grid-stride loop goes round twice", 4096, 320, 1, 1)


# ==================================================================================================================== colsum finish
# cs: partial rows [rows][2][ld] (pre, post), C live columns; out_pre / out_post [C] each, either may be absent
ColsumCase = collections.namedtuple("ColsumCase", "name why rows C ld pre post acc")

COLSUM_CASES = [
    ColsumCase("r1_c1", "one row, one column: lanes 1-3 and three of four pass-B lanes add nothing (n = 1: exact)", 1, 1, 1, 1, 1, 0),
    ColsumCase("r3_c63_acc", "three rows (one lane empty), C = 63 < 64, accumulate", 3, 63, 63, 1, 1, 1),
    ColsumCase("r127_c64", "one short slab, rows % 4 = 3, exactly one column tile", 127, 64, 64, 1, 1, 0),
    ColsumCase("r128_c65_ld80", "one full slab, C = 65 -> a second column tile with one live column, ld = 80 > C (NaN beyond C)", 128, 65, 80, 1, 1, 1),
    ColsumCase("r129_c200_ld256", "two slabs, the second of one row; four column tiles, ld > C", 129, 200, 256, 1, 1, 0),
    ColsumCase("r600_c200_acc", "five slabs (nslab % 4 = 1), the last of 88 rows; accumulate", 600, 200, 200, 1, 1, 1),
    ColsumCase("r600_c65_nopre", "out_pre null", 600, 65, 72, 0, 1, 1),
    ColsumCase("r129_c63_nopost", "out_post null, nslab = 2", 129, 63, 64, 1, 0, 0),
    ColsumCase("r127_c1_ld4_nopre_acc", "C = 1 in ld = 4, out_pre null, accumulate", 127, 1, 4, 0, 1, 1),
    ColsumCase("r3_c200_nopost_acc", "three rows, four column tiles, out_post null", 3, 200, 200, 1, 0, 1),
    ColsumCase("r128_c64_acc", "rows = slab, C = tile", 128, 64, 64, 1, 1, 1),
    ColsumCase("r385_c64", "four slabs (nslab % 4 = 0), the last of one row", 385, 64, 64, 1, 1, 0),
    ColsumCase("r1_c65_ld66_acc", "one row, two column tiles, ld = 66", 1, 65, 66, 1, 1, 1),
    ColsumCase("r257_c63_ld63", "three slabs, odd ld = C = 63", 257, 63, 63, 1, 1, 0),
    ColsumCase("r600_c1_nopost", "five slabs of one column", 600, 1, 1, 1, 0, 0),
    ColsumCase("r130_c129_ld130", "two slabs, three column tiles, the last of one column", 130, 129, 130, 1, 1, 1),
    ColsumCase("r700_c64_acc", "six slabs (nslab % 4 = 2)", 700, 64, 64, 1, 1, 1),
    ColsumCase("r896_c65", "seven full slabs (nslab % 4 = 3)", 896, 65, 65, 1, 1, 0),
    ColsumCase("r2_c64_nopre", "two rows", 2, 64, 64, 0, 1, 0),
    ColsumCase("r1025_c63_acc", "nine slabs: pass-B lane 0 adds three slab rows", 1025, 63, 64, 1, 1, 1),
]
COLSUM_IDS = [c.name for c in COLSUM_CASES]
MANY_COLSUM = (300, 128, 800, 4)    # jobs, C, rows, shared partial buffers


def colsum_geometry(c):
    """-> (nslab, cpad, (pass-A tiles, pass-B tiles))"""
    nslab, cpad = -(-c.rows // COLSUM_SLAB), -(-c.C // 64) * 64
    return nslab, cpad, ((cpad // 64) * nslab, cpad // 64)


def colsum_inputs(c, seed: int):
    """-> (cs [rows][2][ld] with NaN in columns C .. ld, out_pre before, out_post before)"""
    gen = rng(seed)
    cs = np.full((c.rows, 2, c.ld), np.nan, dtype=np.float32)
    cs[:, :, :c.C] = values(gen, (c.rows, 2, c.C))
    outs = [values(gen, (c.C,)) if c.acc else sentinel(c.C, seed + k) for k in range(2)]
    return cs, outs[0], outs[1]


def colsum_sums32(cs, C):
    """Pass A then pass B in float32 -> [2][C].  Pass A, per slab of 128 rows from r0: lane ty adds rows r0 + ty, r0 + ty + 4, ... in order from
    zero; the slab's row is ((l0 + l1) + l2) + l3.  Pass B: the same over the slab rows, lane ty taking slabs ty, ty + 4, ..."""
    x = np.asarray(cs, dtype=np.float32)[:, :, :C]

    def lanes4(rows):   # rows: [k][2][C]
        lane = [np.zeros((2, C), dtype=np.float32) for _ in range(4)]
        for k in range(rows.shape[0]):
            lane[k & 3] = lane[k & 3] + rows[k]
        return ((lane[0] + lane[1]) + lane[2]) + lane[3]
    slabs = np.stack([lanes4(x[r0:r0 + COLSUM_SLAB]) for r0 in range(0, x.shape[0], COLSUM_SLAB)])
    out = lanes4(slabs)
    assert out.dtype == np.float32
    return out


def _finish(s, c, pre, post, dt):
    outs = []
    for k, (have, before) in enumerate(((c.pre, pre), (c.post, post))):
        before = np.asarray(before, dtype=dt)
        outs.append(before.copy() if not have else (before + s[k] if c.acc else s[k].astype(dt)))
    return outs


def colsum_finish_ref32(cs, c, pre, post, sums=None):
    """-> (out_pre, out_post) after the flush: out + s if accumulating, else s; an absent output keeps what it held"""
    return _finish(colsum_sums32(cs, c.C) if sums is None else sums, c, pre, post, np.float32)


def colsum_finish_ref64(cs, c, pre, post):
    """-> ((out_pre, out_post) in float64, (their gamma(n - 1) * sum |terms| bounds)), n = rows (+ 1 when accumulating)"""
    x = np.asarray(cs, dtype=np.float64)[:, :, :c.C]
    outs = _finish(x.sum(0), c, pre, post, np.float64)
    g = gamma(c.rows + c.acc - 1)
    bounds = [g * (np.abs(x[:, k]).sum(0) + (np.abs(np.asarray(b, dtype=np.float64)) if c.acc else 0.0)) if have else np.zeros(c.C)
              for k, (have, b) in enumerate(((c.pre, pre), (c.post, post)))]
    return outs, bounds
