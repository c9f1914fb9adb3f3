"""Weight packs and what is derived from them: the pack registry, the pack entries with their batched refill (PackTable), and the
transformed filters of the F(4x4) Winograd kernel kept per launch shape (filter caches, FilterTable).  How these are stored is known here only.
"""
# One policy: a launch may skip its filter transform iff its cache was derived from what its weight packs hold NOW.
#   * Every persistent pack buffer has a registry record with a version counter, and every writer of a pack bumps it (_PackEntry.fill,
#     PackTable.refill and its replay hook; a foreign writer calls bump_version).  A cache is stamped with the versions it was built from; a
#     launch whose cache carries other stamps re-transforms into the same tensor (crdr_conv2d_grouped_ex, filter_cache_valid = 0).
#   * Only registered packs are cached by address: buffers that live as long as their layer and are refilled in place.  A temporary pack's
#     address says nothing about its content.
#   * Under graph capture nothing new is cached (a tensor born inside a capture belongs to that graph's pool): a launch whose cache does not
#     exist yet transforms into the workspace; the warm-up iterations in front of every capture create the caches.
#   * The packs of an optimiser are refilled by ONE launch behind its update (PackTable.refill), and every cache derived from them is rebuilt
#     by ONE more (FilterTable.refill) and stamped current: inside a training step no convolution launch transforms anything.  A graph
#     replay runs both launches without this code, so the refill leaves a hook (batched.on_replay) that redoes its host bookkeeping.
from __future__ import annotations

import collections
import ctypes as C
import os
import weakref
from typing import Optional

import torch

from . import lib as L
from .batched import JobTable, _capturing, _require_gpu, _stream, on_replay


# ---------------------------------------------------------------------------------------------------------------- the pack registry
class _PackRecord:
    """One pack buffer address: the tensor registered there last (weakly) and how often the buffer was (re)written.  Records are never
    deleted: the version outlives the tensor, so a cache stamped from a dead pack can never look current to a new one at its address."""
    __slots__ = ("ptr", "ref", "version")

    def __init__(self, ptr: int):
        self.ptr, self.ref, self.version = ptr, None, 0   # (ref None: written to, never registered)

    def alive(self) -> bool:
        """the registered tensor still lives at this address (a dead pack's address may be handed to a new, differently shaped tensor)"""
        t = self.ref() if self.ref is not None else None
        return t is not None and t.data_ptr() == self.ptr


_records = {}   # data_ptr -> _PackRecord


def _record(ptr: int) -> _PackRecord:
    r = _records.get(ptr)
    if r is None:
        r = _records[ptr] = _PackRecord(ptr)
    return r


def register(t: torch.Tensor) -> None:
    """`t` is a persistent pack buffer.  Another tensor at a known address voids whatever was derived from the old content."""
    r = _record(t.data_ptr())
    if r.ref is None:
        r.ref = weakref.ref(t)
    elif r.ref() is not t:   # (also the address of a pack that died)
        r.version += 1
        _drop_filter_caches(lambda e: r in e.packs)
        r.ref = weakref.ref(t)


def bump_version(ptr: int) -> None:
    """The pack buffer at `ptr` is being rewritten in place: whatever was derived from its previous content is stale from here on."""
    _record(ptr).version += 1


def version(ptr: int) -> int:
    return _records[ptr].version if ptr in _records else 0


def is_persistent(ptr: int) -> bool:
    return ptr in _records and _records[ptr].alive()


# ------------------------------------------------------------------------------------------------------------ the weight-pack entries
_weights_epoch = 0
PACK_MISS_LOG = {} if os.environ.get("CRDR_DEBUG_PACK") == "1" else None  # {(I, J, T, mode, why): count}
_pack_entries = []   # every pack ever made, in creation order and never removed (PackTable selects the ones of one optimiser)


def bump_weights_epoch() -> None:
    """Invalidate every weight pack (parameters were modified behind torch's back by something other than an optimiser
    that owns a PackTable -- the fused Adam refills its packs itself, see PackTable)."""
    global _weights_epoch
    _weights_epoch += 1


def _current_key(w: torch.Tensor):
    return (w.data_ptr(), w._version, _weights_epoch)


class _PackEntry:
    """One persistent weight pack: destination buffer + how to refill it from its parameter.  A *sub-block* entry
    (`src_off` / `srcJ` / `dst_off` / `dld` / `tstride`, see crdr_pack_item) packs an input-channel range of the parameter
    into a row / column range of a wider pack shared with other parameters (the Charm's hoisted first-layer convs)."""
    __slots__ = ("weight", "dst", "I", "J", "T", "rows", "cols", "mode", "key", "src_off", "srcJ", "dst_off", "dld", "tstride")

    def __init__(self, weight: torch.Tensor, dst: torch.Tensor, mode: int, rows: int, cols: int, j_range=None, dst_off: int = 0,
                 dld: int = 0, tstride: int = 0):
        """Create and register the entry.  j_range = (j0, j1): the sub-block of those input channels, `dst_off` floats into `dst`."""
        _require_gpu(weight)
        assert weight.is_contiguous()
        self.key = None
        self.weight, self.dst, self.mode, self.rows, self.cols = weight.detach(), dst, mode, rows, cols
        self.I, self.J, self.T = weight.shape[0], weight.shape[1], weight.shape[2] * weight.shape[3] if weight.dim() == 4 else 1
        self.src_off = self.srcJ = 0
        if j_range is not None:
            self.J, self.src_off, self.srcJ = j_range[1] - j_range[0], 4 * j_range[0] * self.T, weight.shape[1]
        self.dst_off, self.dld, self.tstride = 4 * dst_off, dld, tstride
        register(dst)
        _pack_entries.append(self)

    def item(self) -> "L.PackItem":
        return L.PackItem(src=self.weight.data_ptr() + self.src_off, dst=self.dst.data_ptr() + self.dst_off, I=self.I, J=self.J,
                          T=self.T, rows=self.rows, cols=self.cols, mode=self.mode, srcJ=self.srcJ, dld=self.dld,
                          tstride=self.tstride)

    def _launch(self) -> None:
        if self.mode in (0, 1):
            L.check(L.load().crdr_pack_weight_item(C.byref(self.item()), _stream()), "pack_weight_item")
        else:
            L.check(L.load().crdr_pack_weight(self.weight.data_ptr(), self.dst.data_ptr(), self.I, self.J, self.T, self.rows, self.cols,
                                                self.mode, _stream()), "pack_weight")

    def fill(self) -> None:
        register(self.dst)
        bump_version(self.dst.data_ptr())
        self._launch()


def sub_pack(weight: torch.Tensor, j0: int, j1: int, dst: torch.Tensor, dst_off: int, rows: int, cols: int, transposed: bool,
             dld: int = 0, tstride: int = 0) -> _PackEntry:
    """Register a sub-block pack: input channels [j0, j1) of `weight` [I][J][kh][kw] -> the [T][rows][cols] block that
    starts `dst_off` floats into `dst` (row stride `dld`, tap stride `tstride`; 0 = dense).  transposed=False: pack row =
    output channel i, column = input channel j (forward operand); True: row = j, column = i (input-gradient operand)."""
    assert weight.dim() == 4
    I, J = weight.shape[0], j1 - j0
    assert rows % 8 == 0 and cols % 32 == 0 and rows >= (J if transposed else I) and cols >= (I if transposed else J)
    return _PackEntry(weight, dst, 1 if transposed else 0, rows, cols, (j0, j1), dst_off, dld, tstride)


def ensure_fresh(entries, log: bool = False) -> None:
    """Refill the entries whose parameter changed since their last fill (first use, load_state_dict, a foreign optimiser);
    the fused Adam keeps them fresh through its PackTable.  log: count the refills in PACK_MISS_LOG."""
    for e in entries:
        k = _current_key(e.weight)
        if e.key != k:
            if log and PACK_MISS_LOG is not None:
                why = "new" if e.key is None else "ptr" if e.key[0] != k[0] else "version" if e.key[1] != k[1] else "epoch"
                m = (e.I, e.J, e.T, e.mode, why)
                PACK_MISS_LOG[m] = PACK_MISS_LOG.get(m, 0) + 1
            e.fill()
            e.key = k


class PackTable:
    """The packs whose parameter lives in one address range (an optimiser's flat buffer, or a partition of it), refilled
    by ONE launch right after that optimiser's update -- instead of one small launch per layer on next use.

    Its batched.JobTable is rewritten in place when new packs appear, also under a graph that replays it
    (frozen_after_capture=False, see batched): the captured launch keeps covering everything."""
    CAP = 4096

    def __init__(self, flat: torch.Tensor, lo: int = 0, hi: Optional[int] = None):
        hi = flat.numel() if hi is None else hi
        self.lo, self.hi = flat.data_ptr() + 4 * lo, flat.data_ptr() + 4 * hi
        self.device = flat.device
        self.table = JobTable(flat.device, L.PackItem, self.CAP, name="PackTable")
        self.entries, self.singles = [], []
        self.filters = FilterTable(self.device)
        self._seen = -1

    def _refresh(self) -> None:
        if self._seen == len(_pack_entries):
            return
        mine = [e for e in _pack_entries if self.lo <= e.weight.data_ptr() < self.hi and e.dst.device == self.device]
        ents = [e for e in mine if e.mode in (0, 1) and e.T <= 32]   # what the batched kernel takes
        self.table.upload([e.item() for e in ents], lambda it: (it.rows // 8) * (it.cols // 32))
        self.entries, self.singles = ents, [e for e in mine if not (e.mode in (0, 1) and e.T <= 32)]
        self._seen = len(_pack_entries)

    def _rewritten(self, filters_follow) -> None:
        """The packs were rewritten on the device, by refill()'s launches or by their replay: FilterTable.refill / .replayed follows."""
        ptrs = {e.dst.data_ptr() for e in self.entries + self.singles}
        for ptr in ptrs:
            bump_version(ptr)
        filters_follow(ptrs)

    def refill(self) -> None:
        """Refill every pack of the range from the current parameter values and mark them fresh."""
        self._refresh()
        if self.entries:
            L.check(L.load().crdr_pack_weights_batched(*self.table.operands, _stream()), "pack_weights_batched")
        for e in self.singles:
            e._launch()
        for e in self.entries + self.singles:
            e.key = _current_key(e.weight)
        # ... and, behind the packs, every transformed-filter cache of the F(4x4) kernel derived from them: one launch
        self._rewritten(self.filters.refill)
        if _capturing():
            on_replay(self._replayed)   # (trainer/graphs.py: a replay runs these launches without this method)

    def _replayed(self) -> None:
        """The graph that captured refill() has just been replayed: refill()'s host-side bookkeeping without its launches.  The packs and the
        filter caches in the device tables AS THE REPLAYED LAUNCHES SAW THEM are fresh; packs / caches that appeared since (an eager
        validation pass at another image size, say) join the tables now and are covered from the next replay on -- until then their own
        staleness checks (pack keys, version stamps) make their launches refill / re-transform."""
        self._rewritten(self.filters.replayed)
        self._refresh()


# ------------------------------------------------------------------------------------------------------------------ the filter caches
FILTER_STATS = {"filled": 0, "reused": 0, "batched": 0}   # launches that transformed / trusted their cache; caches rebuilt by FilterTable
FILTER_CACHE_BUDGET = int(os.environ.get("CRDR_FILTER_CACHE_GB", "24")) << 30   # bytes of transformed filters kept (least recently used go first)
_filter_cache = {}    # FilterKey -> _FilterCache
_filter_serial = 0    # bumped when the set of caches changes (FilterTable re-reads it)
_filter_tick = 0      # launch counter: a cache's `tick` is that of its last launch

FilterKey = collections.namedtuple("FilterKey", "packs G algo N H W C OH OW OC kh kw stride pad transposed wrows wcols")


def filter_key(d, ios, G: int) -> FilterKey:
    """What a cache's content depends on, beside the content of the packs: their addresses and the launch geometry."""
    # (the key leaves the K-split bits of the algorithm id out on purpose: the block layout of the transformed filters does not depend
    # on the split count -- wino4_filter_bytes / wino4_filter_thread take no nsplit)
    return FilterKey(tuple(int(ios[g].w) for g in range(G)), G, d.reserved & 0xFF, d.N, d.H, d.W, d.C, d.OH, d.OW, d.OC, d.kh, d.kw,
                     d.stride, d.pad, d.transposed, d.wrows, d.wcols)


class _FilterCache:
    # u: the tensor of transformed filters (nbytes); packs: the registry records of the launch's weight packs; versions: those the content
    # was derived from (None: not filled yet); item: its row of the batched rebuild; tick: see _filter_tick
    __slots__ = ("u", "packs", "versions", "item", "nbytes", "tick")

    def alive(self) -> bool:
        """every pack this cache was derived from still lives at its address: a cache must never be rebuilt from whatever lives there now"""
        return all(p.alive() for p in self.packs)

    def current_versions(self) -> tuple:
        return tuple(p.version for p in self.packs)


def filter_cache_bytes() -> int:
    return sum(e.nbytes for e in _filter_cache.values())


def _drop_filter_caches(gone) -> None:
    global _filter_serial
    keys = [k for k, e in _filter_cache.items() if gone(e)]
    for k in keys:
        del _filter_cache[k]
    _filter_serial += bool(keys)


def drop_filter_caches(ptr=None) -> None:
    """Drop the filter caches derived from the pack at `ptr` (all of them: None).  Not needed for correctness -- the version stamps decide --
    but it frees the memory of caches whose pack is gone."""
    _drop_filter_caches(lambda e: ptr is None or any(p.ptr == ptr for p in e.packs))


def _evict_filter_caches(need: int) -> None:
    """Make room for `need` more bytes within FILTER_CACHE_BUDGET: the least recently launched caches go first (never under graph capture).
    A FilterTable drops an evicted cache at its next refresh and the tensor is freed then, also where a captured launch holds its address."""
    total, victims = filter_cache_bytes() + need, []
    for e in sorted(_filter_cache.values(), key=lambda e: e.tick):
        if total <= FILTER_CACHE_BUDGET:
            break
        total -= e.nbytes
        victims.append(e)
    _drop_filter_caches(lambda e: e in victims)


def cacheable(ios, G: int) -> bool:
    """An F(4x4) launch on these weight operands keeps its filters: every one of them is a registered, living pack."""
    return all(is_persistent(int(ios[g].w)) for g in range(G))


def filter_cache_for(d, ios, G: int, device):
    """For the F(4x4) launch of G problems that d and ios describe: -> (its cache, whether the content is derived from what the packs hold
    now), or None if the launch keeps no cache.  Creates the cache on first use, and evicts for it -- never while capturing."""
    global _filter_serial, _filter_tick
    if not cacheable(ios, G):
        return None
    key = filter_key(d, ios, G)
    ent = _filter_cache.get(key)   # (alive: its packs are the records just asked, and a new tensor at a known address drops its caches)
    if ent is None:
        lib = L.load()
        nb = 0 if _capturing() else int(lib.crdr_conv2d_filter_cache_bytes(C.byref(d), G))
        if not nb:
            return None
        _evict_filter_caches(nb)
        ent = _filter_cache[key] = _FilterCache()
        ent.u = torch.empty(nb // 4, dtype=torch.float32, device=device)
        ent.packs, ent.versions, ent.nbytes, ent.tick = tuple(_records[p] for p in key.packs), None, nb, 0
        ent.item = L.W4FilterItem()
        L.check(lib.crdr_conv2d_filter_item(C.byref(d), G, C.byref(ent.item)), "conv2d_filter_item")
        for g in range(G):
            ent.item.w[g] = key.packs[g]
        ent.item.u = ent.u.data_ptr()
        _filter_serial += 1
    _filter_tick += 1
    ent.tick = _filter_tick
    now = ent.current_versions()
    valid = ent.versions == now   # derived from the packs' CURRENT content, not merely from the same addresses
    ent.versions = now
    FILTER_STATS["reused" if valid else "filled"] += 1
    return ent, valid


class FilterTable:
    """The filter caches derived from a set of weight packs (an optimiser's), rebuilt by one launch.  Its batched.JobTable is rewritten in place
    when new caches appear, also under a graph that replays it (frozen_after_capture=False): the captured launch keeps covering everything."""
    CAP = 1024

    def __init__(self, device):
        self.device = device
        self.table = JobTable(device, L.W4FilterItem, self.CAP, name="FilterTable")
        self.entries = []
        self._seen = -1
        self._packs = frozenset()

    def _refresh(self, pack_ptrs) -> None:
        pack_ptrs = frozenset(pack_ptrs)
        if self._seen == _filter_serial and pack_ptrs == self._packs:
            return
        if not _capturing():
            _drop_filter_caches(lambda e: not e.alive())
        ents = [e for e in _filter_cache.values() if e.u.device == self.device and e.alive() and all(p.ptr in pack_ptrs for p in e.packs)]
        if len(ents) > self.CAP:   # more caches than the device table holds: the most recently used stay in the batched rebuild, the others
            ents = sorted(ents, key=lambda e: -e.tick)[:self.CAP]   # fall behind their packs' versions and re-transform inside their launches
            ents.sort(key=lambda e: e.tick)
        self.table.upload([e.item for e in ents], lambda it: int(it.units))
        self.entries = ents
        self._seen, self._packs = _filter_serial, pack_ptrs

    def refill(self, pack_ptrs) -> None:
        """Rebuild every cache derived from `pack_ptrs` (just refilled) and stamp it with the packs' current versions."""
        self._refresh(pack_ptrs)
        if self.entries:
            L.check(L.load().crdr_w4_filters_batched(*self.table.operands, _stream()), "w4_filters_batched")
            FILTER_STATS["batched"] += len(self.entries)
            for e in self.entries:
                e.versions = e.current_versions()

    def replayed(self, pack_ptrs) -> None:
        """A captured graph holding this table's rebuild launch has just been replayed (the packs' versions were bumped by the caller): the
        caches in the table AS THE LAUNCH SAW IT are current; caches that appeared since join the table now, are rebuilt from the next replay
        on, and until then stay behind their packs' versions (their launches re-transform)."""
        for e in self.entries:
            e.versions = e.current_versions()
        self._refresh(pack_ptrs)
