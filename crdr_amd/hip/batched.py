"""Host side of the batched launches: the device job table they read and the bump arena their jobs point into.

crdr_pack_weights_batched (packs.PackTable), crdr_w4_filters_batched (packs.FilterTable), crdr_wgrad_reduce_batched (ops.DeferredWgrad)
and crdr_colsum_finish_batched (ops.ColsumQueue) take the same device operands: an item table, a prefix sum of tiles per item and a small
`meta` vector.  These keep their addresses and are rewritten only when their content changes, so a launch captured in a HIP graph replays
with no host work.  What a capture freezes is decided here and nowhere else.

JobTable
  * A table created, or changed, while the stream is capturing raises (a capture cannot upload): run eager warm-up iterations first.
  * A table used under capture is marked `replayed`: a graph launches with its addresses from then on.
  * frozen_after_capture=False (pack and filter tables): an eager upload may rewrite a replayed table in place.  Their items are
    self-contained, and the graph is meant to pick up new packs and caches at its next replay.
  * frozen_after_capture=True (weight-gradient and column-sum tables): an eager upload that would change a replayed table raises
    ("re-capture the graphs").  Their rows name slab addresses that OTHER captured launches write: the replayed reduce would read where
    nothing was written.  SiteTables keeps two such tables per flush site, one for eager and one for captured passes; while a site
    runs eagerly its captured table receives the same content, so that a later capture finds it in place.
BumpArena
  * It grows only outside capture, and a buffer that was current during any capture stays allocated for the life of the arena: the
    addresses handed out then live on in the graph's kernel arguments.
  * Any other superseded buffer is released one reset later (the launch in front of the reset that follows its replacement may read it).
"""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np
import torch

from . import lib as L


def _capturing() -> bool:   # (never before the runtime is up: the classes work on host tensors too)
    return torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _require_gpu(t: torch.Tensor):
    if not t.is_cuda:
        raise L.CrdrHipError("crdr_amd ops run on the HIP device only (got a CPU tensor); there is no CPU fallback")
    if t.dtype != torch.float32:
        raise L.CrdrHipError(f"crdr_amd ops are fp32 (got {t.dtype})")


# Host-side bookkeeping that a captured HIP graph skips on replay (trainer/graphs.py): code that runs under capture and keeps host state in
# step with what its launches do on the device -- packs.PackTable.refill bumps pack versions and stamps the filter caches its batched
# launch rebuilds -- registers a callable here; SegmentGraphs.run collects them per captured segment and calls them after every replay.
REPLAY_HOOKS = None


def on_replay(fn) -> None:
    if REPLAY_HOOKS is not None and fn not in REPLAY_HOOKS:
        REPLAY_HOOKS.append(fn)


def prefix_sums(tiles, rows: int = 1, width: int = 0):
    """int64 [rows][max(width, len(tiles) + 1)]: row r holds the running sum of every item's r-th tile count, from 0 (tiles: one int
    per item, or one tuple of `rows` ints); the columns behind the items stay zero."""
    pre = np.zeros((rows, max(width, len(tiles) + 1)), dtype=np.int64)
    pre[:, 1:len(tiles) + 1] = np.cumsum(np.asarray(tiles, dtype=np.int64).reshape(-1, rows), axis=0).T
    return pre


class JobTable:
    """Fixed-capacity device operands of one batched launch: `items` (cap x sizeof(struct) bytes), `prefix` (int64 [rows][cap + 1]) and
    `meta` (int64: the item count, then the tile total of every prefix row).  The capture rules are in the module docstring."""

    def __init__(self, device, struct, cap: int, rows: int = 1, frozen_after_capture: bool = False, name: str = "JobTable"):
        if _capturing():
            raise L.CrdrHipError(f"{name}: first use of this table happened during graph capture (run eager warm-up iterations first)")
        self.struct, self.cap, self.rows, self.frozen_after_capture, self.name = struct, cap, rows, frozen_after_capture, name
        self.items = torch.zeros(cap * C.sizeof(struct), dtype=torch.uint8, device=device)
        self.prefix = torch.zeros((rows, cap + 1), dtype=torch.int64, device=device)
        self.meta = torch.zeros(1 + rows, dtype=torch.int64, device=device)
        # the device addresses a batched kernel takes: items, one per prefix row, meta
        self.operands = (self.items.data_ptr(), *(self.prefix[r].data_ptr() for r in range(rows)), self.meta.data_ptr())
        self.replayed = False
        self._host = b""   # item bytes + trailer of the last upload (the zeroed operands are those of an empty table)

    def upload(self, items, tiles, trailer: bytes = b"") -> "JobTable":
        """Make the table hold `items` (ctypes structs) and return it; copies to the device only when their bytes differ from what it
        holds.  tiles(item) -> the item's tile count (a tuple of them for a table with several prefix rows), asked only
        when the table is rewritten.  `trailer` takes part in the comparison only: state beside the items that a captured launch
        depends on as well (ColsumQueue's scratch address)."""
        cap = _capturing()
        raw = b"".join(bytes(i) for i in items)
        host = raw + trailer
        if host != self._host:
            if cap:
                raise L.CrdrHipError(f"{self.name}: the table changed during graph capture (run eager warm-up iterations first)")
            if self.replayed and self.frozen_after_capture:
                raise L.CrdrHipError(f"{self.name}: an eager pass would rewrite a job table that a captured HIP graph replays "
                                     "(shapes or buffer addresses changed since the capture): re-capture the graphs")
            n = len(raw) // C.sizeof(self.struct)
            if n > self.cap:
                raise L.CrdrHipError(f"{self.name}: {n} items, the device table holds {self.cap}")
            pre = prefix_sums([tiles(i) for i in items], self.rows, self.cap + 1)
            if n:
                self.items[:len(raw)].copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))
            self.prefix.copy_(torch.from_numpy(pre))
            self.meta.copy_(torch.tensor([n] + [int(t) for t in pre[:, n]], dtype=torch.int64))
            self._host = host
        if cap:
            self.replayed = True
        return self


class SiteTables:
    """The frozen_after_capture JobTables of one batched launch, two per flush site: (site, False) eager passes, (site, True) captured ones."""

    def __init__(self, device, struct, cap: int, rows: int = 1, name: str = "JobTable"):
        self.tables = collections.defaultdict(lambda: JobTable(device, struct, cap, rows, True, name))

    def upload(self, site, items, tiles, trailer: bytes = b"") -> JobTable:
        cap = _capturing()
        if not cap:   # the twin that a later capture of this site finds in place
            self.tables[(site, True)].upload(items, tiles, trailer)
        return self.tables[(site, cap)].upload(items, tiles, trailer)


class BumpArena:
    """Bump allocator of device memory that a queue recycles at every flush, so that a flush site sees the same addresses in every
    iteration and its job tables never change.  The capture rules are in the module docstring."""

    def __init__(self, device, nbytes: int, name: str = "BumpArena"):
        self.device, self.name = device, name
        self.tensor = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.off = self.cycle = 0   # cycle: bytes handed out since the last reset (over all buffers)
        self._captured = False   # the current buffer was used during a capture
        self._pinned = []     # superseded buffers whose addresses are baked into captured graphs: never released
        self._late = []       # superseded since the last reset: the launch in front of the next reset may read them
        self._keep = []       # superseded before the last reset: released at the next one

    def _grow(self, nbytes: int) -> None:
        if _capturing():
            raise L.CrdrHipError(f"{self.name} too small during graph capture (run eager warm-up iterations first)")
        (self._pinned if self._captured else self._late).append(self.tensor)
        self.tensor = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.off, self._captured = 0, False

    def alloc(self, nbytes: int) -> int:
        """-> the address of `nbytes` (rounded up to 256) that stay valid until the launch in front of the next reset has run"""
        nbytes = (nbytes + 255) // 256 * 256
        if self.off + nbytes > self.tensor.numel():
            self._grow(max(2 * self.tensor.numel(), 2 * (self.cycle + nbytes)))   # fits a whole cycle like this one: the next one never grows
        self._captured = self._captured or _capturing()
        p = self.tensor.data_ptr() + self.off
        self.off, self.cycle = self.off + nbytes, self.cycle + nbytes
        return p

    def reserve(self, nbytes: int) -> int:
        """For offset-addressed use (the caller counts the offsets itself): -> the address of a buffer of at least `nbytes`"""
        if nbytes > self.tensor.numel():
            self._grow(2 * nbytes)
        self._captured = self._captured or _capturing()
        return self.tensor.data_ptr()

    def rewind(self) -> None:
        """Forget what was handed out (nothing was launched on it, or the caller has seen to it)."""
        self.off = self.cycle = 0

    def reset(self) -> None:
        """The launch that consumes this cycle's allocations has been issued: hand out the same addresses again."""
        cycle = self.cycle
        self.rewind()
        if not _capturing():
            if self.tensor.numel() < cycle:   # the cycle spilled over several buffers: make the next one fit in one
                self._grow(2 * cycle)
            self._keep, self._late = self._late, []
