"""Fused execution of the channel-autoregressive ("Charm") context model on the HIP conv kernels.

Reference: src/models/subnet/context_model/minnen20_charm_context_model.py:88-141 (forward), :143-240 (codec).  For
slice i the mean / scale / LRP transforms are conv5(->C1)-ReLU-conv5(->C2)-ReLU-conv3(->slice_ch) over
[hyper-prior half, first min(i, ms) decoded slices(, y_hat_i)].  The reference runs 90 small convs in a 10-deep chain
with concatenations in between; here the same arithmetic is re-scheduled:

 * HOIST.  The first conv of every transform is linear in its input channels, so each part of it is computed by the
   launch that has that part of the input.  The hyper-prior part (320 of 320..512 input channels = 72 % of the first-layer
   MACs, 56 % of the whole context model) does not depend on any decoded slice: it is computed for all transforms up front by
   two wide convs (320 -> 19 x 224 from the mean half, 320 -> 9 x 224 from the scale half; slice 0's own transforms have
   no other input and run directly).  The SUPPORT part is scattered the same way (round 3): as soon as slice k is decoded,
   ONE wide conv per half (32 -> 2 (S-1-k) x 224 and 32 -> (S-1-k) x 224, CRDR_EPI_ACCUM) adds its contribution to the
   first-layer pre-activation of EVERY later transform -- 2 x ms efficient launches with N in the thousands instead of a
   small conv per transform and stage whose K grows with the slice index.  A pre-activation that has received all its parts
   is finished by crdr_bias_relu_slots (bias + ReLU in place); the LRP transforms get their last part -- the slice's own
   pre-correction latent -- from a small conv that carries bias + ReLU in its epilogue (CRDR_EPI_PREADD).
 * TAIL.  From slice ms on the support stops growing (`y_hat_slice_list[:5]`, :104-105): the mean / scale transforms of
   ALL remaining slices are independent of each other and run as grouped launches (crdr_conv2d_grouped), then one
   Gaussian-conditional launch over all tail channels, then the LRP transforms as one group.  The sequential depth drops
   from 10 slices to ms + 1.
 * NO CONCATENATION.  Every activation lives in a wide NHWC buffer and is addressed by (channel offset, pixel stride):
   A1 / A2 hold the first / second layer outputs of all 30 transforms ("slots"), MSL holds mu | sigma | lrp, Yh / Ypre
   the decoded latent after / before the LRP correction.
 * BACKWARD is written out by hand in reverse schedule order (no autograd graph inside): ReLU masks ride in the
   input-gradient convs' epilogues (CRDR_EPI_RELUMASK); the gradient of decoded slice k collects the first-layer gradients
   of all its consumers through ONE K-concatenated input-gradient conv per half (CRDR_EPI_ACCUM into dY) and their weight
   gradients through ONE slab launch per half whose rows the batched reduce scatters to the parameters
   (crdr_wgrad_job.gJtot) -- the same two launches per half serve the hoisted hyper-prior parts -- and all bias gradients
   come from three column-sum passes over the wide gradient buffers (crdr_colsum_scatter).

Slot order (A1, A2 and their gradients): [mean_S-1, lrp_S-1, mean_S-2, lrp_S-2, ..., mean_1, lrp_1, lrp_0] (reads the mean
half) [scale_S-1 ... scale_1] (reads the scale half) [mean_0, scale_0]: descending slice index, so the consumers of decoded
slice k -- every transform of a later slice -- are a PREFIX of each half.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple

import torch

from . import functional as HF
from . import lib as L
from . import ops
from . import packs
from .ops import V


def _chunks(n: int, size: int = L.MAX_GROUP):
    return [(a, min(a + size, n)) for a in range(0, n, size)]


class CharmPlan:
    """Static schedule + persistent weight packs of one Minnen20CharmContextModel instance on one device."""

    def __init__(self, module):
        self.S = module.num_slices
        self.sc = module.slice_ch
        ms = module.max_support_slices
        self.ms = self.S if ms < 0 else ms
        if self.S - self.ms < 2:          # a one-slice tail is just another sequential slice
            self.ms = self.S
        S, ms = self.S, self.ms
        T = S - ms
        self.T = T
        self.tr = {"mean": module.mean_slice_transforms, "scale": module.scale_slice_transforms, "lrp": module.lrp_slice_transforms}
        w1 = self.conv("mean", 0, 0).weight
        self.C1, self.hm = w1.shape[0], w1.shape[1]
        self.C2 = self.conv("mean", 0, 1).weight.shape[0]
        self.k1, self.k2, self.k3 = (tuple(self.conv("mean", 0, l).weight.shape[2:]) for l in range(3))
        assert self.C1 % 32 == 0 and self.C2 % 32 == 0 and self.sc % 32 == 0 and self.hm % 32 == 0, \
            "the fused Charm engine needs channel counts that are multiples of 32"
        self.device = w1.device
        # ---- slots
        order: List[Tuple[str, int]] = []
        for j in range(S - 1, 0, -1):
            order += [("mean", j), ("lrp", j)]
        order += [("lrp", 0)]
        self.n_mu = len(order)
        order += [("scale", j) for j in range(S - 1, 0, -1)]
        self.n_sc = len(order) - self.n_mu
        order += [("mean", 0), ("scale", 0)]
        self.order = order
        self.slot = {t: k for k, t in enumerate(order)}
        self.NT = len(order)
        self.signature = self._signature()
        self._packs = {}
        self._tables = None

    # ---- parameters
    def conv(self, kind: str, i: int, layer: int):
        return getattr(self.tr[kind][i].model, ("0", "2", "4")[layer])

    def params(self):
        for kind in ("mean", "scale", "lrp"):
            for i in range(self.S):
                for l in range(3):
                    c = self.conv(kind, i, l)
                    yield c.weight
                    yield c.bias

    def _signature(self):
        return tuple(p.data_ptr() for p in self.params())

    def sup(self, i: int) -> int:
        """support channels of slice i"""
        return self.sc * min(i, self.ms)

    def ncons(self, k: int) -> int:
        """later slices whose transforms read decoded slice k (0 for k >= ms: not a support slice)"""
        return self.S - 1 - k if k < self.ms else 0

    def consumers(self, k: int, half: str):
        """(first slot, [(kind, j)...]) of the transforms that read slice k through the `half` ("mu" / "sc") of A1: a prefix"""
        nc = self.ncons(k)
        lo, cnt = (0, 2 * nc) if half == "mu" else (self.n_mu, nc)
        return lo, self.order[lo:lo + cnt]

    def halves(self):
        """(pack key, first slot, slot count) of the two hoisted hyper-prior convs"""
        return ("hyp_mu", 0, self.n_mu), ("hyp_sc", self.n_mu, self.n_sc)

    # ---- packs
    def pack_layout(self):
        """Every weight pack of the engine, once and in table order: (key, taps, blocks).  A block is (conv weight [I][J'][kh][kw], j0, j1):
        input channels [j0, j1) of that conv; the blocks of a pack are N-concatenated in list order, so in forward orientation the pack
        is [taps][len(blocks) * I][J = j1 - j0]."""
        hm, sc = self.hm, self.sc
        w = lambda kind, i, layer: self.conv(kind, i, layer).weight
        t1, t2, t3 = (k[0] * k[1] for k in (self.k1, self.k2, self.k3))
        for name, lo, n in self.halves():   # the hoisted hyper-prior parts, in slot order
            yield name, t1, [(w(kind, i, 0), 0, hm) for kind, i in self.order[lo:lo + n]]
        for k in range(self.ms):            # the support parts: decoded slice k -> every later transform, in slot order
            for half in ("mu", "sc"):
                _, cons = self.consumers(k, half)
                if cons:
                    yield ("sup_" + half, k), t1, [(w(kind, j, 0), hm + k * sc, hm + (k + 1) * sc) for kind, j in cons]
        for kind in ("mean", "scale", "lrp"):
            for i in range(self.S):
                if i == 0 and kind != "lrp":      # slice 0: the whole first conv directly
                    yield (kind, 0, "l1"), t1, [(w(kind, 0, 0), 0, hm)]
                if kind == "lrp":                 # the slice's own pre-correction latent: the last part of its first conv
                    j0 = hm + self.sup(i)
                    yield (kind, i, "own"), t1, [(w(kind, i, 0), j0, j0 + sc)]
                yield (kind, i, "l2"), t2, [(w(kind, i, 1), 0, self.C1)]
                yield (kind, i, "l3"), t3, [(w(kind, i, 2), 0, self.C2)]

    def _build_packs(self, transposed: bool):
        """-> ({key: address}, entries to keep fresh, buffers).  transposed False: the forward operands [t][n * I][J]; True: the
        input-gradient operands [t][J][n * I] (the blocks K-concatenated)."""
        addr, ents, keep = {}, [], []
        for key, taps, blocks in self.pack_layout():
            n, I, J = len(blocks), blocks[0][0].shape[0], blocks[0][2] - blocks[0][1]
            buf = torch.empty((taps, J, n * I) if transposed else (taps, n * I, J), dtype=torch.float32, device=self.device)
            addr[key] = buf.data_ptr()
            keep.append(buf)
            for blk, (w, j0, j1) in enumerate(blocks):
                ents.append(packs.sub_pack(w, j0, j1, buf, blk * I * (1 if transposed else J), J if transposed else I, I if transposed else J,
                                           transposed, dld=buf.shape[2], tstride=buf.shape[1] * buf.shape[2]))
        return addr, ents, keep

    def _cached_packs(self, transposed: bool):
        if transposed not in self._packs:     # lazy per direction: an inference process never builds the input-gradient packs
            self._packs[transposed] = self._build_packs(transposed)
        return self._packs[transposed]

    def fwd_packs(self):
        """Forward operands: (packs[key] = address, entries to keep fresh, buffers)."""
        return self._cached_packs(False)

    def bwd_packs(self):
        """Input-gradient operands ([tap][in][out]), same keys."""
        return self._cached_packs(True)

    def bias_tables(self):
        """Device pointer tables for crdr_colsum_scatter: L1 / L2 biases in slot order, L3 biases in MSL order."""
        g = HF.grad_slot
        sig = (tuple(g(self.conv(k, i, 0).bias).data_ptr() for (k, i) in self.order),
               tuple(g(self.conv(k, i, 1).bias).data_ptr() for (k, i) in self.order),
               tuple(g(self.conv(k, i, 2).bias).data_ptr() for k in ("mean", "scale", "lrp") for i in range(self.S)))
        if self._tables is None or self._tables[3] != sig:  # (the flat gradient buffers never move: built once in training)
            if torch.cuda.is_current_stream_capturing():
                raise L.CrdrHipError("Charm: bias gradient slots moved during graph capture")
            mk = lambda t: torch.tensor(t, dtype=torch.int64, device=self.device)
            self._tables = (mk(sig[0]), mk(sig[1]), mk(sig[2]), sig)
        return self._tables[:3]


def plan_for(module) -> CharmPlan:
    p = getattr(module, "_charm_plan", None)
    if p is None or p.signature != p._signature():
        if p is not None and torch.cuda.is_current_stream_capturing():
            raise L.CrdrHipError("Charm: the parameters moved during graph capture")
        p = CharmPlan(module)
        object.__setattr__(module, "_charm_plan", p)
    return p


class CharmRun:
    """One pass over a batch: owns the wide buffers; `forward()` runs the whole schedule, the stage methods let the
    decoder interleave the host entropy coder."""

    def __init__(self, plan: CharmPlan, hyper_mu: torch.Tensor, hyper_sc: Optional[torch.Tensor], scale_bound: float, lik_bound: float):
        """hyper_mu / hyper_sc: the two halves of the hyper-decoder output (channel slices of one tensor are fine);
        hyper_sc = None: reconstruction only (no scale transforms, no likelihoods).  The two bounds are the Gaussian conditional's."""
        self.p = plan
        self.scale_bound, self.lik_bound = float(scale_bound), float(lik_bound)
        hyper_mu, ldm = ops.nhwc(hyper_mu)
        n, c, h, w = hyper_mu.shape
        assert c == plan.hm
        self.n, self.h, self.w = n, h, w
        self.M = n * h * w
        self.dev = hyper_mu.device
        self.h_mu = V(hyper_mu.data_ptr(), ldm, plan.hm)
        self.with_scale = hyper_sc is not None
        self.h_sc = None
        if hyper_sc is not None:
            hyper_sc, lds = ops.nhwc(hyper_sc)
            assert lds == ldm, "both hyper-prior halves must share one pixel stride"
            self.h_sc = V(hyper_sc.data_ptr(), lds, plan.hm)
        self._hyper = (hyper_mu, hyper_sc)
        P = plan
        self.Cy = P.S * P.sc
        self.A1, self.A2 = self.wide(P.NT * P.C1), self.wide(P.NT * P.C2)
        self.MSL = self.wide(3 * self.Cy)
        self.Yh, self.Ypre = self.wide(self.Cy), self.wide(self.Cy)
        self.addr, ents, _ = P.fwd_packs()
        packs.ensure_fresh(ents)

    def wide(self, c: int) -> torch.Tensor:
        return torch.empty((self.M, c), dtype=torch.float32, device=self.dev)

    # ---- views: one rule per buffer family; `of` = the backward's gradient buffer of the same layout instead
    def a1(self, slot, n=1, of=None):
        """first-layer slots [slot, slot + n)"""
        return ops.view(self.A1 if of is None else of, slot * self.p.C1, n * self.p.C1)

    def a2(self, slot, n=1, of=None):
        """second-layer slots [slot, slot + n)"""
        return ops.view(self.A2 if of is None else of, slot * self.p.C2, n * self.p.C2)

    def msl(self, which: int, i: int, n=1, of=None):
        """slices [i, i + n) of plane `which` of MSL (mu | sigma | lrp) -- or of G4 (d mu | d sigma | d lrp | dy)"""
        return ops.view(self.MSL if of is None else of, which * self.Cy + i * self.p.sc, n * self.p.sc)

    def lat(self, buf: torch.Tensor, st):
        """the slices of stage `st` (consecutive) of a latent-shaped buffer: Yh, Ypre, their gradient"""
        return ops.view(buf, st[0] * self.p.sc, len(st) * self.p.sc)

    def yh(self, *st):
        return self.lat(self.Yh, st)

    def yp(self, *st):
        return self.lat(self.Ypre, st)

    def bias(self, kind, i, layer):
        return self.p.conv(kind, i, layer).bias.data_ptr()

    def _conv(self, xs, ws, ys, oc, k, *, wrows, wcols, biases=None, pres=None, relu=False, label="", ms=False, accum=False):
        """ms: a launch over mean (+ scale) transforms.  The mean-only pass (with_scale False) runs it with the plan the full
        pass uses for twice the problems, so that mu -- hence y_hat -- comes out bit-identical in both."""
        mult = 2 if (ms and not self.with_scale) else 1
        for a, b in _chunks(len(xs), L.MAX_GROUP // mult):
            ops.conv_group(self.n, self.h, self.w, xs[a:b], ws[a:b], ys[a:b], oc, k, k[0] // 2, False, wrows=wrows, wcols=wcols,
                           biases=None if biases is None else biases[a:b], pres=None if pres is None else pres[a:b],
                           flags=(L.EPI_RELU if relu else 0) | (L.EPI_ACCUM if accum else 0), device=self.dev, label=label,
                           plan_as=mult * (b - a) if mult > 1 else None)

    # ---- stages
    def stages(self):
        P = self.p
        st = [(i,) for i in range(P.ms)]
        if P.T:
            st.append(tuple(range(P.ms, P.S)))
        return st

    def hoist(self):
        P = self.p
        for (name, lo, n), x in zip(P.halves(), (self.h_mu, self.h_sc)):
            if x is not None:
                self._conv([x], [self.addr[name]], [self.a1(lo, n)], n * P.C1, P.k1, wrows=n * P.C1, wcols=P.hm, label="charm.hoist")

    def _l23(self, trs, outs, label, ms=False):
        """second and third layer of the transforms `trs` -> outs (V into MSL)"""
        P = self.p
        sl = [P.slot[t] for t in trs]
        self._conv([self.a1(s) for s in sl], [self.addr[(k, i, "l2")] for k, i in trs], [self.a2(s) for s in sl], P.C2, P.k2,
                   wrows=P.C2, wcols=P.C1, biases=[self.bias(k, i, 1) for k, i in trs], relu=True, label=label + ".l2", ms=ms)
        self._conv([self.a2(s) for s in sl], [self.addr[(k, i, "l3")] for k, i in trs], outs, P.sc, P.k3,
                   wrows=P.sc, wcols=P.C2, biases=[self.bias(k, i, 2) for k, i in trs], label=label + ".l3", ms=ms)

    def finish(self, trs):
        """bias + ReLU in place on the first-layer pre-activations of `trs`, which have received all their parts"""
        P = self.p
        lib = L.load()
        for a, b in _chunks(len(trs)):
            c0 = (C.c_int32 * (b - a))(*[P.slot[t] * P.C1 for t in trs[a:b]])
            bs = (C.c_void_p * (b - a))(*[self.bias(k, i, 0) for k, i in trs[a:b]])
            L.check(lib.crdr_bias_relu_slots(self.A1.data_ptr(), self.A1.shape[1], self.M, P.C1, b - a, c0, bs, ops._stream()), "bias_relu_slots")

    def mean_scale(self, st):
        """mu (and sigma) of the slices of stage `st` -> MSL"""
        P = self.p
        kinds = ("mean", "scale") if self.with_scale else ("mean",)
        trs = [(k, i) for k in kinds for i in st]
        sl = [P.slot[t] for t in trs]
        if st[0] == 0:
            xs = [self.h_mu, self.h_sc][: len(kinds)]
            self._conv(xs, [self.addr[(k, 0, "l1")] for k in kinds], [self.a1(s) for s in sl], P.C1, P.k1, wrows=P.C1, wcols=P.hm,
                       biases=[self.bias(k, 0, 0) for k in kinds], relu=True, label="charm.ms.l1", ms=True)
        else:       # hoisted hyper-prior part + one part per support slice are in: finish
            self.finish(trs)
        outs = [self.msl(0 if k == "mean" else 1, i) for k, i in trs]
        self._l23(trs, outs, "charm.ms", ms=True)

    def push_support(self, k: int):
        """decoded slice k (final: after its LRP correction) -> the first-layer pre-activations of every later transform"""
        P = self.p
        if not P.ncons(k):
            return
        for half in (("mu", "sc") if self.with_scale else ("mu",)):
            lo, cons = P.consumers(k, half)
            n = len(cons)
            self._conv([self.yh(k)], [self.addr[("sup_" + half, k)]], [self.a1(lo, n)], n * P.C1, P.k1, wrows=n * P.C1, wcols=P.sc, accum=True,
                       label="charm.sup")

    def gauss_operands(self, st, philox, bwd: Optional["CharmBackward"] = None):
        """The GcDesc2 / GcIO pair of the Gaussian conditional over the channels of stage `st`.  Both directions read y, mu, sigma and the
        noise source; the forward adds its outputs, the backward (`bwd` given) the gradients it reads and writes."""
        P, Cy, i0 = self.p, self.Cy, st[0]
        c0 = i0 * P.sc
        y, noise = self.yv, self.nv
        d = L.GcDesc2(N=self.n, HW=self.h * self.w, C=len(st) * P.sc, ldy=y.ld, ldmu=self.MSL.shape[1], ldsigma=self.MSL.shape[1],
                      ldnoise=noise.ld if noise is not None else 0, Ctot=Cy, c0=c0, scale_bound=self.scale_bound,
                      likelihood_bound=self.lik_bound)
        io = L.GcIO(y=y.ptr + 4 * c0, mu=self.msl(0, i0).ptr, sigma=self.msl(1 if self.with_scale else 0, i0).ptr,
                    noise=None if noise is None else noise.ptr + 4 * c0, philox=philox)
        if bwd is None:
            d.ldyhat = d.ldyhat2 = d.ldlik = Cy
            io.yhat, io.yhat2 = self.yh(*st).ptr, self.yp(*st).ptr
            io.lik_noisy, io.lik_quant = (None if t is None else t.data_ptr() + 4 * c0 for t in (self.lik_n, self.lik_q))
            io.bits_noisy, io.bits_quant = ops._p(self.bits_n), ops._p(self.bits_q)
        else:   # (G4 carries dy next to d mu | d sigma | d lrp so that the three gradients share one pixel stride)
            d.ldgrad, d.lddyhat = bwd.G4.shape[1], Cy
            io.gbits, io.dyhat = bwd.gbits.data_ptr(), bwd.dyv(*st).ptr
            io.dmu, io.dsigma, io.dy = (bwd.g4(which, i0).ptr for which in (0, 1, 3))
        return d, io

    def quantize(self, st, philox):
        """Gaussian conditional over the channels of stage `st`: Yh = Ypre = round(y - mu) + mu, likelihoods, bit sums."""
        d, io = self.gauss_operands(st, philox)
        HF.gauss_cond_fwd2(d, io, self.dev)

    def lrp(self, st):
        """LRP transforms of stage `st` on the pre-correction latent in Yh, then Yh = Ypre + 0.5 tanh(.); a sequential stage then
        scatters its finished slice to the later transforms"""
        P = self.p
        lt = [("lrp", i) for i in st]
        sl = [self.a1(P.slot[t]) for t in lt]
        self._conv([self.yh(i) for i in st], [self.addr[("lrp", i, "own")] for i in st], sl, P.C1, P.k1,
                   wrows=P.C1, wcols=P.sc, biases=[self.bias("lrp", i, 0) for i in st], pres=sl, relu=True, label="charm.lrp.l1")
        self._l23(lt, [self.msl(2, i) for i in st], "charm.lrp")
        L.check(L.load().crdr_lrp(self.yp(*st).ptr, self.Cy, self.msl(2, st[0]).ptr, self.MSL.shape[1], self.yh(*st).ptr, self.Cy,
                                  self.M, len(st) * P.sc, ops._stream()), "lrp")
        if len(st) == 1:
            self.push_support(st[0])

    # ---- whole pass
    def forward(self, y: torch.Tensor, noise: Optional[torch.Tensor], philox: Optional[int], want_lik: bool, want_bits: bool):
        y, ldy = ops.nhwc(y)
        self.y = y
        self.yv = V(y.data_ptr(), ldy, self.Cy)
        self.nv = None
        if noise is not None:
            noise, ldn = ops.nhwc(noise)
            self.noise = noise
            self.nv = V(noise.data_ptr(), ldn, self.Cy)
        noisy = noise is not None or philox is not None
        self.lik_n = self.wide(self.Cy) if (want_lik and noisy) else None
        self.lik_q = self.wide(self.Cy) if want_lik else None
        self.bits_n = torch.zeros(self.n, dtype=torch.float32, device=self.dev) if (want_bits and noisy) else None
        self.bits_q = torch.zeros(self.n, dtype=torch.float32, device=self.dev) if want_bits else None
        self.hoist()
        for st in self.stages():
            self.mean_scale(st)
            self.quantize(st, philox)
            self.lrp(st)

    def as_nchw(self, buf: torch.Tensor, c0: int = 0, c: Optional[int] = None) -> torch.Tensor:
        c = buf.shape[1] - c0 if c is None else c
        return buf.view(self.n, self.h, self.w, buf.shape[1]).permute(0, 3, 1, 2)[:, c0:c0 + c]


# ---------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------
class CharmBackward:
    """The backward of one CharmRun, step by step: every stage method of the forward has its `_bwd` here and `run()` calls them in reverse
    schedule order.  Owns the gradients of the wide buffers -- dA1 / dA2 (slots), G4 = d mu | d sigma | d lrp | dy, dY (d Yh, which
    d Ypre shares: Yh = Ypre + ... is an identity path), dH (both hyper-prior halves); parameter gradients go straight into the (flat)
    .grad slots."""

    def __init__(self, run: CharmRun, dyhat: Optional[torch.Tensor], gbits: Optional[torch.Tensor], philox: Optional[int]):
        self.r, self.p, self.philox = run, run.p, philox
        P = run.p
        self.baddr, bents, _ = P.bwd_packs()
        packs.ensure_fresh(bents)
        self.dA1, self.dA2 = run.wide(P.NT * P.C1), run.wide(P.NT * P.C2)
        self.G4 = run.wide(4 * run.Cy)
        self.dY = run.wide(run.Cy)
        self.dH = run.wide(2 * P.hm)
        if dyhat is None:
            self.dY.zero_()
        else:
            run.as_nchw(self.dY).copy_(dyhat)
        if gbits is None:
            gbits = torch.zeros(run.n, dtype=torch.float32, device=run.dev)
        self.gbits = gbits.contiguous()

    # ---- views: the forward's, over the gradient buffers
    def da1(self, slot, n=1):
        return self.r.a1(slot, n, of=self.dA1)

    def da2(self, slot, n=1):
        return self.r.a2(slot, n, of=self.dA2)

    def g4(self, which, i, n=1):
        return self.r.msl(which, i, n, of=self.G4)

    def dyv(self, *st):
        return self.r.lat(self.dY, st)

    def dh(self, half: int):
        return ops.view(self.dH, half * self.p.hm, self.p.hm)

    def wg(self, kind, i, layer):
        return HF.grad_slot(self.p.conv(kind, i, layer).weight)

    # ---- launches
    def dgrad(self, xs, ws, ys, oc, k, wrows, wcols, masks=None, accum=False, label=""):
        r = self.r
        for a, b in _chunks(len(xs)):
            ops.conv_group(r.n, r.h, r.w, xs[a:b], ws[a:b], ys[a:b], oc, k, k[0] // 2, True, wrows=wrows, wcols=wcols,
                           masks=None if masks is None else masks[a:b], flags=L.EPI_ACCUM if accum else 0, device=r.dev, label=label)

    def wgrad(self, ps, qs, gs, gi, gj, k, label=""):
        r = self.r
        for a, b in _chunks(len(ps)):
            ops.wgrad_group(r.n, r.h, r.w, ps[a:b], qs[a:b], gs[a:b], gi, gj, k, k[0] // 2, device=r.dev, label=label)

    def l32_bwd(self, trs, douts, label):
        """third + second layer backward of transforms `trs` given the gradients of their outputs (V into G4):
        leaves dz1 (masked) in dA1 slots, queues the weight gradients"""
        P, r = self.p, self.r
        sl = [P.slot[t] for t in trs]
        d1, d2 = [self.da1(s) for s in sl], [self.da2(s) for s in sl]
        a1, a2 = [r.a1(s) for s in sl], [r.a2(s) for s in sl]
        self.dgrad(douts, [self.baddr[(k, i, "l3")] for k, i in trs], d2, P.C2, P.k3, P.C2, P.sc, masks=a2, label=label + ".l3")
        self.wgrad(douts, a2, [(self.wg(k, i, 2).data_ptr(), 0) for k, i in trs], P.sc, P.C2, P.k3, label=label + ".l3")
        self.dgrad(d2, [self.baddr[(k, i, "l2")] for k, i in trs], d1, P.C1, P.k2, P.C1, P.C2, masks=a1, label=label + ".l2")
        self.wgrad(d2, a1, [(self.wg(k, i, 1).data_ptr(), 0) for k, i in trs], P.C2, P.C1, P.k2, label=label + ".l2")

    def wide_l1_bwd(self, pack, lo, trs, x: V, dx: V, j0: int, label):
        """Backward of ONE wide first-layer conv: input x = input channels [j0, j0 + x.c) of the transforms `trs`, which are the slots
        [lo, lo + len(trs)); their (masked) first-layer gradients are final.  ONE K-concatenated input-gradient conv adds them to dx,
        ONE slab launch yields the weight gradients (rows scattered to the parameters' columns by the batched reduce)."""
        P, r = self.p, self.r
        g = self.da1(lo, len(trs))
        self.dgrad([g], [self.baddr[pack]], [dx], dx.c, P.k1, dx.c, g.c, accum=True, label=label)
        gws = [self.wg(kind, i, 0) for kind, i in trs]
        parts = [(idx * P.C1, P.C1, gw.data_ptr() + 4 * j0 * P.k1[0] * P.k1[1], gw.shape[1]) for idx, gw in enumerate(gws)]
        ops.wgrad_split(r.n, r.h, r.w, g, x, parts, P.k1, P.k1[0] // 2, device=r.dev, label=label)

    # ---- the forward's stages, backwards
    def support_bwd(self, k: int):
        """push_support: decoded slice k fed the first layer of every later transform"""
        P = self.p
        if not P.ncons(k):
            return
        for half in ("mu", "sc"):
            lo, cons = P.consumers(k, half)
            self.wide_l1_bwd(("sup_" + half, k), lo, cons, self.r.yh(k), self.dyv(k), P.hm + k * P.sc, "charm.sup")

    def lrp_bwd(self, st):
        P, r = self.p, self.r
        if len(st) == 1:
            self.support_bwd(st[0])
        # Yh = Ypre + 0.5 tanh(lrp): d lrp
        L.check(L.load().crdr_lrp_bwd(self.dyv(*st).ptr, r.Cy, r.msl(2, st[0]).ptr, r.MSL.shape[1], self.g4(2, st[0]).ptr, self.G4.shape[1],
                                      r.M, len(st) * P.sc, ops._stream()), "lrp_bwd")
        lt = [("lrp", i) for i in st]
        self.l32_bwd(lt, [self.g4(2, i) for i in st], "charm.lrp")
        # the slice's own pre-correction latent: d Ypre_i on top of d Yh_i
        d1 = [self.da1(P.slot[t]) for t in lt]
        self.dgrad(d1, [self.baddr[("lrp", i, "own")] for i in st], [self.dyv(i) for i in st], P.sc, P.k1, P.sc, P.C1, accum=True,
                   label="charm.lrp.l1own")
        t1 = P.k1[0] * P.k1[1]
        gws = [self.wg("lrp", i, 0) for i in st]
        self.wgrad(d1, [r.yp(i) for i in st], [(gw.data_ptr() + 4 * (P.hm + P.sup(i)) * t1, gw.shape[1]) for i, gw in zip(st, gws)],
                   P.C1, P.sc, P.k1, label="charm.lrp.l1own")

    def gauss_bwd(self, st):
        d, io = self.r.gauss_operands(st, self.philox, bwd=self)
        L.check(L.load().crdr_gauss_cond_bwd2(C.byref(d), C.byref(io), ops._stream()), "gauss_cond_bwd2")

    def mean_scale_bwd(self, st):
        P, r = self.p, self.r
        trs = [(k, i) for k in ("mean", "scale") for i in st]
        self.l32_bwd(trs, [self.g4(0 if k == "mean" else 1, i) for k, i in trs], "charm.ms")
        if st[0] == 0:
            d1 = [self.da1(P.slot[t]) for t in trs]
            self.dgrad(d1, [self.baddr[(k, 0, "l1")] for k, _ in trs], [self.dh(0), self.dh(1)], P.hm, P.k1, P.hm, P.C1, label="charm.ms.l1")
            self.wgrad(d1, [r.h_mu, r.h_sc], [(self.wg(k, 0, 0).data_ptr(), 0) for k, _ in trs], P.C1, P.hm, P.k1, label="charm.ms.l1")

    def hoist_bwd(self):
        P, r = self.p, self.r
        for half, ((name, lo, n), x) in enumerate(zip(P.halves(), (r.h_mu, r.h_sc))):
            self.wide_l1_bwd(name, lo, P.order[lo:lo + n], x, self.dh(half), 0, "charm.hoist")

    def bias_grads(self):
        """three column-sum passes over the wide gradient buffers"""
        P, r = self.p, self.r
        tb1, tb2, tb3 = P.bias_tables()
        ops.colsum_scatter(ops.view(self.dA1, 0, self.dA1.shape[1]), r.M, P.C1, tb1, r.dev)
        ops.colsum_scatter(ops.view(self.dA2, 0, self.dA2.shape[1]), r.M, P.C2, tb2, r.dev)
        ops.colsum_scatter(ops.view(self.G4, 0, 3 * r.Cy), r.M, P.sc, tb3, r.dev)

    def run(self):
        """-> (dy, dhyper) as NCHW views"""
        r = self.r
        with ops.local_wgrad_defer(r.dev, ("charm-local", r.dev.index)):
            for st in reversed(r.stages()):
                self.lrp_bwd(st)
                self.gauss_bwd(st)
                self.mean_scale_bwd(st)
            self.hoist_bwd()
            self.bias_grads()
        r._keep_bwd = (self.dA1, self.dA2, self.G4, self.dY, self.dH)
        return r.as_nchw(self.G4, 3 * r.Cy), r.as_nchw(self.dH)


def charm_backward(run: CharmRun, dyhat: Optional[torch.Tensor], gbits: Optional[torch.Tensor], philox: Optional[int]):
    """-> (dy, dhyper) as NCHW views; parameter gradients are accumulated straight into the (flat) .grad slots."""
    return CharmBackward(run, dyhat, gbits, philox).run()


class _CharmFn(torch.autograd.Function):
    """(y, hyper_out[, noise]) -> (y_hat, bits_noisy[N], bits_quant[N], lik_noisy?, lik_quant?, mu, sigma)"""

    @staticmethod
    def forward(ctx, y, hyper_out, noise, module, philox_state, scale_bound, lik_bound, want_lik, is_train):
        plan = plan_for(module)
        h_mu, h_sc = torch.chunk(hyper_out, 2, dim=1)
        run = CharmRun(plan, h_mu, h_sc, scale_bound, lik_bound)
        ph = None
        if is_train and noise is None:
            ph_call = torch.empty(2, dtype=torch.int64, device=y.device)
            inc = (y.numel() + 3) // 4 + 1
            L.check(L.load().crdr_philox_fork(philox_state.data_ptr(), ph_call.data_ptr(), inc, ops._stream()), "philox_fork")
            ph = ph_call.data_ptr()
            ctx.ph_call = ph_call
        run.forward(y, noise if is_train else None, ph, want_lik, True)
        ctx.run, ctx.ph = run, ph
        if ops.RELU_MASK_SINK is not None and any(ctx.needs_input_grad):   # (test hook: the activations charm_backward takes its ReLU masks from)
            for (kind, i), slot in plan.slot.items():
                ops.RELU_MASK_SINK(plan.conv(kind, i, 0).weight, run.as_nchw(run.A1, slot * plan.C1, plan.C1), None)
                ops.RELU_MASK_SINK(plan.conv(kind, i, 1).weight, run.as_nchw(run.A2, slot * plan.C2, plan.C2), None)
        yhat = run.as_nchw(run.Yh)
        mu, sigma = run.as_nchw(run.MSL, 0, run.Cy), run.as_nchw(run.MSL, run.Cy, run.Cy)
        lik_n = run.as_nchw(run.lik_n) if run.lik_n is not None else None
        lik_q = run.as_nchw(run.lik_q) if run.lik_q is not None else None
        ctx.mark_non_differentiable(run.bits_q, mu, sigma)
        for t in (lik_n, lik_q):
            if t is not None:
                ctx.mark_non_differentiable(t)
        return yhat, run.bits_n, run.bits_q, lik_n, lik_q, mu, sigma

    @staticmethod
    def backward(ctx, dyhat, dbits_n, *_):
        run = ctx.run
        if run.bits_n is None:
            raise L.CrdrHipError("Charm: backward needs the noisy (training) forward")
        dy, dh = charm_backward(run, dyhat, dbits_n, ctx.ph)
        ctx.run = None
        return dy, dh, None, None, None, None, None, None, None


def charm_forward(module, y, hyper_out, noise, philox_state, scale_bound, lik_bound, want_lik, is_train):
    return _CharmFn.apply(y, hyper_out, noise, module, philox_state, float(scale_bound), float(lik_bound), bool(want_lik),
                          bool(is_train))


@torch.no_grad()
def charm_reconstruct(module, y, hyper_mu, scale_bound, lik_bound) -> CharmRun:
    """y_hat only (the no-grad high-rate pass of stage 3): no scale transforms, no likelihoods.  Returns the run (y_hat =
    run.as_nchw(run.Yh))."""
    run = CharmRun(plan_for(module), hyper_mu, None, scale_bound, lik_bound)
    run.forward(y, None, None, False, False)
    return run
