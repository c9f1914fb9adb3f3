"""The hyperprior-only model (src/models/comp_model/hyperprior_model.py:21-264): transforms + hyper-prior, the latent
coded with the mean and scale the hyper-decoder predicts, no context model.  It is the Charm model with the Charm
replaced by `HyperpriorContext`, an adapter that answers the four calls HyperpriorCharmModel makes to its context
model with ONE fused Gaussian-conditional launch over the whole latent; run / rate / codec / validation plumbing is
inherited.  The state dict is the Charm sibling's minus every `context_model.*` key."""
from __future__ import annotations

from typing import Dict, Tuple

import torch
from torch import Tensor

from crdr_amd.hip import functional as HF
from crdr_amd.models.subnet import build_subnet
from crdr_amd.models.subnet.context_model.base_context_model import ContextRuntime
from crdr_amd.utils.registry import MODEL_REGISTRY

from .hyperprior_charm_model import HyperpriorCharmModel


class HyperpriorContext(ContextRuntime):
    """`context_model` of the hyperprior-only models: no parameters, no state-dict keys, not a registered subnet (and not an
    nn.Module: it does not show up among the model's children).  mean | scale are the two channel halves of the hyper-decoder's
    output, read in place as strided views."""
    record_symbols = None   # parity tests set a list: it receives round(y - mu), one entry

    @staticmethod
    def _halves(hyper_out: Tensor) -> Tuple[Tensor, Tensor]:
        assert hyper_out.shape[1] % 2 == 0
        return torch.chunk(hyper_out, 2, dim=1)

    def _record(self, y: Tensor, mu: Tensor) -> None:
        if self.record_symbols is not None:
            self.record_symbols.append(torch.round(y.detach() - mu.detach()))

    def __call__(self, *args, **kw):
        return self.forward(*args, **kw)

    def forward(self, y: Tensor, hyper_out: Tensor, entropy_model_y, is_train: bool, calc_q_likelihood: bool = True,
                noise: Tensor = None, want_lik: bool = True, bits_out: Dict = None):
        """-> (y_hat, y_likelihood, y_q_likelihood), the contract of Minnen20CharmContextModel.forward: the per-image bit sums go
        out through `bits_out["y"], bits_out["y_q"]` and only they carry the rate gradient (the likelihood tensors are
        non-differentiable outputs of the fused node).  Training noise: the given tensor, else in-kernel Philox."""
        mu, sigma = self._halves(hyper_out)
        philox = self._philox(y.device) if (is_train and noise is None) else None
        yh, bn, bq, lik_n, lik_q = HF.gauss_cond(y, mu, sigma, noise if is_train else None, entropy_model_y.scale_bound,
                                                 entropy_model_y.likelihood_bound, want_lik, philox_state=philox)
        self._record(y, mu)
        if bits_out is not None:
            bits_out["y"], bits_out["y_q"] = (bn if is_train else bq), bq
        if not want_lik:
            return (yh, None, None) if calc_q_likelihood else (yh, None)
        lik = lik_n if is_train else lik_q
        return (yh, lik, lik_q) if calc_q_likelihood else (yh, lik)

    @torch.no_grad()
    def reconstruct_latent(self, y: Tensor, h_mu: Tensor, entropy_model_y) -> Tensor:
        """round(y - mu) + mu only (no likelihood, no bit sums): the same kernel on the same operands as forward(), with the mean
        standing in for the scale it does not need -- bit-identical to forward()'s y_hat."""
        yh = HF.gauss_cond(y, h_mu, h_mu, None, entropy_model_y.scale_bound, entropy_model_y.likelihood_bound, False)[0]
        self._record(y, h_mu)
        return yh

    @torch.no_grad()
    def forward_compress_device(self, y: Tensor, hyper_out: Tensor, entropy_model_y):
        """-> (symbols, indexes, y_hat, likelihood) on the device: the eval likelihoods plus ONE launch for the int32 symbols and
        CDF indexes in coder order; nothing synchronises."""
        mu, sigma = self._halves(hyper_out)
        yh, _, _, _, lik_q = HF.gauss_cond(y, mu, sigma, None, entropy_model_y.scale_bound, entropy_model_y.likelihood_bound, True)
        sym, idx = entropy_model_y.symbols_and_indexes(y, mu, sigma)
        return sym, idx, yh, lik_q

    @torch.no_grad()
    def forward_decompress(self, y_str: bytes, hyper_out: Tensor, entropy_model_y) -> Tuple[Tensor, Tensor]:
        """Decoder side: the CDF indexes of the whole latent in one launch, ONE pinned round trip through the host rANS decoder,
        then y_hat = symbols + mean in NHWC.  -> (y_hat, symbols)"""
        from crdr_amd.codec import rans
        from crdr_amd.hip import ops
        cdf, sizes, offs = entropy_model_y.host_tables()
        mu, sigma = self._halves(hyper_out)
        n, c, h, w = mu.shape
        t = self._tick(None)
        _, idx = entropy_model_y.symbols_and_indexes(None, None, sigma)
        cnt = idx.numel()
        pin_idx, pin_sym = self._pinned_pair(idx.shape)
        hi, hs = pin_idx[:cnt], pin_sym[:cnt]
        hi.copy_(idx.view(-1), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        ev.synchronize()
        t = self._tick("charm", t)
        dec = rans.RansDecoder()
        dec.set_stream(y_str)
        dec.decode_stream_into(hi.numpy(), cdf, sizes, offs, hs.numpy())
        sym = torch.empty((n, c, h, w), dtype=torch.int32, device=mu.device)
        sym.view(-1).copy_(hs, non_blocking=True)
        y_hat = ops.empty_nhwc(n, c, h, w, mu.device)
        y_hat.copy_(entropy_model_y.dequantize(sym, mu))
        ev.record()       # the pinned symbol buffer is reused by this thread's next image: its upload must have been consumed by then
        ev.synchronize()
        self._tick("rans", t)
        return y_hat, sym


@MODEL_REGISTRY.register()
class HyperpriorModel(HyperpriorCharmModel):
    staged_backward = False   # data parallel: one all-reduce of the flat gradient (there is no context-model piece to overlap)

    def _build_subnets(self):
        sn = self.opt.subnet
        self.encoder = build_subnet(sn.encoder, "encoder")
        self.decoder = build_subnet(sn.decoder, "decoder")
        self.hyperencoder = build_subnet(sn.hyperencoder, "hyperencoder")
        self.hyperdecoder = build_subnet(sn.hyperdecoder, "hyperdecoder")
        self.entropy_model_z = build_subnet(sn.entropy_model_z, "entropy_model")
        self.entropy_model_y = build_subnet(sn.entropy_model_y, "entropy_model")
        self.context_model = HyperpriorContext()
        self.return_likelihoods = bool(self.opt.get("return_likelihoods", False))
