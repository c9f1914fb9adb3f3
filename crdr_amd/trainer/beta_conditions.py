"""The per-batch draw of (rate index q, realism weight beta) that the beta-conditioned trainers share (reference: one draw per batch,
interpca_hyperprior_model.py:43-45 and beta_cond_interpca_hyperprior_model.py:41-46).  q selects the captured graph; beta enters
through device buffers (the decoder's static embedding, the loss weight `_beta_t`), so one graph serves every beta."""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from . import dist as D


class BetaConditions:
    """Mixin of a trainer whose comp_model is beta-conditioned and multi-rate.  Call `_init_conditions(opt)` once the model exists."""

    def _init_conditions(self, opt) -> None:
        self.rate_level = self.comp_model.rate_level
        seed = int(opt.get("cond_seed", 0))
        self._q_gen = torch.Generator().manual_seed(seed)   # data parallel: every rank draws the same (q, beta)
        self._b_rng = np.random.default_rng(seed)
        self._beta_t = None

    def _conditions(self, data_dict: Dict):
        """-> ({"rate_ind": q (int), "beta": beta}, graph key)"""
        q = data_dict.get("rate_ind")
        if q is None:
            q = torch.randint(self.rate_level, (1,), generator=self._q_gen) if D.is_dist() else self.comp_model.sample_rate_ind()
        q = int(q.item()) if isinstance(q, torch.Tensor) else int(q)
        beta = data_dict.get("beta")
        if beta is None:
            beta = (self.comp_model.max_beta * (float(self._b_rng.integers(0, 101)) / 100.0)) if D.is_dist() else self.comp_model.sample_beta()
        beta = float(beta)
        dec = self.comp_model.decoder
        if getattr(dec, "static_embed", None) is None or self._beta_t is None:
            dec.static_embed = torch.zeros(1, dec.embed.embed(0.0).shape[1], 1, 1, device=self.device)
            self._beta_t = torch.zeros(1, device=self.device)
        dec.static_embed.copy_(dec.embed.embed(beta).reshape(dec.static_embed.shape))
        self._beta_t.fill_(beta)
        return {"rate_ind": q, "beta": beta}, ("s3", q)
