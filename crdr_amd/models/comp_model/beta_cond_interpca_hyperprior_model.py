"""Hyperprior-only model with the rate index q and the realism weight beta as run-time knobs
(src/models/comp_model/beta_cond_interpca_hyperprior_model.py:18-208): `max_beta` / `sample_beta`, the beta-conditioned
decoder call and the validation conditions are the Charm sibling's; the latent is coded as in HyperpriorModel."""
from __future__ import annotations

from crdr_amd.utils.registry import MODEL_REGISTRY

from .beta_cond_interpca_hyperprior_charm_model import BetaCondInterpCaHyperpriorCharmModel
from .hyperprior_model import HyperpriorModel


@MODEL_REGISTRY.register()
class BetaCondInterpCaHyperpriorModel(HyperpriorModel, BetaCondInterpCaHyperpriorCharmModel):
    pass
