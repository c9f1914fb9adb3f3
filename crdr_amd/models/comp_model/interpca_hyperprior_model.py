"""Variable-rate hyperprior-only model (src/models/comp_model/interpca_hyperprior_model.py:19-224): the rate index
conditions the transforms through InterpChAtt; the latent is coded as in HyperpriorModel.  Rate-index handling, the
multi-rate header and the `_{q+1}` validation columns are the Charm sibling's."""
from __future__ import annotations

from crdr_amd.utils.registry import MODEL_REGISTRY

from .hyperprior_model import HyperpriorModel
from .interpca_hyperprior_charm_model import InterpCaHyperpriorCharmModel


@MODEL_REGISTRY.register()
class InterpCaHyperpriorModel(HyperpriorModel, InterpCaHyperpriorCharmModel):
    pass
