"""InstanceNorm++ over one axis (mirror of the reference's ``ncsn/models/normalization1d.py:151-186``): parameters ``alpha``,
``gamma``, ``beta``; the per-(sequence, channel) statistics run over L, through the same coefficient kernel as the 2-D form
(ops.instnorm_plus_coef takes any trailing extent).  The conditional 1-D normalisations are not built."""
from .normalization import InstanceNorm2dPlus


class InstanceNorm1dPlus(InstanceNorm2dPlus):
    pass


def get_normalization(config, conditional=True):
    norm = config.model.normalization
    if conditional:
        raise NotImplementedError("conditional 1-D normalisations: no gfx950 kernel (the NCSN1D family is unconditional)")
    if norm == "InstanceNorm++":
        return InstanceNorm1dPlus
    raise NotImplementedError(f"{norm}: only InstanceNorm++ (every shipped config) has a gfx950 kernel")
