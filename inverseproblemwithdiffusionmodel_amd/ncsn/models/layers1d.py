"""1-D clones of the RefineNet blocks for the temporal prior on (B', kx*ky, T) sequences (mirror of the reference's
``ncsn/models/layers1d.py`` = layers.py with Conv1d / MaxPool1d / linear interpolation and the pair mean).  The blocks in
layers.py are dimension-generic (``ndim``); these are the ndim=1 bindings with the reference's names."""
from functools import partial

from . import layers
from .layers import get_act  # noqa: F401
from .normalization1d import InstanceNorm1dPlus, get_normalization  # noqa: F401

conv1x1 = partial(layers.conv1x1, ndim=1)
conv3x3 = partial(layers.conv3x3, ndim=1)
dilated_conv3x3 = partial(layers.dilated_conv3x3, ndim=1)
ConvMeanPool = partial(layers.ConvMeanPool, ndim=1)
CRPBlock = partial(layers.CRPBlock, ndim=1)
RCUBlock = partial(layers.RCUBlock, ndim=1)
MSFBlock = partial(layers.MSFBlock, ndim=1)
RefineBlock = partial(layers.RefineBlock, ndim=1)
ResidualBlock = partial(layers.ResidualBlock, ndim=1, normalization=InstanceNorm1dPlus)
Conv1d = partial(layers.Conv2d, ndim=1)
