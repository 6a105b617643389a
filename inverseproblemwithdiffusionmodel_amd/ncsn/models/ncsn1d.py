"""Temporal score networks on (B', kx*ky, T) sequences (mirror of the reference's ``ncsn/models/ncsn1d.py``: NCSN1D :40-130, the
"Diffusion1D" of helpers/load_model.py:25; NCSN1DDeeper :133-224; NCSN1DDeepest :227-328).  Same constructor (``Ctor(config)``),
``.sigmas`` buffer, ``.config``, module tree and state-dict keys; the channels are the kx*ky patch positions and every
convolution runs along T (csrc/conv1d.hip, or the one-row form on the direct 2-D kernel: ops.conv1d_pays).  The reference's
UNET1D (a MONAI network) is not built."""
import torch
import torch.nn as nn

from . import get_sigmas
from .layers1d import ResidualBlock, RefineBlock, Conv1d, get_act, get_normalization
from ... import ops


class _NCSN1DBase(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.logit_transform = config.data.logit_transform
        self.rescaled = config.data.rescaled
        self.norm = get_normalization(config, conditional=False)
        self.ngf = ngf = config.model.ngf
        self.num_classes = config.model.num_classes
        self.act = get_act(config)
        self.register_buffer('sigmas', get_sigmas(config))
        self.config = config
        self.begin_conv = Conv1d(config.data.channels, ngf, 3)
        self.normalizer = self.norm(ngf)
        self.end_conv = Conv1d(ngf, config.data.channels, 3)

    def _stage(self, cin, cout, resample=None, dilation=None):
        kw = dict(act=self.act, normalization=self.norm)
        if dilation is not None:
            kw["dilation"] = dilation
        return nn.ModuleList([ResidualBlock(cin, cout, resample=resample, **kw),
                              ResidualBlock(cout, cout, resample=None, **kw)])

    def _compute_cond_module(self, module, x):
        """a res stage; its last block also emits the activated copy the RefineNet branch starts from"""
        n = len(module)
        for i, m in enumerate(module):
            x = m(x, want_act=(i == n - 1))
        return x

    def _begin(self, x):
        if not x.is_cuda:
            raise RuntimeError(f"{type(self).__name__}: expected GPU tensors (no CPU fallback in this build)")
        if x.dim() != 3:
            raise ValueError(f"{type(self).__name__}: expected (B, channels, T) sequences, got {tuple(x.shape)}")
        x = x.contiguous().float()
        if not self.logit_transform and not self.rescaled:
            h = ops.scale_shift_amax(x, 2.0, -1.0)            # 2x - 1; its per-sequence maxima feed begin_conv's input scale
        else:
            h = ops.scale_shift_amax(x, 1.0, 0.0)
        return self.begin_conv(h)

    def _end(self, output, y):
        output = self.end_conv(self.normalizer(output, self.act.code), feeds_conv=False)
        sig = self.sigmas if self.sigmas.dtype == torch.float32 else self.sigmas.to(torch.float32)
        return ops.div_sigma(output, sig, y.to(torch.int64))

    @staticmethod
    def _refine(block, pairs, shape, want_act=True):
        return block([p[0] for p in pairs], shape, [p[1] for p in pairs], want_act=want_act)

    def forward(self, x, y):
        with ops.amax_scope():                           # one zero-fill for all the per-sequence maxima slots of the evaluation
            return self._forward(x, y)


class NCSN1D(_NCSN1DBase):
    def __init__(self, config):
        super().__init__(config)
        ngf = self.ngf
        self.res1 = self._stage(ngf, ngf)
        self.res2 = self._stage(ngf, 2 * ngf, 'down')
        self.res3 = self._stage(2 * ngf, 2 * ngf, 'down', dilation=2)
        # the reference's 28-sample branch (ncsn1d.py:79-85) passes adjust_padding=True to a DILATED block, whose constructor
        # ignores it: both branches build the same modules
        self.res4 = self._stage(2 * ngf, 2 * ngf, 'down', dilation=4)
        self.refine1 = RefineBlock([2 * ngf], 2 * ngf, act=self.act, start=True)
        self.refine2 = RefineBlock([2 * ngf, 2 * ngf], 2 * ngf, act=self.act)
        self.refine3 = RefineBlock([2 * ngf, 2 * ngf], ngf, act=self.act)
        self.refine4 = RefineBlock([ngf, ngf], ngf, act=self.act, end=True)

    def _forward(self, x, y):
        output = self._begin(x)
        layer1 = self._compute_cond_module(self.res1, output)
        layer2 = self._compute_cond_module(self.res2, layer1[0])
        layer3 = self._compute_cond_module(self.res3, layer2[0])
        layer4 = self._compute_cond_module(self.res4, layer3[0])
        ref1 = self._refine(self.refine1, [layer4], layer4[0].shape[2:])
        ref2 = self._refine(self.refine2, [layer3, ref1], layer3[0].shape[2:])
        ref3 = self._refine(self.refine3, [layer2, ref2], layer2[0].shape[2:])
        output = self._refine(self.refine4, [layer1, ref3], layer1[0].shape[2:], want_act=False)
        return self._end(output, y)


class NCSN1DDeeper(_NCSN1DBase):
    def __init__(self, config):
        super().__init__(config)
        ngf = self.ngf
        self.res1 = self._stage(ngf, ngf)
        self.res2 = self._stage(ngf, 2 * ngf, 'down')
        self.res3 = self._stage(2 * ngf, 2 * ngf, 'down')
        self.res4 = self._stage(2 * ngf, 4 * ngf, 'down', dilation=2)
        self.res5 = self._stage(4 * ngf, 4 * ngf, 'down', dilation=4)
        self.refine1 = RefineBlock([4 * ngf], 4 * ngf, act=self.act, start=True)
        self.refine2 = RefineBlock([4 * ngf, 4 * ngf], 2 * ngf, act=self.act)
        self.refine3 = RefineBlock([2 * ngf, 2 * ngf], 2 * ngf, act=self.act)
        self.refine4 = RefineBlock([2 * ngf, 2 * ngf], ngf, act=self.act)
        self.refine5 = RefineBlock([ngf, ngf], ngf, act=self.act, end=True)

    def _forward(self, x, y):
        output = self._begin(x)
        layer1 = self._compute_cond_module(self.res1, output)
        layer2 = self._compute_cond_module(self.res2, layer1[0])
        layer3 = self._compute_cond_module(self.res3, layer2[0])
        layer4 = self._compute_cond_module(self.res4, layer3[0])
        layer5 = self._compute_cond_module(self.res5, layer4[0])
        ref1 = self._refine(self.refine1, [layer5], layer5[0].shape[2:])
        ref2 = self._refine(self.refine2, [layer4, ref1], layer4[0].shape[2:])
        ref3 = self._refine(self.refine3, [layer3, ref2], layer3[0].shape[2:])
        ref4 = self._refine(self.refine4, [layer2, ref3], layer2[0].shape[2:])
        output = self._refine(self.refine5, [layer1, ref4], layer1[0].shape[2:], want_act=False)
        return self._end(output, y)


class NCSN1DDeepest(_NCSN1DBase):
    def __init__(self, config):
        super().__init__(config)
        ngf = self.ngf
        self.res1 = self._stage(ngf, ngf)
        self.res2 = self._stage(ngf, 2 * ngf, 'down')
        self.res3 = self._stage(2 * ngf, 2 * ngf, 'down')
        self.res31 = self._stage(2 * ngf, 2 * ngf, 'down')
        self.res4 = self._stage(2 * ngf, 4 * ngf, 'down', dilation=2)
        self.res5 = self._stage(4 * ngf, 4 * ngf, 'down', dilation=4)
        self.refine1 = RefineBlock([4 * ngf], 4 * ngf, act=self.act, start=True)
        self.refine2 = RefineBlock([4 * ngf, 4 * ngf], 2 * ngf, act=self.act)
        self.refine3 = RefineBlock([2 * ngf, 2 * ngf], 2 * ngf, act=self.act)
        self.refine31 = RefineBlock([2 * ngf, 2 * ngf], 2 * ngf, act=self.act)
        self.refine4 = RefineBlock([2 * ngf, 2 * ngf], ngf, act=self.act)
        self.refine5 = RefineBlock([ngf, ngf], ngf, act=self.act, end=True)

    def _forward(self, x, y):
        output = self._begin(x)
        layer1 = self._compute_cond_module(self.res1, output)
        layer2 = self._compute_cond_module(self.res2, layer1[0])
        layer3 = self._compute_cond_module(self.res3, layer2[0])
        layer31 = self._compute_cond_module(self.res31, layer3[0])
        layer4 = self._compute_cond_module(self.res4, layer31[0])
        layer5 = self._compute_cond_module(self.res5, layer4[0])
        ref1 = self._refine(self.refine1, [layer5], layer5[0].shape[2:])
        ref2 = self._refine(self.refine2, [layer4, ref1], layer4[0].shape[2:])
        ref31 = self._refine(self.refine31, [layer31, ref2], layer31[0].shape[2:])
        ref3 = self._refine(self.refine3, [layer3, ref31], layer3[0].shape[2:])
        ref4 = self._refine(self.refine4, [layer2, ref3], layer2[0].shape[2:])
        output = self._refine(self.refine5, [layer1, ref4], layer1[0].shape[2:], want_act=False)
        return self._end(output, y)
