"""CPU-only checks of the NCSN1D family's host side: the three networks' state-dict keys and shapes against the reference's
(g33_ncsn1d: tiny networks with weights, g34_ncsn1d_full: key names and shapes at the cine127_1d.yml size), the `Diffusion1D`
registry entry, and the 1-D entries of the C ABI in the header and in the ctypes table."""
import os
import re
from argparse import Namespace

import pytest
import torch

from conftest import state_dict_from_golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = pytest.importorskip("inverseproblemwithdiffusionmodel_amd")

ABI_1D = ["ipdm_conv1d_hx2_supported", "ipdm_conv1d_hx2_weight_bytes", "ipdm_conv1d_hx2_pack_weight", "ipdm_conv1d_hx2_f32",
          "ipdm_meanpool1d2_f32", "ipdm_scale_shift_amax_f32"]


def cfg1d(ngf=4, num_classes=6, sigma_begin=0.5, sigma_end=0.01, channels=16, image_size=24, device="cpu"):
    return Namespace(
        device=torch.device(device),
        data=Namespace(channels=channels, image_size=image_size, logit_transform=False, rescaled=False,
                       uniform_dequantization=False, gaussian_dequantization=False),
        model=Namespace(ngf=ngf, num_classes=num_classes, sigma_begin=sigma_begin, sigma_end=sigma_end,
                        sigma_dist="geometric", normalization="InstanceNorm++", nonlinearity="elu", spec_norm=False),
        recons=Namespace(sigma_dist="geometric", sigma_begin=sigma_begin, sigma_end=sigma_end, num_classes=num_classes),
        sampling=Namespace(n_steps_each=3, step_lr=9e-7, final_only=True, denoise=True))


@pytest.mark.parametrize("prefix,cls,L", [("n1d", "NCSN1D", 24), ("n1d_deeper", "NCSN1DDeeper", 24),
                                          ("n1d_deepest", "NCSN1DDeepest", 32)])
def test_state_dict_keys_and_shapes(golden, prefix, cls, L):
    from inverseproblemwithdiffusionmodel_amd.ncsn.models import ncsn1d
    ref = state_dict_from_golden(golden("g33_ncsn1d"), prefix)
    net = getattr(ncsn1d, cls)(cfg1d(image_size=L))
    mine = net.state_dict()
    assert sorted(mine) == sorted(ref)
    assert {k: tuple(v.shape) for k, v in mine.items()} == {k: tuple(v.shape) for k, v in ref.items()}
    net.load_state_dict(ref, strict=True)
    assert torch.equal(net.state_dict()["begin_conv.weight"], ref["begin_conv.weight"])
    assert net.begin_conv.weight.dim() == 3 and hasattr(net.normalizer, "alpha") and hasattr(net.normalizer, "gamma") \
        and hasattr(net.normalizer, "beta")


def test_full_size_keys_and_shapes(golden):
    from inverseproblemwithdiffusionmodel_amd.ncsn.models.ncsn1d import NCSN1D
    g = golden("g34_ncsn1d_full")
    net = NCSN1D(cfg1d(ngf=128, num_classes=400, sigma_begin=40, sigma_end=0.01, channels=64, image_size=24))
    sd = net.state_dict()
    assert list(sd.keys()) == list(g["key_names"])
    assert [",".join(map(str, v.shape)) for v in sd.values()] == list(g["key_shapes"])
    assert sum(p.numel() for p in net.parameters()) == int(g["n_params"])


def test_diffusion1d_registry_entry_builds(golden):
    from inverseproblemwithdiffusionmodel_amd.helpers import load_model
    from inverseproblemwithdiffusionmodel_amd.ncsn.models.ncsn1d import NCSN1D
    assert load_model.TASK_NAME_TO_MODEL_CTOR["Diffusion1D"] is NCSN1D
    assert "UNET1D" not in load_model.TASK_NAME_TO_MODEL_CTOR and "UNet1D" not in load_model.TASK_NAME_TO_MODEL_CTOR
    for ds in ("CINE127", "CINE127_1D"):                        # both resolve to the `_1D` config, as Diffusion3D does
        net = load_model.reload_model("Diffusion1D", ds, device=torch.device("cpu"))
        assert isinstance(net, NCSN1D)
        assert net.config.data.channels == 64 and net.config.data.image_size == 24 and net.ngf == 128
        assert net.sigmas.shape == (400,)
        assert list(net.state_dict().keys()) == list(golden("g34_ncsn1d_full")["key_names"])
    # a Lightning-style checkpoint of the reference (EMA weights under `model.`) loads
    sd = {"model." + k: v.clone() for k, v in net.state_dict().items()}
    ckpt = {"callbacks": {"EMA": {"ema_state_dict": sd}}}
    res = load_model.load_scorenet_weights(net, ckpt)
    assert not res.missing_keys and not res.unexpected_keys


def test_cpu_tensors_raise():
    from inverseproblemwithdiffusionmodel_amd.ncsn.models.ncsn1d import NCSN1D
    net = NCSN1D(cfg1d())
    with pytest.raises(RuntimeError):
        net(torch.zeros(1, 16, 24), torch.zeros(1, dtype=torch.long))


def test_abi_names_in_header_and_table():
    from inverseproblemwithdiffusionmodel_amd import _lib
    header = open(os.path.join(REPO, "include", "ipdm.h")).read()
    declared = set(re.findall(r"\b(ipdm_[a-z0-9_]+)\s*\(", header))
    for name in ABI_1D:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.lib, name), name
    assert "ncsn/models/layers1d.py" in header
    assert re.search(r"#define\s+IPDM_ABI_VERSION\s+4\b", header) and _lib.lib.ipdm_abi_version() == 4
    # the shape rule is host logic: the census shapes are the kernel's, tiny / ragged ones are not
    sup = _lib.lib.ipdm_conv1d_hx2_supported
    for cin, cout in [(64, 128), (128, 128), (128, 256), (256, 256), (256, 128), (128, 64)]:
        for L in (12, 24, 48):
            assert sup(cin, cout, L, 3, 1) and sup(cin, cout, L, 3, 2) and sup(cin, cout, L, 3, 4) and sup(cin, cout, L, 1, 1)
    assert not sup(16, 4, 24, 3, 1) and not sup(4, 16, 24, 3, 1) and not sup(128, 128, 10, 3, 1) and not sup(128, 128, 24, 3, 3)
    assert not sup(128, 128, 6, 3, 1)


def test_served_lengths_are_the_divisors_of_96_from_12():
    """the launcher's shape rule and ops.conv1d_pays agree for L = 1..200 on every census shape and (k, dilation), and the lengths
    served are exactly 12, 16, 24, 32, 48 and 96 (whole sequences in a 96-column group)"""
    from inverseproblemwithdiffusionmodel_amd import _lib, ops
    sup = _lib.lib.ipdm_conv1d_hx2_supported
    on = ops.USE_CONV1D and ops.CONV_IMPL == "hx2"
    for cin, cout in [(64, 128), (128, 128), (128, 256), (256, 256), (256, 128), (128, 64)]:
        for k, d in [(1, 1), (3, 1), (3, 2), (3, 4)]:
            served = [L for L in range(1, 201) if sup(cin, cout, L, k, d)]
            assert served == [12, 16, 24, 32, 48, 96], (cin, cout, k, d, served)
            for L in range(1, 201):
                assert ops.conv1d_pays(cin, cout, L, k, d) == (on and L in served), (cin, cout, L, k, d)
