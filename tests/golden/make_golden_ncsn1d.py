#!/usr/bin/env python3
"""Generate the NCSN1D fixtures (g33_ncsn1d, g34_ncsn1d_full, g35_ald2dtime_1d) by importing the Python reference, as
make_golden.py does (same symlinked alias, same stubs: this script imports make_golden for them).  CPU only; the outputs are
DATA.

    python tests/golden/make_golden_ncsn1d.py            # rewrites tests/golden/g33_*.npz, g34_*.npz, g35_*.npz

  g33_ncsn1d         InstanceNorm1dPlus, 1-D CRPBlock, RCUBlock, MSFBlock (second input at half length), RefineBlock (start /
                     two inputs / end), ResidualBlock (plain / down / dilated-down / dilated-same), tiny NCSN1D (ngf 4,
                     16 channels, L = 24, 6 levels), tiny NCSN1DDeeper (L = 24) and tiny NCSN1DDeepest (L = 32), each with
                     its weights stored.  NCSN1DDeepest pools four times and the reference's own pair sum
                     (layers1d.py:324, `sum([output[:, :, ::2], output[:, :, 1::2]])`) raises on an odd length -- 24 reaches
                     3 at the fourth pooling --, hence L = 32 for that network.
  g34_ncsn1d_full    NCSN1D at the cine127_1d.yml size (ngf 128, 64 channels, T = 24, 400 levels) on
                     synthetic.synth_state_dict(seed=0) weights (NOT stored: key names and shapes are); N = 6 sequences,
                     labels spread over the 400 levels, sequence 0 at the top level's noise amplitude
  g35_ald2dtime_1d   the reference's ALD2DTime with g33's tiny NCSN1D as scorenet_T (16 channels: 4 x 4 patches), by the
                     procedure of g17 (measurement and spatial network of g17 / g07; injected noise = Generator(350), its call
                     count and sum recorded; mode diffusion1d) plus one run with if_random_shift=True (np.random.seed(351),
                     shifts recorded)
"""
import importlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (imports the reference under its alias, stubs the absent packages)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

ref_ncsn1d = importlib.import_module("InverseProblemWithDiffusionModel.ncsn.models.ncsn1d")
ref_layers1d = importlib.import_module("InverseProblemWithDiffusionModel.ncsn.models.layers1d")
ref_norm1d = importlib.import_module("InverseProblemWithDiffusionModel.ncsn.models.normalization1d")

npy, _sd = mg.npy, mg._sd
NC = 6                                      # noise levels of the tiny networks


def _perturb(module, scale=0.05):
    """make biases and betas non-trivial (the reference initialises beta at 0)"""
    for p in module.parameters():
        if p.ndim == 1:
            p.data.add_(scale * torch.randn_like(p))


def tiny_cfg(ngf=4, channels=16, image_size=24):
    return mg.tiny_config(ngf=ngf, num_classes=NC, sigma_begin=0.5, sigma_end=0.01, channels=channels, image_size=image_size)


def g33_layers(out):
    torch.manual_seed(33)
    act = nn.ELU()
    norm = ref_norm1d.InstanceNorm1dPlus
    x = torch.randn(2, 6, 24) * 1.5 + 0.3
    out["blk_x"] = npy(x)
    n = norm(6)
    _perturb(n, 0.1)
    out.update(_sd(n, "in1d"))
    out["in1d_y"] = npy(n(x))
    m = ref_layers1d.CRPBlock(6, 2, act)
    out.update(_sd(m, "crp"))
    out["crp_y"] = npy(m(x.clone()))
    m = ref_layers1d.RCUBlock(6, 2, 2, act)
    out.update(_sd(m, "rcu"))
    out["rcu_y"] = npy(m(x.clone()))                           # (the reference adds the residual in place)
    variants = {
        "rb_plain": dict(input_dim=6, output_dim=6, resample=None),
        "rb_pool": dict(input_dim=6, output_dim=8, resample="down"),
        "rb_dil_down": dict(input_dim=6, output_dim=8, resample="down", dilation=2),
        "rb_dil_same": dict(input_dim=6, output_dim=6, resample=None, dilation=4),
    }
    for name, kw in variants.items():
        m = ref_layers1d.ResidualBlock(act=act, normalization=norm, **kw)
        _perturb(m)
        out.update(_sd(m, name))
        out[name + "_y"] = npy(m(x.clone()))
    xa = torch.randn(2, 6, 24)
    xb = torch.randn(2, 4, 12)
    out["rf_xa"], out["rf_xb"] = npy(xa), npy(xb)
    m = ref_layers1d.MSFBlock([6, 4], 5)
    _perturb(m)
    out.update(_sd(m, "msf"))
    out["msf_y"] = npy(m([xa, xb], xa.shape[2:]))
    for name, (planes, feats, kw) in {"rf_start": ([6], 6, dict(start=True)), "rf_two": ([6, 4], 5, {}),
                                      "rf_end": ([6, 4], 6, dict(end=True))}.items():
        m = ref_layers1d.RefineBlock(planes, feats, act=act, **kw)
        _perturb(m)
        out.update(_sd(m, name))
        xs = [xa.clone()] if len(planes) == 1 else [xa.clone(), xb.clone()]
        out[name + "_y"] = npy(m(xs, xa.shape[2:]))


def _tiny_net(cls, seed, L):
    cfg = tiny_cfg(image_size=L)
    torch.manual_seed(seed)
    with mg.quiet:
        net = cls(cfg).eval()
    _perturb(net)
    return net, cfg


def g33_nets(out):
    for name, cls, seed, L in [("n1d", ref_ncsn1d.NCSN1D, 330, 24), ("n1d_deeper", ref_ncsn1d.NCSN1DDeeper, 331, 24),
                               ("n1d_deepest", ref_ncsn1d.NCSN1DDeepest, 332, 32)]:
        net, cfg = _tiny_net(cls, seed, L)
        g = torch.Generator().manual_seed(333)
        x = torch.rand(3, cfg.data.channels, L, generator=g)
        labels = torch.tensor([0, 3, 5])
        out.update(_sd(net, name))
        out[name + "_x"], out[name + "_labels"] = npy(x), npy(labels)
        with torch.no_grad():
            out[name + "_y"] = npy(net(x, labels))


def g34_full():
    from inverseproblemwithdiffusionmodel_amd.synthetic import synth_state_dict
    cfg = mg.tiny_config(ngf=128, num_classes=400, sigma_begin=40, sigma_end=0.01, channels=64, image_size=24)
    with mg.quiet:
        net = ref_ncsn1d.NCSN1D(cfg).eval()
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict(synth_state_dict(shapes, seed=0), strict=False)
    g = torch.Generator().manual_seed(34)
    x = torch.rand(6, 64, 24, generator=g)
    x[0] = x[0] + 40.0 * torch.randn(64, 24, generator=g)      # a sequence at the top noise level (label 0: sigma 40)
    labels = torch.tensor([0, 80, 160, 240, 320, 399])
    with torch.no_grad():
        y = net(x, labels)
    mg.save("g34_ncsn1d_full", x=npy(x), labels=npy(labels), y=npy(y), key_names=np.array(list(shapes.keys())),
            key_shapes=np.array([",".join(map(str, s)) for s in shapes.values()]),
            n_params=np.array(sum(p.numel() for p in net.parameters())))


class _SeededNoise:
    def __init__(self, seed):
        self.g, self.calls, self.total = torch.Generator().manual_seed(seed), 0, 0.0

    def __call__(self, like):
        n = torch.randn(like.shape, generator=self.g, dtype=like.dtype)
        self.calls += 1
        self.total += float(n.double().sum())
        return n


def g35_ald2dtime():
    """g17's procedure with the tiny NCSN1D of g33 as the temporal prior (T = 8: the network is fully convolutional)"""
    ref_ald, ref_uf, ref_prox = mg.ref_ald, mg.ref_uf, mg.ref_prox
    T, H, W = 8, 32, 32
    g7 = np.load(os.path.join(HERE, "g07_layers.npz"))
    g17 = np.load(os.path.join(HERE, "g17_ald2dtime.npz"))
    g33 = np.load(os.path.join(HERE, "g33_ncsn1d.npz"))
    cfg2d = mg.tiny_config()
    with mg.quiet:
        net2d = mg.ref_ncsnv2.NCSNv2Deepest(cfg2d).eval()
    net2d.load_state_dict({k[len("net__"):].replace("__", "."): torch.from_numpy(g7[k]) for k in g7.files
                           if k.startswith("net__")})
    cfgT = tiny_cfg(image_size=T)
    sdT = {k[len("n1d__"):].replace("__", "."): torch.from_numpy(g33[k]) for k in g33.files if k.startswith("n1d__")}
    ref_ald.vis_images = lambda *a, **k: None
    ref_ald.vis_multi_channel_signal = lambda *a, **k: None
    orig = ref_uf.RandomUndersamplingFourier._generate_mask
    try:
        ref_uf.RandomUndersamplingFourier._generate_mask = mg.t1_mask_patch(mg.MASK_PARAMS["R8"])
        with mg.quiet:
            op = ref_uf.SENSE("exp", 4, 8, 0.04, (1, H, W), seed=0)
    finally:
        ref_uf.RandomUndersamplingFourier._generate_mask = orig
    meas = torch.from_numpy(g17["measurement"])
    sigmas = mg.ref_get_sigmas(cfg2d, "recons")
    sigmas_T = mg.ref_get_sigmas(cfgT, "recons")
    out = {"sigmas": npy(sigmas), "sigmas_T": npy(sigmas_T)}
    params = dict(n_steps_each=2, step_lr=2e-5, denoise=False, final_only=True)
    for tag, shift in [("plain", False), ("shift", True)]:
        noise = _SeededNoise(350)
        real_randn_like, real_randint = torch.randn_like, np.random.randint
        shifts = []

        def randint(*a, **k):
            v = real_randint(*a, **k)
            shifts.append(np.array(v))
            return v
        torch.randn_like = noise
        np.random.randint = randint
        np.random.seed(351)
        try:
            with mg.quiet:
                netT = ref_ncsn1d.NCSN1D(cfgT).eval()
            netT.load_state_dict(sdT)
            sampler = ref_ald.ALD2DTime(ref_prox.get_proximal("L2Penalty")(op), netT, sigmas_T.clone(), (1, T, 1, H, W), net2d,
                                        sigmas.clone(), params, cfg2d, meas, op, device=torch.device("cpu"))
            with mg.quiet:
                res = sampler(save_dir="/tmp/ipdm_oracle/out", lr_scaled=1.0e5, mode_T="diffusion1d", lamda_T=3.0,
                              if_random_shift=shift)[0]
        finally:
            torch.randn_like, np.random.randint = real_randn_like, real_randint
            torch.set_grad_enabled(True)
        out[f"{tag}_x"] = npy(res)
        out[f"{tag}_meta"] = np.array([3.0, noise.calls, noise.total])
        out[f"{tag}_shifts"] = np.stack(shifts) if shifts else np.zeros((0, 2), dtype=np.int64)
        print(f"  {tag}: noise calls {noise.calls}, shifts {len(shifts)}")
    mg.save("g35_ald2dtime_1d", **out)


if __name__ == "__main__":
    which = sys.argv[1:] or None
    torch.set_num_threads(8)
    if which is None or "g33" in which:
        out = {}
        g33_layers(out)
        g33_nets(out)
        mg.save("g33_ncsn1d", **out)
    if which is None or "g34" in which:
        g34_full()
    if which is None or "g35" in which:
        g35_ald2dtime()
