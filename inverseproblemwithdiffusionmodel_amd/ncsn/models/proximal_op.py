"""Data-consistency proximal operators (mirror of the reference's ``ncsn/models/proximal_op.py``).

``L2Penalty`` in the reference is ONE SGD(lr=0.05) step through autograd on
``0.5|x-z|^2.mean + 0.5 (alpha/lamda) |Ax-y|^2.sum(1,2,3).mean`` starting at x = z (:19-51).  Its update is
the closed form  x = z - 0.05 (alpha/lamda) A^H(A z - y) / K  with K = num_sens * W for SENSE (the .mean()
runs over the (num_sens, W) axes that .sum(dim=(1,2,3)) leaves) and K = B for a single-coil operator
(pinned by tests/golden/g05_prox.npz).  That closed form runs as one fused HIP kernel.

That one step hardly moves x towards the argmin its docstring states (the factor is 0.05 a / K); ``L2PenaltyCG`` is the
exact proximal, ``(I + a A^H A) x = z + a A^H y`` by conjugate gradients in HIP kernels, and
``L2Penalty(num_steps=k)`` is the reference's own knob: k of its SGD steps, composed from the operator kernels."""
import torch

from ..linear_transforms import LinearTransform
from ..linear_transforms.undersampling_fourier import RandomUndersamplingFourier, SENSE
from ..linear_transforms.noncartesian import NonCartesianSENSE
from ... import ops

SGD_LR = 5e-2


def _refuse_noncartesian(lin_tfm, name):
    """the one-SGD-step rule divides by K = num_sens * W, a count of grid lines: it has no meaning off the grid"""
    if isinstance(lin_tfm, NonCartesianSENSE):
        raise NotImplementedError(f"{name}: no rule for a non-Cartesian operator (NonCartesianSENSE); use L2PenaltyCG, the "
                                  "exact proximal")


def _singlecoil(lin_tfm, z, y, coef, mode):
    """z, y (B, C, H, W) complex -> the single-coil operator `mode` of ipdm_singlecoil_prox_f32"""
    zr = torch.view_as_real(z.to(torch.complex64))
    o_re, o_im = ops.singlecoil_prox(zr[..., 0].contiguous(), zr[..., 1].contiguous(),
                                     y.to(torch.complex64).contiguous(), lin_tfm.mask_u8(z.device), coef, mode)
    return torch.complex(o_re, o_im)


class Proximal(object):
    def __init__(self, lin_tfm: LinearTransform):
        self.lin_tfm = lin_tfm

    def __call__(self, *args, **kwargs):
        pass


class L2Penalty(Proximal):
    def __init__(self, lin_tfm: LinearTransform):
        _refuse_noncartesian(lin_tfm, "L2Penalty")
        super(L2Penalty, self).__init__(lin_tfm)

    def coef(self, alpha, lamda, z_shape):
        if isinstance(self.lin_tfm, SENSE):
            K = self.lin_tfm.sens_maps.shape[-3] * z_shape[-1]
        else:
            K = z_shape[0]
        return SGD_LR * (alpha / lamda) / K

    def __call__(self, z, y, alpha, lamda, num_steps=1):
        """x <- num_steps gradient steps on 1/2 |x - z|^2 + 1/2 alpha/lamda |Ax - y|^2 from x = z (one: a fused kernel)"""
        if int(num_steps) != num_steps or num_steps < 0:
            raise ValueError(f"L2Penalty: num_steps must be an integer >= 0, got {num_steps}")
        if not z.is_cuda:
            raise RuntimeError("L2Penalty: expected GPU tensors (no CPU fallback in this build)")
        if num_steps != 1:
            return self._multi_step(z.to(torch.complex64), y, float(alpha) / float(lamda), int(num_steps))
        c = self.coef(float(alpha), float(lamda), z.shape)
        z = z.to(torch.complex64)
        if isinstance(self.lin_tfm, SENSE):
            zr = torch.view_as_real(z)
            o_re, o_im = ops.sense_l2prox(zr[..., 0].contiguous(), zr[..., 1].contiguous(), y,
                                          self.lin_tfm.sens_dev(z.device), self.lin_tfm.mask_u8(z.device), c)
            return torch.complex(o_re, o_im)
        if isinstance(self.lin_tfm, RandomUndersamplingFourier):
            return _singlecoil(self.lin_tfm, z, y, c, ops.SC_L2PENALTY)
        raise NotImplementedError(f"L2Penalty: no kernel chain for {type(self.lin_tfm).__name__}")

    def _multi_step(self, z, y, a, num_steps):
        """the reference's loop (:19-51) step by step.  Its loss is 1/2 |x-z|^2 .sum(1,2,3).mean() + a/2 |Ax-y|^2
        .sum(1,2,3).mean(): the first mean runs over the batch (1/B), the second over (num_sens, W) for SENSE and over the
        batch for a single-coil operator, so
            SENSE        x <- x - 0.05 [ (x - z) / B + a A^H(A x - y) / (num_sens W) ]
            single coil  x <- x - 0.05 [ (x - z) + a A^H(A x - y) ] / B
        from x = z; zero steps return a copy of z.  Host glue over the operator kernels, off the sampler's fused path;
        y is the masked measurement, as A produces it."""
        lin = self.lin_tfm
        sense = isinstance(lin, SENSE)
        if not sense and not isinstance(lin, RandomUndersamplingFourier):
            raise NotImplementedError(f"L2Penalty: no kernel chain for {type(lin).__name__}")
        z = z.contiguous()
        y = y.to(torch.complex64).contiguous()
        B = z.shape[0]
        mask = lin.mask_u8(z.device)
        if sense:
            sens = lin.sens_dev(z.device)
            w_prior, w_data = SGD_LR / B, SGD_LR * a / (sens.shape[-3] * z.shape[-1])
        else:
            w_prior, w_data = SGD_LR / B, SGD_LR * a / B
        zf = torch.view_as_real(z)
        x = z.clone()
        for _ in range(num_steps):
            ax = ops.sense_forward(x, sens if sense else None, mask)
            if not sense:
                ax = ax[0]
            res = torch.view_as_complex(ops.axpby(torch.view_as_real(ax), torch.view_as_real(y).reshape(ax.shape + (2,)),
                                                  1.0, -1.0))
            g = ops.sense_adjoint(res, sens, mask, apply_mask=True) if sense else ops.fft2c(res, inverse=True)
            t = ops.axpby(torch.view_as_real(x), zf, 1.0 - w_prior, w_prior)
            x = torch.view_as_complex(ops.axpby(t, torch.view_as_real(g.reshape(x.shape)), 1.0, -w_data))
        return x

    @torch.no_grad()
    def check_solution(self, x_sol, z, y, alpha, lamda):
        b = z + alpha / lamda * self.lin_tfm.conj_op(y)
        lhs = x_sol + alpha / lamda * self.lin_tfm.conj_op(self.lin_tfm(x_sol))
        return (torch.abs(lhs - b) ** 2).sum(dim=(1, 2, 3)).mean()


class Constrained(Proximal):
    """Proximal operator from Yang et al (MRI)."""

    def __call__(self, X: torch.Tensor, S: torch.Tensor, lamda: float):
        return self.lin_tfm.projection(X, S, lamda)


class SingleCoil(Proximal):
    def __init__(self, lin_tfm: RandomUndersamplingFourier):
        _refuse_noncartesian(lin_tfm, "SingleCoil")
        super(SingleCoil, self).__init__(lin_tfm)
        assert isinstance(self.lin_tfm, RandomUndersamplingFourier), "only supporting RandomUnversamplingFourier"

    def __call__(self, z, y, alpha, lamda):
        """closed form  x = F' diag(1 / (1 + alpha M)) F (z + alpha F' y), one kernel (two LDS-resident FFTs)"""
        if not z.is_cuda:
            raise RuntimeError("SingleCoil: expected GPU tensors (no CPU fallback in this build)")
        return _singlecoil(self.lin_tfm, z, y, self.coef(float(alpha), float(lamda), z.shape), ops.SC_CLOSED_FORM)

    def coef(self, alpha, lamda, z_shape=None):
        return alpha / lamda

    @torch.no_grad()
    def check_solution(self, x_out, z, y, alpha, lamda):
        alpha = alpha / lamda
        lhs = x_out + alpha * self.lin_tfm.conj_op(self.lin_tfm(x_out))
        rhs = alpha * self.lin_tfm.conj_op(y) + z
        return (torch.abs(lhs - rhs) ** 2).sum(dim=(1, 2, 3)).mean()


class L2PenaltyCG(Proximal):
    """The exact proximal  argmin_x 1/2 |x - z|^2 + 1/2 (alpha/lamda) |Ax - y|^2, i.e. the solution of the normal
    equations  (I + a A^H A) x = z + a A^H y,  a = alpha/lamda,  that ``L2Penalty.check_solution`` tests.  With a SENSE
    operator (real or complex maps) it is solved per sample by conjugate gradients in HIP kernels, warm-started at z and
    stopped at |r| <= tol |b| or after max_iter iterations; with a single-coil operator the exact solution is
    ``SingleCoil``'s closed form and that kernel runs.  ``last_iters``: device int32 (B,), the iterations each sample ran
    in the last call (never synchronised here; None after a single-coil call)."""

    def __init__(self, lin_tfm: LinearTransform, max_iter=10, tol=1e-5):
        super(L2PenaltyCG, self).__init__(lin_tfm)
        if int(max_iter) != max_iter or max_iter < 1:
            raise ValueError(f"L2PenaltyCG: max_iter must be an integer >= 1, got {max_iter}")
        tol = float(tol)
        if not (0.0 <= tol < float("inf")):
            raise ValueError(f"L2PenaltyCG: tol must be finite and >= 0, got {tol}")
        self.max_iter, self.tol = int(max_iter), tol
        self.last_iters = None

    def coef(self, alpha, lamda, z_shape=None):
        return alpha / lamda

    def __call__(self, z, y, alpha, lamda, ahy=None):
        """ahy (non-Cartesian operator only): A^H W y = ``lin_tfm.adjoint_weighted(y)``, (B, 1, H, W) complex64, formed once
        by a caller that applies the proximal in a loop; None: formed here, by the direct transform, in every call"""
        if not z.is_cuda:
            raise RuntimeError("L2PenaltyCG: expected GPU tensors (no CPU fallback in this build)")
        a = self.coef(float(alpha), float(lamda), z.shape)
        z = z.to(torch.complex64)
        if isinstance(self.lin_tfm, SENSE):
            zr = torch.view_as_real(z)
            o_re, o_im, self.last_iters = ops.sense_cgprox(
                zr[..., 0].contiguous(), zr[..., 1].contiguous(), y, self.lin_tfm.sens_dev(z.device),
                self.lin_tfm.mask_u8(z.device), a, max_iter=self.max_iter, tol=self.tol)
            return torch.complex(o_re, o_im)
        if isinstance(self.lin_tfm, NonCartesianSENSE):
            # y: the samples (n, B, 1, M); A^H W y by the direct transform (unless the caller holds it), then the Toeplitz CG
            # (a framed operator: row b with the spectrum of frame b % T, 4.4m)
            lin = self.lin_tfm
            zr = torch.view_as_real(z)
            if ahy is None:
                ahy = lin.adjoint_weighted(y)
            o_re, o_im, self.last_iters = ops.nc_sense_cgprox(
                zr[..., 0].contiguous(), zr[..., 1].contiguous(), ahy.to(torch.complex64).contiguous(),
                lin.sens_dev(z.device), lin.psf_dev(z.device), a, max_iter=self.max_iter, tol=self.tol)
            return torch.complex(o_re, o_im)
        if isinstance(self.lin_tfm, RandomUndersamplingFourier):
            self.last_iters = None
            return _singlecoil(self.lin_tfm, z, y, a, ops.SC_CLOSED_FORM)
        raise NotImplementedError(f"L2PenaltyCG: no kernel chain for {type(self.lin_tfm).__name__}")

    check_solution = L2Penalty.check_solution


PROXIMALS = {"L2Penalty": L2Penalty, "Constrained": Constrained, "SingleCoil": SingleCoil, "L2PenaltyCG": L2PenaltyCG}


def get_proximal(proximal_name: str):
    """the reference's three names plus "L2PenaltyCG" """
    assert proximal_name in PROXIMALS, f"unknown proximal {proximal_name!r}: one of {sorted(PROXIMALS)}"
    return PROXIMALS[proximal_name]
