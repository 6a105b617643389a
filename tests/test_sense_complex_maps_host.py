"""SENSE with complex coil sensitivity maps, host side: the numpy oracle against the reference's own outputs for complex
maps (g36, tests/golden/make_golden_csm.py; tolerances of test_oracle_golden.py for g04 / g05), and the host behaviour
of the SENSE class (sens_maps property, sens_type="custom", sens_f32 refusing complex maps, "exp" unchanged)."""
import numpy as np
import pytest
import torch

from oracle import kspace


def test_oracle_reproduces_reference_with_complex_maps(golden):
    g = golden("g36_sense_complex_maps")
    maps, mask = g["maps"], g["mask_T1"]
    assert maps.dtype == np.complex128 and maps.shape == (4, 32, 32)
    np.testing.assert_allclose((np.abs(maps) ** 2).sum(0), 1.0, atol=1e-12)
    assert np.abs(maps.imag).max() > 0.3                                     # the phase is not a formality
    assert np.array_equal(mask[0], kspace.generate_mask(1, 32, seed=0, **kspace.MASK_PARAMS["R8"]))
    np.testing.assert_allclose(kspace.sense_forward(g["x"], maps, mask), g["Ax"], atol=3e-6)
    np.testing.assert_allclose(kspace.sense_adjoint(g["s"], maps), g["AHs"], atol=3e-6)
    np.testing.assert_allclose(kspace.sense_ssos(g["s"], maps), g["ssos_s"], atol=3e-6)
    # the real part alone is another operator altogether
    assert np.abs(kspace.sense_forward(g["x"], maps.real, mask) - g["Ax"]).max() > 100 * 3e-6


def test_oracle_l2_penalty_with_complex_maps(golden):
    g = golden("g36_sense_complex_maps")
    y = g["Ax"]
    for i in range(3):
        alpha, lamda = g[f"l2_{i}_alpha_lamda"]
        x = kspace.l2_penalty_sense(g["z"], y, alpha, lamda, g["maps"], g["mask_T1"])
        np.testing.assert_allclose(x, g[f"l2_{i}_x"], atol=2e-6)
        assert np.abs(g[f"l2_{i}_x"] - g["z"]).max() > 1e-3                  # the update is visible


@pytest.fixture(scope="module")
def SENSE():
    from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms.undersampling_fourier import SENSE as cls
    return cls


def test_exp_maps_unchanged(SENSE, golden):
    g = golden("g02_sens")
    op = SENSE("exp", 4, 20, 0.04, (1, 32, 32), seed=0)
    assert op.sens_maps.dtype == torch.float64
    assert np.array_equal(op.sens_maps.numpy(), g["maps_32x32"])
    op = SENSE("exp", 3, 20, 0.04, (1, 32, 32), seed=7)
    assert np.array_equal(op.sens_maps.numpy(), g["maps_32x32_seed7_n3"])


def test_sens_maps_setter_validates(SENSE, golden):
    maps = golden("g36_sense_complex_maps")["maps"]
    op = SENSE("exp", 4, 8, 0.04, (1, 32, 32), seed=0)
    op.sens_maps = maps                                                      # ndarray, the reference's idiom
    assert op.sens_maps.dtype == torch.complex128 and np.array_equal(op.sens_maps.numpy(), maps)
    op.sens_maps = torch.from_numpy(maps).to(torch.complex64)                # kept complex, widened on the host
    assert op.sens_maps.dtype == torch.complex128
    op.sens_maps = torch.from_numpy(maps.real.astype(np.float32))
    assert op.sens_maps.dtype == torch.float64
    for bad in (maps[:3], maps[:, :16], maps[:, :, :16], maps.transpose(0, 2, 1)[:, :, :16], maps[0]):
        with pytest.raises(ValueError):
            op.sens_maps = bad
    with pytest.raises(TypeError):
        op.sens_maps = np.ones((4, 32, 32), dtype=np.int32)
    with pytest.raises(TypeError):
        op.sens_maps = [[1.0]]
    assert op.sens_maps.dtype == torch.float64                               # a refused assignment changes nothing


def test_custom_maps_normalize_and_zero_support(SENSE, golden):
    maps = golden("g36_sense_complex_maps")["maps"]
    raw = maps * (1.0 + np.arange(32)[None, :, None])                        # undo the normalisation row by row
    raw[:, :5, :] = 0                                                        # outside the body: no support
    op = SENSE("custom", 4, 8, 0.04, (1, 32, 32), seed=0, sens_maps=raw)
    got = op.sens_maps.numpy()
    assert got.dtype == np.complex128 and np.isfinite(got.view(np.float64)).all()
    assert not got[:, :5].any()
    np.testing.assert_allclose(got[:, 5:], maps[:, 5:], atol=1e-14)
    energy = (np.abs(got) ** 2).sum(0)
    np.testing.assert_allclose(energy[5:], 1.0, atol=1e-12)
    op = SENSE("custom", 4, 8, 0.04, (1, 32, 32), seed=0, sens_maps=raw, normalize=False)
    assert np.array_equal(op.sens_maps.numpy(), raw)
    op = SENSE("custom", 4, 8, 0.04, (1, 32, 32), seed=0, sens_maps=torch.from_numpy(maps.real))     # real custom maps
    assert op.sens_maps.dtype == torch.float64
    with pytest.raises(ValueError):
        SENSE("custom", 4, 8, 0.04, (1, 32, 32), seed=0)
    with pytest.raises(ValueError):
        SENSE("custom", 3, 8, 0.04, (1, 32, 32), seed=0, sens_maps=maps)
    with pytest.raises(ValueError):
        SENSE("exp", 4, 8, 0.04, (1, 32, 32), seed=0, sens_maps=maps)


def test_sens_f32_raises_on_complex_maps(SENSE, golden):
    maps = golden("g36_sense_complex_maps")["maps"]
    op = SENSE("custom", 4, 8, 0.04, (1, 32, 32), seed=0, sens_maps=maps)
    with pytest.raises(TypeError):
        op.sens_f32("cpu")
    d = op.sens_dev("cpu")
    assert d.dtype == torch.complex64 and d.is_contiguous()
    op.sens_maps = maps.real
    assert op.sens_f32("cpu").dtype == torch.float32                         # and the cached complex copy is gone


def test_synthetic_complex_maps_and_loader(tmp_path):
    from inverseproblemwithdiffusionmodel_amd import synthetic
    from inverseproblemwithdiffusionmodel_amd.helpers.load_data import load_sens_maps
    m = synthetic.complex_coil_maps(5, 16, 64, seed=3)
    assert m.dtype == torch.complex128 and tuple(m.shape) == (5, 16, 64)
    np.testing.assert_allclose((m.abs() ** 2).sum(0).numpy(), 1.0, atol=1e-12)
    assert m.imag.abs().max() > 0.1
    assert torch.equal(m, synthetic.complex_coil_maps(5, 16, 64, seed=3))
    assert not torch.equal(m, synthetic.complex_coil_maps(5, 16, 64, seed=4))
    np.save(tmp_path / "m.npy", m.numpy().astype(np.complex64))
    torch.save(m.real.clone(), tmp_path / "m.pt")
    a, b = load_sens_maps(str(tmp_path / "m.npy")), load_sens_maps(str(tmp_path / "m.pt"))
    assert a.dtype == torch.complex128 and b.dtype == torch.float64 and tuple(a.shape) == (5, 16, 64)
    with pytest.raises(ValueError):
        load_sens_maps(str(tmp_path / "m.txt"))
