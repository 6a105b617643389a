"""Edge shapes of the non-Cartesian kernels, host side (no GPU): the conditions under which
tests/test_noncart_edges_gpu.py runs the sample loop past one stage (the first direct float64 comparison there; the
Cartesian cross-check and the 474-sample symmetry check reach a second stage indirectly), and is the first to run the column
tiles past the first, the phasor kernel past one grid round and H > W -- stated from the shapes alone, so that a change of
a shape that takes a case back inside one tile fails here.  Also that the float64 conjugate-gradient reference of the tiled proximal cases stops
below its cap, and that the float64 references move by at least 1000 times the tolerance when the one sample or pixel a
wrong stage count or tile offset would lose is taken out (so the tolerances can tell)."""
import numpy as np
import pytest

import noncart_helpers as nh
from test_noncart_gpu import TOL               # the bounds tests/test_noncart_edges_gpu.py asserts (importing needs no GPU)

STAGE, TILE, ROUND = nh.NC_STAGE, nh.NC_FORWARD_TILE, nh.NC_GRID_ROUND


@pytest.fixture(scope="module")
def ops():
    from inverseproblemwithdiffusionmodel_amd import ops as _ops
    return _ops


def _tiles(L):
    """-> (column tiles of 256, live lanes of the last one)"""
    return -(-L // STAGE), (L - 1) % STAGE + 1


@pytest.mark.parametrize("name", sorted(nh.EDGE_CASES))
def test_every_case_is_served(ops, name):
    H, W, B, n, spokes, readout = nh.EDGE_CASES[name]
    assert ops.nc_supported(H, W)
    assert len(nh.edge_trajectory(spokes, readout, H, W)) == spokes * readout + 6
    # the padded grid goes through the strip passes at the three tiled shapes, through one LDS image at the smallest
    want = ops.KSPACE_LDS if name.startswith("smallest") else ops.KSPACE_STRIPS
    assert ops.kspace_size_class(2 * H, 2 * W) == want


def test_wide_case_size_classes():
    H, W, B, n, spokes, readout = nh.EDGE_CASES["wide"]
    M = spokes * readout + 6
    assert M == 1734 == 6 * STAGE + 198                       # 7 stages, the last one partial, after 6 full ones
    assert _tiles(W) == (2, 64)                               # image adjoint: 2 column tiles, 64 live lanes in the second
    assert _tiles(2 * W) == (3, 128)                          # lag kernel: 3 tiles, 128 live lanes in the last
    assert ROUND < W * M == 554_880 < 2 * ROUND               # ex / exp tables: past one grid round
    assert 2 * ROUND < 2 * W * M == 1_109_760                 # lx / lxp tables: past two
    assert H * M < ROUND and 2 * H * M < ROUND                # the short side stays inside one
    assert M % TILE == 6                                      # forward: the last tile of 64 has 6 live lanes
    assert (2 * W) % 5 == 0 and 2 * H * 2 * W > 16384         # 32 x 640: radix 5, strips


def test_tall_case_size_classes():
    H, W, B, n, spokes, readout = nh.EDGE_CASES["tall"]
    M = spokes * readout + 6
    assert H > W and M == 1734
    assert ROUND < H * M < 2 * ROUND and 2 * ROUND < 2 * H * M          # ey, ly past a grid round / two
    assert W * M < ROUND and _tiles(W) == (1, 16) and _tiles(2 * W) == (1, 32)
    assert (H, 2 * H) == (320, 640)                           # grid.y of the image adjoint and of the lag kernel


def test_widest_case_size_classes(ops):
    H, W, B, n, spokes, readout = nh.EDGE_CASES["widest"]
    M = spokes * readout + 6
    assert M == 582 == 2 * STAGE + 70
    assert _tiles(W) == (4, 256) and _tiles(2 * W) == (8, 256)          # full tiles only
    assert ROUND < W * M and 2 * ROUND < 2 * W * M
    assert ops.nc_supported(H, W) and not ops.nc_supported(H, W + 16) and not ops.nc_supported(H, 2 * W)   # the served limit


@pytest.mark.parametrize("name", ["smallest_wide", "smallest_tall"])
def test_smallest_case_size_classes(ops, name):
    H, W, B, n, spokes, readout = nh.EDGE_CASES[name]
    M = spokes * readout + 6
    assert M == 326 == STAGE + 70 and min(H, W) == 2
    assert 2 * min(H, W) == 4                                 # the padded short side: a length-4 FFT
    assert not ops.nc_supported(1, 64) and not ops.nc_supported(64, 1)  # nothing smaller is served


@pytest.mark.parametrize("name", sorted(nh.EDGE_FRAME_CASES))
def test_frame_case_size_classes(ops, name):
    H, W, T, B, n = nh.EDGE_FRAME_CASES[name]
    k = nh.frame_trajectory(T, H, W, 27, 33)
    M = k.shape[1]
    assert ops.nc_supported(H, W) and k.shape == (T, 897, 2) and M == 3 * STAGE + 129
    assert B == 2 * T                                         # every frame is read by two rows
    for t in range(1, T):
        assert (t * M) % TILE and (t * M) % STAGE             # the frame offset is a multiple of neither 64 nor 256
    assert ROUND < max(H, W) * T * M                          # the long side's table over T M samples: past a grid round
    if name == "wide":
        assert W * T * M == 574_080
    # two frames differ enough that the set index cannot be ignored (tests/test_noncart_frames_gpu.py's test_frames_differ)
    P0, P1 = nh.toeplitz_psf(k[0], H, W), nh.toeplitz_psf(k[1], H, W)
    assert np.abs(P0 - P1).max() / np.abs(P0).max() > 1e-2


@pytest.mark.parametrize("name", sorted(nh.EDGE_CASES))
def test_blocky_weights(name):
    H, W, B, n, spokes, readout = nh.EDGE_CASES[name]
    k = nh.edge_trajectory(spokes, readout, H, W)
    w, ramp = nh.blocky_weights(k, H, W), nh.ramp_weights(k, H, W).astype(np.float32)
    M = len(k)
    last = M // STAGE * STAGE
    assert w.dtype == np.float32 and M % STAGE != 0
    assert not w[STAGE:2 * STAGE].any() and not w[last:].any()
    keep = np.ones(M, dtype=bool)
    keep[STAGE:2 * STAGE] = False
    keep[last:] = False
    assert keep[:STAGE].all() and np.array_equal(w[keep], ramp[keep]) and (w[keep] > 0).all()


# ---- the tolerances can tell -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["none", "ramp"])
@pytest.mark.parametrize("name", sorted(nh.EDGE_CASES))
def test_references_move_by_1000_tolerances(name, kind):
    """sample 256 -- the first of the second stage -- dropped: A^H W y (combined and per coil) and P move; the last pixel
    zeroed: A x moves (with maps and as coil images).  Each by at least 1000 times the bound the GPU file asserts."""
    c, r = nh.edge_inputs(name), nh.edge_refs(name, kind)
    w = np.ones(c.M, dtype=np.float32) if r.w is None else r.w.copy()
    assert w[STAGE] > 0
    w[STAGE] = 0
    x, imgs = c.x.copy(), c.imgs.copy()
    x[:, -1, -1] = 0
    imgs[..., -1, -1] = 0
    moved = dict(adjoint=nh.relerr(nh.sense_adjoint(c.y, c.S, c.k, c.H, c.W, w), r.AHy),
                 adjoint_coils=nh.relerr(nh.ndft_adjoint(c.y, c.k, c.H, c.W, w), r.coil_imgs),
                 psf=nh.relerr(nh.toeplitz_psf(c.k, c.H, c.W, w), r.P),
                 forward=nh.relerr(nh.sense_forward(x, c.S, c.k), c.Ax),
                 forward_coils=nh.relerr(nh.ndft_forward(imgs, c.k), c.Aimgs))
    print(f"sensitivity {name} {kind}: " + "  ".join(f"{q} {v:.3g}" for q, v in moved.items()))
    for q, v in moved.items():
        assert v >= 1000 * TOL[q.split("_")[0]], (q, v)


# ---- the float64 solver of the tiled proximal cases stops below its cap ------------------------------------------------
@pytest.mark.parametrize("a", [1.0, 4.0])
@pytest.mark.parametrize("H,W", [(16, 320), (320, 16)])
def test_float64_cg_stops_below_the_cap(H, W, a):
    p, ahy, ref, it64 = nh.prox_reference(H, W, 27, 64, 2, 3, a, 40, 1e-5)
    print(f"float64 cg {H}x{W} a={a}: iters {it64}")
    assert p.k.shape == (27 * 64, 2) and p.z.shape == (2, H, W) and p.S.shape == (3, H, W)
    assert (0 < it64).all() and (it64 < 40).all()
    res = nh.prox_residual(ref, p.z.astype(np.complex128), ahy, p.S, p.k, a)
    assert res.max() <= 1e-5 * (1 + 1e-6)                          # the stopping rule, seen through the direct transforms
