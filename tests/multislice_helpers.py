"""Shared pieces of the per-slice coil map tests (test_multislice_host.py, test_multislice_gpu.py): map sets that differ
strongly between slices, masks in both layouts with their plane-per-row rule, and the per-slice float64 expectation --
the existing oracle (oracle/kspace.py) called once per slice and interleaved back into batch order."""
import numpy as np

from oracle import kspace


def map_sets(S, n, H, W, complex_maps, seed):
    """(S, n, H, W) float64 / complex128, unit root-sum-of-squares over each set's own coils.  Set s is drawn from its own
    seed (seed + 1000 s) as white noise, so two sets have nothing in common: a wrong set index moves every pixel."""
    sets = []
    for s in range(S):
        rng = np.random.default_rng(seed + 1000 * s)
        m = rng.standard_normal((n, H, W))
        if complex_maps:
            m = m + 1j * rng.standard_normal((n, H, W))
        sets.append(m / np.sqrt((np.abs(m) ** 2).sum(0)))
    return np.stack(sets)


def sampling_mask(kind, T, H, W, rng):
    """uint8 planes as ops takes them -- "line": (T, W), "2d": (T, H, W) -- about 35 % sampled, the centre kept"""
    if kind == "line":
        m = rng.random((T, W)) < 0.35
        m[:, W // 2 - 2:W // 2 + 2] = True
    else:
        m = rng.random((T, H, W)) < 0.35
        m[:, H // 2 - 2:H // 2 + 2, W // 2 - 2:W // 2 + 2] = True
    return m.astype(np.uint8)


def mask_rows(mask, rows):
    """the planes batch rows `rows` read (row b reads plane b % T) as a mask of len(rows) planes; one plane stays one"""
    return mask if mask.shape[0] == 1 else np.ascontiguousarray(mask[[b % mask.shape[0] for b in rows]])


def oracle_mask(mask, rows):
    """bool mask broadcastable against (len(rows), 1, H, W) for the oracle"""
    m = mask_rows(mask, rows).astype(bool)
    return m[:, None, None, :] if m.ndim == 2 else m[:, None]


def slice_rows(s, S, B):
    return list(range(s, B, S))


def per_slice(fn, S, B, out_shape, batch_axis):
    """fn(s, rows) -> the oracle's result for the rows of slice s; scattered back to batch order along batch_axis"""
    out = np.zeros(out_shape, dtype=np.complex64)
    for s in range(S):
        rows = slice_rows(s, S, B)
        idx = [slice(None)] * len(out_shape)
        idx[batch_axis] = rows
        out[tuple(idx)] = fn(s, rows)
    return out


def forward_expected(x, maps, mask, wrong_set=None):
    """x (B, 1, H, W), maps (S, n, H, W) -> (n, B, 1, H, W); wrong_set: every row through that one set (what an index
    that ignores b would compute)"""
    S, n, B = maps.shape[0], maps.shape[1], x.shape[0]
    return per_slice(lambda s, rows: kspace.sense_forward(x[rows], maps[s if wrong_set is None else wrong_set],
                                                          oracle_mask(mask, rows)),
                     S, B, (n,) + x.shape, 1)


def adjoint_expected(sig, maps, mask=None, wrong_set=None):
    """sig (n, B, 1, H, W) -> (B, 1, H, W); mask: the true (masked) adjoint"""
    S, B = maps.shape[0], sig.shape[1]
    return per_slice(lambda s, rows: kspace.sense_adjoint(sig[:, rows], maps[s if wrong_set is None else wrong_set],
                                                          None if mask is None else oracle_mask(mask, rows)),
                     S, B, sig.shape[1:], 0)


def l2prox_expected(z, y, alpha, maps, mask, wrong_set=None):
    S, B = maps.shape[0], z.shape[0]
    return per_slice(lambda s, rows: kspace.l2_penalty_sense(z[rows], y[:, rows], alpha, 1.0,
                                                             maps[s if wrong_set is None else wrong_set],
                                                             oracle_mask(mask, rows)),
                     S, B, z.shape, 0)
