"""The shape queries of the convolution launchers answer what they answered before their host code was gathered into one plan
(csrc/wino_plan.h), one ConvArgs builder and one switch reader: every query over a grid of layer shapes, under every IPDM_WBX3_* /
IPDM_BX3_* switch that a query can see, compared cell by cell with tests/golden/g38_conv_queries.npz.  The fixture was recorded
ONCE from a build of the commit BEFORE that change (its hash is in the fixture, `parent_commit`) and is never re-recorded from the
code under test:

    python tests/test_conv_plan_host.py --record --lib <libipdm.so of the parent build> --commit <its hash>

The switches are read once per process, so every arm is a fresh child process (this file run as a script with --child); the
children only call shape queries through ctypes -- no GPU, no torch -- and run side by side."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(TESTS)
LIB = os.path.join(REPO, "inverseproblemwithdiffusionmodel_amd", "libipdm.so")
FIXTURE = os.path.join(TESTS, "golden", "g38_conv_queries.npz")

CIN = [8, 16, 24, 32, 64, 256, 512]
COUT = [32, 64, 128, 192, 256, 512]
SIDE = [4, 6, 8, 12, 14, 16, 18, 24, 32, 48, 64, 128]
DIL = [1, 2, 3, 4, 5]
ARMS = {
    "default": {},
    "WBX3_PERSIST=0": {"IPDM_WBX3_PERSIST": "0"},
    "WBX3_POLY=0": {"IPDM_WBX3_POLY": "0"},
    "WBX3_CO32=0": {"IPDM_WBX3_CO32": "0"},
    "WBX3_HALF=0": {"IPDM_WBX3_HALF": "0"},
    "WBX3_KSPLIT=0": {"IPDM_WBX3_KSPLIT": "0"},
    "WBX3_DMA4=0": {"IPDM_WBX3_DMA4": "0"},
    "WBX3_CO32=0+WBX3_KSPLIT=0": {"IPDM_WBX3_CO32": "0", "IPDM_WBX3_KSPLIT": "0"},
    "BX3_KSPLIT=0": {"IPDM_BX3_KSPLIT": "0"},
    "BX3_KSPLIT=1": {"IPDM_BX3_KSPLIT": "1"},
    "BX3_ZT2=0": {"IPDM_BX3_ZT2": "0"},
}


def _queries(lib):
    """query name -> (axes of its grid beyond (Cin, Cout, H, W), function of one cell)"""
    return {
        "wino_bx3_supported": ([DIL], lambda ci, co, h, w, d: lib.ipdm_conv2d_wino_bx3_supported(ci, co, h, w, d)),
        "wino_bx3_splitk": ([DIL], lambda ci, co, h, w, d: lib.ipdm_conv2d_wino_bx3_splitk(ci, co, h, w, d)),
        "wino_hx2_form": ([DIL], lambda ci, co, h, w, d: lib.ipdm_conv2d_wino_hx2_form(ci, co, h, w, d)),
        "wino_bx3_stats_partials": ([DIL, [0, 1]], lambda ci, co, h, w, d, p: lib.ipdm_conv2d_wino_bx3_stats_partials(ci, co, h, w, d, p)),
        "wino_supported": ([DIL], lambda ci, co, h, w, d: lib.ipdm_conv2d_wino_supported(ci, co, h, w, d)),
        "wino1d_supported": ([], lambda ci, co, h, w: lib.ipdm_conv2d_wino1d_supported(ci, co, h, w)),
        "wino1d_stats_partials": ([], lambda ci, co, h, w: lib.ipdm_conv2d_wino1d_stats_partials(ci, co, h, w)),
        "wino1d_vol_supported": ([[1, 2, 8]], lambda ci, co, h, w, dd: lib.ipdm_conv3d_wino1d_supported(ci, co, dd, h, w)),
        "bx3_splitk": ([DIL, [1, 14, 28], [1, 8], [1, 3]],
                       lambda ci, co, h, w, d, b, dd, k: lib.ipdm_conv_bx3_splitk(b, dd, ci, co, h, w, k, d)),
    }


def _axes(extra):
    return [CIN, COUT, SIDE, SIDE] + extra


def _child(lib_path, out):
    lib = ctypes.CDLL(lib_path)
    res = {}
    for name, (extra, fn) in _queries(lib).items():
        axes = _axes(extra)
        res[name] = np.array([fn(*cell) for cell in itertools.product(*axes)], dtype=np.int16).reshape([len(a) for a in axes])
    np.savez(out, **res)


def _run_arms(lib_path, workdir):
    """every arm in a child of its own -> {arm: {query: array}}"""
    procs = {}
    for i, (arm, env) in enumerate(ARMS.items()):
        out = os.path.join(workdir, f"arm{i}.npz")
        clean = {k: v for k, v in os.environ.items() if not k.startswith(("IPDM_WBX3_", "IPDM_BX3_"))}
        procs[arm] = (out, subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", lib_path, out], env=dict(clean, **env),
                                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    got = {}
    for arm, (out, p) in procs.items():
        log = p.communicate(timeout=600)[0]
        assert p.returncode == 0, (arm, p.returncode, log[-2000:])
        got[arm] = dict(np.load(out))
    return got


def test_queries_answer_as_before_the_plan(tmp_path):
    want = np.load(FIXTURE)
    assert len(str(want["parent_commit"])) == 40
    got = _run_arms(LIB, str(tmp_path))
    assert sorted(f"{arm}/{q}" for arm in got for q in got[arm]) == sorted(k for k in want.files if k != "parent_commit")
    for arm in ARMS:
        for q, (extra, _) in _queries(None).items():
            g, w = got[arm][q], want[f"{arm}/{q}"]
            assert g.shape == w.shape, (arm, q, g.shape, w.shape)
            if not np.array_equal(g, w):
                idx = tuple(int(i) for i in np.argwhere(g != w)[0])
                cell = tuple(a[i] for a, i in zip(_axes(extra), idx))
                raise AssertionError(f"arm {arm}, query {q}, cell (Cin, Cout, H, W, ...) = {cell}: {int(g[idx])}, was {int(w[idx])}; "
                                     f"{int((g != w).sum())} cells differ")
    # the grid exercises the rules: every form and both split-K answers occur, and every switch changes some answer -- but for
    # IPDM_WBX3_DMA4, which no query sees (_stats_partials answers as if it were on; the call itself then says "unsupported")
    base = got["default"]
    assert set(np.unique(base["wino_hx2_form"])) == {-2, 0, 1, 2, 3} and set(np.unique(base["wino_bx3_splitk"])) == {1, 2}
    for arm in ARMS:
        changed = any(not np.array_equal(got[arm][q], base[q]) for q in base)
        assert changed == (arm not in ("default", "WBX3_DMA4=0")), arm


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        _child(sys.argv[2], sys.argv[3])
    elif sys.argv[1] == "--record":
        import tempfile
        lib_path, commit = sys.argv[sys.argv.index("--lib") + 1], sys.argv[sys.argv.index("--commit") + 1]
        assert len(commit) == 40, "the full hash of the commit the library was built from"
        with tempfile.TemporaryDirectory() as tmp:
            got = _run_arms(os.path.abspath(lib_path), tmp)
        np.savez_compressed(FIXTURE, parent_commit=np.array(commit), **{f"{arm}/{q}": a for arm, qs in got.items() for q, a in qs.items()})
        print(FIXTURE, os.path.getsize(FIXTURE), "bytes")
