"""The convolution wrappers of ops.py hand the native entry points what they handed them before their common frame (output pair,
res_second check, want_amax gate and maxima slots, CONV_TRACE bracket, batch-chunk loop, tag-and-return tail) was gathered into
helpers: one case per branch of each wrapper, with `ops.call` wrapped (the real call still runs), compared with
tests/golden/g40_conv_calls.json -- per wrapper invocation the sequence of entry names, every scalar argument, for every pointer
argument which operand it is and the byte offset into it, the fields of the `ext` struct, the structure of what comes back and
the CONV_TRACE record without its events.  The fixture was recorded ONCE on an MI355X from a build of the commit BEFORE that
change (its hash is in the fixture, `parent_commit`) and is never re-recorded from the code under test:

    python tests/test_conv_frame_gpu.py --record --repo <tree of the parent build> --commit <its hash> --out <file>
"""
import json
import os
import sys

import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(TESTS, "golden", "g40_conv_calls.json")


class _Ctx:
    def __init__(self, ops):
        import torch
        self.ops, self.torch = ops, torch
        self.gen = torch.Generator(device="cuda").manual_seed(40)

    def T(self, *shape):
        return self.torch.randn(*shape, device="cuda", generator=self.gen)

    def amax(self, B):                                   # a caller's maxima vector (a bound, not a measurement)
        return self.torch.full((B, self.ops.AMAX_SLOT), 8.0, device="cuda")

    def wino(self, Cin, Cout, fmt="hx2"):
        return self.ops.conv_wino_split_weight(self.T(Cout, Cin, 3, 3), fmt)

    def wino1d(self, Cin, Cout):
        return self.ops.conv_wino1d_weight(self.T(Cout, Cin, 3, 3))

    def direct(self, Cin, Cout, *k, impl="hx2"):
        return self.ops.conv_weight(self.T(Cout, Cin, *k), impl)


def _wbx3(c, Cin, Cout, H, W, B=2, fmt="hx2", one_d=False, patch=None, **kw):
    U = c.wino1d(Cin, Cout) if one_d else c.wino(Cin, Cout, fmt)
    return "conv2d_wino_bx3", c.T(B, Cin, H, W), U, kw, patch or {}


def _bx3(c, Cin, Cout, k, *sp, B=2, **kw):
    return "conv_bx3", c.T(B, Cin, *sp), c.direct(Cin, Cout, *([k] * len(sp))), kw, {}


def _strided_bias(c, B, Cout):
    return c.T(B, 2 * Cout)[:, :Cout]                    # per-image bias rows with a row stride


def _splitk_case(c, **kw):
    """64 -> 64 channels at 8 x 16 runs as two K halves on the three-piece family (the f16x2 one: with IPDM_WBX3_CO32 off)"""
    assert c.ops.wino_bx3_splitk(64, 64, 8, 16) > 1
    return _wbx3(c, 64, 64, 8, 16, fmt="bx3", **kw)


def _bx3_splitk_case(c, Cin, Cout, *sp):
    D = sp[0] if len(sp) == 3 else 1
    from inverseproblemwithdiffusionmodel_amd import _lib
    assert _lib.lib.ipdm_conv_bx3_splitk(2, D, Cin, Cout, sp[-2], sp[-1], 3, 1) > 1
    return _bx3(c, Cin, Cout, 3, *sp)


ELU, COPY = 1, 5                                         # ops.ACT_ELU, ops.ACT_COPY
CHUNK = {"wino_bx3_max_batch": lambda *a, **k: 2}
CASES = {
    "wbx3_plain": lambda c: _wbx3(c, 16, 64, 8, 32, bias=c.T(64)),
    "wbx3_splitk": lambda c: _splitk_case(c, bias=c.T(64), residual=c.T(2, 64, 8, 16), act_out=ELU, want_amax=True),
    "wbx3_splitk_hx2_co32_off": lambda c: _wbx3(c, 64, 64, 8, 16, patch={"WBX3_CO32": False}, in_amax=c.amax(2)),
    "wbx3_stats": lambda c: _wbx3(c, 32, 64, 8, 32, want_stats=True),
    "wbx3_stats_pool": lambda c: _wbx3(c, 32, 64, 8, 32, want_stats=True, pool2=True, residual=c.T(2, 64, 4, 16)),
    "wbx3_1d": lambda c: _wbx3(c, 32, 128, 8, 32, one_d=True, in_amax=c.amax(2), want_amax=True),
    "wbx3_1d_stats": lambda c: _wbx3(c, 32, 128, 8, 32, one_d=True, want_stats=True),
    "wbx3_1d_fused_input": lambda c: _wbx3(c, 32, 128, 8, 32, one_d=True, coef=c.T(2, 32, 3), act=ELU, in_amax=c.amax(2),
                                           want_stats=True),
    "wbx3_1d_pool": lambda c: _wbx3(c, 32, 128, 8, 32, one_d=True, pool2=True, act_out=ELU),
    "wbx3_chunked": lambda c: _wbx3(c, 16, 64, 8, 32, B=5, patch=CHUNK, bias=_strided_bias(c, 5, 64), in_amax=c.amax(5),
                                    residual=c.T(5, 64, 8, 32), act_out=ELU, want_amax=True, want_stats=True),
    "wbx3_1d_chunked": lambda c: _wbx3(c, 32, 128, 8, 32, B=5, one_d=True, patch=CHUNK, coef=c.T(5, 32, 3), act=ELU,
                                       in_amax=c.amax(5), want_stats=True, want_amax=True),
    "wbx3_splitk_chunked": lambda c: _splitk_case(c, B=5, patch=CHUNK, bias=_strided_bias(c, 5, 64),
                                                  residual=c.T(5, 64, 8, 16), act_out=COPY, res_second=True, want_amax=True),
    "wbx3_res_second": lambda c: _wbx3(c, 16, 64, 8, 32, residual=c.T(2, 64, 8, 32), act_out=COPY, res_second=True),
    "wbx3_act_only": lambda c: _wbx3(c, 16, 64, 8, 32, act_out=ELU, raw=False, want_amax=True),
    "wbx3_want_amax_measured": lambda c: _wbx3(c, 16, 64, 8, 32, in_amax=True, want_amax=True),
    "wbx3_bias_rows_out_scale": lambda c: _wbx3(c, 16, 64, 8, 32, bias=_strided_bias(c, 2, 64), out_scale=0.5),
    "bx3_k1": lambda c: _bx3(c, 16, 64, 1, 8, 8, bias=c.T(64)),
    "bx3_k3": lambda c: _bx3(c, 16, 64, 3, 8, 8, coef=c.T(2, 16, 3), act=ELU, residual=c.T(2, 64, 8, 8), act_out=ELU, want_amax=True),
    "bx3_res_second": lambda c: _bx3(c, 16, 64, 3, 8, 8, residual=c.T(2, 64, 8, 8), act_out=COPY, res_second=True),
    "bx3_act_only_bias_rows": lambda c: _bx3(c, 16, 64, 3, 8, 8, bias=_strided_bias(c, 2, 64), out_scale=0.5, act_out=ELU, raw=False),
    "bx3_3d": lambda c: _bx3(c, 16, 32, 3, 2, 4, 4, dilation=2, want_amax=True),
    "bx3_splitk": lambda c: _bx3_splitk_case(c, 256, 32, 4, 4),
    "bx3_splitk_3d": lambda c: _bx3_splitk_case(c, 64, 32, 2, 4, 4),
    "bx3_out": lambda c: _bx3(c, 16, 64, 3, 8, 8, out=c.T(2, 64, 8, 8), want_amax=True),
    "bx3_in_amax_measured": lambda c: _bx3(c, 16, 64, 3, 8, 8, in_amax=True),
    "wino1d_vol": lambda c: ("conv3d_wino1d", c.T(2, 32, 2, 4, 4), c.ops.conv_wino1d_weight3d(c.T(128, 32, 3, 3, 3)),
                             dict(bias=c.T(128), residual=c.T(2, 128, 2, 4, 4), act_out=ELU, in_amax=c.amax(2), want_amax=True), {}),
    "wino1d_vol_res_second": lambda c: ("conv3d_wino1d", c.T(2, 32, 2, 4, 4), c.ops.conv_wino1d_weight3d(c.T(128, 32, 3, 3, 3)),
                                        dict(residual=c.T(2, 128, 2, 4, 4), act_out=COPY, res_second=True, in_amax=True), {}),
    "conv1d": lambda c: ("conv1d", c.T(2, 16, 16), c.ops.conv1d_weight(c.T(64, 16, 1)),
                         dict(bias=c.T(64), residual=c.T(2, 64, 16), act_out=ELU, in_amax=c.amax(2), want_amax=True), {}),
    "conv1d_pool": lambda c: ("conv1d", c.T(2, 16, 16), c.ops.conv1d_weight(c.T(64, 16, 3)),
                              dict(residual=c.T(2, 64, 8), pool2=True, want_amax=True), {}),
    "conv1d_res_second": lambda c: ("conv1d", c.T(2, 16, 16), c.ops.conv1d_weight(c.T(64, 16, 3)),
                                    dict(residual=c.T(2, 64, 16), act_out=COPY, res_second=True, dilation=2), {}),
    "conv2d_f32": lambda c: ("conv2d", c.T(2, 16, 8, 8), c.direct(16, 64, 3, 3, impl="f32"),
                             dict(bias=c.T(64), coef=c.T(2, 16, 3), act=ELU, residual=c.T(2, 64, 8, 8), act_out=ELU), {}),
    "conv2d_f32_out": lambda c: ("conv2d", c.T(2, 16, 8, 8), c.direct(16, 64, 3, 3, impl="f32"), dict(out=c.T(2, 64, 8, 8), dilation=2), {}),
    "conv3d_f32": lambda c: ("conv3d", c.T(2, 16, 2, 4, 4), c.direct(16, 32, 3, 3, 3, impl="f32"),
                             dict(bias=c.T(32), residual=c.T(2, 32, 2, 4, 4), act_out=ELU, raw=False), {}),
    "conv2d_wino_f32": lambda c: ("conv2d_wino", c.T(2, 8, 8, 16), c.ops.conv_wino_weight(c.T(64, 8, 3, 3)),
                                  dict(bias=c.T(64), residual=c.T(2, 64, 8, 16), act_out=ELU), {}),
    "conv3x3_thin": lambda c: ("conv3x3_thin", c.T(2, 1, 4, 4), c.T(8, 1, 3, 3), dict(bias=c.T(8), coef=c.T(2, 1, 3)), {}),
}


def _observe(ops, case):
    """run one case with ops.call wrapped -> what the wrapper handed the native entries and what it gave back"""
    import ctypes
    import torch
    fn, x, w, kw, patch = case(_Ctx(ops))
    named = [("x", x), ("weight", getattr(w, "blob", w))] + [(k, v) for k, v in kw.items() if isinstance(v, torch.Tensor)]
    raw_calls, saved = [], {k: getattr(ops, k) for k in list(patch) + ["call", "CONV_TRACE"]}
    real = ops.call

    def spy(name, *args):
        row = []
        for a in args:
            if isinstance(a, ctypes.c_void_p):
                row.append(("ptr", a.value))
            elif hasattr(a, "_obj"):                     # ctypes.byref(ConvExt)
                row.append(("ext", {f: getattr(a._obj, f) for f, _ in a._obj._fields_}))
            else:
                row.append(("val", a))
        raw_calls.append((name, row))
        return real(name, *args)

    out_given = kw.get("out")
    v0 = None if out_given is None else out_given._version
    try:
        for k, v in patch.items():
            setattr(ops, k, v)
        ops.call, ops.CONV_TRACE = spy, []
        res = getattr(ops, fn)(x, w, **kw)
        trace = [{k: v for k, v in r.items() if k not in ("e0", "e1")} for r in ops.CONV_TRACE]
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)
    torch.cuda.synchronize()
    results = list(res) if isinstance(res, tuple) else [res]
    for label, t in zip(("out", "out_act"), results):
        if t is None:
            continue
        if t is not out_given:
            named.append((label, t))
        if hasattr(t, "_ipdm_amax"):
            named.append(("slot_" + label, t._ipdm_amax[0]))
        if hasattr(t, "_ipdm_partials"):
            named.append(("part", t._ipdm_partials[0]))

    def where(p):
        if p is None:
            return None
        for label, t in named:
            if t.data_ptr() <= p < t.data_ptr() + max(t.untyped_storage().nbytes() - (t.data_ptr() - t.untyped_storage().data_ptr()), 1):
                return f"{label}+{p - t.data_ptr()}"
        return "fresh"                                   # allocated inside the wrapper and gone: split-K work, measured maxima

    calls = []
    for name, row in raw_calls:
        args = []
        for i, (kind, v) in enumerate(row):
            if kind == "ptr":
                args.append("stream" if i == len(row) - 1 else where(v))
            elif kind == "ext":
                args.append({f: where(x_) if f in ("in_amax", "out_amax", "act_amax") else x_ for f, x_ in v.items()})
            else:
                args.append(v)
        calls.append([name, args])
    got = dict(calls=calls, trace=trace, tuple=isinstance(res, tuple),
               results=[None if t is None else dict(shape=list(t.shape), amax=hasattr(t, "_ipdm_amax"),
                                                    amax_valid=ops.amax_of(t) is not None, partials=hasattr(t, "_ipdm_partials"),
                                                    is_out=t is out_given, version=t._version) for t in results],
               out_version_moved=None if out_given is None else out_given._version != v0)
    return json.loads(json.dumps(got))


@pytest.fixture(scope="module")
def want():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_names_every_case(want):
    assert len(want["parent_commit"]) == 40
    assert sorted(want["cases"]) == sorted(CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_wrapper_calls_as_before_the_frame(name, want):
    from inverseproblemwithdiffusionmodel_amd import ops
    got, was = _observe(ops, CASES[name]), want["cases"][name]
    assert [c[0] for c in got["calls"]] == [c[0] for c in was["calls"]]
    for g, w in zip(got["calls"], was["calls"]):
        assert g == w, (name, g[0])
    assert got == was


if __name__ == "__main__":
    assert sys.argv[1] == "--record"
    repo, commit, out = (sys.argv[sys.argv.index(f) + 1] for f in ("--repo", "--commit", "--out"))
    assert len(commit) == 40, "the full hash of the commit the tree was built from"
    sys.path.insert(0, os.path.abspath(repo))
    from inverseproblemwithdiffusionmodel_amd import ops
    assert os.path.abspath(ops.__file__).startswith(os.path.abspath(repo))
    with open(out, "w") as f:
        json.dump(dict(parent_commit=commit, cases={name: _observe(ops, CASES[name]) for name in sorted(CASES)}), f, indent=0)
    print(out, os.path.getsize(out), "bytes")
