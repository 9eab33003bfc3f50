"""The BatchNorm passes' call trace (host only, no GPU).  The Python side of a BN layer computes nothing itself: what it does is
the ordered list of library entry points it calls and their arguments.  A recording stand-in for the library drives the three
autograd Functions of gkgnet_amd/fused.py (``.apply``, then the backward) on CPU tensors through every launch sequence a layer
can take — projection arithmetic, GKG_DETERMINISTIC, a statistics group, DropPath scale, the NCHW / dual / XM / k-NN-preparing
outputs, a two-layer chain that hands statistics over, frozen BN with and without wanted gradients — and this test compares each
case's text with tests/bn_trace/expected.txt.  A change to the host code that is meant to keep its launches leaves that file
byte-identical.

    python tests/test_bn_passes_trace_host.py <checkout>

prints the text for the package in that checkout (its root directory; default: this one): that is how expected.txt is made —
from the commit BEFORE a restructuring, whose ``.apply`` signatures are the same.

What is recorded: every call but the weight-plane preparation (gkg_x6_*), the ``*_supported`` queries and
gkg_linear_stats_doubles (cached per process: they would tie a case's text to the cases before it).  Integers and floats verbatim;
a pointer (the header's ``void*`` arguments) by the known tensor it falls inside plus its byte offset — the case's inputs,
parameters and BN buffers, the two halves of the fp64 scratch pair —, ``null``, or ``buf`` for anything the call allocated; behind
a call, the label _lib.check would report its failure under (tests inject failures by that label).

Every BN entry point is reached (test_every_bn_entry_point_is_reached lists them); nothing had to be left out."""
from __future__ import annotations

import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = os.path.join(ROOT, "tests", "bn_trace", "expected.txt")
if __name__ == "__main__" and len(sys.argv) > 1:
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
elif ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch                                                     # noqa: E402

B, N, CIN, COUT = 2, 64, 32, 64
R = B * N
NCHW = (B, COUT, 8, 8)
_SKIP = ("gkg_x6_", "gkg_linear_stats_doubles")


class _Group:
    """Stands in for a process group (fused._sync_group is patched to return it; all_reduce is a no-op)."""


class _Recorder:
    """The library: answers 0 (1 for ``*_supported``, 1024 for ``*_bytes``, 32768 for gkg_linear_stats_doubles) and writes down
    what it was asked."""

    def __init__(self, protos, known, scratch):
        self.protos, self.known, self.scratch, self.lines = protos, known, scratch, []
        self.open = False                                        # the last line still waits for its _lib.check label

    def _name(self, p):
        if not p:
            return "null"
        named = list(self.known.items())
        inst = self.scratch._inst.get(("cpu", None))
        if inst is not None:
            named += [("scratch0", inst.store[0]), ("scratch1", inst.store[1])]
        for name, t in named:
            base = t.data_ptr()
            if base <= p < base + t.numel() * t.element_size():
                return "%s+%d" % (name, p - base)
        return "buf"

    def __getattr__(self, entry):
        if not entry.startswith("gkg_"):
            raise AttributeError(entry)
        rc = 1 if entry.endswith("_supported") else 1024 if entry.endswith("_bytes") else 32768 if entry.endswith("_doubles") else 0

        def call(*args):
            self.open = False
            if entry.startswith(_SKIP) or entry.endswith("_supported"):
                return rc
            argtypes = self.protos[entry][1]
            assert len(args) == len(argtypes), (entry, len(args), len(argtypes))
            text = [self._name(a) if ty is C.c_void_p else repr(a) for a, ty in zip(args, argtypes)]
            self.lines.append("%s(%s)" % (entry, ", ".join(text)))
            self.open = True
            return rc
        return call

    def check(self, rc, what):
        """_lib.check: the label a failure of the call just made would be reported under (tests inject failures by it)."""
        assert rc == 0
        if self.open:
            self.lines[-1] += " as %r" % what
            self.open = False


class _Env:
    """One case's world: its named tensors, the switches, the stubs; everything put back on exit."""

    def __init__(self, math="x6", det=False, group=False):
        self.known, self.undo = {}, []
        self.math, self.det, self.group = math, det, group

    def set(self, obj, name, value):
        self.undo.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    def __enter__(self):
        import torch.distributed as dist
        from gkgnet_amd import _abi, _lib, bn_scratch, fused, planes
        self._clear = lambda: [d.clear() for d in (bn_scratch._BnScratch._inst, planes._PLANES, fused._STATS, fused._SK)]
        self._clear()
        self.rec = _Recorder(_abi.header().protos, self.known, bn_scratch._BnScratch)
        self.set(_lib, "load", lambda: self.rec)
        self.set(_lib, "check", self.rec.check)
        for name, mod in list(sys.modules.items()):
            if name.startswith("gkgnet_amd.") and hasattr(mod, "_stream"):
                self.set(mod, "_stream", lambda: 0)
        self.set(torch.cuda, "is_current_stream_capturing", lambda: False)
        self.set(bn_scratch._BnScratch, "_current_stream", lambda self_: 0)
        self.set(bn_scratch._BnScratch, "_raw_stream", lambda self_: 0)
        self.set(dist, "all_reduce", lambda *a, **k: None)
        for name, value in (("GEMM_MATH", self.math), ("DETERMINISTIC", self.det), ("BWD_FUSE", True), ("DGRAD_STATS", True),
                            ("BN_EPILOGUE", True), ("BN_EPILOGUE_MIN_ROWS", 0), ("X6_WALK", True)):
            self.set(fused, name, value)
        if self.group:
            self.set(fused, "_sync_group", lambda bn: _Group if bn.training else None)
        return self

    def __exit__(self, *exc):
        for obj, name, old in reversed(self.undo):
            setattr(obj, name, old)
        self._clear()
        return False

    # ---- named tensors
    def t(self, name, *shape, grad=False):
        self.known[name] = torch.zeros(shape).requires_grad_(grad)
        return self.known[name]

    def layer(self, tag, cin, cout, train=True, bias=True, track=True, learn=True):
        """conv weight (cout, cin, 1, 1) (+ bias) and a BatchNorm2d(cout) -> (weight, bias, gamma, beta, bn)."""
        w = self.t(tag + ".W", cout, cin, 1, 1, grad=True)
        b = self.t(tag + ".bias", cout, grad=learn) if bias else None
        bn = torch.nn.BatchNorm2d(cout, track_running_stats=track).train(train)
        bn.weight.requires_grad_(learn)
        bn.bias.requires_grad_(learn)
        for nm in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked"):
            if getattr(bn, nm) is not None:
                self.known["%s.bn.%s" % (tag, nm)] = getattr(bn, nm)
        return w, b, bn.weight, bn.bias, bn


def _backward(outs):
    outs = [o for o in (outs if isinstance(outs, tuple) else (outs,)) if o.requires_grad]
    torch.autograd.backward(outs, [torch.zeros(o.shape) for o in outs])


def _lin(env, tag="l", x=None, cin=CIN, cout=COUT, act=1, residual=None, nchw=None, out_lowp=False, scale=None, rps=0,
         dual=False, xm=None, knn=None, **layer):
    """_LinearBNAct.apply with its eighteen positionals."""
    from gkgnet_amd import fused
    w, b, gamma, beta, bn = env.layer(tag, cin, cout, **layer)
    x = env.t(tag + ".x", R, cin, grad=True) if x is None else x
    return fused._LinearBNAct.apply(x, w, b, gamma, beta, residual, bn, act, nchw, out_lowp, None, scale, rps, False, False, dual,
                                    xm, knn)


def _knn(as_keys=0):
    from gkgnet_amd import _lib, knn_prep
    p = knn_prep.KnnProblem(B, 4, COUT // 4, N, N, 9, 1, bool(as_keys), None, True, _lib.KNN_NORMALIZE)
    p.as_keys = as_keys
    return p


# ---- the cases: name -> (switches, body(env) -> outputs to run the backward from, or None: forward only)
def _c_plain(env):
    return _lin(env)


def _c_eval(env):
    return _lin(env, train=False)


def _c_eval_no_bias(env):
    return _lin(env, train=False, bias=False)


def _c_eval_frozen_params(env):
    return _lin(env, train=False, learn=False)


def _c_eval_scale(env):
    return _lin(env, train=False, scale=env.t("scale", B), rps=N)


def _c_notrack(env):
    return _lin(env, train=False, track=False)


def _c_lowp_forward(env):
    _lin(env, out_lowp=True)


def _c_scale(env):
    return _lin(env, scale=env.t("scale", B), rps=N)


def _c_residual(env):
    return _lin(env, act=0, residual=env.t("res", R, COUT, grad=True))


def _c_nchw(env):
    return _lin(env, act=0, residual=env.t("res", *NCHW, grad=True), nchw=NCHW)


def _c_nchw_scale(env):
    return _lin(env, act=0, nchw=NCHW, scale=env.t("scale", B))


def _c_dual(env):
    return _lin(env, act=0, residual=env.t("res", R, COUT, grad=True), nchw=NCHW, dual=True)


def _c_dual_keys(env):
    return _lin(env, act=0, residual=env.t("res", R, COUT, grad=True), nchw=NCHW, dual=True, knn=_knn(1))


def _c_xm(env):
    return _lin(env, act=0, xm=(B, N))


def _c_xm_knn(env):
    return _lin(env, act=0, xm=(B, N), knn=_knn())


def _c_chain(env):
    h = _lin(env, "l1")
    return _lin(env, "l2", x=h, cin=COUT, cout=CIN, act=0)


def _grouped(env, act=1, **layer):
    from gkgnet_amd import fused
    XM = env.t("g.XM", R, 64, grad=True)
    w, b, gamma, beta, bn = env.layer("g", 16, 64, **layer)
    return fused._GroupedLinearBNAct.apply(XM, w, b, gamma, beta, bn, act, False, None)


def _c_grouped(env):
    return _grouped(env)


def _c_grouped_act0(env):
    return _grouped(env, act=0)


def _c_grouped_eval(env):
    return _grouped(env, train=False)


def _bnact(env, **layer):
    from gkgnet_amd import fused
    _, _, gamma, beta, bn = env.layer("s", CIN, COUT, bias=False, **layer)
    return fused._BNActTM.apply(env.t("s.Y", R, COUT, grad=True), gamma, beta, bn, 1)


def _c_bnact(env):
    return _bnact(env)


def _c_bnact_eval(env):
    return _bnact(env, train=False)


_BODIES = [("plain", _c_plain), ("eval", _c_eval), ("eval_no_bias", _c_eval_no_bias), ("eval_frozen_params", _c_eval_frozen_params),
           ("eval_scale", _c_eval_scale), ("notrack", _c_notrack), ("lowp_forward", _c_lowp_forward), ("scale", _c_scale),
           ("residual", _c_residual), ("nchw", _c_nchw), ("nchw_scale", _c_nchw_scale), ("dual", _c_dual), ("dual_keys", _c_dual_keys),
           ("xm", _c_xm), ("xm_knn", _c_xm_knn), ("chain", _c_chain), ("grouped", _c_grouped), ("grouped_act0", _c_grouped_act0),
           ("grouped_eval", _c_grouped_eval), ("bnact", _c_bnact), ("bnact_eval", _c_bnact_eval)]
_MODES = [("x6", dict()), ("x6_det", dict(det=True)), ("x6_group", dict(group=True)), ("x6_det_group", dict(det=True, group=True)),
          ("vendor", dict(math="vendor")), ("vendor_group", dict(math="vendor", group=True))]
CASES = [("%s.%s" % (mode, name), kw, body) for mode, kw in _MODES for name, body in _BODIES]


def trace() -> dict:
    """{case name: the case's text}, in CASES' order."""
    import gkgnet_amd.fused                                      # noqa: F401  (every module that binds _stream is loaded)
    cases = {}
    for name, kw, body in CASES:
        with _Env(**kw) as env:
            outs = body(env)
            if outs is not None:
                _backward(outs)
            cases[name] = "".join(ln + "\n" for ln in env.rec.lines)
    return cases


def text(cases: dict) -> str:
    return "".join("== case %s\n%s" % (name, body) for name, body in cases.items())


def _expected() -> dict:
    with open(EXPECTED) as fh:
        chunks = fh.read().split("== case ")[1:]
    return {c.partition("\n")[0]: c.partition("\n")[2] for c in chunks}


def test_bn_call_trace_matches_the_recorded_one():
    got, want = trace(), _expected()
    assert list(got) == list(want)
    bad = [name for name in got if got[name] != want[name]]
    for name in bad[:3]:
        print("== case %s (actual trace)\n%s== recorded\n%s" % (name, got[name], want[name]))
    assert not bad, "%d of %d cases differ from tests/bn_trace/expected.txt, first: %s" % (len(bad), len(want), bad[0])


def test_every_bn_entry_point_is_reached():
    """The coverage the recorded file must have: each BN entry point in at least one case, gkg_bn_eval_bwd in its three forms."""
    calls = [ln for body in _expected().values() for ln in body.splitlines()]
    seen = {ln.partition("(")[0] for ln in calls}
    want = {"gkg_bn_train_stats", "gkg_bn_stats_sums", "gkg_bn_finalize", "gkg_bn_eval_affine", "gkg_bn_apply_train",
            "gkg_bn_apply_train_sync", "gkg_bn_apply_train_dual", "gkg_bn_apply_train_dual_sync", "gkg_bn_apply_knn_prep",
            "gkg_bn_apply_knn_prep_sync", "gkg_bn_bwd", "gkg_bn_bwd_atomic", "gkg_bn_bwd_atomic_scaled", "gkg_bn_bwd_stats_f64",
            "gkg_bn_bwd_apply_sync", "gkg_bn_bwd_apply_from_sums", "gkg_bn_bwd_sums", "gkg_bn_bwd_apply", "gkg_bn_eval_bwd",
            "gkg_nchw_to_tm_add_bnstats", "gkg_bn_workspace_bytes"}
    assert want <= seen, sorted(want - seen)
    forms = set()
    for ln in calls:
        if ln.startswith("gkg_bn_eval_bwd("):
            args = ln[len("gkg_bn_eval_bwd("):ln.rindex(")")].split(", ")
            sums, ws = args[-6], args[-3]                        # ..., sums, zero_buf, zero_doubles, ws, ws_bytes, stream
            forms.add("pair" if sums.startswith("scratch") else "workspace" if ws == "buf" else "none")
            assert (sums == "null") or (ws == "null")
    assert forms == {"none", "pair", "workspace"}, forms


def test_bn_entry_points_have_one_python_caller():
    """gkg_bn_* and gkg_nchw_to_tm_add_bnstats are called from bn_passes.py only, which reads no switch of fused."""
    import re
    pkg = os.path.join(ROOT, "gkgnet_amd")
    call = re.compile(r"lib\.(gkg_bn_\w+|gkg_nchw_to_tm_add_bnstats)\(|getattr\(lib, \"gkg_bn_")
    callers = sorted(f for f in os.listdir(pkg) if f.endswith(".py") and call.search(open(os.path.join(pkg, f)).read()))
    assert callers == ["bn_passes.py"], callers
    src = open(os.path.join(pkg, "bn_passes.py")).read()
    assert not re.search(r"^\s*(from|import)\b.*\bfused\b", src, re.M)


if __name__ == "__main__":
    sys.stdout.write(text(trace()))
