"""GKG_ENABLE=wgrad_det at module level: under GKG_DETERMINISTIC a Grapher -> GrapherLabel step takes every projection's weight
gradient through the run-independent x6 entry points (no vendor GEMM, no un-permute pass, no atomic kernel), repeats bit for bit,
agrees with today's deterministic path — and without GKG_DETERMINISTIC the switch changes no launch."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ENTRIES = ("gkg_linear_wgrad_x6", "gkg_linear_wgrad_x6_batch", "gkg_linear_wgrad_x6_det", "gkg_linear_wgrad_x6_batch_det")


class _Step:
    """One Grapher (C = 64, G = 2, k = 9) -> GrapherLabel pair in train mode with its gradients in a GradBucket; ``run`` does one
    forward + backward from the same parameters and inputs and returns {parameter name: gradient}.  Every slot holds 7.0 when
    the backward starts: a kernel that added into its slot instead of overwriting it would show."""

    def __init__(self, H, B, L):
        from gkgnet_amd import parallel
        from gkgnet_amd.grapher import Grapher, GrapherLabel
        torch.manual_seed(3)
        C = 64
        self.g = Grapher(C, 9, 1, "mr", "gelu", "batch", True, False, 0.2, 1, n=H * H, relative_pos=True, use_multi_group=True,
                         num_group=2).cuda().train()
        self.gl = GrapherLabel(C, 9, 1, "mr", "gelu", "batch", True, False, 0.2, 1, n=H * H, relative_pos=False, num_nodes=L,
                               use_multi_group=True, num_group=2).cuda().train()
        self.named = [("g." + n, p) for n, p in self.g.named_parameters()] + [("gl." + n, p) for n, p in self.gl.named_parameters()]
        self.bucket = parallel.GradBucket([p for _, p in self.named])
        self.x = torch.randn(B, C, H, H, device="cuda").requires_grad_(True)
        self.e = torch.randn(B, L, C, device="cuda").requires_grad_(True)
        self.cx, self.ce = torch.randn(B, C, H, H, device="cuda"), torch.randn(B, L, C, device="cuda")

    def run(self):
        from gkgnet_amd.wgrad_queue import QUEUE
        self.bucket.flat.fill_(7.0)
        self.bucket.release()
        self.x.grad = None
        self.e.grad = None
        out = self.g(self.x)
        e2, _ = self.gl(self.e, out)
        torch.autograd.backward([out, e2], [self.cx, self.ce])
        self.bucket.pack()
        torch.cuda.synchronize()
        assert not QUEUE.items and not QUEUE.keep
        return {n: p.grad.detach().clone() for n, p in self.named if p.requires_grad}


class _Calls:
    """Counting wrappers: the four weight-gradient entry points of the library (with the number of problems of a batch),
    fused._wgrad / _wgrad_grouped (one call per projection), torch.bmm and fused._kperm_grad_back."""

    def __init__(self, monkeypatch):
        from gkgnet_amd import _lib, fused
        lib = _lib.load()
        self.log, self.projections, self.bmm, self.unpermute = [], 0, 0, 0
        for name in ENTRIES:
            real = getattr(lib, name)

            def entry(*a, _real=real, _name=name):
                self.log.append((_name, a[1]) if "batch" in _name else (_name,))
                return _real(*a)
            monkeypatch.setattr(lib, name, entry)
        for name in ("_wgrad", "_wgrad_grouped"):
            real = getattr(fused, name)

            def proj(*a, _real=real, **k):
                self.projections += 1
                return _real(*a, **k)
            monkeypatch.setattr(fused, name, proj)
        real_bmm, real_back = torch.bmm, fused._kperm_grad_back

        def bmm(*a, **k):
            self.bmm += 1
            return real_bmm(*a, **k)

        def back(*a, **k):
            self.unpermute += 1
            return real_back(*a, **k)
        monkeypatch.setattr(torch, "bmm", bmm)
        monkeypatch.setattr(fused, "_kperm_grad_back", back)

    def reset(self):
        self.log, self.projections, self.bmm, self.unpermute = [], 0, 0, 0

    def problems(self, *names):
        return sum((c[1] if len(c) > 1 else 1) for c in self.log if c[0] in names)


def _switches(monkeypatch, det, sw):
    from gkgnet_amd import fused
    monkeypatch.setattr(fused, "GEMM_MATH", "x6")
    monkeypatch.setattr(fused, "DETERMINISTIC", det)
    monkeypatch.setattr(fused, "WGRAD_DET", sw)


# the issue's shapes (162 and 40 rows: ragged, every dW its own call) and whole 128-row units (2048 rows: the deferred batch)
@pytest.mark.parametrize("H,B,L", [(9, 2, 20), (16, 8, 24)], ids=["ragged", "units"])
def test_deterministic_step_stays_on_the_x6_kernels_and_repeats(monkeypatch, H, B, L):
    from gkgnet_amd import fused
    step = _Step(H, B, L)
    _switches(monkeypatch, True, False)
    base = step.run()                                                   # today's deterministic path
    calls = _Calls(monkeypatch)
    _switches(monkeypatch, True, True)
    first = step.run()
    n_proj, log = calls.projections, list(calls.log)
    assert n_proj >= 6                                                  # fc1, grouped projection, fc2 of the Grapher; the label block's
    assert calls.problems("gkg_linear_wgrad_x6_det", "gkg_linear_wgrad_x6_batch_det") == n_proj, log
    assert calls.problems("gkg_linear_wgrad_x6", "gkg_linear_wgrad_x6_batch") == 0, log
    assert calls.bmm == 0 and calls.unpermute == 0
    if H * H * B % 128 == 0 and fused.WGRAD_BATCH:
        assert calls.problems("gkg_linear_wgrad_x6_batch_det") >= 3, log        # the token-side projections ride in the batch
    second = step.run()
    assert first.keys() == second.keys() == base.keys()
    for n in first:
        assert torch.isfinite(first[n]).all(), n
        assert torch.equal(first[n], second[n]), n
    # against today's deterministic path: the project's module bar on every weight gradient (and nothing else moved)
    for n, g in base.items():
        tol = 1e-3 * float(g.abs().max())
        assert float((first[n] - g).abs().max()) <= tol, (n, float((first[n] - g).abs().max()), tol)


def test_without_deterministic_the_switch_changes_nothing(monkeypatch):
    step = _Step(16, 8, 24)
    calls = _Calls(monkeypatch)
    logs = []
    for sw in (False, True):
        _switches(monkeypatch, False, sw)
        calls.reset()
        grads = step.run()
        assert all(torch.isfinite(g).all() for g in grads.values())
        logs.append(list(calls.log))
    assert logs[0] == logs[1] and logs[0]
    assert all("_det" not in c[0] for c in logs[1])
