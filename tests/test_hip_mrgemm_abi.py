"""gkg_mr_linear_bf16 / gkg_mr_linear_bf16_nn16 (csrc/gkg_mrgemm.hip) through the C ABI, with the test's own operands: the weight
fragments are built here from the header's description ([4][ci_pad/8][co_pad][8] bf16, fragment (q, f, n) = W[q co + n][8f .. 8f+7],
zero outside ci / co; include/gkg_hip.h), not by the package's plane builder, and every output sits between guard bands.

REFERENCE.  m from tests/mr_ref.py (exact); the reference's interleave [x_0, m_0, x_1, m_1, ...] (torch_vertex.py:57-61) rounded to
bf16; Conv2d(2C, 2C, 1, groups=4) with the bf16-rounded weight in fp64; a y + c; exact erf-GELU in fp64 (act 1).
BAR.  The one tests/test_hip_mrgemm.py already holds this kernel to: every element |got - want| <= 2^-7 |want| + 1e-3 (bf16 output
of an fp32 accumulation: one bf16 ulp plus an absolute floor).  NaN positions of reference and kernel must be identical; where the
reference is +-inf the kernel must give that infinity.  Each case prints its largest err / tol under ``pytest -s`` (figures:
EXPERIMENTS.md "max-relative forward at the C ABI").

Shapes (B, G, C, N, M or self, k), after the dispatch at the end of gkg_mrgemm.hip:
    (1, 2, 16, 64, self, 3)      narrow; ci = 8 padded to 16; one tile on one XCD
    (2, 2, 80, 150, self, 9)     narrow; ci = 40 -> 48, co = 40 -> 64; 300 tokens: a tile straddling two images, a ragged last tile
    (3, 2, 160, 100, 25, 9)      all four conv groups per workgroup, three blocks per wave; bipartite
    (2, 8, 192, 70, self, 18)    LDS image above 64 KB with the index rows: one conv group per workgroup; the k = 18 instantiation
    (2, 3, 288, 100, self, 9)    G = 3
    (1, 8, 768, 70, self, 1)     widest C; k = 1
    (1, 2, 64, 65, 40, 64)       largest k
Each in kinds 'normal' (out-of-range list entries: clamped) and 'nonfinite', with int64 and u16 lists, act 0 and 1, ldo = 2C and
ldo = 2C + 8 (the extra columns stay untouched)."""
import math

import numpy as np
import pytest
import torch

import mr_ref as R
from util import Buf

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2, 16, 64, None, 3), (2, 2, 80, 150, None, 9), (3, 2, 160, 100, 25, 9), (2, 8, 192, 70, None, 18),
          (2, 3, 288, 100, None, 9), (1, 8, 768, 70, None, 1), (1, 2, 64, 65, 40, 64)]


def _L():
    from gkgnet_amd import _lib
    return _lib


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    from gkgnet_amd.ops import _stream
    return _stream()


def build_planes(W, C):
    """W (2C, C/2) fp32, the grouped convolution's weight in the reference's layout -> the fragment array of the header, bf16."""
    ci = co = C // 2
    ci_pad, co_pad = (ci + 15) // 16 * 16, (co + 31) // 32 * 32
    P = torch.zeros(4, co_pad, ci_pad, dtype=torch.bfloat16)
    P[:, :co, :ci] = W.bfloat16().view(4, co, ci)
    P = P.view(4, co_pad, ci_pad // 8, 8).permute(0, 2, 1, 3).contiguous()      # [q][f][n][8]
    assert P.numel() * 2 == _L().load().gkg_mr_linear_planes_bytes(C)
    return P


def operands(C, seed):
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(2 * C, C // 2, generator=g) / math.sqrt(C // 2)
    a = torch.rand(2 * C, generator=g) + 0.5
    c = torch.randn(2 * C, generator=g) * 0.2
    return W, a, c


def definition(case, lists, W, a, c):
    """-> z = a y + c (T, 2C) in fp64, before the activation."""
    B = case["shape"][0]
    m = R.mr_fwd(case["x"], case["src"], case[lists], case["M"])[0]
    x_tm, m_tm = torch.from_numpy(R.to_tm(case["x"], B)), torch.from_numpy(R.to_tm(m, B))
    C = x_tm.shape[-1]
    u = torch.stack([x_tm, m_tm], dim=-1).reshape(-1, 4, C // 2).bfloat16().double()          # (T, q, ci) interleaved [x, m]
    Wq = W.bfloat16().double().view(4, C // 2, C // 2)                                        # (q, co, ci)
    y = torch.einsum("tqi,qoi->tqo", u, Wq).reshape(-1, 2 * C)
    return a.double() * y + c.double()


def gelu64(z):
    return 0.5 * z * (1.0 + torch.erf(z * math.sqrt(0.5)))


def judge(got, want, what):
    """The bar.  -> largest err / tol over the finite elements."""
    got = got.double()
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), f"{what}: NaN at {int((gn != wn).sum())} different places ({int(gn.sum())} got, {int(wn.sum())} wanted)"
    inf = torch.isinf(want)
    assert torch.equal(got[inf], want[inf]), f"{what}: infinities differ"
    fin = ~(wn | inf)
    ratio = (got[fin] - want[fin]).abs() / (2.0 ** -7 * want[fin].abs() + 1e-3)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    assert worst <= 1.0, f"{what}: err / tol = {worst:.3f} at {int((ratio > 1).sum())} elements"
    return worst


@pytest.mark.parametrize("kind", ("normal", "nonfinite"))
@pytest.mark.parametrize("shape", SHAPES, ids=R.shape_id)
def test_fused_aggregation_projection_through_the_c_abi(shape, kind):
    L = _L()
    B, G, C, N, M_, k = shape
    M, T = (N if M_ is None else M_), B * N
    case = R.make_case((B, G, C // G, N, M_, k), kind)
    W, a, c = operands(C, seed=C + N)
    planes, a_dev, c_dev = build_planes(W, C).cuda(), a.cuda(), c.cuda()
    x_dev = torch.from_numpy(R.to_tm(case["x"], B)).cuda()
    src_dev = None if case["src"] is None else torch.from_numpy(R.to_tm(case["src"], B)).cuda()
    worst = {}
    for lists in ("idx", "idx16"):
        z = definition(case, lists, W, a, c)
        if kind == "nonfinite":
            assert torch.isnan(z).any() and (k < 2 or torch.isinf(z).any())
        want = {0: z, 1: gelu64(z)}
        u16 = lists == "idx16"
        fn = L.load().gkg_mr_linear_bf16_nn16 if u16 else L.load().gkg_mr_linear_bf16
        lists_dev = (torch.from_numpy(case[lists].astype(np.uint16).view(np.int16)) if u16 else torch.from_numpy(case[lists])).cuda()
        for act in (0, 1):
            for ldo in (2 * C, 2 * C + 8):
                out = Buf((T, ldo), torch.bfloat16)
                what = f"{fn.__name__} act={act} ldo={ldo}"
                L.check(fn(_p(x_dev), _p(src_dev), _p(lists_dev), _p(planes), _p(a_dev), _p(c_dev), _p(out.t), ldo, B, G, C // G, N, M, k,
                           act, _st()), what)
                torch.cuda.synchronize()
                assert out.guards_ok(), what + ": wrote outside its output"
                got = out.cpu()
                assert bool(torch.isnan(got[:, 2 * C:]).all()), what + ": wrote beyond column 2C"
                worst[(lists, act)] = max(worst.get((lists, act), 0.0), judge(got[:, :2 * C], want[act], what))
    print(f"mr_linear_bf16 {R.shape_id(shape)} {kind}: max err/tol " + ", ".join(f"{l} act{a_}: {v:.3f}" for (l, a_), v in worst.items()))


def test_rejected_calls_return_the_documented_code_and_write_nothing():
    L = _L()
    K = L._K
    SHAPE, UNSUP = K["ERR_SHAPE"], K["ERR_UNSUPPORTED"]
    # (what, entry point, B, G, c, N, M, k, ldo - 2C, code); every buffer has the size the call describes
    table = [("k = 65", "gkg_mr_linear_bf16", 1, 2, 8, 70, 70, 65, 0, SHAPE),
             ("C = 784", "gkg_mr_linear_bf16", 1, 2, 392, 8, 8, 3, 0, UNSUP),
             ("ldo % 8 != 0", "gkg_mr_linear_bf16", 1, 2, 8, 8, 8, 3, 4, SHAPE),
             ("ldo < 2C", "gkg_mr_linear_bf16", 1, 2, 8, 8, 8, 3, -8, SHAPE),
             ("M = 65537 with u16 lists", "gkg_mr_linear_bf16_nn16", 1, 2, 8, 8, 65537, 3, 0, UNSUP)]
    for what, name, B, G, c, N, M, k, dl, code in table:
        C = G * c
        x = torch.zeros(B, N, C, device="cuda")
        src = torch.zeros(B, M, C, device="cuda")
        u16 = name.endswith("nn16")
        lists = torch.zeros((B * G, N, k), dtype=torch.int16 if u16 else torch.int64, device="cuda")
        planes = torch.zeros(max(int(L.load().gkg_mr_linear_planes_bytes(C)), 16), dtype=torch.uint8, device="cuda")
        ac = torch.ones(2 * C, device="cuda")
        out = Buf((B * N, 2 * C + 8), torch.bfloat16)
        rc = getattr(L.load(), name)(_p(x), _p(src), _p(lists), _p(planes), _p(ac), _p(ac), _p(out.t), 2 * C + dl, B, G, c, N, M, k, 1, _st())
        torch.cuda.synchronize()
        assert rc == code, f"{name}: {what}: returned {rc}, documented {code}"
        assert bool(torch.isnan(out.full).all()), f"{name}: {what}: output written"
