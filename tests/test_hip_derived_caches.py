"""The parameter-derived caches (gkgnet_amd/derived.py) on the device: a Grapher + FFN pair in bf16 inference must compute, after its
weights and running statistics moved, exactly what it computes with every cache emptied — on the vendor-GEMM path (bf16 / BN-folded
weight copies), with the fused aggregation + grouped projection (its fragment array) and with the own bf16 projection kernel (its
fragment arrays and the eval-mode BN coefficients)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _pair():
    from gkgnet_amd import layers
    from gkgnet_amd.backbone import FFN
    from gkgnet_amd.grapher import Grapher
    from tests.util import keyed_fill_
    layers.norm_cfg["type"] = "BN"                                # the guarded norm classes: they carry the statistics epoch
    torch.manual_seed(0)
    C, H = 32, 6
    g = Grapher(C, 9, 1, "mr", "gelu", "batch", True, False, 0.2, 1, n=H * H, drop_path=0.0, relative_pos=True,
                use_multi_group=True, num_group=4)
    ffn = FFN(C, 4 * C, act="gelu")
    for m in (g, ffn):
        sd = m.state_dict()
        keyed_fill_(sd)
        m.load_state_dict(sd)
        m.cuda().eval()
    x = torch.randn(2, C, H, H, device="cuda").to(memory_format=torch.channels_last)
    return g, ffn, x


@pytest.mark.parametrize("lin_bf16,mr_gemm", [(False, True), (True, True), (False, False)], ids=["mr_gemm", "lin_bf16+mr_gemm", "vendor"])
def test_outputs_follow_the_parameters_as_if_nothing_were_cached(lin_bf16, mr_gemm, monkeypatch):
    from gkgnet_amd import derived, fused
    monkeypatch.setattr(fused, "LIN_BF16", lin_bf16)
    monkeypatch.setattr(fused, "MR_GEMM", mr_gemm)
    derived.clear()
    g, ffn, x = _pair()

    def forward():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return ffn(g(x)).float().clone()
    y0 = forward()
    # the entries this configuration reads are there to go stale
    grouped = g.graph_conv.gconv.nn[0]
    assert derived.peek(ffn.fc1[0], "lin_planes" if lin_bf16 else "folded") is not None
    assert derived.peek(grouped, "mr_planes" if mr_gemm else "w16") is not None
    weights = [p for m in (g, ffn) for p in m.parameters() if p.dim() == 4]
    for p in weights:
        p.grad = torch.randn_like(p)
    torch.optim.AdamW(weights, lr=0.05, fused=True).step()        # moves no version counter (tests/test_param_staleness.py)
    g.train(), ffn.train()
    with torch.no_grad():
        ffn(g(3.0 * x + 1.0))                                     # the running statistics move, through raw pointers
    g.eval(), ffn.eval()
    y1 = forward()
    derived.clear()
    assert derived.peek(grouped, "mr_planes" if mr_gemm else "w16") is None
    y2 = forward()
    assert bool(torch.isfinite(y1).all())
    assert torch.equal(y1, y2), float((y1 - y2).abs().max())
    assert not torch.equal(y0, y1)
