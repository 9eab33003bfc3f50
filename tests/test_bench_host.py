"""Host-side pieces of bench.py that run without a GPU: the whole-backbone CPU baseline (a CPU copy of the network with the
graph operators routed to the oracle) and the workload tables."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_backbone_cpu_baseline_runs_forward_and_train_step_on_the_oracle():
    import bench
    from gkgnet_amd import layers
    from gkgnet_amd.backbone import GKGNet
    from gkgnet_amd.head import LabelQueryHead
    import gkgnet_amd.graph as graph
    layers.norm_cfg["type"] = "BN"
    torch.manual_seed(0)
    net = GKGNet(choice="t", k=4, k_label_gcn=4, n_classes=8, size=128)
    head = LabelQueryHead(8, GKGNet.arch_settings["t"]["channels"][-1])
    img = torch.randn(2, 3, 128, 128)
    tgt = (torch.rand(2, 8) < 0.3).float()
    real = graph.ops
    fwd = bench.cpu_baseline_backbone(net.eval(), None, img[:1], None, "forward", budget_s=0.5, threads=2)
    assert fwd["value"] > 0 and fwd["kind"] == "port" and fwd["cores"] == 2 and "oracle/torch_ref.py" in fwd["sample"]
    trn = bench.cpu_baseline_backbone(net.train(), head.train(), img, tgt, "train", budget_s=0.5, threads=2)
    assert trn["value"] > 0 and "backward" in trn["sample"]
    assert graph.ops is real                     # the operator swap is undone
    assert all(p.grad is None for p in net.parameters())      # the timed copy, not the caller's network, was stepped


def test_workload_tables_cover_every_baseline_config():
    import bench
    assert {"cfg2", "cfg2ref", "stage3", "stage1"} <= set(bench.WORKLOADS)
    assert set(bench.BACKBONE_WORKLOADS) == {"cfg3", "cfg4", "cfg5"}
    assert bench.BACKBONE_WORKLOADS["cfg5"]["kw"]["num_group"] == 8 and bench.BACKBONE_WORKLOADS["cfg5"]["B"] == 16
    assert bench.WORKLOADS["stage1"]["H"] ** 2 == 20736 and bench.WORKLOADS["stage1"]["r"] == 4


def test_dump_outputs_writes_float_arrays_within_the_budget(tmp_path):
    """--dump-outputs: float32 / float64 .npy files, whole arrays when they fit, a fixed seeded sample (the same positions in
    every run) when together they exceed the budget."""
    import numpy as np
    import bench
    small = dict(out=torch.randn(3, 4, dtype=torch.float64), edge=torch.arange(10))
    bench.dump_outputs(str(tmp_path / "a"), small)
    a = np.load(tmp_path / "a" / "out.npy")
    assert a.dtype == np.float32 and a.shape == (3, 4) and np.array_equal(a, small["out"].float().numpy())
    e = np.load(tmp_path / "a" / "edge.npy")
    assert e.dtype == np.float64 and np.array_equal(e, np.arange(10))
    big = dict(x=torch.randn(bench.DUMP_BUDGET_BYTES // 4 + 1000), y=torch.randn(7))
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), big)
    assert sum(os.path.getsize(p) for p in (tmp_path / "b").iterdir()) <= 64e6
    xb, xc = np.load(tmp_path / "b" / "x.npy"), np.load(tmp_path / "c" / "x.npy")
    assert xb.size < big["x"].numel() and np.array_equal(xb, xc)
    assert np.isin(xb, big["x"].numpy()).all()
    assert np.array_equal(np.load(tmp_path / "b" / "y.npy"), big["y"].numpy())
