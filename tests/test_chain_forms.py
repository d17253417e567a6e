"""CPU check of the forms the fused SharedMLP node (pytorch_utils._FusedMLPChain) runs its first and
last layers in at the network's real shapes (ScanNet, B = 8).  pytorch_utils.chain_forms asks only
host-side shape gates of the library, so CPU tensors of the right shapes stand in for the GPU ones."""
import importlib

import pytest
import torch

from conftest import load_pkg

B = 8


def _forms():
    load_pkg()
    return importlib.import_module("pointnet2.pytorch_utils")


def _weights(widths):
    return [torch.empty(o, i) for i, o in zip(widths[:-1], widths[1:])]


@pytest.fixture(autouse=True)
def _default_thresholds(monkeypatch):
    monkeypatch.delenv("MLP_POOL_GRAM256_MIN_CHUNKS", raising=False)
    monkeypatch.delenv("MLP_FIRST4_VIRTUAL", raising=False)
    monkeypatch.delenv("MLP_SMALL_GEMM_COLS", raising=False)


def test_sa1_forms():
    U = _forms()
    x = torch.empty(B, 4, 2048, 64)  # the grouped (xyz, height) tensor: no gradient
    ws = _weights([4, 64, 64, 128])
    # training: layer 0 virtual, layers 1 + 2 chained, the last raw output left to the Gram backward
    assert U.chain_forms(ws, x, None, True, True, False) == ("chained", "gram")
    assert U.chain_forms(ws, x, None, False, True, False) == ("virtual", "apply")
    assert U.chain_forms(ws, x, None, True, True, True) == ("plain", "gram")  # (input with a gradient)
    assert U.chain_forms(ws, x, None, True, False, False) == ("plain", "bn_relu_pool")  # eval


@pytest.mark.parametrize("name,n,m,ns,widths,last", [
    ("SA2", 2048, 1024, 32, [131, 128, 128, 256], "gram"),   # 8192 32-column chunks
    ("SA3", 1024, 512, 16, [259, 128, 128, 256], "extrema"),  # 2048: below the Gram-256 threshold
    ("SA4", 512, 256, 16, [259, 128, 128, 256], "extrema"),
    ("vote aggregation", 1024, 256, 16, [259, 128, 128, 128], "extrema"),
])
def test_pregathered_forms(name, n, m, ns, widths, last):
    U = _forms()
    pre = U.Pregathered(torch.empty(B, m, ns, dtype=torch.int32), None, n)
    x = torch.empty(B, widths[0], n + m)  # src_ext: the n points, then the m centroids
    ws = _weights(widths)
    assert U.chain_forms(ws, x, pre, True, True, True) == ("pregathered", last), name
    assert U.chain_forms(ws, x, pre, True, False, True) == ("pregathered", "bn_relu_pool"), name


def test_iou_branch_interpolated_form():
    U = _forms()
    k, g3 = 256, 64  # proposals, grid points per proposal
    pre = U.Interpolated(None, None, None, (B, 128, k, g3))
    x = torch.empty(B, 256, 1024)  # the seeds' features
    ws = _weights([259, 128, 128, 128])
    assert U.chain_forms(ws, x, pre, True, True, False) == ("interpolated", "extrema")
    assert U.chain_forms(ws, x, pre, True, False, False) == ("interpolated", "bn_relu_pool")


def test_gram256_threshold_moves_the_forward_decision(monkeypatch):
    U = _forms()
    pre = U.Pregathered(torch.empty(B, 512, 16, dtype=torch.int32), None, 1024)
    x = torch.empty(B, 259, 1024 + 512)
    ws = _weights([259, 128, 128, 256])
    monkeypatch.setenv("MLP_POOL_GRAM256_MIN_CHUNKS", "64")
    assert U.chain_forms(ws, x, pre, True, True, True) == ("pregathered", "gram")
