"""CPU tests of the inference engine (votenet/inference.py): the BatchNorm folding it relies on, its
refusal of detectors it cannot serve, and the host-side shape gates of the one-pass eval kernels
(csrc/mlp_eval_pool.hip) at the network's call sites and just outside."""
import ctypes
import importlib
import os

import pytest
import torch

from conftest import load_pkg


def _lib():
    pkg = load_pkg()
    return ctypes.CDLL(os.path.join(os.path.dirname(pkg.__file__), "lib3dioumatch_hip.so"))


def test_bn_folding_matches_eval_batchnorm_in_float64():
    load_pkg()
    U = importlib.import_module("pointnet2.pytorch_utils")
    g = torch.Generator().manual_seed(0)
    c = 37
    bn = torch.nn.BatchNorm2d(c, eps=1e-5).double().eval()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(c, generator=g, dtype=torch.float64) * 2)  # some negative
        bn.bias.copy_(torch.randn(c, generator=g, dtype=torch.float64))
        bn.running_mean.copy_(torch.randn(c, generator=g, dtype=torch.float64) * 3 + 1)
        bn.running_var.copy_(torch.rand(c, generator=g, dtype=torch.float64) * 5 + 0.01)
    assert (bn.weight < 0).any()
    y = torch.randn(2, c, 5, 7, generator=g, dtype=torch.float64) * 4
    scale, shift = U.fold_bn_affine(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
    want = bn(y)
    got = y * scale.view(1, c, 1, 1) + shift.view(1, c, 1, 1)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    # ... and the max of the activation is the activation of the max or of the MIN (negative scale)
    pooled = torch.relu(want).amax(3)
    ext = torch.where(scale.view(1, c, 1) >= 0, y.amax(3), y.amin(3))
    torch.testing.assert_close(torch.relu(ext * scale.view(1, c, 1) + shift.view(1, c, 1)), pooled,
                               rtol=1e-12, atol=1e-12)


def test_engine_refuses_what_it_cannot_serve():
    load_pkg()
    V = importlib.import_module("3dioumatch_amd.votenet")
    step = importlib.import_module("3dioumatch_amd.votenet.step")
    I = importlib.import_module("3dioumatch_amd.votenet.inference")
    det = step.build_detector(V.scannet_config(), seed=0)
    assert det.training
    with pytest.raises(ValueError, match="eval mode"):
        I.InferenceEngine(det)
    with pytest.raises(ValueError, match="GPU"):
        I.InferenceEngine(det.eval())  # parameters on the CPU
    with pytest.raises(ValueError):
        I.InferenceEngine(torch.nn.Linear(3, 3).eval())


def test_eval_plan_refuses_layer_shapes_without_a_kernel():
    load_pkg()
    U = importlib.import_module("pointnet2.pytorch_utils")
    # (folding needs the GPU; the shape check comes first)
    with pytest.raises(ValueError):
        U.EvalPlan(U.SharedMLP([131, 128, 128], bn=True))       # two layers
    with pytest.raises(ValueError):
        U.EvalPlan(U.SharedMLP([131, 256, 256, 256], bn=True))  # 256 -> 256 tail: no kernel


def test_host_side_shape_gates_of_the_eval_kernels():
    lib = _lib()
    lin4 = lib.mlp_eval_lin4_supported
    assert lin4(8, 4, 64, 128, 2048, 64) == 1     # SA1, ScanNet
    assert lin4(16, 4, 64, 128, 2048, 64) == 1    # SA1, SUN RGB-D
    assert lin4(1, 4, 64, 128, 2048, 32) == 1
    assert lin4(2, 4, 64, 128, 2048, 16) == 1
    assert lin4(8, 4, 64, 128, 2047, 64) == 0     # m * ns not a multiple of 256
    assert lin4(8, 4, 64, 128, 2048, 24) == 0     # nsample not supported
    assert lin4(8, 4, 64, 128, 2048, 128) == 0
    assert lin4(8, 5, 64, 128, 2048, 64) == 0     # wrong channel counts
    assert lin4(8, 4, 64, 256, 2048, 64) == 0
    assert lin4(0, 4, 64, 128, 2048, 64) == 0     # b = 0
    assert lin4(4096, 4, 64, 128, 1 << 16, 64) == 0  # m * ns * b beyond range
    st = lib.mlp_eval_stored_supported
    assert st(8, 128, 128, 256, 1024, 32) == 1    # SA2
    assert st(8, 128, 128, 256, 512, 16) == 1     # SA3
    assert st(8, 128, 128, 256, 256, 16) == 1     # SA4
    assert st(8, 128, 128, 128, 256, 16) == 1     # vote aggregation
    assert st(8, 128, 128, 128, 256, 64) == 1     # GridConv / IoU branch
    assert st(16, 128, 128, 256, 1024, 32) == 1   # SUN RGB-D batch
    assert st(8, 128, 128, 256, 1024, 24) == 0    # nsample not supported
    assert st(8, 128, 128, 256, 255, 16) == 0     # m * ns not a multiple of 32
    assert st(8, 256, 128, 256, 1024, 32) == 0    # wrong channel counts
    assert st(8, 128, 64, 256, 1024, 32) == 0
    assert st(8, 128, 128, 64, 1024, 32) == 0
    assert st(0, 128, 128, 256, 1024, 32) == 0    # b = 0
    assert st(8, 128, 128, 256, 1 << 22, 64) == 0  # m * ns beyond range
    size = lib.mlp_eval_stored_image_bytes
    size.restype = ctypes.c_size_t
    assert size(256) == 3 * 8 * 2 * (128 + 256) * 16 and size(128) == 3 * 8 * 2 * 256 * 16
    assert size(64) == 0
