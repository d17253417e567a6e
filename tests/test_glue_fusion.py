"""The train step's fused glue forms against the compositions they replace, BIT FOR BIT (torch.equal):
every fusion keeps each output element's arithmetic, so nothing but equality is asked.

  * interpolate + copied rows in one launch (_ext.three_interpolate_rows_into) against
    three_interpolate_into followed by a slice copy;
  * a weight's column slices read in place (gemm_forward / three_interpolate_affine on views) against the
    same calls on contiguous copies;
  * the last head layer's bias in the GEMM's store (gemm_forward(..., bias=)) against the GEMM followed
    by the broadcast add;
  * the vote tail (heads.vote_tail) and the IoU head's score slice (heads.iou_score_slices) against
    autograd through the tensor compositions they replace.
"""
import importlib

import pytest
import torch

from conftest import load_pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def K():
    load_pkg()
    return importlib.import_module("pointnet2._mlp_ext")


@pytest.fixture(scope="module")
def heads():
    load_pkg()
    return importlib.import_module("3dioumatch_amd.votenet.heads")


def _rand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32).to(DEV)


def _interp_inputs(b, c, m, n, seed):
    g = torch.Generator().manual_seed(seed)
    points = torch.randn((b, c, m), generator=g)
    idx = torch.randint(0, m, (b, n, 3), generator=g, dtype=torch.int32)
    weight = torch.rand((b, n, 3), generator=g)
    weight = weight / weight.sum(2, keepdim=True)
    return points.to(DEV), idx.to(DEV), weight.to(DEV).contiguous()


# n = 100: the last lanes of the only column block are idle; 1028: a second 1024-column block of
# one live lane; 2052: the same in the kernel that stages its source rows in LDS (n >= 2048)
@pytest.mark.parametrize("n", [100, 1028, 2052])
@pytest.mark.parametrize("rows_c", [3, 7])
@pytest.mark.parametrize("rows_first", [True, False])
def test_interpolate_rows_into_equals_interpolate_then_copy(ext, n, rows_c, rows_first):
    b, m, c = 2, 7, 5  # 5 interpolated channels fill no channel group of 4 or 8
    points, idx, weight = _interp_inputs(b, c, m, n, seed=n + rows_c)
    rows = _rand((b, rows_c, n), seed=1)
    channel0, rows_channel0 = (rows_c, 0) if rows_first else (0, c)
    want = torch.full((b, c + rows_c, n), float("nan"), device=DEV)
    ext.three_interpolate_into(points, idx, weight, want, channel0)
    want[:, rows_channel0:rows_channel0 + rows_c].copy_(rows)
    got = torch.full((b, c + rows_c, n), float("nan"), device=DEV)
    ext.three_interpolate_rows_into(points, idx, weight, got, channel0, rows, rows_channel0)
    assert not torch.isnan(got).any(), "an element of out was not written"
    assert torch.equal(got, want)


def test_interpolate_rows_into_unaligned_takes_the_scalar_form(ext):
    """n = 99: no 16-byte path for either half."""
    b, m, c, rows_c, n = 2, 7, 5, 3, 99
    points, idx, weight = _interp_inputs(b, c, m, n, seed=5)
    rows = _rand((b, rows_c, n), seed=2)
    want = torch.full((b, c + rows_c, n), float("nan"), device=DEV)
    ext.three_interpolate_into(points, idx, weight, want, rows_c)
    want[:, :rows_c].copy_(rows)
    got = torch.full((b, c + rows_c, n), float("nan"), device=DEV)
    ext.three_interpolate_rows_into(points, idx, weight, got, rows_c, rows, 0)
    assert torch.equal(got, want)


def test_interpolate_rows_into_rejects_overlapping_ranges(ext):
    points, idx, weight = _interp_inputs(2, 5, 7, 100, seed=3)
    out = torch.zeros((2, 8, 100), device=DEV)
    rows = _rand((2, 3, 100), seed=4)
    with pytest.raises(RuntimeError):
        ext.three_interpolate_rows_into(points, idx, weight, out, 0, rows, 4)  # channels 4 of both
    with pytest.raises(RuntimeError):
        ext.three_interpolate_rows_into(points, idx, weight, out, 0, rows, 6)  # past the last channel
    assert not out.any()


def test_weight_column_slices_are_read_in_place(ext, K):
    b, r, m_out, c = 2, 100, 70, 37
    w = _rand((m_out, 3 + c), seed=10)
    x = _rand((b, c, r), seed=11)
    feat_w, xyz_w = w[:, 3:], w[:, :3]
    assert not feat_w.is_contiguous() and not xyz_w.is_contiguous()
    z = K.gemm_forward(feat_w, x)
    assert torch.equal(z, K.gemm_forward(feat_w.contiguous(), x))
    scale, shift = _rand((c,), seed=12), _rand((c,), seed=13)
    assert torch.equal(K.gemm_forward(feat_w, x, (scale, shift)),
                       K.gemm_forward(feat_w.contiguous(), x, (scale, shift)))
    n = 128
    _, idx, weight = _interp_inputs(b, m_out, r, n, seed=14)
    rel = _rand((b, 3, n), seed=15)
    assert torch.equal(ext.three_interpolate_affine(z, idx, weight, xyz_w, rel),
                       ext.three_interpolate_affine(z, idx, weight, xyz_w.contiguous(), rel))


# rows = 79: a full and a partial 64-row tile; k = 40: one partial K chunk, 128: two full ones;
# r = 100: a full and a partial 64-column tile
@pytest.mark.parametrize("k", [40, 128])
@pytest.mark.parametrize("with_coeff", [False, True])
def test_bias_in_the_gemm_store_equals_gemm_then_add(K, k, with_coeff):
    rows, b, r = 79, 2, 100
    w, x, bias = _rand((rows, k), seed=20 + k), _rand((b, k, r), seed=21), _rand((rows,), seed=22)
    coeff = (_rand((k,), seed=23), _rand((k,), seed=24)) if with_coeff else None
    want = K.gemm_forward(w, x, coeff) + bias.view(1, -1, 1)
    assert torch.equal(K.gemm_forward(w, x, coeff, bias=bias), want)
    images = K.WeightImages([w])
    images.refresh()
    with K.weight_images(images):  # the form that reads the weight's bf16 image
        assert torch.equal(K.gemm_forward(w, x, coeff, bias=bias), want)


def test_bias_and_slice_outside_the_small_regime_fall_back(K):
    """b * r above the small kernels' range: the slice is copied, the bias added in its own pass."""
    rows, k, b, r = 70, 37, 2, 8448
    w, x, bias = _rand((rows, 3 + k), seed=30), _rand((b, k, r), seed=31), _rand((rows,), seed=32)
    want = K.gemm_forward(w[:, 3:].contiguous(), x) + bias.view(1, -1, 1)
    assert torch.equal(K.gemm_forward(w[:, 3:], x, bias=bias), want)


def _vote_tail_composed(net, seed_xyz, seed_features):
    """The tensor composition of VotingModule.forward (one vote per seed) followed by the one-kernel
    normalisation (votenet_channel_normalize[_grad]) that the fused tail replaces."""
    load_pkg()
    detector = importlib.import_module("3dioumatch_amd.votenet.detector")
    b, n = seed_xyz.shape[:2]
    c = seed_features.shape[1]
    t = net.transpose(2, 1).view(b, n, 1, 3 + c)
    offset, residual = torch.split(t, [3, c], dim=-1)
    vote_xyz = (seed_xyz.unsqueeze(2) + offset).reshape(b, n, 3)
    feats = (seed_features.transpose(2, 1).unsqueeze(2) + residual).reshape(b, n, c)
    return vote_xyz, detector.unit_length_features(feats.transpose(2, 1).contiguous())


# C = 37: uneven wave shares (9, 9, 9, 10 channels) and the remainder loop behind one 8-row group;
# C = 256: the network's width, eight 8-row groups per wave.  N = 100: a full and a partial block
@pytest.mark.parametrize("c", [37, 256])
def test_vote_tail_equals_the_tensor_composition(heads, c):
    b, n = 2, 100
    leaves = [_rand((b, 3 + c, n), seed=40 + c), _rand((b, n, 3), seed=41), _rand((b, c, n), seed=42)]
    g_xyz, g_feat = _rand((b, n, 3), seed=43), _rand((b, c, n), seed=44)
    results = []
    for fused in (False, True):
        net, xyz, feats = (t.clone().requires_grad_(True) for t in leaves)
        if fused:
            assert heads.vote_tail_fused(xyz, feats)
            vote_xyz, vote_feats, norm = heads.vote_tail(net, xyz, feats)
            # the length the separate kernel leaves behind, for the same pre-normalisation features
            pre = (feats.detach().transpose(2, 1) + net.detach().transpose(2, 1)[:, :, 3:])
            pre = pre.transpose(2, 1).contiguous()
            _L = importlib.import_module("3dioumatch_amd._lib")
            want_norm, scratch = torch.empty((b, n), device=DEV), torch.empty_like(pre)
            _L.check(_L.lib.votenet_channel_normalize(b, c, n, pre.data_ptr(), scratch.data_ptr(),
                                                      want_norm.data_ptr(),
                                                      torch.cuda.current_stream().cuda_stream),
                     "votenet_channel_normalize")
            assert torch.equal(norm, want_norm)
            assert not norm.requires_grad
        else:
            vote_xyz, vote_feats = _vote_tail_composed(net, xyz, feats)
        torch.autograd.backward([vote_xyz, vote_feats], [g_xyz, g_feat])
        results.append((vote_xyz.detach(), vote_feats.detach(), net.grad, xyz.grad, feats.grad))
    for name, want, got in zip(("vote_xyz", "vote_features", "d net", "d seed_xyz", "d seed_features"),
                               *results):
        assert got.is_contiguous(), name
        assert torch.equal(got, want), name


def test_vote_tail_without_a_coordinate_gradient(heads):
    """seed_xyz without gradient and no gradient into vote_xyz: zero coordinate rows of d net."""
    b, c, n = 2, 37, 100
    net = _rand((b, 3 + c, n), seed=50).requires_grad_(True)
    xyz, feats = _rand((b, n, 3), seed=51), _rand((b, c, n), seed=52).requires_grad_(True)
    _, vote_feats, _ = heads.vote_tail(net, xyz, feats)
    vote_feats.backward(_rand((b, c, n), seed=53))
    assert not net.grad[:, :3].any()
    assert torch.equal(net.grad[:, 3:], feats.grad)


@pytest.mark.parametrize("split", [True, False])
def test_iou_score_slices_equal_slice_and_split(heads, split):
    b, k, c_out, iou_size = 2, 5, 11, 3
    leaf = _rand((b, c_out, 2 * k), seed=60)
    grads = [_rand((b, k, iou_size), seed=61), _rand((b, k, iou_size), seed=62)] if split else \
        [_rand((b, 2 * k, iou_size), seed=63)]
    results = []
    for fused in (False, True):
        net = leaf.clone().requires_grad_(True)
        if fused:
            pieces = heads.iou_score_slices(net * 1.0, iou_size, k if split else None)
            assert type(pieces[0].grad_fn).__name__.startswith("_IouScoreSlices")
        else:
            scores = (net * 1.0).transpose(2, 1)[:, :, -iou_size:]
            pieces = torch.split(scores, [k, k], dim=1) if split else (scores,)
        assert len(pieces) == len(grads)
        torch.autograd.backward(list(pieces), grads)
        results.append([p.detach() for p in pieces] + [net.grad])
    for want, got in zip(*results):
        assert got.shape == want.shape
        assert torch.equal(got, want)


def test_iou_score_slices_with_one_unused_piece(heads):
    b, k, c_out, iou_size = 2, 5, 11, 3
    net = _rand((b, c_out, 2 * k), seed=70).requires_grad_(True)
    first, _ = heads.iou_score_slices(net * 1.0, iou_size, k)
    g = _rand((b, k, iou_size), seed=71)
    first.backward(g)
    want = torch.zeros_like(net)
    want[:, -iou_size:, :k] = g.transpose(1, 2)
    assert torch.equal(net.grad, want)
