"""Test-time IoU optimisation of the predicted boxes and the evaluation entry point around it.

Host-side mirror of the reference train.py:431-491 (evaluate_with_opt, run by run_eval_opt.sh):
every predicted box climbs the gradient of its own IoU logit -- centre and half size move, the
heading stays -- before the NMS of parse_predictions(use_iou_for_nms=True).  evaluate() is
evaluate_one_epoch / evaluate_with_opt without TensorBoard (the loss statistics with with_loss=True).

Two engines compute the same ascent:
  * "autograd": the reference loop written literally, with forward_onlyiou_faster and the
    tensor-op branch of GridConv.forward (its gradient flows through the interpolation weights).
    The definition; CPU (oracle stand-in) and GPU.
  * "hip" (the default on the GPU): no autograd.  Per pass the eval-mode forward of the IoU branch
    on the existing kernels, keeping what the data gradient needs (the layers' raw outputs and the
    pool arg-max); the one-hot IoU gradient back through the small head with tensor ops; the
    shared MLP's data gradient through mlp_gemm_dgrad (pooled and on-the-fly forms); then ONE
    kernel (csrc/iou_opt.hip, votenet_iou_opt_box_step) for the box gradient and the ascent step.
    No weight gradient, no host synchronisation inside the loop.
"""
import importlib

import torch
import torch.nn.functional as F


def _lib():
    return importlib.import_module("3dioumatch_amd._lib")


def _check_detector(detector):
    gc = detector.grid_conv
    if detector.training:
        raise ValueError("optimize_boxes: the detector must be in eval mode (train.py:436 calls "
                         "detector.eval(); batch-statistics BatchNorm would couple the boxes)")
    if gc.iou_size == 1:
        raise ValueError("optimize_boxes: iou_class_depend=False (one IoU output) is not supported: "
                         "the reference gathers the IoU of the predicted class (train.py:452)")
    return gc


def _finish(detector, end_points, center, size, iou):
    """end_points as train.py:480-487 leaves them: final centres, size_residuals rebuilt from the
    final half sizes (broadcast over the size clusters), the final IoU scores."""
    out = dict(end_points)
    size_scores = end_points['size_scores']
    b, k, ns = size_scores.shape
    size_class = torch.argmax(size_scores, -1)
    mean = detector._mean_size.to(size.dtype)
    size_base = torch.index_select(mean, 0, size_class.view(-1)).view(b, k, 3)
    out['center'] = center
    out['size_residuals'] = (size * 2 - size_base).unsqueeze(2).expand(-1, -1, ns, -1).contiguous()
    out['iou_scores'] = iou
    return out


# ---- the definition: the reference loop over autograd ---------------------------------------------

def _autograd_pass(detector, end_points, center, size, heading, sem_cls, want_grad=True):
    c = center.detach().clone().requires_grad_(True)
    s = size.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        ep = detector.forward_onlyiou_faster(dict(end_points), c, s, heading.detach())
        iou = ep['iou_scores']
        if not want_grad:
            return iou.detach(), None, None
        picked = torch.gather(iou, 2, sem_cls.unsqueeze(-1)).sum()
        gc, gs = torch.autograd.grad(picked, (c, s))
    return iou.detach(), gc, gs


def _optimize_autograd(detector, end_points, opt_rate, opt_step, trace=None):
    sem_cls = torch.argmax(end_points['sem_cls_scores'], -1)
    heading = end_points['heading'].detach()
    center, size = end_points['center'].detach(), end_points['size'].detach()
    _, gc, gs = _autograd_pass(detector, end_points, center, size, heading, sem_cls)
    iou = None
    for count in range(1, opt_step + 2):  # opt_step + 1 updates (the loop breaks at count > opt_step)
        center = center + opt_rate * gc
        size = size + opt_rate * gs
        # the reference's last backward is never used: that pass is a forward only here
        iou, gc, gs = _autograd_pass(detector, end_points, center, size, heading, sem_cls,
                                     want_grad=count <= opt_step)
        if trace is not None:
            trace.append((center, size, iou))
    return center, size, iou


# ---- the device engine ----------------------------------------------------------------------------

def _eval_bn(bn):
    invstd = torch.rsqrt(bn.running_var + bn.eps)
    gain = bn.weight * invstd
    return gain, bn.bias - bn.running_mean * gain


class HipBoxStep(object):
    """The per-batch state of the device engine: constants of one batch (projected seed features,
    BatchNorm coefficients, the head's IoU rows of the predicted classes) and one pass
    (forward at the current boxes, data gradient, ascent step in place)."""

    def __init__(self, detector, end_points):
        gc = _check_detector(detector)
        L = _lib()
        from pointnet2 import _mlp_ext as K
        self.gc, self.L, self.K = gc, L, K
        origin_xyz, origin_feats = gc._origin(end_points)
        self.xyz = origin_xyz.detach().contiguous()
        feats = origin_feats.detach().contiguous()
        if not (feats.is_cuda and feats.dtype == torch.float32):
            raise ValueError("the hip engine needs float32 GPU tensors")
        layers = list(gc.mlp_before_iou)
        if len(layers) != 3 or not all(gc.mlp_before_iou._fusable(layer) for layer in layers):
            raise ValueError("the hip engine needs the reference's 3-layer shared MLP with BatchNorm")
        self.w = [layer.conv.weight.detach().reshape(layer.conv.weight.shape[0], -1) for layer in layers]
        self.dev = feats.device
        b, c, nseed = feats.shape
        m = self.w[0].shape[0]
        if self.w[0].shape[1] != c + 3:
            raise ValueError("seed features: %d channels, the IoU branch expects %d" % (c, self.w[0].shape[1] - 3))
        from pointnet2 import _ext
        self.ext = _ext
        if not _ext.three_interpolate_affine_supported(m, nseed, end_points['center'].shape[1] * 64):
            raise ValueError("the hip engine needs <= 2048 seeds (pn2_three_interpolate_affine)")
        self.m, self.nseed = m, nseed
        w0 = self.w[0].contiguous()
        self.w0 = w0
        self.w0xyz = w0[:, :3].contiguous()
        # the first layer commutes with the interpolation: W0[:, 3:] . F once per batch
        self.proj = K.gemm_forward(w0[:, 3:].contiguous(), feats)
        self.coef = []
        for layer in layers:
            bn = next(layer.bn.children())
            mean, invstd, scale, shift = K.bn_coefficients(self.proj, bn.weight, bn.bias, bn.running_mean,
                                                           bn.running_var, bn.momentum, bn.eps, False)
            gain = bn.weight.detach() * invstd
            # eval-mode coefficients of the BatchNorm backward: (gamma * invstd, 0, 0)
            bcoef = torch.stack([gain, torch.zeros_like(gain), torch.zeros_like(gain)], 1).contiguous()
            self.coef.append((mean, invstd, scale, shift, gain.contiguous(), bcoef))
        self.unit = gc._unit_grid(self.dev)
        sem_cls = torch.argmax(end_points['sem_cls_scores'], -1)
        self.heading = end_points['heading'].detach().contiguous()
        # the head (B*K columns, torch ops): conv1 -> bn1 -> relu -> conv2 -> bn2 -> relu -> conv3
        self.h1 = (gc.conv1_iou.weight.detach()[:, :, 0], gc.conv1_iou.bias.detach()) + _eval_bn(gc.bn1_iou)
        self.h2 = (gc.conv2_iou.weight.detach()[:, :, 0], gc.conv2_iou.bias.detach()) + _eval_bn(gc.bn2_iou)
        w3 = gc.conv3_iou.weight.detach()[:, :, 0]
        self.w3 = w3[-gc.iou_size:]
        self.b3 = gc.conv3_iou.bias.detach()[-gc.iou_size:]
        # d(iou[b, k, sem_cls]) / d(head input of layer 3): the predicted class's row, (B, 128, K)
        self.d_a2 = self.w3[sem_cls].permute(0, 2, 1).contiguous()
        self.b, self.k = sem_cls.shape

    def forward(self, center, size):
        """eval-mode IoU branch at (center, size): iou_scores (B,K,iou_size) and what the backward keeps"""
        K, b, k = self.K, self.b, self.k
        cols = k * 64
        whole = torch.empty((b, cols, 3), dtype=torch.float32, device=self.dev)
        rel = torch.empty((b, 3, cols), dtype=torch.float32, device=self.dev)
        L = self.L
        stream = torch.cuda.current_stream(self.dev).cuda_stream
        with torch.cuda.device(self.dev):
            L.check(L.lib.votenet_gridconv_points(b, k, 3, self.unit.data_ptr(), center.data_ptr(),
                                                  size.data_ptr(), self.heading.data_ptr(), whole.data_ptr(),
                                                  rel.data_ptr(), stream), "votenet_gridconv_points")
        from pointnet2 import pointnet2_utils
        idx, weight = pointnet2_utils.three_nn_with_weights(whole, self.xyz)
        y0 = self.ext.three_interpolate_affine(self.proj, idx, weight, self.w0xyz, rel)
        c0, c1, c2 = self.coef
        y1 = K.gemm_forward(self.w[1], y0, (c0[2], c0[3]))
        y2 = K.gemm_forward(self.w[2], y1, (c1[2], c1[3])).view(b, self.m, k, 64)
        pooled, argmax, _ = K.bn_relu_pool(y2, c2[2], c2[3])
        w1, bias1, g1, s1 = self.h1
        w2, bias2, g2, s2 = self.h2
        t1 = (torch.matmul(w1, pooled) + bias1.view(1, -1, 1)) * g1.view(1, -1, 1) + s1.view(1, -1, 1)
        a1 = torch.relu(t1)
        t2 = (torch.matmul(w2, a1) + bias2.view(1, -1, 1)) * g2.view(1, -1, 1) + s2.view(1, -1, 1)
        a2 = torch.relu(t2)
        iou = (torch.matmul(self.w3, a2) + self.b3.view(1, -1, 1)).transpose(1, 2)
        return iou, (idx, y0, y1, y2, argmax, t1, t2)

    def step(self, center, size, rate, saved, grad=None):
        """the ascent step from the forward's `saved`: center, size += rate * dL/d(center, size), in place"""
        K, L = self.K, self.L
        idx, y0, y1, y2, argmax, t1, t2 = saved
        w1, _, g1, _ = self.h1
        w2, _, g2, _ = self.h2
        d_t2 = torch.where(t2 > 0, self.d_a2, torch.zeros_like(self.d_a2)) * g2.view(1, -1, 1)
        d_a1 = torch.matmul(w2.t(), d_t2)
        d_t1 = torch.where(t1 > 0, d_a1, torch.zeros_like(d_a1)) * g1.view(1, -1, 1)
        dpooled = torch.matmul(w1.t(), d_t1).contiguous()
        c0, c1, c2 = self.coef
        dz1 = K.gemm_dgrad(self.w[2], pooled=(y2, dpooled, argmax, c2[2], c2[3], c2[0], c2[1], c2[5]))
        dz0 = K.gemm_dgrad(self.w[1], fly=(y1, dz1, c1[2], c1[3], c1[0], c1[1], c1[5]))
        with torch.cuda.device(self.dev):
            L.check(L.lib.votenet_iou_opt_box_step(
                self.b, self.k, self.nseed, self.m, self.unit.data_ptr(), self.xyz.data_ptr(), idx.data_ptr(),
                self.proj.data_ptr(), self.w0.data_ptr(), self.w0.shape[1], dz0.data_ptr(), y0.data_ptr(),
                c0[2].data_ptr(), c0[3].data_ptr(), c0[4].data_ptr(), self.heading.data_ptr(), float(rate),
                center.data_ptr(), size.data_ptr(), None if grad is None else grad.data_ptr(),
                torch.cuda.current_stream(self.dev).cuda_stream), "votenet_iou_opt_box_step")

    def gradient(self, center, size):
        """(dL/dcenter, dL/dsize) at the given boxes, (B,K,3) each; the boxes are not changed"""
        c, s = center.detach().clone().contiguous(), size.detach().clone().contiguous()
        grad = torch.empty((self.b, self.k, 6), dtype=torch.float32, device=self.dev)
        _, saved = self.forward(c, s)
        self.step(c, s, 0.0, saved, grad)
        return grad[..., :3], grad[..., 3:]


def _optimize_hip(detector, end_points, opt_rate, opt_step, trace=None):
    run = HipBoxStep(detector, end_points)
    center = end_points['center'].detach().contiguous().clone()
    size = end_points['size'].detach().contiguous().clone()
    with torch.no_grad():
        for count in range(opt_step + 1):
            _, saved = run.forward(center, size)
            run.step(center, size, opt_rate, saved)
            if trace is not None:
                trace.append((center.clone(), size.clone()))
        iou, _ = run.forward(center, size)
    return center, size, iou


def optimize_boxes(detector, end_points, opt_rate, opt_step=10, engine="auto"):
    """train.py:444-491: opt_step + 1 ascent steps of every box (centre and half size) up the
    gradient of its own IoU logit at the predicted class.  end_points: a VoteNet eval forward's
    (center, size, heading, sem_cls_scores, size_scores and the seeds).  Returns a new dict with
    the final 'center', 'size_residuals' (2 * final half size - mean size of the predicted size
    class, for every size cluster) and 'iou_scores'; everything else as given."""
    _check_detector(detector)
    if engine == "auto":
        engine = "hip" if end_points['center'].is_cuda else "autograd"
    if engine == "autograd":
        center, size, iou = _optimize_autograd(detector, end_points, opt_rate, opt_step)
    elif engine == "hip":
        center, size, iou = _optimize_hip(detector, end_points, opt_rate, opt_step)
    else:
        raise ValueError("engine must be 'auto', 'hip' or 'autograd', not %r" % (engine,))
    return _finish(detector, end_points, center, size, iou)


def evaluate(detector, batches, config_dict, opt_step=0, opt_rate=5e-4, ap_iou_thresholds=(0.25, 0.5),
             engine="auto", device_ap=False, with_loss=False):
    """evaluate_one_epoch (opt_step = 0) / evaluate_with_opt (opt_step > 0) of the reference
    train.py:384-425 / :431-507: for every batch (a dict with
    'point_clouds' and the ground-truth labels parse_groundtruths reads) a no-grad forward, the
    IoU optimisation of the boxes, parse_predictions / parse_groundtruths and one APCalculator per
    threshold.  Returns the list of compute_metrics() dicts, one per threshold.
    device_ap: the device forms of the two parsers and one DeviceAPCalculator for all thresholds
    instead (labels on the host are moved with non-blocking copies; no host round trip per batch).
    with_loss: also the loss statistics -- the test-time criterion on every batch (losses.get_loss after the box
    optimisation, train.py:400 / :486-502; the batch then needs losses.EVAL_LABEL_KEYS) through one
    EvalLossMeter; returns (metrics, the meter's result(): the epoch mean of each logged key and 'mean_loss')."""
    from .eval_helper import (APCalculator, DeviceAPCalculator, EvalLossMeter, parse_groundtruths,
                              parse_groundtruths_device, parse_predictions, parse_predictions_device)
    if detector.training:
        raise ValueError("evaluate: the detector must be in eval mode")
    if opt_step > 0:
        _check_detector(detector)
    class2type = getattr(config_dict['dataset_config'], 'class2type', None)
    if device_ap:
        calc = DeviceAPCalculator(ap_iou_thresholds, class2type)
    else:
        calcs = [APCalculator(t, class2type) for t in ap_iou_thresholds]
    meter = EvalLossMeter(next(detector.parameters()).device) if with_loss else None
    for batch in batches:
        with torch.no_grad():
            end_points = detector({'point_clouds': batch['point_clouds']})
        if opt_step > 0:
            end_points = optimize_boxes(detector, end_points, opt_rate, opt_step, engine)
        for key in batch:
            if key not in end_points:
                value = batch[key]
                if (device_ap or with_loss) and torch.is_tensor(value):
                    value = value.to(end_points['center'].device, non_blocking=True)
                end_points[key] = value
        if with_loss:
            meter.step(end_points, config_dict['dataset_config'])
        if device_ap:
            calc.step(parse_predictions_device(end_points, config_dict),
                      parse_groundtruths_device(end_points, config_dict))
            continue
        pred = parse_predictions(end_points, config_dict)
        gt = parse_groundtruths(end_points, config_dict)
        for calc in calcs:
            calc.step(pred, gt)
    metrics = calc.compute_metrics() if device_ap else [calc.compute_metrics() for calc in calcs]
    return (metrics, meter.result()) if with_loss else metrics
