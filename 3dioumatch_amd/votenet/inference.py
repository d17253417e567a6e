"""Inference engine: the eval-mode forward of a detector with fused set-abstraction kernels, captured
graphs and the next batch's index chain prefetched on a side stream.

    engine = InferenceEngine(detector)          # detector.eval(), on the GPU
    end_points = engine(point_clouds)           # one batch
    for end_points in engine.run(clouds): ...   # batch i+1's index chain beside batch i's forward
    metrics = evaluate(engine, batches, config_dict)

The end_points carry every key of the plain `detector({'point_clouds': ...})` under no_grad, so
parse_predictions and iou_opt.optimize_boxes take them unchanged.  What differs from the plain eval
forward:
  * the six pooled shared MLPs (SA1-SA4, vote aggregation, the IoU branch) run their layers 1-2, the
    folded BatchNorms, the ReLUs and the max over nsample as ONE kernel (csrc/mlp_eval_pool.hip,
    pointnet2.pytorch_utils.EvalPlan) where its shape gate allows -- elsewhere the plain path;
  * the coordinate-only index chain (detector.compute_geometry) runs ahead of the forward, for the
    next batch on a side stream while the current one replays (the training step's pattern,
    votenet/step.py prefetch_geometry);
  * the forward replays from one linear captured graph per input signature.
The detector's parameters and buffers are only read; refresh() re-folds after they change.
"""
import torch

from pointnet2.pytorch_utils import EvalPlan, SharedMLP, fused_eval


def _plans_of(detector):
    plans = {}
    for module in detector.modules():
        if isinstance(module, SharedMLP) and len(module) == 3 and all(SharedMLP._fusable(l) for l in module):
            try:
                plans[id(module)] = EvalPlan(module)
            except ValueError:
                pass  # no one-pass kernel for these layer shapes: the plain path serves it
    return plans


class InferenceEngine(object):
    def __init__(self, detector, graphs=True):
        if not isinstance(detector, torch.nn.Module) or not hasattr(detector, "compute_geometry"):
            raise ValueError("InferenceEngine: a VoteNet detector (nn.Module with compute_geometry)")
        if detector.training:
            raise ValueError("InferenceEngine: the detector must be in eval mode (detector.eval())")
        params = list(detector.parameters())
        if not params or any(not p.is_cuda or p.dtype != torch.float32 for p in params):
            raise ValueError("InferenceEngine: the detector's parameters must be float32 on a GPU")
        self.detector = detector
        self.device = params[0].device
        self.graphs = bool(graphs)
        with torch.cuda.device(self.device):
            self.plans = _plans_of(detector)
        if not self.plans:
            raise ValueError("InferenceEngine: the detector has no pooled shared MLP the engine can fuse")
        self._captured = {}  # signature -> (graph, static point clouds, static geometry, static outputs)
        self._side = None

    # ------------------------------------------------------------------ state
    def refresh(self):
        """Re-fold every BatchNorm and rebuild the weight images (in place: captured graphs stay
        valid) after the detector's weights or running statistics changed."""
        if self.detector.training:
            raise ValueError("InferenceEngine.refresh: the detector must be in eval mode")
        with torch.cuda.device(self.device):
            for plan in self.plans.values():
                plan.refresh()

    def fused_calls(self):
        """How many pooled forwards the one-pass kernels served so far (eager runs and captures)."""
        return sum(plan.hits for plan in self.plans.values())

    def side_stream(self):
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.device)  # default priority (NEXT_ROUND.md)
        return self._side

    # ------------------------------------------------------------------ forward
    def _geometry(self, point_clouds):
        return self.detector.compute_geometry({'point_clouds': point_clouds})

    def _forward(self, point_clouds, geometry):
        with torch.no_grad(), fused_eval(self.plans):
            end_points = self.detector({'point_clouds': point_clouds, 'geometry': geometry})
        end_points.pop('precomputed_proposal_inds', None)  # an input, not an output of the plain forward
        return end_points

    @staticmethod
    def _signature(point_clouds, geometry):
        return (tuple(point_clouds.shape),) + tuple(
            (k, tuple(v.shape), v.dtype) for k, v in sorted(geometry.items()))

    def _capture(self, point_clouds, geometry):
        static_pc = point_clouds.clone()
        static_geo = {k: v.clone() for k, v in geometry.items()}
        # warm-up outside the capture: first launches set kernel attributes, allocators settle
        warm = torch.cuda.Stream(device=self.device)
        warm.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(warm):
            self._forward(static_pc, static_geo)
        torch.cuda.current_stream(self.device).wait_stream(warm)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = self._forward(static_pc, static_geo)
        return graph, static_pc, static_geo, out

    def _run_forward(self, point_clouds, geometry):
        """The forward of one batch whose geometry is ready on the current stream -> end_points
        (fresh tensors: nothing aliases the graph's buffers)."""
        if not self.graphs:
            return self._forward(point_clouds, geometry)
        sig = self._signature(point_clouds, geometry)
        entry = self._captured.get(sig)
        if entry is None:
            entry = self._captured[sig] = self._capture(point_clouds, geometry)
        graph, static_pc, static_geo, out = entry
        static_pc.copy_(point_clouds)
        for k, v in geometry.items():
            static_geo[k].copy_(v)
        graph.replay()
        return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in out.items()}

    def __call__(self, point_clouds):
        """end_points of one batch (B, N, 3 + C) -- its index chain inline."""
        point_clouds = point_clouds.to(self.device).contiguous()
        with torch.cuda.device(self.device):
            return self._run_forward(point_clouds, self._geometry(point_clouds))

    def _prefetch(self, point_clouds):
        """Launch the index chain of a batch on the side stream -> (clouds, geometry, ready event)."""
        main = torch.cuda.current_stream(self.device)
        point_clouds = point_clouds.to(self.device).contiguous()
        side = self.side_stream()
        side.wait_stream(main)  # the clouds are ready
        with torch.cuda.stream(side):
            geometry = self._geometry(point_clouds)
            ready = torch.cuda.Event()
            ready.record(side)
        for t in geometry.values():
            t.record_stream(main)
        point_clouds.record_stream(side)
        return point_clouds, geometry, ready

    def run(self, batches):
        """end_points of every batch of point clouds, in order.  While batch i's forward replays on the
        current stream, batch i+1's index chain runs on the side stream."""
        with torch.cuda.device(self.device):
            main = torch.cuda.current_stream(self.device)
            it = iter(batches)
            first = next(it, None)
            if first is None:
                return
            cur = self._prefetch(first)
            while cur is not None:
                nxt = next(it, None)
                pending = self._prefetch(nxt) if nxt is not None else None
                point_clouds, geometry, ready = cur
                main.wait_event(ready)
                yield self._run_forward(point_clouds, geometry)
                cur = pending


def evaluate(engine, batches, config_dict, opt_step=0, opt_rate=5e-4, ap_iou_thresholds=(0.25, 0.5),
             device_ap=False, with_loss=False):
    """iou_opt.evaluate(engine.detector, batches, ...) with the engine's forward: for every batch (a dict
    with 'point_clouds' and the labels parse_groundtruths reads) the engine's end_points, for
    opt_step > 0 the IoU optimisation of the boxes (iou_opt.optimize_boxes), parse_predictions /
    parse_groundtruths and one APCalculator per threshold.  Returns the compute_metrics() dicts.
    device_ap: the device forms of the two parsers and one DeviceAPCalculator for all thresholds
    instead -- labels on the host are moved with non-blocking copies and nothing in the loop waits
    for the GPU, so the next batch's index chain really runs beside this one's forward.
    with_loss: also the test-time criterion on every batch (losses.get_loss after the box optimisation, as
    train.py:486-502 orders them; the batch then needs losses.EVAL_LABEL_KEYS) through one EvalLossMeter,
    which never reads the device inside the loop; returns (metrics, the meter's result())."""
    from .eval_helper import (APCalculator, DeviceAPCalculator, EvalLossMeter, parse_groundtruths,
                              parse_groundtruths_device, parse_predictions, parse_predictions_device)
    from .iou_opt import _check_detector, optimize_boxes
    detector = engine.detector
    if detector.training:
        raise ValueError("evaluate: the detector must be in eval mode")
    if opt_step > 0:
        _check_detector(detector)
    batches = list(batches)
    class2type = getattr(config_dict['dataset_config'], 'class2type', None)
    if device_ap:
        calc = DeviceAPCalculator(ap_iou_thresholds, class2type)
    else:
        calcs = [APCalculator(t, class2type) for t in ap_iou_thresholds]
    meter = EvalLossMeter(engine.device) if with_loss else None
    for batch, end_points in zip(batches, engine.run(b['point_clouds'] for b in batches)):
        if opt_step > 0:
            end_points = optimize_boxes(detector, end_points, opt_rate, opt_step)
        for key in batch:
            if key not in end_points:
                value = batch[key]
                if (device_ap or with_loss) and torch.is_tensor(value):
                    value = value.to(engine.device, non_blocking=True)
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
