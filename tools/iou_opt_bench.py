"""Time the test-time IoU optimisation (votenet/iou_opt.py, train.py:444-491 of the reference) on
one ScanNet-sized batch: B = 8 scenes of N = 40 000 points, K = 256 proposals, opt_step = 10, a
detector with seeded weights in eval mode.

    python tools/iou_opt_bench.py [--iters 20] [--warmup 3] [--opt-step 10]

Prints one JSON line: ms per batch (device events, median) of optimize_boxes with the HIP engine
and with the autograd engine, the plain eval forward for context, and the largest difference of
the final boxes between the two engines.
"""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
importlib.import_module("3dioumatch_amd")
V = importlib.import_module("3dioumatch_amd.votenet")
O = importlib.import_module("3dioumatch_amd.votenet.iou_opt")
step = importlib.import_module("3dioumatch_amd.votenet.step")
data = importlib.import_module("3dioumatch_amd.votenet.data")


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--opt-step", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--points", type=int, default=40000)
    args = ap.parse_args()
    cfg = V.scannet_config()
    det = step.build_detector(cfg, num_proposal=256, seed=0).cuda().eval()
    batch = data.make_batch(args.batch, args.points, cfg, seed=3, device="cuda:0")
    inputs = {"point_clouds": batch["point_clouds"]}

    def forward():
        with torch.no_grad():
            return det(inputs)

    ep = forward()
    sem_cls = torch.argmax(ep["sem_cls_scores"], -1)
    _, gc, gs = O._autograd_pass(det, ep, ep["center"], ep["size"], ep["heading"], sem_cls)
    rate = 0.01 / torch.cat([gc, gs], -1).abs().median().item()
    out = {}
    for engine in ("hip", "autograd"):
        out[engine] = O.optimize_boxes(det, ep, rate, args.opt_step, engine=engine)
    ms_hip = timed(lambda: O.optimize_boxes(det, ep, rate, args.opt_step, engine="hip"), args.iters, args.warmup)
    ms_auto = timed(lambda: O.optimize_boxes(det, ep, rate, args.opt_step, engine="autograd"),
                    args.iters, args.warmup)
    ms_fwd = timed(forward, args.iters, args.warmup)
    dc = (out["hip"]["center"] - out["autograd"]["center"]).abs()
    ds = (out["hip"]["size_residuals"] - out["autograd"]["size_residuals"]).abs() / 2
    moved = (out["autograd"]["center"] - ep["center"]).abs().max().item()
    print(json.dumps({
        "workload": "iou_opt", "device": torch.cuda.get_device_name(0), "batch": args.batch,
        "points": args.points, "proposals": int(sem_cls.shape[1]), "opt_step": args.opt_step,
        "opt_rate": rate, "ms_per_batch_hip": round(ms_hip, 3), "ms_per_batch_autograd": round(ms_auto, 3),
        "speedup": round(ms_auto / ms_hip, 2), "ms_eval_forward": round(ms_fwd, 3),
        "max_center_diff": dc.max().item(), "max_half_size_diff": ds.max().item(),
        "median_center_diff": dc.median().item(), "max_center_move": moved}))


if __name__ == "__main__":
    main()
