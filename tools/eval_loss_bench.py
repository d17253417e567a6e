"""Time the test-time criterion (votenet.get_loss, models/loss_helper.py:222-291) per batch at the ScanNet
evaluation shape -- B = 8 scenes, K = 256 proposals, G = 64 ground-truth slots, S = 1024 seeds, 18 classes --
on the end points of a real eval forward (random detector weights, 40000 points) and make_batch's labels.

    python tools/eval_loss_bench.py [--iters 200] [--scans 312] [--repeats 3] [--out profiles/eval_loss.json]

Within one process, after a warm-up, alternating per iteration:
  * the tensor formulation on the GPU (VOTENET_FUSED_LOSS=0) and the fused path (four launches), each as
    device time between two events and as the wall clock of issuing it (the launches' host cost);
  * the fused path feeding an EvalLossMeter (the same launches, accum passed to the statistics kernel);
and alternating per repeat: inference.evaluate(device_ap=True) over --scans scans with and without with_loss,
wall clock to the final synchronisation.  Also the launches of each formulation, counted by the profiler of
torch on one call (not timed under it).  One JSON line; nothing here asserts a time."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
importlib.import_module("3dioumatch_amd")
V = importlib.import_module("3dioumatch_amd.votenet")
I = importlib.import_module("3dioumatch_amd.votenet.inference")
step = importlib.import_module("3dioumatch_amd.votenet.step")
data = importlib.import_module("3dioumatch_amd.votenet.data")

DEV = torch.device("cuda:0")
B, N = 8, 40000


def med(xs):
    return round(statistics.median(xs), 4)


def config_dict(cfg):
    return {"dataset_config": cfg, "remove_empty_box": False, "use_3d_nms": True, "nms_iou": 0.25,
            "use_old_type_nms": False, "cls_nms": True, "use_iou_for_nms": False,
            "per_class_proposal": True, "conf_thresh": 0.05}


def criterion(ep, cfg, fused, meter=None):
    os.environ["VOTENET_FUSED_LOSS"] = "1" if fused else "0"
    ep = dict(ep)
    return meter.step(ep, cfg) if meter is not None else V.get_loss(ep, cfg)


def timed(fn):
    """(device ms between two events, wall ms of issuing) of fn()"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    issue = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), issue


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--scans", type=int, default=312)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_loss_bench: needs the GPU (no timing without it)")
    cfg = V.scannet_config()
    cd = config_dict(cfg)
    det = step.build_detector(cfg, seed=0).to(DEV).eval()
    engine = I.InferenceEngine(det)
    distinct = [data.make_batch(B, N, cfg, seed=100 + s, device=DEV) for s in range(4)]
    eps = []
    for batch in distinct:
        ep = engine(batch["point_clouds"])
        ep.update({k: v for k, v in batch.items() if k not in ep})
        eps.append(ep)
    shape = dict(B=B, K=eps[0]["center"].shape[1], G=eps[0]["center_label"].shape[1], S=eps[0]["seed_xyz"].shape[1],
                 classes=cfg.num_class, iou_channels=eps[0]["iou_scores"].shape[2])

    meter = V.EvalLossMeter(DEV)
    modes = {"tensor": lambda ep: criterion(ep, cfg, False), "fused": lambda ep: criterion(ep, cfg, True),
             "fused_meter": lambda ep: criterion(ep, cfg, True, meter)}
    dev_ms, issue_ms = {m: [] for m in modes}, {m: [] for m in modes}
    for it in range(args.iters + 20):                  # the first 20: warm-up, not recorded
        ep = eps[it % len(eps)]
        for name, fn in modes.items():
            d, i = timed(lambda: fn(ep))
            if it >= 20:
                dev_ms[name].append(d)
                issue_ms[name].append(i)
    want = criterion(eps[0], cfg, False)[1]
    got = criterion(eps[0], cfg, True)[1]
    losses = importlib.import_module("3dioumatch_amd.votenet.losses")
    worst = max(abs(float(got[k]) - float(want[k])) / max(1.0, abs(float(want[k]))) for k in losses.EVAL_STAT_KEYS)
    out = {"what": "votenet.get_loss per batch on the end points of an eval forward, %s" % json.dumps(shape),
           "device": torch.cuda.get_device_name(0), "iters": args.iters,
           "fused_vs_tensor_worst_statistic_difference": float("%.3g" % worst),
           "positives_per_batch": float(want["pos_ratio"]) * B * shape["K"]}
    for name in modes:
        out[name + "_device_ms"] = med(dev_ms[name])
        out[name + "_issue_ms"] = med(issue_ms[name])
        out[name + "_device_ms_p10_p90"] = [round(float(np.percentile(dev_ms[name], p)), 4) for p in (10, 90)]
    out["tensor_launches"] = launches(lambda: criterion(eps[0], cfg, False))
    out["fused_launches"] = launches(lambda: criterion(eps[0], cfg, True))

    os.environ["VOTENET_FUSED_LOSS"] = "1"
    n_batches = args.scans // B
    batches = [distinct[i % len(distinct)] for i in range(n_batches)]
    times = {False: [], True: []}
    for rep in range(args.repeats + 1):                # rep 0: warm-up
        for flag in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with np.errstate(invalid="ignore", divide="ignore"):
                res = I.evaluate(engine, batches, cd, device_ap=True, with_loss=flag)
            torch.cuda.synchronize()
            if rep:
                times[flag].append((time.perf_counter() - t0) * 1e3)
    out.update({"evaluate_batches": n_batches,
                "evaluate_ms_per_batch": round(statistics.median(times[False]) / n_batches, 4),
                "evaluate_with_loss_ms_per_batch": round(statistics.median(times[True]) / n_batches, 4),
                "evaluate_ms_repeats": [round(x, 1) for x in times[False]],
                "evaluate_with_loss_ms_repeats": [round(x, 1) for x in times[True]],
                "mean_loss": res[1]["mean_loss"], "repeats": args.repeats})
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
