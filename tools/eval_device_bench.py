"""Time the tail of the evaluation loop -- what consumes the inference engine's end points -- on the
host path (parse_predictions + parse_groundtruths + APCalculator.step per threshold) and on the
device path (their *_device forms + DeviceAPCalculator.step) at ScanNet-val size: 312 scans, B = 8,
K = 256, 18 classes, per_class_proposal, synthetic head outputs (half of the proposals scattered
around the true boxes, half anywhere in the room; random objectness).  Both paths alternate in one
process, after a warm-up, three repeats.

    python tools/eval_device_bench.py [--match-stats ms_kernel_stats.csv] [--out profiles/eval_device_ap.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ms -- \\
        python tools/eval_device_bench.py --match-only 20

The second form runs only the match kernel (for its device duration without launch overhead; a run
of its own) and prints the pair count; its DIR/ms_kernel_stats.csv goes to --match-stats of the
first.  Reported per batch: the host tail as wall clock up to its last synchronisation, the device
tail from device events and the wall clock of issuing it; compute_metrics of both paths;
inference.evaluate end to end with device_ap off and on (random detector weights, 40000 points)."""
import argparse
import csv
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
D = importlib.import_module("3dioumatch_amd.votenet.eval_det")
E = importlib.import_module("3dioumatch_amd.votenet.eval_helper")
data = importlib.import_module("3dioumatch_amd.votenet.data")

DEV = torch.device("cuda:0")
B, K = 8, 256


def config_dict(cfg):
    return {"dataset_config": cfg, "remove_empty_box": False, "use_3d_nms": True, "nms_iou": 0.25,
            "use_old_type_nms": False, "cls_nms": True, "use_iou_for_nms": False,
            "per_class_proposal": True, "conf_thresh": 0.05}


def head_outputs(cfg, seed):
    """Labels of make_batch and head outputs around them: proposal j < K/2 decodes to a true box of its
    scene with the centre off by N(0, 0.15 m) and the size by N(0, 0.1 m), the others sit anywhere in
    the room with a random size class; objectness logits N(-1.5, 2.5), class logits 6 on the box's class."""
    g = torch.Generator().manual_seed(seed)
    batch = data.make_batch(B, 2048, cfg, seed=seed)
    nh, ns, nc = cfg.num_heading_bin, cfg.num_size_cluster, cfg.num_class
    n_obj = batch["box_label_mask"].sum(1).long()
    src = (torch.rand(B, K, generator=g) * n_obj.view(B, 1)).long()
    take = lambda t: torch.gather(t, 1, src.view(B, K, *[1] * (t.dim() - 2)).expand(B, K, *t.shape[2:]))  # noqa: E731
    near = (torch.arange(K) < K // 2).view(1, K)
    room = torch.rand(B, K, 3, generator=g) * torch.tensor([6.0, 5.0, 3.0])
    center = torch.where(near.unsqueeze(-1), take(batch["center_label"]) + 0.15 * torch.randn(B, K, 3, generator=g), room)
    size_cls = torch.where(near, take(batch["size_class_label"]), torch.randint(0, ns, (B, K), generator=g))
    sem_cls = torch.where(near, take(batch["sem_cls_label"]), torch.randint(0, nc, (B, K), generator=g))
    head_cls = torch.where(near, take(batch["heading_class_label"]), torch.randint(0, nh, (B, K), generator=g))
    ep = {"center": center,
          "objectness_scores": torch.stack([torch.zeros(B, K), -1.5 + 2.5 * torch.randn(B, K, generator=g)], -1),
          "heading_scores": 8.0 * torch.nn.functional.one_hot(head_cls, nh).float(),
          "heading_residuals": 0.05 * torch.randn(B, K, nh, generator=g),
          "size_scores": 8.0 * torch.nn.functional.one_hot(size_cls, ns).float(),
          "size_residuals": 0.1 * torch.randn(B, K, ns, 3, generator=g),
          "sem_cls_scores": 6.0 * torch.nn.functional.one_hot(sem_cls, nc).float() + torch.randn(B, K, nc, generator=g),
          "iou_scores": torch.zeros(B, K, nc)}
    ep.update({k: v for k, v in batch.items() if k != "point_clouds"})
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in ep.items()}


def med(xs):
    return round(statistics.median(xs), 3)


def match_only(cfg, reps):
    ep = head_outputs(cfg, 0)
    cd = config_dict(cfg)
    pred, gt = E.parse_predictions_device(ep, cd), E.parse_groundtruths_device(ep, cd)
    for _ in range(reps):
        D.eval_match_gpu(pred["corners"], pred["keep"], pred["cls"], gt["corners"], gt["valid"], gt["cls"],
                         cfg.num_class)
    torch.cuda.synchronize()
    kept, valid = pred["keep"].sum(1), gt["valid"].sum(1)
    print(json.dumps({"match_only_launches": reps, "kept_proposals": int(kept.sum()),
                      "valid_ground_truth": int(valid.sum()), "pairs": int((kept * valid).sum())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=312)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=6, help="distinct synthetic batches, cycled")
    ap.add_argument("--match-only", type=int, default=0, metavar="LAUNCHES")
    ap.add_argument("--match-stats", default=None, help="kernel_stats.csv of a --match-only run under rocprofv3")
    ap.add_argument("--no-end-to-end", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cfg = V.scannet_config()
    if args.match_only:
        return match_only(cfg, args.match_only)
    cd = config_dict(cfg)
    thresholds = (0.25, 0.5)
    n_batches = args.scans // B
    eps = [head_outputs(cfg, s) for s in range(args.distinct)]
    kept = float(np.mean([E.parse_predictions_device(ep, cd)["keep"].float().mean().item() for ep in eps]))

    host_tail, dev_tail, dev_issue, host_metrics, dev_metrics = [], [], [], [], []
    for rep in range(args.repeats + 1):                # rep 0: warm-up, not recorded
        hosts = [E.APCalculator(t, None, device="cuda:0") for t in thresholds]
        devc = E.DeviceAPCalculator(thresholds, None)
        h_ms, d_ms, i_ms = [], [], []
        for i in range(n_batches):
            ep = dict(eps[i % len(eps)])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pred, gt = E.parse_predictions(ep, cd), E.parse_groundtruths(ep, cd)
            for calc in hosts:
                calc.step(pred, gt)
            h_ms.append((time.perf_counter() - t0) * 1e3)   # its last .cpu() was the last synchronisation
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            devc.step(E.parse_predictions_device(ep, cd), E.parse_groundtruths_device(ep, cd))
            e1.record()
            i_ms.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            d_ms.append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        with np.errstate(invalid="ignore", divide="ignore"):
            want = [calc.compute_metrics() for calc in hosts]
        hm = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = devc.compute_metrics()                         # ends in its one device->host copy
        dm = (time.perf_counter() - t0) * 1e3
        for g, w in zip(got, want):
            assert list(g) == list(w)
            np.testing.assert_allclose([g[k] for k in w], [w[k] for k in w], rtol=0, atol=1e-12, equal_nan=True)
        if rep:
            host_tail.append(statistics.median(h_ms))
            dev_tail.append(statistics.median(d_ms))
            dev_issue.append(statistics.median(i_ms))
            host_metrics.append(hm)
            dev_metrics.append(dm)
    out = {"what": "evaluation tail, %d scans as %d batches of %d x %d proposals x %d classes, thresholds %s"
                   % (n_batches * B, n_batches, B, K, cfg.num_class, list(thresholds)),
           "device": torch.cuda.get_device_name(0), "kept_fraction": round(kept, 3),
           "host_tuples_per_batch": int(round(kept * B * K * cfg.num_class)),
           "host_tail_ms_per_batch": med(host_tail), "host_tail_ms_repeats": [round(x, 3) for x in host_tail],
           "device_tail_ms_per_batch": med(dev_tail), "device_tail_ms_repeats": [round(x, 3) for x in dev_tail],
           "device_tail_issue_ms_per_batch": med(dev_issue),
           "host_compute_metrics_ms": med(host_metrics), "host_compute_metrics_ms_repeats": [round(x, 1) for x in host_metrics],
           "device_compute_metrics_ms": med(dev_metrics),
           "device_compute_metrics_ms_repeats": [round(x, 1) for x in dev_metrics],
           "mAP_0.25": float(got[0]["mAP"]), "metrics_equal_within": 1e-12, "repeats": args.repeats}

    if args.match_stats:
        for row in csv.DictReader(open(args.match_stats)):
            if "eval_match_kernel" in row["Name"]:
                out["match_kernel_us"] = round(float(row["AverageNs"]) / 1e3, 2)
                out["match_kernel_calls"] = int(row["Calls"])
        ep = eps[0]
        pred, gt = E.parse_predictions_device(ep, cd), E.parse_groundtruths_device(ep, cd)
        out["match_kernel_pairs"] = int((pred["keep"].sum(1) * gt["valid"].sum(1)).sum())
        out["match_kernel_dense_pairs"] = B * K * gt["valid"].shape[1]

    if not args.no_end_to_end:
        I = importlib.import_module("3dioumatch_amd.votenet.inference")
        step = importlib.import_module("3dioumatch_amd.votenet.step")
        det = step.build_detector(cfg, seed=0).to(DEV).eval()
        engine = I.InferenceEngine(det)
        distinct = [data.make_batch(B, 40000, cfg, seed=100 + s, device=DEV) for s in range(4)]
        batches = [distinct[i % 4] for i in range(n_batches)]
        times = {False: [], True: []}
        res = {}
        for rep in range(args.repeats + 1):
            for flag in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with np.errstate(invalid="ignore", divide="ignore"):
                    res[flag] = I.evaluate(engine, batches, cd, device_ap=flag)
                torch.cuda.synchronize()
                if rep:
                    times[flag].append((time.perf_counter() - t0) * 1e3)
        for g, w in zip(res[True], res[False]):
            np.testing.assert_allclose([g[k] for k in w], [w[k] for k in w], rtol=0, atol=1e-12, equal_nan=True)
        with torch.no_grad():
            frac = E.parse_predictions_device(engine(batches[0]["point_clouds"]), cd)["keep"].float().mean().item()
        out.update({"evaluate_host_ap_ms": med(times[False]), "evaluate_host_ap_ms_repeats": [round(x, 1) for x in times[False]],
                    "evaluate_device_ap_ms": med(times[True]),
                    "evaluate_device_ap_ms_repeats": [round(x, 1) for x in times[True]],
                    "evaluate_ms_per_batch_host_ap": round(statistics.median(times[False]) / n_batches, 3),
                    "evaluate_ms_per_batch_device_ap": round(statistics.median(times[True]) / n_batches, 3),
                    "evaluate_kept_fraction_random_weights": round(frac, 3)})
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
