"""Measure the ScanNet scene loader (votenet/scannet_data.py, csrc/scene_batch.hip) on one GPU:

    python tools/scene_loader_bench.py [--scenes 16] [--steps 20] [--repeats 3]

ScanNet-sized synthetic scans (50k points, 40 instances, 25 boxes) are written in the preprocessed
layout into a temporary directory and loaded through the real reader.  Prints ONE JSON line:
  build_ms          device time per batch: 20 builds captured into one graph, replayed between
                    events (pretrain 8 x 40k, semi-supervised 4 + 8 x 40k)
  build_host_ms     the same builds issued from Python one after another: the host's enqueue cost
  step_ms           per-step time of SupervisedStep / SemiSupervisedStep fed by the loader on the
                    side stream (`feed`) and fed by bench.py-style rotating pinned batches (three
                    device sets, one copy stream), the two alternated, --repeats each: median and
                    spread (max - min) of the repeats
  host_ms_per_scene the numpy restatement per scene on this host's CPU (one core), the comparison
Kernel times: `rocprofv3 --kernel-trace --stats -f csv -d DIR -o run -- python tools/scene_loader_bench.py`.
"""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
importlib.import_module("3dioumatch_amd")
V = importlib.import_module("3dioumatch_amd.votenet")
SD = importlib.import_module("3dioumatch_amd.votenet.scannet_data")
NPTS, B, LAB, UNL = 40000, 8, 4, 8


def build_ms(loader, kind, reps=20):
    """(device ms, host ms) per build.  Device: `reps` builds captured into ONE graph and replayed,
    so the host's enqueue rate does not enter (events around the replays).  Host: `reps` builds
    issued back to back from Python, the rate a caller can enqueue them."""
    out = loader.allocate(kind, B if kind == "pretrain" else LAB, 0 if kind == "pretrain" else UNL)
    ids = np.arange(B) % len(loader.labeled)

    def one(c):
        if kind == "pretrain":
            loader.pretrain_batch(ids, c, out=out)
        else:
            loader.semi_batch(ids[:LAB], np.arange(UNL) % len(loader.unlabeled), c, out=out)

    one(0)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for c in range(reps):
        one(c + 1)
    torch.cuda.synchronize()
    host = (time.perf_counter() - t) * 1e3 / reps
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for c in range(reps):
            one(1000 + c)
    graph.replay()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(5):
        graph.replay()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / (5 * reps), host


def plan_of(kind, loader, steps, epoch0):
    items = []
    e = epoch0
    while len(items) < steps:
        if kind == "semi":
            items += list(SD.epoch_plan(len(loader.labeled), LAB, e, num_unlabeled=len(loader.unlabeled),
                                        unlabeled_batch_size=UNL))
        else:
            items += list(SD.epoch_plan(len(loader.labeled), B, e))
        e += 1
    return items[:steps]


def fed_ms(runner, loader, kind, steps, epoch0):
    main = torch.cuda.current_stream()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    losses = []
    for i, b in enumerate(SD.feed(runner, loader, plan_of(kind, loader, steps + 2, epoch0), kind=kind)):
        if i == 2:
            t0.record(main)
        loss, _ = runner(b)
        losses.append(loss.detach().clone())  # graph mode returns one static loss buffer
    t1.record(main)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(torch.stack(losses)).all()), "non-finite loss"
    return t0.elapsed_time(t1) / steps


def rotating_ms(runner, pinned, steps, copy_stream):
    main = torch.cuda.current_stream()
    sets = [{k: torch.empty_like(v, device="cuda") if torch.is_tensor(v) else v for k, v in pinned[0].items()}
            for _ in range(3)]
    filled, consumed = [torch.cuda.Event() for _ in range(3)], [torch.cuda.Event() for _ in range(3)]
    for ev in consumed:
        ev.record(main)

    def upload(i):
        s = i % 3
        copy_stream.wait_event(consumed[s])
        with torch.cuda.stream(copy_stream):
            for k, v in pinned[i % len(pinned)].items():
                if torch.is_tensor(v):
                    sets[s][k].copy_(v, non_blocking=True)
            filled[s].record(copy_stream)

    def view(i):
        return dict(sets[i % 3])

    upload(0)
    upload(1)
    main.wait_event(filled[0])
    views = {0: view(0)}
    runner.prefetch_geometry(views[0])
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    losses = []
    for i in range(steps + 2):
        if i == 2:
            t0.record(main)
        upload(i + 2)
        main.wait_event(filled[(i + 1) % 3])
        views[i + 1] = view(i + 1)
        runner.prefetch_geometry(views[i + 1])
        main.wait_event(filled[i % 3])
        loss, _ = runner(views.pop(i))
        losses.append(loss.detach().clone())
        consumed[i % 3].record(main)
    t1.record(main)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(torch.stack(losses)).all()), "non-finite loss"
    runner(views.pop(steps + 2))  # leave no prefetched slot pending
    return t0.elapsed_time(t1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    result = {"num_points": NPTS}
    with tempfile.TemporaryDirectory() as tmp:
        names = ["scene%04d_00" % i for i in range(args.scenes)]
        SD.write_synthetic_scans(tmp, names, num_points=50000, instances=40, boxes=25, seed=0)
        t = time.perf_counter()
        scenes = SD.ScanNetScenes(tmp, names, dev, use_color=False, use_height=True)
        result["load_s"] = round(time.perf_counter() - t, 3)
    cfg = V.scannet_config()
    half = args.scenes // 2
    loader = SD.ScanNetLoader(scenes, cfg, NPTS, seed=0, labeled=names[:max(half, B)],
                              unlabeled=names[half:] if args.scenes - half >= UNL else names)
    result["build_ms"], result["build_host_ms"] = {}, {}
    for k in ("pretrain", "semi"):
        dev_ms, host_ms = build_ms(loader, k)
        result["build_ms"][k], result["build_host_ms"][k] = round(dev_ms, 4), round(host_ms, 4)
    # host restatement, one core of this host
    t = time.perf_counter()
    for c in range(4):
        loader.host_batch("pretrain", [c % len(loader.labeled)], None, c)
    result["host_ms_per_scene"] = {"pretrain": round((time.perf_counter() - t) / 4 * 1e3, 2)}
    t = time.perf_counter()
    for c in range(4):
        loader.host_batch("semi", [], [c % len(loader.unlabeled)], c)
    result["host_ms_per_scene"]["semi_unlabeled"] = round((time.perf_counter() - t) / 4 * 1e3, 2)
    copy_stream = torch.cuda.Stream(device=dev)
    steps = {}
    for kind in ("pretrain", "semi"):
        if kind == "semi":
            runner = V.SemiSupervisedStep(cfg, dev, num_proposal=256, lr=2e-3)
            ids = [(np.arange(LAB) + i) % len(loader.labeled) for i in range(4)]
            pinned = [loader.semi_batch(l, (np.arange(UNL) + i) % len(loader.unlabeled), 100 + i)
                      for i, l in enumerate(ids)]
        else:
            runner = V.SupervisedStep(cfg, dev, num_proposal=256, lr=1e-3)
            pinned = [loader.pretrain_batch((np.arange(B) + i) % len(loader.labeled), 100 + i)
                      for i in range(4)]
        pinned = [{k: (v.cpu().pin_memory() if torch.is_tensor(v) else v) for k, v in p.items()}
                  for p in pinned]
        fed, rot = [], []
        fed_ms(runner, loader, kind, 4, 1000)  # capture + warm-up
        rotating_ms(runner, pinned, 4, copy_stream)
        for r in range(args.repeats):
            fed.append(fed_ms(runner, loader, kind, args.steps, 10 * r))
            rot.append(rotating_ms(runner, pinned, args.steps, copy_stream))
        steps[kind] = {"fed_ms": round(float(np.median(fed)), 4), "fed_spread_ms": round(max(fed) - min(fed), 4),
                       "rotating_ms": round(float(np.median(rot)), 4),
                       "rotating_spread_ms": round(max(rot) - min(rot), 4),
                       "fed_runs": [round(x, 4) for x in fed], "rotating_runs": [round(x, 4) for x in rot]}
        del runner
        torch.cuda.synchronize()
    result["step_ms"] = steps
    print(json.dumps(result))


if __name__ == "__main__":
    main()
