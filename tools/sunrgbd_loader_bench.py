"""Measure the SUN RGB-D scene loader (votenet/sunrgbd_data.py, csrc/sunrgbd_batch.hip) on one GPU:

    python tools/sunrgbd_loader_bench.py [--scenes 24] [--steps 20] [--repeats 3] [--builds-only]
                                         [--votes {file,boxes}] [--compare-votes]

SUN RGB-D-sized synthetic scans (50k points, 12 oriented boxes, votes) are written in the on-disk
layout into a temporary directory and loaded through the real reader.  Prints ONE JSON line:
  build_ms          device time per batch: 20 builds captured into one graph, replayed between
                    events (pretrain 16 x 20k, semi-supervised 4 + 8 x 20k; xyz + height)
  build_bytes       the bytes such a batch must move (gathered rows read, outputs written), the
                    achieved bytes per second, and that as a fraction of PEAK_HBM
  build_host_ms     the same builds issued from Python one after another: the host's enqueue cost
  scannet_build_ms  the ScanNet builder's pretrain batch of the same B x N (8 x 40k), measured here
                    with tools/scene_loader_bench.py's build_ms: the yardstick of the points kernel
  step_ms           per-step time of SupervisedStep / SemiSupervisedStep fed by the loader on the
                    side stream (`feed`) and fed by bench.py-style rotating pinned batches (three
                    device sets, one copy stream), the two alternated, --repeats each: median and
                    spread (max - min) of the repeats
  host_ms_per_scene the numpy restatement per scene on this host's CPU (one core), the comparison
--votes boxes measures a store without vote rows (the builder computes them from the boxes; the vote
files of the synthetic scans are then never opened).  --compare-votes holds BOTH stores in one
process and alternates them: `votes_ab` = store_bytes, build_ms (median and spread of --repeats per
store and batch kind) and, unless --builds-only, the supervised step fed by each store.
Kernel times: `rocprofv3 --kernel-trace --stats -f csv -d DIR -o run -- python
tools/sunrgbd_loader_bench.py --builds-only`.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
importlib.import_module("3dioumatch_amd")
V = importlib.import_module("3dioumatch_amd.votenet")
SD = importlib.import_module("3dioumatch_amd.votenet.sunrgbd_data")
SN = importlib.import_module("3dioumatch_amd.votenet.scannet_data")
SB = importlib.import_module("scene_loader_bench")
NPTS, B, LAB, UNL = 20000, 16, 4, 8
PEAK_HBM = 8.0e12  # bytes / s, the MI355X's nominal HBM3E rate


def batch_bytes(kind, channels, votes="file"):
    """Bytes one batch must move: per student slot of a vote row a cloud row and (a "file" store) a
    vote row read, a cloud row, nine vote floats and an int64 mask written; other slots (unlabeled
    students, every teacher slot) a cloud row read and written.  Box labels and draws are a few KB:
    left out."""
    cloud = 4 * channels
    vote_rows, rows, copies = (B, B, 1) if kind == "pretrain" else (LAB, LAB + UNL, 2)
    return NPTS * (rows * copies * 2 * cloud + vote_rows * ((40 if votes == "file" else 0) + 36 + 8))


def store_bytes(scenes):
    return int(sum(t.numel() * t.element_size() for t in scenes.dev.values()))


def compare_votes(stores, loaders, cfg, args):
    """Both stores in one process, alternated: device time per batch and the fed supervised step."""
    out = {"store_bytes": {m: store_bytes(stores[m]) for m in stores}, "build_ms": {}}
    for kind in ("pretrain", "semi"):
        runs = {m: [] for m in loaders}
        for _ in range(args.repeats):
            for m in loaders:
                runs[m].append(build_ms(loaders[m], kind, replays=50)[0])
        out["build_ms"][kind] = {m: {"median": round(float(np.median(r)), 4), "spread": round(max(r) - min(r), 4),
                                     "runs": [round(x, 4) for x in r]} for m, r in runs.items()}
    if args.builds_only:
        return out
    runner = V.SupervisedStep(cfg, torch.device("cuda", 0), num_proposal=256, lr=1e-3)
    for m in loaders:
        fed_ms(runner, loaders[m], "pretrain", 4, 1000)  # capture + warm-up
    runs = {m: [] for m in loaders}
    for r in range(args.repeats):
        for m in loaders:
            runs[m].append(fed_ms(runner, loaders[m], "pretrain", args.steps, 10 * r))
    out["fed_step_ms"] = {m: {"median": round(float(np.median(r)), 4), "spread": round(max(r) - min(r), 4),
                              "runs": [round(x, 4) for x in r]} for m, r in runs.items()}
    return out


def build_ms(loader, kind, reps=20, replays=5):
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
    for _ in range(replays):
        graph.replay()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / (replays * reps), host


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


def scannet_build_ms(tmp):
    """The ScanNet builder's pretrain batch at the same B x N (8 x 40k of 50k-point scans)."""
    names = ["scene%04d_00" % i for i in range(SB.B)]
    SN.write_synthetic_scans(tmp, names, num_points=50000, instances=40, boxes=25, seed=0)
    scenes = SN.ScanNetScenes(tmp, names, torch.device("cuda", 0), use_color=False, use_height=True)
    loader = SN.ScanNetLoader(scenes, V.scannet_config(), SB.NPTS, seed=0)
    return SB.build_ms(loader, "pretrain")[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=24)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--builds-only", action="store_true", help="no train steps (for a kernel trace)")
    ap.add_argument("--votes", choices=("file", "boxes"), default="file",
                    help="the store's vote rows: read from _votes.npz, or computed from the boxes")
    ap.add_argument("--compare-votes", action="store_true",
                    help="measure a 'file' and a 'boxes' store alternated in this process, and nothing else")
    args = ap.parse_args()
    if args.scenes < B + UNL:
        ap.error("--scenes must be at least %d" % (B + UNL))
    dev = torch.device("cuda", 0)
    result = {"num_points": NPTS, "batch": {"pretrain": B, "semi": [LAB, UNL]}, "votes": args.votes}
    with tempfile.TemporaryDirectory() as tmp:
        names = ["%06d" % (i + 1) for i in range(args.scenes)]
        SD.write_synthetic_scans(tmp, names, num_points=50000, boxes=12, seed=0)
        if args.compare_votes:
            cfg = V.sunrgbd_config()
            stores = {m: SD.SunRgbdScenes(tmp, names, dev, use_color=False, use_height=True, votes=m)
                      for m in ("file", "boxes")}
            loaders = {m: SD.SunRgbdLoader(st, cfg, NPTS, seed=0, labeled=names[:B], unlabeled=names[B:])
                       for m, st in stores.items()}
            del result["votes"]
            result["votes_ab"] = compare_votes(stores, loaders, cfg, args)
            print(json.dumps(result))
            return
        t = time.perf_counter()
        scenes = SD.SunRgbdScenes(tmp, names, dev, use_color=False, use_height=True, votes=args.votes)
        result["load_s"] = round(time.perf_counter() - t, 3)
        result["store_bytes"] = store_bytes(scenes)
    with tempfile.TemporaryDirectory() as tmp:
        result["scannet_build_ms"] = {"pretrain_8x40000": round(scannet_build_ms(tmp), 4)}
    cfg = V.sunrgbd_config()
    loader = SD.SunRgbdLoader(scenes, cfg, NPTS, seed=0, labeled=names[:B], unlabeled=names[B:])
    result["build_ms"], result["build_host_ms"], result["build_bytes"] = {}, {}, {}
    for k in ("pretrain", "semi"):
        dev_ms, host_ms = build_ms(loader, k)
        nbytes = batch_bytes(k, scenes.channels, args.votes)
        result["build_ms"][k], result["build_host_ms"][k] = round(dev_ms, 4), round(host_ms, 4)
        result["build_bytes"][k] = {"bytes": nbytes, "bytes_per_s": round(nbytes / (dev_ms * 1e-3), 0),
                                    "fraction_of_peak_hbm": round(nbytes / (dev_ms * 1e-3) / PEAK_HBM, 4)}
    # host restatement, one core of this host
    t = time.perf_counter()
    for c in range(4):
        loader.host_batch("pretrain", [c % len(loader.labeled)], None, c)
    result["host_ms_per_scene"] = {"pretrain": round((time.perf_counter() - t) / 4 * 1e3, 2)}
    t = time.perf_counter()
    for c in range(4):
        loader.host_batch("semi", [], [c % len(loader.unlabeled)], c)
    result["host_ms_per_scene"]["semi_unlabeled"] = round((time.perf_counter() - t) / 4 * 1e3, 2)
    if args.builds_only:
        print(json.dumps(result))
        return
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
        SB.rotating_ms(runner, pinned, 4, copy_stream)
        for r in range(args.repeats):
            fed.append(fed_ms(runner, loader, kind, args.steps, 10 * r))
            rot.append(SB.rotating_ms(runner, pinned, args.steps, copy_stream))
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
