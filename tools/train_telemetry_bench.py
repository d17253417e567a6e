"""What the training loop's logging costs per step, at the bench's ScanNet shapes with the feeding loop
(scannet_data.feed): pretrain B = 8, semi 4 + 8, N = 40000 points, K = 256 proposals.

    python tools/train_telemetry_bench.py [--steps 50] [--repeats 3] [--out profiles/train_telemetry.json]

Four arms per stage, alternated inside ONE process (boxes differ by 2-3 %):
  a  everything off: the step as it was before the meter and the guard existed
  b  meter + guard on, the meter read once per 25 steps (the loop of votenet/trainer.py)
  c  everything off, plus the reference's statistics loop: one .item() per logged key and step
     (train.py:356-360), over the same keys
  d  b without the buffer rollback: no state arena, no votenet_guard_state_sync launch (the guard
     as it was before the rollback existed)
b - a is what the feature costs, c - a what it saves, b - d what the rollback's one launch adds.
Nothing here asserts a time."""
import argparse
import importlib
import json
import os
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
importlib.import_module("3dioumatch_amd")
V = importlib.import_module("3dioumatch_amd.votenet")
SD = importlib.import_module("3dioumatch_amd.votenet.scannet_data")
TM = importlib.import_module("3dioumatch_amd.votenet.train_meter")

NPTS, B, LAB, UNL, PRINT = 40000, 8, 4, 8, 25


def plan_of(kind, loader, steps, epoch0):
    items, e = [], epoch0
    while len(items) < steps:
        if kind == "semi":
            items += list(SD.epoch_plan(len(loader.labeled), LAB, e, num_unlabeled=len(loader.unlabeled),
                                        unlabeled_batch_size=UNL))
        else:
            items += list(SD.epoch_plan(len(loader.labeled), B, e))
        e += 1
    return items[:steps]


def fed_ms(runner, loader, kind, steps, epoch0, arm):
    """ms per step of `steps` fed steps (two more first, untimed), wall clock == device time at the end"""
    main = torch.cuda.current_stream()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    keys = None
    for i, batch in enumerate(SD.feed(runner, loader, plan_of(kind, loader, steps + 2, epoch0), kind=kind)):
        if i == 2:
            t0.record(main)
        _, ep = runner(batch)
        if arm == "c":
            keys = keys or TM.logged_keys(ep)
            stat = {}
            for k in keys:
                stat[k] = stat.get(k, 0) + ep[k].item()
        elif arm in ("b", "d") and (i + 1) % PRINT == 0:
            runner.meter.result()
    t1.record(main)
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def without_rollback(step_class):
    """arm d: the guarded runner of `step_class` that homes no buffers and so launches no state sync"""
    class NoRollback(step_class):
        def _home_guard_state(self, modules):
            pass
    return NoRollback


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=16)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_telemetry_bench: needs the GPU (no timing without it)")
    dev = torch.device("cuda", 0)
    with tempfile.TemporaryDirectory() as tmp:
        names = ["scene%04d_00" % i for i in range(args.scenes)]
        SD.write_synthetic_scans(tmp, names, num_points=50000, instances=40, boxes=25, seed=0)
        scenes = SD.ScanNetScenes(tmp, names, dev, use_color=False, use_height=True)
    cfg = V.scannet_config()
    half = args.scenes // 2
    loader = SD.ScanNetLoader(scenes, cfg, NPTS, seed=0, labeled=names[:max(half, B)],
                              unlabeled=names[half:] if args.scenes - half >= UNL else names)
    out = {"what": "ms per fed training step, ScanNet shapes (N = %d, K = 256); a: meter and guard off, "
                   "b: both on + one read per %d steps, c: off + one .item() per logged key and step, "
                   "d: b without the buffer rollback (no arena, no state-sync launch)"
                   % (NPTS, PRINT), "device": torch.cuda.get_device_name(0), "steps": args.steps,
           "repeats": args.repeats}
    for kind in ("pretrain", "semi"):
        step_class, lr = (V.SemiSupervisedStep, 2e-3) if kind == "semi" else (V.SupervisedStep, 1e-3)
        make = lambda cls=step_class, **kw: cls(cfg, dev, num_proposal=256, lr=lr, **kw)  # noqa: E731
        runners = {"a": make(), "b": make(meter=True, guard=True), "c": make(),
                   "d": make(without_rollback(step_class), meter=True, guard=True)}
        assert runners["d"].state_arena is None and runners["b"].state_arena is not None
        runs = {arm: [] for arm in runners}
        for arm, runner in runners.items():
            fed_ms(runner, loader, kind, 4, 1000, arm)  # capture + warm-up
        for r in range(args.repeats):
            for arm, runner in runners.items():
                runs[arm].append(fed_ms(runner, loader, kind, args.steps, 10 * r, arm))
        med = {arm: statistics.median(v) for arm, v in runs.items()}
        rep = runners["b"].guard_report()
        out[kind] = {
            "a_ms": round(med["a"], 4), "b_ms": round(med["b"], 4), "c_ms": round(med["c"], 4),
            "runs_ms": {arm: [round(x, 4) for x in v] for arm, v in runs.items()},
            "b_minus_a_us": round((med["b"] - med["a"]) * 1e3, 1),
            "b_minus_a_percent": round((med["b"] - med["a"]) / med["a"] * 100, 2),
            "c_minus_a_us": round((med["c"] - med["a"]) * 1e3, 1),
            "c_minus_a_percent": round((med["c"] - med["a"]) / med["a"] * 100, 2),
            "d_ms": round(med["d"], 4), "b_minus_d_us": round((med["b"] - med["d"]) * 1e3, 1),
            "b_minus_d_percent": round((med["b"] - med["d"]) / med["d"] * 100, 2),
            "state_arena_bytes": int(runners["b"].state_arena.numel()),
            "spread_ms": {arm: round(max(v) - min(v), 4) for arm, v in runs.items()},
            "logged_keys": len(runners["b"].meter.keys), "skipped_total": rep["skipped_total"],
            "meter_host_reads": runners["b"].meter.host_reads}
        del runners
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
