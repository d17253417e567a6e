"""Time the inference engine (votenet/inference.py) against the plain eval forward on ScanNet-sized
(B = 8, N = 40 000, K = 256) and SUN RGB-D-sized (B = 16, N = 20 000) batches, a detector with
seeded weights and non-trivial running statistics in eval mode.

    python tools/infer_bench.py [--iters 20] [--warmup 3] [--batches 4] [--profile-one]

Prints one JSON line; per config (device events, medians):
  plain_ms        detector({'point_clouds': pc}) under no_grad, ms per batch (index chain inline)
  engine_ms       engine(pc): one batch, index chain inline + the captured forward, ms
  forward_ms      the engine's forward alone (index chain computed beforehand), ms
  geometry_ms     the index chain alone (detector.compute_geometry), ms
  pipelined_scenes_per_s   engine.run() over --batches rotating distinct batches
  max_abs_diff    largest |engine - plain| over the float end_points keys of one batch
  bound           which of forward / index chain the pipelined loop is bound by
--profile-one: one eager ScanNet engine batch and one plain eval forward of it, each after a warm-up
(for rocprofv3 --kernel-trace --stats: the fused kernels next to the unfused ones they replace).
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
I = importlib.import_module("3dioumatch_amd.votenet.inference")
step = importlib.import_module("3dioumatch_amd.votenet.step")
data = importlib.import_module("3dioumatch_amd.votenet.data")

CONFIGS = {"scannet": (8, 40000), "sunrgbd": (16, 20000)}


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


def seeded_detector(tag, dev):
    cfg = V.scannet_config() if tag == "scannet" else V.sunrgbd_config()
    det = step.build_detector(cfg, seed=0).to(dev)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for bn in det.modules():
            if isinstance(bn, torch.nn.modules.batchnorm._BatchNorm):
                c = bn.num_features
                bn.running_mean.copy_(torch.randn(c, generator=g) * 0.3)
                bn.running_var.copy_(0.3 + torch.rand(c, generator=g) * 2.0)
    return det.eval(), cfg


def bench(tag, args, dev):
    b, n = CONFIGS[tag]
    det, cfg = seeded_detector(tag, dev)
    clouds = [data.make_batch(b, n, cfg, seed=100 + s, device=dev)["point_clouds"] for s in range(args.batches)]
    engine = I.InferenceEngine(det)
    pc = clouds[0]
    with torch.no_grad():
        plain = det({"point_clouds": pc})
    got = engine(pc)
    diff = 0.0
    for k, v in plain.items():
        if torch.is_tensor(v) and v.is_floating_point():
            diff = max(diff, (got[k] - v).abs().max().item())
    with torch.no_grad():
        plain_ms = timed(lambda: det({"point_clouds": pc}), args.iters, args.warmup)
    engine_ms = timed(lambda: engine(pc), args.iters, args.warmup)
    geo = engine._geometry(pc)
    forward_ms = timed(lambda: engine._run_forward(pc, geo), args.iters, args.warmup)
    geometry_ms = timed(lambda: engine._geometry(pc), args.iters, args.warmup)
    rounds = max(1, args.iters // len(clouds))
    run_ms = timed(lambda: [None for _ in engine.run(clouds * rounds)], 3, 1)
    per_batch = run_ms / (len(clouds) * rounds)
    return {"B": b, "N": n, "plain_ms": round(plain_ms, 3), "engine_ms": round(engine_ms, 3),
            "forward_ms": round(forward_ms, 3), "geometry_ms": round(geometry_ms, 3),
            "pipelined_ms_per_batch": round(per_batch, 3),
            "pipelined_scenes_per_s": round(1000.0 * b / per_batch, 1),
            "bound": "index chain" if geometry_ms >= forward_ms else "forward",
            "fused_call_sites": sum(1 for p in engine.plans.values() if p.hits > 0),
            "max_abs_diff": diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--profile-one", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("infer_bench needs a GPU")
    dev = torch.device("cuda:0")
    if args.profile_one:
        det, cfg = seeded_detector("scannet", dev)
        engine = I.InferenceEngine(det, graphs=False)
        pc = data.make_batch(8, 40000, cfg, seed=100, device=dev)["point_clouds"]
        engine(pc)
        with torch.no_grad():
            det({"point_clouds": pc})
        torch.cuda.synchronize()
        engine(pc)  # the profiled pair: one engine batch, one plain eval forward of the same batch
        with torch.no_grad():
            det({"point_clouds": pc})
        torch.cuda.synchronize()
        print(json.dumps({"profiled": "one eager engine batch + one plain eval forward, after a warm-up of each"}))
        return
    out = {"tool": "infer_bench", "device": torch.cuda.get_device_name(0)}
    for tag in CONFIGS:
        out[tag] = bench(tag, args, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
