"""Time the point-count kernel of `remove_empty_box` (csrc/box_points.hip) at the evaluation shape
(B = 8 scenes, K = 256 proposals, N = 40 000 points of 4 floats) against the plain tensor formulation
of the same count -- a broadcast (B,K,N) mask summed over N, what one would write without the
kernel -- in one process:

    python tools/parse_empty_bench.py [--out profiles/parse_empty_box.json] [--reps 200]

Device time between two events, after a warm-up of every shape, the two alternating over `--rounds`
windows; the counts of both are compared first.  The kernel's calls are captured into one HIP graph
of `--reps` calls and the window replays it, so that the tens of microseconds of a call are not
hidden behind the host's enqueue (`kernel_call_us` is the same window with eager calls, enqueue
included); the tensor formulation runs eagerly, its kernels take milliseconds.  Prints one JSON line
and writes it to --out.  Needs the GPU: there is no host fall-back.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
importlib.import_module("3dioumatch_amd")
P = importlib.import_module("3dioumatch_amd.votenet.pseudo_nms")


def make_case(b, k, n, pstride, seed, dev):
    """boxes and points around common clumps of a room-sized scene, so that boxes hold points"""
    rng = np.random.default_rng(seed)
    clumps = rng.uniform(-3, 3, (b, 12, 3))
    pick = lambda m: np.take_along_axis(clumps, rng.integers(0, 12, (b, m))[..., None].repeat(3, -1), 1)  # noqa: E731
    points = np.zeros((b, n, pstride), np.float32)
    points[..., :3] = pick(n) + rng.normal(0, 0.5, (b, n, 3))
    center = (pick(k) + rng.normal(0, 0.3, (b, k, 3))).astype(np.float32)
    size = rng.uniform(0.3, 2.0, (b, k, 3))
    heading = rng.uniform(-np.pi, np.pi, (b, k))
    return [torch.from_numpy(a).to(dev) for a in (points, center, size, heading)]


def count_tensor(points, center, size, heading):
    """the same test as broadcast tensor ops: (B,K,N) intermediates, summed over N"""
    c, s = torch.cos(heading).float()[..., None], torch.sin(heading).float()[..., None]
    half = (size / 2).float()
    dx = points[:, None, :, 0] - center[:, :, None, 0]
    dy = points[:, None, :, 1] - center[:, :, None, 1]
    dz = points[:, None, :, 2] - center[:, :, None, 2]
    inside = ((c * dx - s * dy).abs() <= half[..., 0:1]) & ((s * dx + c * dy).abs() <= half[..., 1:2]) & \
        (dz.abs() <= half[..., 2:3])
    return inside.sum(-1, dtype=torch.int32)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3     # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--boxes", type=int, default=256)
    ap.add_argument("--points", type=int, default=40000)
    ap.add_argument("--pstride", type=int, default=4)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parse_empty_box.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("parse_empty_bench: needs the GPU (nothing is measured on the host)")
    dev = torch.device("cuda:0")
    case = make_case(args.scenes, args.boxes, args.points, args.pstride, 0, dev)
    out = torch.empty((args.scenes, args.boxes), dtype=torch.int32, device=dev)
    kernel = lambda: P.box_point_count_gpu(*case, out=out)  # noqa: E731
    tensor = lambda: count_tensor(*case)                     # noqa: E731
    got, want = kernel().cpu(), tensor().cpu()
    # both forms round every float32 operation in the same order; their float64 cos / sin come from
    # different libraries, so a count can differ only where a last-bit difference there survives the
    # rounding to float32 AND a point grazes that face: reported, expected 0
    differ = int((got != want).sum())
    for _ in range(3):
        kernel()
        tensor()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(args.reps):
            kernel()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), got)
    k_us, c_us, t_us = [], [], []
    for _ in range(args.rounds):             # alternate, so that both see the same machine
        k_us.append(timed(graph.replay, 4) / args.reps)
        c_us.append(timed(kernel, args.reps))
        t_us.append(timed(tensor, max(1, args.reps // 10)))
    pairs = args.scenes * args.boxes * args.points
    res = {"what": "points inside each box, %d scenes x %d boxes x %d points (pstride %d)" %
                   (args.scenes, args.boxes, args.points, args.pstride),
           "device": torch.cuda.get_device_name(0), "pairs": pairs,
           "kernel_us": round(float(np.median(k_us)), 2), "kernel_us_rounds": [round(v, 2) for v in k_us],
           "kernel_call_us": round(float(np.median(c_us)), 2),
           "kernel_includes": "the zero fill of the counts and the count kernel (one entry-point call)",
           "tensor_us": round(float(np.median(t_us)), 1), "tensor_us_rounds": [round(v, 1) for v in t_us],
           "tensor_over_kernel": round(float(np.median(t_us) / np.median(k_us)), 1),
           "kernel_pairs_per_s": round(pairs / (float(np.median(k_us)) * 1e-6)),
           "boxes_nonempty": int((got >= 5).sum()), "boxes": int(got.numel()),
           "counts_differing_from_tensor_form": differ,
           "reps": args.reps, "rounds": args.rounds}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
