"""Where the time of a raw SUN RGB-D export goes (votenet/sunrgbd_raw.py, csrc/sunrgbd_raw.hip), per scene
of a synthetic depth cloud of the real size (sunrgbd_raw.synthetic_trainval: 300 000 raw points kept to
50 000, 12 objects), for float32 and for float64 clouds:

    python tools/sunrgbd_raw_bench.py [--repeats 5] [--out profiles/sunrgbd_raw.json]
    python tools/sunrgbd_raw_bench.py --no_device --reference REFERENCE_TREE --out profiles/sunrgbd_raw.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o raw -- python tools/sunrgbd_raw_bench.py --trace_pass
    python tools/sunrgbd_raw_bench.py --kernel_stats DIR --out profiles/sunrgbd_raw.json

  read_ms        host: read_mat_points of one depth file (`inflate`: its zlib.decompress alone) and
                 read_labels of one label file
  numpy_ms       host_export_trainval_scene, the numpy restatement
  device_us      the three launches of scene_sunrgbd_raw_export for a chunk of 8 scenes, per scene: 10
                 exports captured into one graph, replayed 50 times between events; --repeats times:
                 median, spread, runs
  export_ms      export_trainval on the device end to end for the chunk, per scene: pack, upload,
                 launches, copy back, slicing
  launch_us      with --kernel_stats: each kernel's mean time per scene from the profiler's summary of a
                 --trace_pass run (20 exports of the chunk per dtype, nothing else timed in that run)
  reference_ms   with --reference: extract_sunrgbd_data(save_votes=True) of the reference tree on this CPU
                 for two of the float32 scenes, per scene, its unused imports stubbed as in
                 tests/golden/make_sunrgbd_raw_golden.py; votes_ms is sunrgbd_data.compute_votes, the
                 part of it that a store built here does per sampled point on the device instead
  equal          the device export compared with the restatement word for word at the timed shape

--out merges the keys it measured into the file's JSON line, so that the host-only run with the
reference, the run on the GPU and the profiler's summary fill one record.  Nothing here asserts a time."""
import argparse
import csv
import importlib
import json
import os
import re
import sys
import tempfile
import time
import types
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
importlib.import_module("3dioumatch_amd")
R = importlib.import_module("3dioumatch_amd.votenet.sunrgbd_raw")
RAW_POINTS, OBJECTS, SCENES = 300000, 12, 8
BUILDS, REPLAYS, TRACE_EXPORTS = 10, 50, 20
DTYPES = (("float32", np.float32), ("float64", np.float64))


def best(f, repeats):
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = f()
        times.append((time.perf_counter() - t0) * 1e3)
    return r, {"median": round(float(np.median(times)), 3), "spread": round(max(times) - min(times), 3)}


def inflate(path):
    with open(path, "rb") as f:
        buf = f.read()
    return zlib.decompress(buf[136:])  # the header, the compressed element's tag, its data


def reference_extract(tree, trainval, scenes):
    for name in ("cv2", "mayavi", "mayavi.mlab", "plyfile", "trimesh", "matplotlib", "matplotlib.pyplot"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["mayavi"].mlab = sys.modules["mayavi.mlab"]
    sys.modules["plyfile"].PlyData = sys.modules["plyfile"].PlyElement = object
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    sys.modules["matplotlib.pyplot"].cm = types.SimpleNamespace(jet=None)
    for p in (os.path.join(tree, "utils"), os.path.join(tree, "sunrgbd")):
        sys.path.insert(0, p)
    ref = importlib.import_module("sunrgbd_data")
    here, parent = os.getcwd(), os.path.dirname(trainval)  # it opens './sunrgbd_trainval'
    idx = os.path.join(parent, "idx.txt")
    with open(idx, "w") as f:
        f.write("".join("%d\n" % int(s) for s in scenes))
    os.chdir(parent)
    try:
        with open(os.devnull, "w") as quiet:
            stdout, sys.stdout = sys.stdout, quiet
            try:
                t0 = time.perf_counter()
                ref.extract_sunrgbd_data(idx, "training", os.path.join(parent, "ref_out"), num_point=R.NUM_POINT,
                                         save_votes=True, use_v1=True, skip_empty_scene=False)
                elapsed = (time.perf_counter() - t0) * 1e3
            finally:
                sys.stdout = stdout
    finally:
        os.chdir(here)
    return {"per_scene": round(elapsed / len(scenes), 1), "scenes": len(scenes)}


def kernel_stats(where):
    """{kernel: mean microseconds per scene} of the sun_raw kernels in the profiler's *kernel_stats.csv."""
    out = {}
    for folder, _, files in os.walk(where):
        for name in files:
            if not name.endswith("kernel_stats.csv"):
                continue
            with open(os.path.join(folder, name), newline="") as f:
                for row in csv.DictReader(f):
                    kernel = re.search(r"sun_raw_\w+<\w+>", row.get("Name", ""))
                    if kernel:
                        out[kernel.group(0)] = {"us_per_scene": round(float(row["AverageNs"]) / 1e3 / SCENES, 2),
                                                "calls": int(row["Calls"])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="merge the measured keys into this file's JSON line")
    ap.add_argument("--no_device", action="store_true", help="host measurements only")
    ap.add_argument("--reference", default=None, metavar="DIR", help="the reference tree: time its extraction too")
    ap.add_argument("--trace_pass", action="store_true", help="only launch, for a profiler's kernel trace")
    ap.add_argument("--kernel_stats", default=None, metavar="DIR", help="merge a --trace_pass run's kernel summary")
    args = ap.parse_args()
    result = {"raw_points": RAW_POINTS, "num_point": R.NUM_POINT, "objects": OBJECTS, "chunk_scenes": SCENES}
    if args.kernel_stats:
        result = {"launch_us": kernel_stats(args.kernel_stats)}
        if not result["launch_us"]:
            raise SystemExit("no sun_raw kernel in a *kernel_stats.csv under %s" % args.kernel_stats)
    for tag, dtype in () if args.kernel_stats else DTYPES:
        part = result[tag] = {}
        with tempfile.TemporaryDirectory() as tmp:
            trainval = os.path.join(tmp, "sunrgbd_trainval")
            names = R.synthetic_trainval(trainval, SCENES, RAW_POINTS, OBJECTS, seed=1, dtype=dtype)
            depth = os.path.join(trainval, "depth", names[0] + ".mat")
            if not args.trace_pass:
                _, mat = best(lambda: R.read_mat_points(depth), args.repeats)
                _, unzip = best(lambda: inflate(depth), args.repeats)
                _, labels = best(lambda: R.read_labels(os.path.join(trainval, "label_v1", names[0] + ".txt")), args.repeats)
                part["read_ms"] = {"read_mat_points": mat, "inflate": unzip, "read_labels": labels,
                                   "file_bytes": os.path.getsize(depth)}
                rec = R.read_trainval_scene(trainval, names[0])
                host, part["numpy_ms"] = best(lambda: R.host_export_trainval_scene(rec), args.repeats)
                if args.reference and dtype == np.float32:
                    SUN = importlib.import_module("3dioumatch_amd.votenet.sunrgbd_data")
                    _, part["votes_ms"] = best(lambda: SUN.compute_votes(host["rows"], host["bbox"]), args.repeats)
                    part["reference_ms"] = reference_extract(args.reference, trainval, names[:2])
            records = None if args.no_device else [R.read_trainval_scene(trainval, s) for s in names]
        if records is None:
            continue
        import torch
        dev = torch.device("cuda", 0)
        staged = R._stage_chunk(list(enumerate(records)), dev, R.NUM_POINT, 0, None)
        if args.trace_pass:
            for _ in range(TRACE_EXPORTS):
                R._launch_staged(staged, fresh=False)
            torch.cuda.synchronize()
            continue
        got, end = best(lambda: R.export_trainval(records, dev), args.repeats)
        part["export_ms"] = {k: round(v / SCENES, 3) for k, v in end.items()}
        keys = ("pc", "bbox", "rows")
        equal = all(np.array_equal(got[0][k].view(np.uint8), host[k].view(np.uint8)) for k in keys)
        R._launch_staged(staged)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(BUILDS):
                R._launch_staged(staged, fresh=False)
        graph.replay()
        torch.cuda.synchronize()
        runs = []
        for _ in range(args.repeats):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(REPLAYS):
                graph.replay()
            t1.record()
            torch.cuda.synchronize()
            runs.append(t0.elapsed_time(t1) * 1e3 / (REPLAYS * BUILDS * SCENES))
        part["device_us"] = {"median": round(float(np.median(runs)), 2), "spread": round(max(runs) - min(runs), 2),
                             "runs": [round(x, 2) for x in runs], "launches": 3}
        after = R._collect(staged)
        part["equal"] = bool(equal and got[0]["floor"] == host["floor"] and all(
            np.array_equal(after[0][k].view(np.uint8), host[k].view(np.uint8)) for k in keys))
    if args.trace_pass:
        return
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            merged = json.loads(f.read() or "{}")
        for k, v in result.items():  # a dtype's record is filled by several runs
            if isinstance(v, dict) and isinstance(merged.get(k), dict):
                merged[k].update(v)
            else:
                merged[k] = v
        result = merged
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
