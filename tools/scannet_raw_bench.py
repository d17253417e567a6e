"""Where the time of a raw-ScanNet export goes (votenet/scannet_raw.py, csrc/scannet_raw.hip), per scan
of a synthetic 150 000-vertex mesh (scannet_raw.synthetic_raw_scan: 1500 segments, 40 objects):

    python tools/scannet_raw_bench.py [--repeats 5] [--out profiles/scannet_raw.json]
    python tools/scannet_raw_bench.py --no_device --reference REFERENCE_TREE --out profiles/scannet_raw.json

  parse_ms       host: the mesh file, the two JSON files and the seg tables (read_raw_scan), split into
                 ply / json / tables
  numpy_ms       host_export_raw_scan, the numpy restatement
  device_us      the launches of scannet_raw_export for a chunk of 8 scans, per scan: 10 exports captured
                 into one graph, replayed 50 times between events; --repeats times: median, spread, runs
  export_ms      export_raw_scans on the device end to end for the chunk, per scan: pack, upload,
                 launches, copy back, slicing
  reference_ms   with --reference: load_scannet_data.export of the reference tree on this CPU, its
                 `plyfile` a stub backed by read_ply_vertices as in tests/golden/make_scannet_raw_golden.py
  equal          the device export compared with the restatement word for word at the timed shape

--out merges the keys it measured into the file's JSON line, so that the host-only run with the
reference and the run on the GPU fill one record.  Nothing here asserts a time."""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
importlib.import_module("3dioumatch_amd")
R = importlib.import_module("3dioumatch_amd.votenet.scannet_raw")
VERTICES, OBJECTS, SCANS = 150000, 40, 8
BUILDS, REPLAYS = 10, 50


def best(f, repeats):
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = f()
        times.append((time.perf_counter() - t0) * 1e3)
    return r, {"median": round(float(np.median(times)), 3), "spread": round(max(times) - min(times), 3)}


def reference_export(tree, paths, tsv, repeats):
    class Element(object):
        def __init__(self, table):
            self.count = table.shape[0]
            self.data = {k: table[:, i] for i, k in enumerate(("x", "y", "z", "red", "green", "blue"))}

    class PlyData(object):
        @staticmethod
        def read(f):
            return {"vertex": Element(R.read_ply_vertices(f.name))}

    sys.modules["plyfile"] = types.ModuleType("plyfile")
    sys.modules["plyfile"].PlyData, sys.modules["plyfile"].PlyElement = PlyData, object
    sys.path.insert(0, os.path.join(tree, "scannet"))
    ref = importlib.import_module("load_scannet_data")
    return best(lambda: ref.export(paths["mesh"], paths["agg"], paths["seg"], paths["meta"], tsv), repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="merge the measured keys into this file's JSON line")
    ap.add_argument("--no_device", action="store_true", help="host measurements only")
    ap.add_argument("--reference", default=None, metavar="DIR", help="the reference tree: time its export too")
    args = ap.parse_args()
    result = {"vertices": VERTICES, "objects": OBJECTS, "chunk_scans": SCANS}
    with tempfile.TemporaryDirectory() as tmp:
        tsv = os.path.join(tmp, "labels.tsv")
        with open(tsv, "w") as f:
            f.write("id\traw_category\tnyu40id\n")
            for k, (label, nyu) in enumerate(sorted(R.SYNTHETIC_LABELS.items())):
                f.write("%d\t%s\t%d\n" % (k, label, nyu))
        names = ["scene%04d_00" % i for i in range(SCANS)]
        for i, name in enumerate(names):
            R.write_raw_scan(tmp, name, *R.synthetic_raw_scan(VERTICES, OBJECTS, seed=i))
        label_map = R.read_label_map(tsv)
        paths = {k: os.path.join(tmp, names[0], names[0] + s) for k, s in R.SUFFIXES.items()}
        _, ply = best(lambda: R.read_ply_vertices(paths["mesh"]), args.repeats)

        def jsons():
            with open(paths["seg"]) as f:
                seg = np.asarray(json.load(f)["segIndices"])
            with open(paths["agg"]) as f:
                return seg, json.load(f)["segGroups"]

        (seg, groups), js = best(jsons, args.repeats)
        _, tables = best(lambda: R.seg_tables(names[0], seg, [(g["objectId"], g["label"], g["segments"])
                                                              for g in groups], label_map), args.repeats)
        rec, whole = best(lambda: R.read_raw_scan(tmp, names[0], label_map), args.repeats)
        result["parse_ms"] = {"read_raw_scan": whole, "ply": ply, "json": js, "tables": tables}
        host, result["numpy_ms"] = best(lambda: R.host_export_raw_scan(rec), args.repeats)
        if args.reference:
            _, result["reference_ms"] = reference_export(args.reference, paths, tsv, max(1, args.repeats // 2))
        records = None if args.no_device else [R.read_raw_scan(tmp, s, label_map) for s in names]
    if records is not None:
        import torch
        dev = torch.device("cuda", 0)
        got, end = best(lambda: R.export_raw_scans(records, dev), args.repeats)
        result["export_ms"] = {k: round(v / SCANS, 3) for k, v in end.items()}
        result["equal"] = all(np.array_equal(got[0][k].view(np.uint8), host[k].view(np.uint8)) for k in host)
        staged = R._stage_chunk(list(enumerate(records)), dev, R.MAX_NUM_POINT, 0, None)
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
            runs.append(t0.elapsed_time(t1) * 1e3 / (REPLAYS * BUILDS * SCANS))
        result["device_us"] = {"median": round(float(np.median(runs)), 2), "spread": round(max(runs) - min(runs), 2),
                               "runs": [round(x, 2) for x in runs], "launches": 4}
        after = R._collect(staged)
        result["equal"] = bool(result["equal"] and all(
            np.array_equal(after[0][k].view(np.uint8), host[k].view(np.uint8)) for k in host))
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            merged = json.loads(f.read() or "{}")
        merged.update(result)
        result = merged
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
