"""Which tensor-library (ATen) operators launch device kernels in the supervised train step, and
from which line of this package?  Needs no profiler: three EAGER steps at the benchmark's shapes
(8 scenes of 40 000 points, 256 proposals) run under a TorchDispatchMode -- re-entered in the
autograd engine's worker thread -- with the next batch's index chain prefetched on the side stream
as the benchmark's loop does.  Per site (operator, shapes and strides of its tensor arguments,
innermost frame inside the package, stream) the launches of the LAST of the three steps are counted.

    python tools/glue_sites.py OUT.json [--reasons REASONS.json]

OUT.json: {"steps": 3, "counted_step": 3, "launches_per_step": N, "sites": [{"op", "args": [{"shape",
"stride", "dtype"}], "source", "stream": "main" | "prefetch", "count", "elements"[, "reason"]}]}.
--reasons: a JSON list of [regular expression, reason] pairs; a site whose "op @ source [stream]"
matches gets that one-line reason why it stays (first match wins; "unexplained" otherwise).
"""
import argparse
import collections
import importlib
import json
import os
import re
import sys
import traceback

import torch
from torch.utils._python_dispatch import TorchDispatchMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# operators that launch nothing: views, metadata, allocation
NO_KERNEL = {
    "aten::view", "aten::_unsafe_view", "aten::reshape", "aten::_reshape_alias", "aten::transpose",
    "aten::permute", "aten::slice", "aten::select", "aten::expand", "aten::unsqueeze", "aten::squeeze",
    "aten::detach", "aten::alias", "aten::as_strided", "aten::t", "aten::empty", "aten::empty_like",
    "aten::empty_strided", "aten::new_empty", "aten::new_empty_strided", "aten::size", "aten::stride",
    "aten::is_contiguous", "aten::unbind", "aten::split", "aten::split_with_sizes", "aten::narrow",
    "aten::view_as", "aten::numel", "aten::sym_size", "aten::sym_stride", "aten::sym_numel",
    "aten::sym_storage_offset", "aten::unflatten", "aten::flatten", "aten::chunk", "aten::lift_fresh",
    "aten::record_stream", "aten::is_pinned", "aten::unfold", "aten::movedim", "aten::diagonal",
    "aten::expand_as", "aten::resize_", "aten::set_", "aten::is_same_size", "aten::dim",
    "aten::result_type", "aten::_local_scalar_dense", "aten::item",
}


def _tensors(args, kwargs):
    found = []

    def walk(v):
        if isinstance(v, torch.Tensor):
            found.append(v)
        elif isinstance(v, (list, tuple)):
            for e in v:
                walk(e)
    for a in list(args) + list((kwargs or {}).values()):
        walk(a)
    return found


def _source():
    for fs in reversed(traceback.extract_stack()[:-2]):
        fn = fs.filename
        if "3dioumatch_amd" in fn and os.sep + "tools" + os.sep not in fn:
            return "%s:%d %s" % (fn.split("3dioumatch_amd" + os.sep)[-1], fs.lineno, fs.name)
    return "?"


class Sites(TorchDispatchMode):
    def __init__(self, device):
        super().__init__()
        self.device = device
        self.main = torch.cuda.default_stream(device)
        self.count = collections.Counter()
        self.elements = {}
        self.on = False

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        name = func._schema.name
        if self.on and name not in NO_KERNEL:
            ts = _tensors(args, kwargs)
            # (a conversion that changes neither dtype nor device returns its argument)
            same = name in ("aten::_to_copy", "aten::to") and ts and not kwargs
            ts = ts or _tensors((out,), None)  # a factory function (zeros, full, randn): its result
            if any(t.is_cuda for t in ts) and not same:
                stream = torch.cuda.current_stream(self.device)
                desc = tuple((tuple(t.shape), tuple(t.stride()), str(t.dtype).replace("torch.", ""))
                             for t in ts[:6])
                key = (name, desc, _source(), "main" if stream == self.main else "prefetch")
                self.count[key] += 1
                self.elements[key] = max(t.numel() for t in ts)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reasons", default=None)
    opts = ap.parse_args()
    importlib.import_module("3dioumatch_amd")
    V = importlib.import_module("3dioumatch_amd.votenet")
    data = importlib.import_module("3dioumatch_amd.votenet.data")
    dev = torch.device("cuda:0")
    cfg = V.scannet_config()
    runner = V.SupervisedStep(cfg, dev, world_size=1, num_proposal=256, lr=1e-3, graphs=False)
    batches = [data.make_batch(8, 40000, cfg, seed=100 + j, device=dev) for j in range(4)]
    for batch in batches:  # the host-side facts the step's graphs bake in (every scene supervised)
        batch.update(runner._host_info(batch))
    sites = Sites(dev)

    # the autograd engine's worker thread: the mode is entered there once, by a hook on the loss,
    # where the engine has not carried it over itself
    backward = torch.Tensor.backward

    def reenter(grad):
        from torch.utils._python_dispatch import _get_current_dispatch_mode_stack
        if not any(m is sites for m in _get_current_dispatch_mode_stack()):
            sites.__enter__()
        return grad

    def traced_backward(self, *args, **kwargs):
        self.register_hook(reenter)
        return backward(self, *args, **kwargs)

    torch.Tensor.backward = traced_backward
    steps = 3
    runner.prefetch_geometry(batches[0])
    with sites:
        for j in range(steps):
            sites.on = j == steps - 1
            runner.prefetch_geometry(batches[j + 1])
            runner(batches[j])
    torch.cuda.synchronize()
    reasons = json.load(open(opts.reasons)) if opts.reasons else None
    rows = []
    for (name, desc, source, stream), n in sorted(sites.count.items(), key=lambda kv: (-kv[1], kv[0][2])):
        row = {"op": name, "args": [{"shape": list(s), "stride": list(st), "dtype": d} for s, st, d in desc],
               "source": source, "stream": stream, "count": n,
               "elements": sites.elements[(name, desc, source, stream)]}
        if reasons is not None:
            tag = "%s @ %s [%s]" % (name, source, stream)
            row["reason"] = next((why for pat, why in reasons if re.search(pat, tag)), "unexplained")
        rows.append(row)
    with open(opts.out, "w") as f:
        json.dump({"steps": steps, "counted_step": steps, "launches_per_step": sum(r["count"] for r in rows),
                   "sites": rows}, f, indent=1)
        f.write("\n")
    print("%d ATen launches per step at %d sites -> %s" % (sum(r["count"] for r in rows), len(rows), opts.out))


if __name__ == "__main__":
    main()
