"""The training meter on the MI355X: votenet_train_meter_add (csrc/train_meter.hip) against float64 adds in
the same order on the host, and the meter and the guard inside the captured steps -- logging only when
nothing is wrong, bit for bit; a step whose loss is not finite leaves parameters, moments, Adam's step and
the teacher where they were.  (Pattern: tests/test_view_stats_gpu.py.)"""
import importlib

import pytest
import torch

from conftest import load_pkg
from test_semi_step import _loose_filter

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _rule(key):
    return 'loss' in key or 'acc' in key or 'ratio' in key or 'value' in key


# ------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("layout", ["scattered", "views"])
@pytest.mark.parametrize("mode", ["no-guard", "applied", "skip-middle"])
@pytest.mark.parametrize("count", [1, 37, 64, 65, 300])
def test_meter_kernel_matches_host_doubles(count, mode, layout):
    load_pkg()
    L = importlib.import_module("3dioumatch_amd._lib")
    g = torch.Generator().manual_seed(count)
    if layout == "scattered":  # one allocation per scalar, handed over in a shuffled order
        scalars = [torch.zeros((), device=DEV) for _ in range(count)]
        order = torch.randperm(count, generator=g).tolist()
        scalars = [scalars[i] for i in order]
    else:  # strided views of one vector
        vector = torch.zeros(2 * count + 1, device=DEV)
        scalars = [vector[2 * i + 1] for i in range(count)]
    table = torch.tensor([t.data_ptr() for t in scalars], dtype=torch.int64, device=DEV)
    start = torch.randn(count + 3, generator=g, dtype=torch.float64)  # the sums add to what is there
    start[count], start[count + 1] = 4.0, 9.0
    accum = start.to(DEV)
    guard = None if mode == "no-guard" else torch.zeros(4, dtype=torch.float64, device=DEV)
    want = start.clone()
    for call in range(3):
        values = torch.randn(count, generator=g) * 10.0 ** (call - 1)
        for t, x in zip(scalars, values.tolist()):
            t.fill_(x)
        skip = mode == "skip-middle" and call == 1
        norm = float(torch.rand((), generator=g, dtype=torch.float64)) * 1e3
        if guard is not None:
            guard.copy_(torch.tensor([norm, 0.5, 1.0 if skip else 0.0, 7.0], dtype=torch.float64))
        L.check(L.lib.votenet_train_meter_add(count, table.data_ptr(), None if guard is None else guard.data_ptr(),
                                              accum.data_ptr(), torch.cuda.current_stream().cuda_stream), "meter")
        if skip:
            want[count + 1] += 1.0
        else:
            want[:count] += values.double()
            want[count] += 1.0
            if guard is not None:
                want[count + 2] += norm
    got = accum.cpu()
    assert torch.equal(got.view(torch.int64), want.view(torch.int64))
    assert float(got[count]) == 4.0 + (2.0 if mode == "skip-middle" else 3.0)
    assert float(got[count + 1]) == 9.0 + (1.0 if mode == "skip-middle" else 0.0)
    if guard is None:
        assert got[count + 2] == start[count + 2]


# ------------------------------------------------------------------ in the steps
def _runner(V, cfg, kind, **kw):
    if kind == "semi":
        return V.SemiSupervisedStep(cfg, DEV, num_proposal=64, seed=4, graphs=True,
                                    config_dict=_loose_filter(V, cfg), **kw)
    return V.SupervisedStep(cfg, DEV, num_proposal=64, seed=4, graphs=True, **kw)


def _batches(V, cfg, kind, bad=None):
    if kind == "semi":
        out = [{k: v.to(DEV) for k, v in V.make_semi_batch(2, 3, 3000, cfg, seed=s, num_objects=5).items()}
               for s in (5, 6, 7)]
    else:
        data = importlib.import_module("3dioumatch_amd.votenet.data")
        out = [{k: v.to(DEV) for k, v in data.make_batch(2, 20000, cfg, seed=s, num_objects=5).items()}
               for s in (5, 6, 7)]
    if bad is not None:
        # read by the loss's arithmetic only (csrc/loss_core.h loss_seed: `d < best` never holds for an
        # infinite d, the arg-min stays 0; no index is formed from it): the loss is not finite
        out[bad]["vote_label"] = out[bad]["vote_label"].clone()
        out[bad]["vote_label"][0] = float("inf")
    return out


def _adam(runner):
    st = runner.optimizer.state[runner.flat_params]
    out = {"p": runner.flat_params.data.clone(), "m": st["exp_avg"].clone(), "v": st["exp_avg_sq"].clone(),
           "step": st["step"].clone()}
    if hasattr(runner, "flat_teacher"):
        out["teacher"] = runner.flat_teacher.clone()
    return out


def _run(V, cfg, kind, batches, **kw):
    runner = _runner(V, cfg, kind, **kw)
    torch.manual_seed(9)
    torch.cuda.manual_seed_all(9)
    views = [dict(bt) for bt in batches]
    runner.prefetch_geometry(views[0])
    out = []
    for i in range(len(views)):
        if i + 1 < len(views):
            runner.prefetch_geometry(views[i + 1])
        loss, ep = runner(views[i])
        out.append({"loss": loss.detach().clone(), "grad": runner.flat_grad.detach().clone(),
                    "scalars": {k: ep[k].detach().clone() for k, v in ep.items()
                                if _rule(k) and torch.is_tensor(v) and v.numel() == 1},
                    "adam": _adam(runner)})
    torch.cuda.synchronize()
    assert runner.graphs
    return runner, out


@pytest.mark.parametrize("kind", ["supervised", "semi"])
def test_captured_step_meter_and_guard_are_logging_only(kind):
    load_pkg()
    V = importlib.import_module("3dioumatch_amd.votenet")
    cfg = V.scannet_config()
    batches = _batches(V, cfg, kind)
    plain, off = _run(V, cfg, kind, batches)
    runner, on = _run(V, cfg, kind, batches, meter=True, guard=True)
    assert plain.meter is None and plain._guard is None
    for a, b in zip(off, on):
        assert torch.equal(a["loss"], b["loss"])
        assert torch.equal(a["grad"], b["grad"])
        for k in a["adam"]:
            assert torch.equal(a["adam"][k], b["adam"][k]), k
    got = runner.meter.result()
    keys = sorted(on[0]["scalars"])
    assert "loss" in keys and "pos_ratio" in keys and len(keys) >= 10
    assert sorted(k for k in got if k not in ("steps", "skipped_steps", "grad_norm_value")) == keys
    assert got["steps"] == 3 and got["skipped_steps"] == 0 and runner.meter.host_reads == 1
    for k in keys:
        want = sum(float(step["scalars"][k].double()) for step in on) / 3
        assert got[k] == want, (k, got[k], want)
    norms = [float(step["grad"].double().square().sum().sqrt()) for step in on]
    assert abs(got["grad_norm_value"] - sum(norms) / 3) <= 1e-9 * got["grad_norm_value"]
    rep = runner.guard_report()
    assert rep["skipped_total"] == 0 and not rep["skipped_last"] and rep["coefficient"] == 1.0
    assert abs(rep["norm"] - norms[-1]) <= 1e-9 * norms[-1]


@pytest.mark.parametrize("kind", ["supervised", "semi"])
def test_captured_step_skips_a_non_finite_loss(kind):
    load_pkg()
    V = importlib.import_module("3dioumatch_amd.votenet")
    cfg = V.scannet_config()
    runner, out = _run(V, cfg, kind, _batches(V, cfg, kind, bad=1), meter=True, guard=True)
    assert bool(torch.isfinite(out[0]["loss"])) and not bool(torch.isfinite(out[1]["loss"]))
    assert bool(torch.isfinite(out[2]["loss"]))
    first, second, third = (step["adam"] for step in out)
    assert float(first["step"]) == 1.0
    for k in first:  # parameters, both moments, Adam's step (and the teacher): where step 1 left them
        assert torch.equal(first[k], second[k]), k
    assert float(third["step"]) == 2.0
    assert bool(torch.isfinite(third["p"]).all()) and not torch.equal(third["p"], second["p"])
    if kind == "semi":
        assert bool(torch.isfinite(third["teacher"]).all()) and not torch.equal(third["teacher"], second["teacher"])
    rep = runner.guard_report()
    assert rep["skipped_total"] == 1 and not rep["skipped_last"]
    got = runner.meter.result()
    assert got["steps"] == 2 and got["skipped_steps"] == 1
    for k, v in got.items():
        assert v == v and abs(v) != float("inf"), k
    keys = sorted(out[0]["scalars"])
    for k in keys:  # the means are over the two applied steps
        want = (float(out[0]["scalars"][k].double()) + float(out[2]["scalars"][k].double())) / 2
        assert got[k] == want, k
