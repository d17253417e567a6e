"""The guard's buffer rollback without a GPU (votenet/step.py: flatten_buffers, the state arena and its
shadow, the CPU form of the sync in _apply_cpu_guarded): the arena's layout and that state_dict /
load_state_dict do not see it, and a skipped step that leaves the BatchNorm running statistics and
num_batches_tracked of the student (and the teacher) where the step before left them.  Steps run on the
oracle stand-ins, as tests/test_trainer.py."""
import importlib

import pytest
import torch

from conftest import load_pkg
from test_semi_step import _loose_filter, _setup

N, K = 2600, 32


def _named(*nets):
    return [("%d.%s" % (i, k), b) for i, net in enumerate(nets) for k, b in net.named_buffers()]


def _randomise(net, seed):
    g = torch.Generator().manual_seed(seed)
    for _, b in net.named_buffers():
        if b.dtype.is_floating_point:
            b.copy_(torch.rand(b.shape, generator=g) + 0.5)
        else:
            b.copy_(torch.randint(1, 1000, b.shape, generator=g))


# ------------------------------------------------------------------ the arena
def test_flatten_buffers_layout_and_state_dict():
    load_pkg()
    S = importlib.import_module("3dioumatch_amd.votenet.step")
    V = importlib.import_module("3dioumatch_amd.votenet")
    cfg = V.scannet_config()
    net, teacher, other = (S.build_detector(cfg, num_proposal=K, seed=s) for s in (0, 0, 1))
    for i, m in enumerate((net, teacher, other)):
        _randomise(m, 10 + i)
    before = {k: v.clone() for k, v in _named(net, teacher)}
    sd_before = {k: v.clone() for k, v in net.state_dict().items()}
    flags = [(set(m._non_persistent_buffers_set), sorted(m._buffers)) for m in net.modules()]
    objects = [id(b) for _, b in _named(net, teacher)]
    assert any(b.dtype == torch.int64 and b.dim() == 0 for b in before.values())  # num_batches_tracked
    assert any(b.dtype == torch.float32 for b in before.values())

    arena = S.flatten_buffers([net, teacher, net])  # (a module given twice: its buffers once)
    assert arena.dtype == torch.uint8 and arena.dim() == 1 and arena.is_contiguous()
    assert arena.numel() % 16 == 0
    assert [id(b) for _, b in _named(net, teacher)] == objects  # the same tensors, another home
    sd = net.state_dict()
    assert list(sd) == list(sd_before)
    for k in sd:
        assert sd[k].dtype == sd_before[k].dtype and sd[k].shape == sd_before[k].shape, k
        assert torch.equal(sd[k], sd_before[k]), k
    assert [(set(m._non_persistent_buffers_set), sorted(m._buffers)) for m in net.modules()] == flags
    base, spans = arena.data_ptr(), []
    for k, b in _named(net, teacher):
        assert torch.equal(b, before[k]) and b.dtype == before[k].dtype and b.shape == before[k].shape, k
        off, nbytes = b.data_ptr() - base, b.numel() * b.element_size()
        assert b.is_contiguous() and off % 256 == 0 and 0 <= off and off + nbytes <= arena.numel(), k
        spans.append((off, off + nbytes))
    assert len(spans) == len(before)
    ordered = sorted(spans)
    assert ordered == spans  # named_buffers() order, the student's first
    for (_, end), (start, _) in zip(ordered, ordered[1:]):
        assert end <= start

    # load_state_dict copies in place: it writes through to the arena
    snapshot = arena.clone()
    net.load_state_dict(other.state_dict())
    assert not torch.equal(arena, snapshot)
    loaded = other.state_dict()
    assert any(k not in loaded for k, _ in net.named_buffers())  # (a non-persistent one: it keeps its value)
    for (k, b), (_, want) in zip(net.named_buffers(), other.named_buffers()):
        if k not in loaded:
            assert torch.equal(b, before["0." + k]), k
            continue
        off = b.data_ptr() - base
        raw = arena[off:off + b.numel() * b.element_size()].view(b.dtype).view(b.shape)
        assert torch.equal(raw, want) and torch.equal(b, want), k
    # ... and a copy into the arena is a copy into every buffer
    arena.copy_(snapshot)
    for k, b in _named(net, teacher):
        assert torch.equal(b, before[k]), k
    # one module instead of a list; no buffers at all
    alone = S.flatten_buffers(other)
    assert alone.numel() % 16 == 0 and 0 < alone.numel() < arena.numel()
    assert S.flatten_buffers(torch.nn.Linear(2, 2)).numel() == 0


def test_unguarded_runner_homes_nothing():
    load_pkg()
    V = importlib.import_module("3dioumatch_amd.votenet")
    cfg, dev = V.scannet_config(), torch.device("cpu")
    for runner in (V.SupervisedStep(cfg, dev, num_proposal=K, meter=True),
                   V.SemiSupervisedStep(cfg, dev, num_proposal=K, graphs=False)):
        assert runner.state_arena is None and runner.state_shadow is None
        nets = [runner.net] + ([runner.teacher] if hasattr(runner, "teacher") else [])
        storages = [b.untyped_storage().data_ptr() for _, b in _named(*nets)]
        assert len(set(storages)) == len(storages)  # every buffer still owns its allocation
        assert all(b.storage_offset() == 0 for _, b in _named(*nets))
        runner.sync_guard_state()  # nothing to do, and says nothing
        assert len(runner._state()) == len(list(runner.net.buffers())) + 1 + \
            (len(list(runner.teacher.buffers())) + 1 if hasattr(runner, "teacher") else 0)
    guarded = V.SupervisedStep(cfg, dev, num_proposal=K, clip_grad_norm=1.0)  # clipping implies the guard
    assert guarded.state_arena is not None and torch.equal(guarded.state_shadow, guarded.state_arena)
    assert guarded.state_shadow.data_ptr() != guarded.state_arena.data_ptr()
    semi = V.SemiSupervisedStep(cfg, dev, num_proposal=K, graphs=False, guard=True)
    base, size = semi.state_arena.data_ptr(), semi.state_arena.numel()
    offs = [b.data_ptr() - base for _, b in _named(semi.net, semi.teacher)]
    assert offs == sorted(offs) and offs[0] == 0 and offs[-1] < size  # ONE arena: the student, then the teacher
    assert size == 2 * guarded.state_arena.numel()


# ------------------------------------------------------------------ the steps
def _make(V, cfg, dev, kind, seed=4, **kw):
    if kind == "semi":
        return V.SemiSupervisedStep(cfg, dev, num_proposal=K, seed=seed, graphs=False,
                                    config_dict=_loose_filter(V, cfg), **kw)
    return V.SupervisedStep(cfg, dev, num_proposal=K, seed=seed, **kw)


def _batches(V, cfg, kind, bad=None, seeds=(5, 6, 7)):
    if kind == "semi":
        out = [V.make_semi_batch(1, 3, N, cfg, seed=s, num_objects=5) for s in seeds]
    else:
        data = importlib.import_module("3dioumatch_amd.votenet.data")
        out = [data.make_batch(1, N, cfg, seed=s, num_objects=5) for s in seeds]
    if bad is not None:  # read by the loss's arithmetic only (as tests/test_train_meter_gpu.py makes it)
        out[bad]["vote_label"] = out[bad]["vote_label"].clone()
        out[bad]["vote_label"][0] = float("inf")
    return out


def _nets(runner):
    return [runner.net] + ([runner.teacher] if hasattr(runner, "teacher") else [])


def _buffers(runner):
    return {k: b.clone() for k, b in _named(*_nets(runner))}


def _adam(runner):
    st = runner.optimizer.state[runner.flat_params]
    out = {"p": runner.flat_params.data.clone(), "m": st["exp_avg"].clone(), "v": st["exp_avg_sq"].clone(),
           "step": torch.tensor(float(st["step"]))}
    if hasattr(runner, "flat_teacher"):
        out["teacher"] = runner.flat_teacher.clone()
    return out


def _run(runner, batches):
    torch.manual_seed(9)
    out = []
    for batch in batches:
        loss, _ = runner(dict(batch))
        out.append({"loss": loss.detach().clone(), "buffers": _buffers(runner), "adam": _adam(runner),
                    "grad": runner.flat_grad.clone()})
    return out


def _bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def _moving(name):
    return name.endswith("running_mean") or name.endswith("running_var")


@pytest.mark.parametrize("kind", ["supervised", "semi"])
def test_cpu_skipped_step_restores_the_buffers(kind, oracle_omp, monkeypatch):
    V, dev = _setup(False, oracle_omp, monkeypatch)
    cfg = V.scannet_config()
    runner = _make(V, cfg, dev, kind, guard=True)
    start = _buffers(runner)
    first, second, third = _run(runner, _batches(V, cfg, kind, bad=1))
    assert bool(torch.isfinite(first["loss"])) and not bool(torch.isfinite(second["loss"]))
    assert bool(torch.isfinite(third["loss"]))
    rep = runner.guard_report()
    assert rep["skipped_total"] == 1 and not rep["skipped_last"]
    names = sorted(first["buffers"])
    assert any(_moving(k) for k in names) and any(k.startswith("1.") for k in names) == (kind == "semi")
    for k in names:
        if _moving(k):
            assert not torch.equal(first["buffers"][k], start[k]), k  # the forward passes do write them
    # the bad step did not happen: every buffer of the student (and the teacher), bit for bit
    for k in names:
        a, b = first["buffers"][k], second["buffers"][k]
        assert a.dtype == b.dtype and torch.equal(_bytes(a), _bytes(b)), k
    for k in first["adam"]:
        assert torch.equal(first["adam"][k], second["adam"][k]), k
    # the third step is the second one that happened
    assert int(runner.net.pnet.bn1.num_batches_tracked) == 2
    for k in names:
        a, b = second["buffers"][k], third["buffers"][k]
        if k.endswith("num_batches_tracked"):
            assert int(b) == 2 * int(a), k
        elif b.dtype.is_floating_point:
            assert bool(torch.isfinite(b).all()), k
            if _moving(k):
                assert not torch.equal(a, b), k
    assert torch.equal(runner.state_shadow, runner.state_arena)


@pytest.mark.parametrize("kind", ["supervised", "semi"])
def test_cpu_loaded_weights_rearm_the_shadow(kind, oracle_omp, monkeypatch):
    V, dev = _setup(False, oracle_omp, monkeypatch)
    cfg = V.scannet_config()
    good, bad = _batches(V, cfg, kind, bad=1, seeds=(5, 6))
    other = _make(V, cfg, dev, kind, seed=9)
    _run(other, [_batches(V, cfg, kind, seeds=(8,))[0]])  # statistics of its own
    runner = _make(V, cfg, dev, kind, guard=True)
    _run(runner, [good])
    for mine, theirs in zip(_nets(runner), _nets(other)):
        mine.load_state_dict(theirs.state_dict())
    assert torch.equal(runner.state_shadow, runner.state_arena)
    loaded = _buffers(runner)
    assert loaded.keys() == _buffers(other).keys()
    for k, v in _buffers(other).items():
        assert torch.equal(loaded[k], v), k
    loss, _ = runner(dict(bad))
    assert not bool(torch.isfinite(loss)) and runner.guard_report()["skipped_last"]
    for k, v in _buffers(runner).items():
        assert torch.equal(v, loaded[k]), k  # the loaded statistics, not those from before the load
    # a buffer written in place is declared good by hand
    bn = runner.net.pnet.bn1
    bn.running_mean.add_(1.0)
    written = bn.running_mean.clone()
    runner.sync_guard_state()
    runner(dict(bad))
    assert torch.equal(bn.running_mean, written)


@pytest.mark.parametrize("kind", ["supervised", "semi"])
def test_cpu_finite_steps_do_not_see_the_rollback(kind, oracle_omp, monkeypatch):
    V, dev = _setup(False, oracle_omp, monkeypatch)
    cfg = V.scannet_config()
    batches = _batches(V, cfg, kind)
    plain = _run(_make(V, cfg, dev, kind), batches)
    runner = _make(V, cfg, dev, kind, guard=True)
    guarded = _run(runner, batches)
    for a, b in zip(plain, guarded):
        assert bool(torch.isfinite(a["loss"])) and torch.equal(a["loss"], b["loss"])
        assert torch.equal(a["grad"], b["grad"])
        assert a["buffers"].keys() == b["buffers"].keys()
        for k in a["buffers"]:
            assert torch.equal(a["buffers"][k], b["buffers"][k]), k
        for k in a["adam"]:
            assert torch.equal(a["adam"][k], b["adam"][k]), k
    assert float(guarded[-1]["adam"]["step"]) == 3.0 and runner.guard_report()["skipped_total"] == 0
    assert torch.equal(runner.state_shadow, runner.state_arena)
