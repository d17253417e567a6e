"""The guard's buffer rollback on the MI355X: votenet_guard_state_sync (csrc/optim.hip) through the C ABI
on raw bytes -- both verdicts, every size class of its grid, guard words around both buffers, the error
returns -- and the sync inside the captured steps: a step whose loss is not finite leaves the BatchNorm
buffers of the student (and the teacher) where the step before left them, finite steps do not see the
feature, loaded weights re-arm the shadow.  (Shapes and the bad batch: tests/test_train_meter_gpu.py.)"""
import importlib

import pytest
import torch

from conftest import load_pkg
from test_semi_step import _loose_filter

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
INVALID = 1  # hipErrorInvalidValue
WORD = 64    # bytes of each guard word around the buffers


def _lib():
    load_pkg()
    return importlib.import_module("3dioumatch_amd._lib")


def _fill(nbytes, seed, int64_first=False):
    """random bytes with float32 NaN payloads, -0.0 and int64 patterns in their first words"""
    g = torch.Generator().manual_seed(seed)
    raw = torch.randint(0, 256, (nbytes,), generator=g, dtype=torch.uint8)
    special = torch.cat([torch.tensor([0x7fc00001, 0xffc12345, 0x7f800001, 0x80000000], dtype=torch.int64)
                         .to(torch.int32).view(torch.uint8),               # NaNs with payloads, -0.0
                         torch.tensor([-1, 2 ** 62 + 5], dtype=torch.int64).view(torch.uint8)])
    if int64_first:
        special = special.roll(16)
    k = min(nbytes, special.numel())
    raw[:k] = special[:k]
    return raw


@pytest.mark.parametrize("verdict", [0, 1])
@pytest.mark.parametrize("nbytes", [16, 48, 16 * 255, 16 * 256, 16 * 257, 16 * 70001])
def test_sync_kernel_copies_by_verdict(nbytes, verdict):
    L = _lib()
    # ONE allocation: word | state | word | shadow | word, every piece 16-byte aligned
    whole_host = torch.cat([torch.full((WORD,), 0xA5, dtype=torch.uint8), _fill(nbytes, 2 * nbytes + 1),
                            torch.full((WORD,), 0x5A, dtype=torch.uint8), _fill(nbytes, 2 * nbytes + 2, int64_first=True),
                            torch.full((WORD,), 0xC3, dtype=torch.uint8)])
    whole = whole_host.to(DEV)
    state = whole[WORD:WORD + nbytes]
    shadow = whole[2 * WORD + nbytes:2 * WORD + 2 * nbytes]
    old_state, old_shadow = whole_host[WORD:WORD + nbytes], whole_host[2 * WORD + nbytes:2 * WORD + 2 * nbytes]
    assert not torch.equal(old_state, old_shadow)
    assert state.data_ptr() % 16 == 0 and shadow.data_ptr() % 16 == 0
    record = torch.tensor([3.25, 0.5, float(verdict), 7.0], dtype=torch.float64)
    guard = record.to(DEV)
    L.check(L.lib.votenet_guard_state_sync(nbytes, state.data_ptr(), shadow.data_ptr(), guard.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream), "votenet_guard_state_sync")
    torch.cuda.synchronize()
    got = whole.cpu()
    want = old_shadow if verdict else old_state  # skipped: state <- shadow; applied: shadow <- state
    assert torch.equal(got[WORD:WORD + nbytes], want)
    assert torch.equal(got[2 * WORD + nbytes:2 * WORD + 2 * nbytes], want)
    for at, fill in ((0, 0xA5), (WORD + nbytes, 0x5A), (2 * WORD + 2 * nbytes, 0xC3)):
        assert bool((got[at:at + WORD] == fill).all()), at
    assert torch.equal(guard.cpu().view(torch.int64), record.view(torch.int64))


def test_sync_entry_refuses_bad_arguments_without_a_launch():
    L = _lib()
    host = _fill(256, 3)
    buf = host.to(DEV)
    record = torch.tensor([1.0, 1.0, 1.0, 2.0], dtype=torch.float64)
    guard = record.to(DEV)
    state, shadow, stream = buf[:64], buf[128:192], torch.cuda.current_stream().cuda_stream
    call = L.lib.votenet_guard_state_sync
    assert call(0, state.data_ptr(), shadow.data_ptr(), guard.data_ptr(), stream) == 0
    assert call(0, None, None, None, stream) == 0
    assert call(64, None, shadow.data_ptr(), guard.data_ptr(), stream) == INVALID
    assert call(64, state.data_ptr(), None, guard.data_ptr(), stream) == INVALID
    assert call(64, state.data_ptr(), shadow.data_ptr(), None, stream) == INVALID
    assert call(24, state.data_ptr(), shadow.data_ptr(), guard.data_ptr(), stream) == INVALID
    assert call(-16, state.data_ptr(), shadow.data_ptr(), guard.data_ptr(), stream) == INVALID
    assert call(32, state.data_ptr() + 8, shadow.data_ptr(), guard.data_ptr(), stream) == INVALID
    assert call(32, state.data_ptr(), shadow.data_ptr() + 8, guard.data_ptr(), stream) == INVALID
    torch.cuda.synchronize()
    assert torch.equal(buf.cpu(), host)  # with verdict 1 a launch would have overwritten `state`
    assert torch.equal(guard.cpu().view(torch.int64), record.view(torch.int64))


# ------------------------------------------------------------------ in the captured steps
def _runner(V, cfg, kind, seed=4, **kw):
    if kind == "semi":
        return V.SemiSupervisedStep(cfg, DEV, num_proposal=64, seed=seed, graphs=True,
                                    config_dict=_loose_filter(V, cfg), **kw)
    return V.SupervisedStep(cfg, DEV, num_proposal=64, seed=seed, graphs=True, **kw)


_BATCHES = {}


def _batches(V, cfg, kind):
    """four batches per kind, made once and never written (a bad one is a shallow copy with its own label)"""
    if kind not in _BATCHES:
        if kind == "semi":
            made = [V.make_semi_batch(2, 3, 3000, cfg, seed=s, num_objects=5) for s in (5, 6, 7, 8)]
        else:
            data = importlib.import_module("3dioumatch_amd.votenet.data")
            made = [data.make_batch(2, 20000, cfg, seed=s, num_objects=5) for s in (5, 6, 7, 8)]
        _BATCHES[kind] = [{k: v.to(DEV) for k, v in bt.items()} for bt in made]
    return [dict(bt) for bt in _BATCHES[kind]]


def _bad(batch):
    # read by the loss's arithmetic only (csrc/loss_core.h loss_seed: no index is formed from it)
    batch = dict(batch)
    batch["vote_label"] = batch["vote_label"].clone()
    batch["vote_label"][0] = float("inf")
    return batch


def _nets(runner):
    return [runner.net] + ([runner.teacher] if hasattr(runner, "teacher") else [])


def _buffers(runner):
    return {"%d.%s" % (i, k): b.detach().clone() for i, net in enumerate(_nets(runner))
            for k, b in net.named_buffers()}


def _adam(runner):
    st = runner.optimizer.state[runner.flat_params]
    out = {"p": runner.flat_params.data.clone(), "m": st["exp_avg"].clone(), "v": st["exp_avg_sq"].clone(),
           "step": st["step"].clone()}
    if hasattr(runner, "flat_teacher"):
        out["teacher"] = runner.flat_teacher.clone()
    return out


def _run(runner, batches, after_capture=None):
    torch.manual_seed(9)
    torch.cuda.manual_seed_all(9)
    views = [dict(bt) for bt in batches]
    runner.prefetch_geometry(views[0])  # (captures the graphs: warm-up steps, then everything put back)
    if after_capture is not None:
        torch.cuda.synchronize()
        after_capture()
    out = []
    for i in range(len(views)):
        if i + 1 < len(views):
            runner.prefetch_geometry(views[i + 1])
        loss, _ = runner(views[i])
        out.append({"loss": loss.detach().clone(), "grad": runner.flat_grad.detach().clone(),
                    "buffers": _buffers(runner), "adam": _adam(runner)})
    torch.cuda.synchronize()
    assert runner.graphs
    return out


def _bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def _moving(name):
    return name.endswith("running_mean") or name.endswith("running_var")


@pytest.mark.parametrize("kind", ["supervised", "semi"])
def test_captured_skipped_step_restores_the_buffers(kind):
    load_pkg()
    V = importlib.import_module("3dioumatch_amd.votenet")
    cfg = V.scannet_config()
    good0, mid, good2, _ = _batches(V, cfg, kind)
    runner = _runner(V, cfg, kind, meter=True, guard=True)
    base, size = runner.state_arena.data_ptr(), runner.state_arena.numel()
    assert size % 16 == 0 and runner.state_shadow.numel() == size
    for net in _nets(runner):
        for k, b in net.named_buffers():
            assert (b.data_ptr() - base) % 256 == 0 and 0 <= b.data_ptr() - base < size, k
    start = _buffers(runner)

    def after_capture():  # no step has run: the warm-up's forward passes and updates are undone
        assert runner._captured is not None
        assert torch.equal(runner.state_shadow, runner.state_arena)
        for k, b in _buffers(runner).items():
            assert torch.equal(_bytes(b), _bytes(start[k])), k
        assert runner.guard_report()["skipped_total"] == 0

    first, second, third = _run(runner, [good0, _bad(mid), good2], after_capture)
    assert bool(torch.isfinite(first["loss"])) and not bool(torch.isfinite(second["loss"]))
    assert bool(torch.isfinite(third["loss"]))
    names = sorted(first["buffers"])
    assert any(k.startswith("1.") for k in names) == (kind == "semi")
    for k in names:
        if _moving(k):
            assert not torch.equal(first["buffers"][k], start[k]), k  # capture put back what its warm-up wrote
    for k in names:  # the bad step did not happen, for the student's buffers (and the teacher's), bit for bit
        a, b = first["buffers"][k], second["buffers"][k]
        assert a.dtype == b.dtype and torch.equal(_bytes(a), _bytes(b)), k
    for k in first["adam"]:
        assert torch.equal(first["adam"][k], second["adam"][k]), k
    assert int(runner.net.pnet.bn1.num_batches_tracked) == 2
    for k in names:
        a, b = second["buffers"][k], third["buffers"][k]
        if k.endswith("num_batches_tracked"):
            assert int(b) == 2 * int(a), k
        elif b.dtype.is_floating_point:
            assert bool(torch.isfinite(b).all()), k
            if _moving(k):
                assert not torch.equal(a, b), k
    rep = runner.guard_report()
    assert rep["skipped_total"] == 1 and not rep["skipped_last"]
    assert torch.equal(runner.state_shadow, runner.state_arena)


@pytest.mark.parametrize("kind", ["supervised", "semi"])
def test_captured_finite_steps_do_not_see_the_rollback(kind):
    load_pkg()
    V = importlib.import_module("3dioumatch_amd.votenet")
    cfg = V.scannet_config()
    batches = _batches(V, cfg, kind)[:3]
    plain_runner = _runner(V, cfg, kind)
    assert plain_runner.state_arena is None and plain_runner.state_shadow is None
    plain = _run(plain_runner, batches)
    runner = _runner(V, cfg, kind, guard=True)
    guarded = _run(runner, batches)
    for a, b in zip(plain, guarded):
        assert bool(torch.isfinite(a["loss"])) and torch.equal(a["loss"], b["loss"])
        assert torch.equal(a["grad"], b["grad"])
        for k in a["adam"]:
            assert torch.equal(a["adam"][k], b["adam"][k]), k
        assert a["buffers"].keys() == b["buffers"].keys()
        for k in a["buffers"]:
            assert torch.equal(_bytes(a["buffers"][k]), _bytes(b["buffers"][k])), k
    assert runner.guard_report()["skipped_total"] == 0
    assert torch.equal(runner.state_shadow, runner.state_arena)


def _run_more(runner, batches):
    """further steps of a run that _run began (no re-seeding: the noise stream goes on)"""
    out = []
    views = [dict(bt) for bt in batches]
    for i in range(len(views)):
        loss, _ = runner(views[i])
        out.append({"loss": loss.detach().clone(), "grad": runner.flat_grad.detach().clone(),
                    "buffers": _buffers(runner), "adam": _adam(runner)})
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("kind", ["supervised", "semi"])
def test_captured_loaded_weights_rearm_the_shadow(kind):
    load_pkg()
    V = importlib.import_module("3dioumatch_amd.votenet")
    cfg = V.scannet_config()
    good0, mid, _, other_batch = _batches(V, cfg, kind)
    other = _runner(V, cfg, kind, seed=9)
    _run(other, [other_batch])  # statistics of its own
    runner = _runner(V, cfg, kind, guard=True)
    _run(runner, [good0])
    for mine, theirs in zip(_nets(runner), _nets(other)):
        mine.load_state_dict(theirs.state_dict())
    assert torch.equal(runner.state_shadow, runner.state_arena)
    loaded = _buffers(runner)
    for k, v in _buffers(other).items():
        assert torch.equal(_bytes(loaded[k]), _bytes(v)), k
    out = _run_more(runner, [_bad(mid)])
    assert not bool(torch.isfinite(out[0]["loss"])) and runner.guard_report()["skipped_last"]
    for k, v in out[0]["buffers"].items():
        assert torch.equal(_bytes(v), _bytes(loaded[k])), k  # the loaded statistics, not those before the load
