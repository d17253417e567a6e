"""The training loop's host logic without a GPU (votenet/train_meter.py, votenet/trainer.py, the guard's
CPU form in votenet/step.py, tools/train.py): the eager meter against .item() means and the reference's
key rule (train.py:356-360), the guard and clip semantics with tensor operations, the loop's intervals,
log lines and checkpoint keys (train.py:362-369, :566-611), a bit-exact resume, the all-rank read-out
over gloo, and the front end's argument wiring.  Steps run on the oracle stand-ins, as
tests/test_semi_step.py's CPU leg."""
import importlib
import importlib.util
import json
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT, load_pkg
from test_semi_step import _loose_filter, _setup

N, K = 2600, 32


def _rule(key):
    return 'loss' in key or 'acc' in key or 'ratio' in key or 'value' in key


def _batch(V, cfg, seed):
    data = importlib.import_module("3dioumatch_amd.votenet.data")
    return data.make_batch(1, N, cfg, seed=seed, num_objects=5)


# ------------------------------------------------------------------ the meter
def test_eager_meter_matches_item_means(oracle_omp, monkeypatch):
    V, dev = _setup(False, oracle_omp, monkeypatch)
    cfg = V.scannet_config()
    runner = V.SupervisedStep(cfg, dev, num_proposal=K, meter=True)
    assert runner.meter is not None and runner._guard is None
    torch.manual_seed(1)
    sums, keys = {}, None
    for s in range(2):
        _, ep = runner(_batch(V, cfg, seed=10 + s))
        want = sorted(k for k, v in ep.items() if _rule(k) and torch.is_tensor(v) and v.numel() == 1)
        assert keys is None or keys == want
        keys = want
        for k in keys:
            sums[k] = sums.get(k, 0.0) + ep[k].item()  # the reference's loop
    got = runner.meter.result(reset=True)
    assert "loss" in keys and "pos_ratio" in keys and "obj_acc" in keys
    assert sorted(k for k in got if k not in ("steps", "skipped_steps")) == keys
    assert got["steps"] == 2 and got["skipped_steps"] == 0
    for k in keys:
        assert got[k] == sums[k] / 2, k  # doubles added in the same order: the same bits
    assert runner.meter.host_reads == 1
    again = runner.meter.result()
    assert again["steps"] == 0
    # keys that are not one-element tensors, or match no tag, are left out
    T = importlib.import_module("3dioumatch_amd.votenet.train_meter")
    assert T.logged_keys({"box_loss": torch.zeros(()), "center": torch.zeros(2, 3), "loss_map": torch.zeros(4),
                          "iou_value": torch.zeros(1), "other": torch.zeros(()), "labeled_num": 3}) == \
        ["box_loss", "iou_value"]
    assert T.tb_name("grad_norm_value") == "value/grad_norm_value" and T.tb_name("box_loss") == "loss/box_loss"
    assert T.tb_name("obj_acc") == "acc/obj_acc" and T.tb_name("center") == "other/center"


def test_meter_with_guard_counts_a_skipped_step():
    load_pkg()
    T = importlib.import_module("3dioumatch_amd.votenet.train_meter")
    meter = T.TrainMeter(torch.device("cpu"), guarded=True)
    rec = torch.zeros(4, dtype=torch.float64)
    rows = [(1.5, 0.25, 0.0, 3.0), (float("nan"), float("inf"), 1.0, float("nan")), (2.5, 0.75, 0.0, 5.0)]
    for loss, acc, skip, norm in rows:
        rec[0], rec[2] = norm, skip
        meter.add({"loss": torch.tensor(loss), "acc": torch.tensor(acc)}, rec)
    out = meter.result()
    assert out == {"acc": 0.5, "loss": 2.0, "grad_norm_value": 4.0, "steps": 2, "skipped_steps": 1}
    with pytest.raises(ValueError):
        meter.add({"loss": torch.tensor(1.0), "acc": torch.tensor(1.0)})
    with pytest.raises(RuntimeError):
        meter.add({"loss": torch.tensor(1.0)}, rec)  # the key set may not change


# ------------------------------------------------------------------ the guard, CPU form
def _pair(V, cfg, dev, semi=False, **kw):
    make = (lambda **k: V.SemiSupervisedStep(cfg, dev, num_proposal=K, seed=4, graphs=False, **k)) if semi \
        else (lambda **k: V.SupervisedStep(cfg, dev, num_proposal=K, seed=4, **k))
    return make(), make(**kw)


def _state(runner):
    st = runner.optimizer.state.get(runner.flat_params, {})
    out = [runner.flat_params.data.clone(), runner.flat_grad.clone()]
    out += [st[k].clone() for k in ("exp_avg", "exp_avg_sq")] if st else []
    out.append(torch.tensor(float(st["step"]) if st else 0.0))
    if hasattr(runner, "flat_teacher"):
        out.append(runner.flat_teacher.clone())
    return out


def test_cpu_guard_and_clip_semantics():
    load_pkg()
    V = importlib.import_module("3dioumatch_amd.votenet")
    cfg, dev = V.scannet_config(), torch.device("cpu")
    plain, guarded = _pair(V, cfg, dev, semi=True, guard=True)
    g = torch.Generator().manual_seed(0)
    n = plain.flat_grad.numel()

    def step(runner, grad, loss=1.0):
        runner.flat_grad.copy_(grad)
        runner._last_loss = torch.tensor(loss)
        runner._before_apply()
        runner._apply()

    # finite: bit-equal to the plain update, the norm in float64
    for it in range(2):
        grad = torch.randn(n, generator=g) * 0.1
        step(plain, grad)
        step(guarded, grad)
        for a, b in zip(_state(plain), _state(guarded)):
            assert torch.equal(a, b)
        rep = guarded.guard_report()
        want = float(grad.double().square().sum().sqrt())
        assert abs(rep["norm"] - want) <= 1e-12 * want and rep["coefficient"] == 1.0
        assert not rep["skipped_last"] and rep["skipped_total"] == 0
    # a non-finite gradient element, then a non-finite loss over a finite gradient: nothing moves
    before = _state(guarded)
    bad = grad.clone()
    bad[n - 1] = float("nan")
    step(guarded, bad)
    after = _state(guarded)
    for i, (a, b) in enumerate(zip(before, after)):
        if i != 1:  # (the gradient is what this test wrote; the update did not rewrite it)
            assert torch.equal(a, b), i
    assert torch.equal(after[1][:-1], bad[:-1]) and bool(torch.isnan(after[1][-1]))
    assert guarded.guard_report()["skipped_last"] and guarded.guard_report()["skipped_total"] == 1
    for loss in (float("inf"), float("nan")):
        step(guarded, grad, loss)
        for i, (a, b) in enumerate(zip(before, _state(guarded))):
            if i != 1:
                assert torch.equal(a, b), i
    assert guarded.guard_report()["skipped_total"] == 3
    # two entries of 3e38: the float64 norm is finite, the step applies (plain: the same bits)
    big = grad.clone()
    big[0], big[7] = 3e38, -3e38
    plain.global_step = guarded.global_step  # (the EMA ramp follows the loop's count, skipped steps included)
    step(plain, big)
    step(guarded, big)
    for a, b in zip(_state(plain), _state(guarded)):
        assert torch.equal(a, b)
    assert float(_state(guarded)[4]) == 3.0  # Adam's step advanced by the applied steps only
    rep = guarded.guard_report()
    assert not rep["skipped_last"] and rep["norm"] > 3.4e38 and rep["norm"] < float("inf")

    # more than one rank: a rank's own non-finite loss reaches every rank through the exchanged gradient
    grad = torch.randn(n, generator=g)
    guarded.world = 2
    guarded.flat_grad.copy_(grad)
    guarded._last_loss = torch.tensor(3.0)
    guarded._share_verdict()
    assert torch.equal(guarded.flat_grad, grad)
    guarded._last_loss = torch.tensor(float("inf"))
    guarded._share_verdict()
    assert bool(torch.isnan(guarded.flat_grad[0])) and torch.equal(guarded.flat_grad[1:], grad[1:])
    guarded.world = 1

    # clipping == clip_grad_norm_ + Adam
    ref, clipped = _pair(V, cfg, dev, clip_grad_norm=0.5)
    assert clipped.guarded
    for it in range(3):
        grad = torch.randn(n, generator=g) * (1e-4 if it == 1 else 1.0)
        ref.flat_grad.copy_(grad)
        total = torch.nn.utils.clip_grad_norm_([ref.flat_params], 0.5)
        ref._before_apply()
        ref._apply()
        step(clipped, grad)
        rep = clipped.guard_report()
        norm = float(grad.double().square().sum().sqrt())
        assert abs(rep["norm"] - norm) <= 1e-12 * norm and abs(float(total) - norm) <= 1e-4 * norm
        assert rep["coefficient"] == min(1.0, 0.5 / (norm + 1e-6))
        assert (rep["coefficient"] < 1.0) == (it != 1)
        # (torch's norm is a float32 sum over 1e6 elements: it is the reference's coefficient that is ~1e-5 off)
        assert torch.allclose(clipped.flat_grad, ref.flat_grad, rtol=1e-4, atol=0)
        assert torch.equal(clipped.flat_grad, grad * torch.tensor(rep["coefficient"], dtype=torch.float32))
        assert torch.allclose(clipped.flat_params.data, ref.flat_params.data, rtol=0, atol=2e-6)


# ------------------------------------------------------------------ the loop
class _StubRunner(object):
    """What Trainer touches of a runner, around a two-parameter network."""

    def __init__(self):
        T = importlib.import_module("3dioumatch_amd.votenet.train_meter")
        self.device = torch.device("cpu")
        self.net = torch.nn.Linear(2, 1)
        self.meter = T.TrainMeter(self.device)
        self.optimizer = torch.optim.Adam(self.net.parameters(), lr=1.0)
        self.global_step = 0
        self.epochs = []

    def set_epoch(self, epoch, base_lr):
        self.epochs.append((epoch, base_lr))

    def optimizer_state_dict(self):
        return self.optimizer.state_dict()

    def __call__(self, batch):
        self.global_step += 1
        ep = {"loss": torch.tensor(float(batch)), "obj_acc": torch.tensor(0.5), "center": torch.zeros(3)}
        self.meter.add(ep)
        return ep["loss"], ep


def test_trainer_intervals_log_lines_and_checkpoints(tmp_path):
    load_pkg()
    V = importlib.import_module("3dioumatch_amd.votenet")
    runner = _StubRunner()
    lines, evaluated = [], []

    def evaluate(net):
        assert not net.training
        evaluated.append(runner.epochs[-1][0])
        m = {2: 0.3, 4: 0.2, 6: 0.4}[evaluated[-1]]
        return {"mean_loss": 7.0, "detection_loss": 7.0}, [{"mAP": m, "AR": 0.5}, {"mAP": m / 2, "AR": 0.25}]

    trainer = V.Trainer(runner, lambda epoch: [epoch + 1.0, epoch + 2.0, epoch + 3.0, epoch + 4.0, 100.0],
                        evaluate=evaluate, log_dir=str(tmp_path), print_interval=2, eval_interval=2,
                        save_interval=3, log=lines.append)
    assert (trainer.print_interval, trainer.eval_interval, trainer.save_interval) == (2, 2, 3)
    assert V.Trainer(runner, None).base_lr == 1e-3  # pretrain.py:48; intervals: train.py:62-64
    d = V.Trainer(runner, None)
    assert (d.print_interval, d.eval_interval, d.save_interval) == (25, 25, 200)
    best = trainer.fit(7)
    assert evaluated == [2, 4, 6] and runner.net.training
    assert [e for e, _ in runner.epochs] == list(range(7))
    assert best == [0.4, 0.2]
    saved = sorted(os.listdir(tmp_path))
    assert saved == ["best_checkpoint_sum.tar", "checkpoint.tar", "checkpoint_0.tar", "checkpoint_3.tar",
                     "checkpoint_6.tar", "log_train.txt"]
    assert torch.load(tmp_path / "checkpoint.tar", weights_only=False)["epoch"] == 7
    best_ckpt = torch.load(tmp_path / "best_checkpoint_sum.tar", weights_only=False)
    assert best_ckpt["epoch"] == 7 and best_ckpt["loss"] == 7.0
    assert torch.load(tmp_path / "checkpoint_3.tar", weights_only=False)["epoch"] == 4
    # two read-outs per epoch of five batches; the fifth is in no printed mean, of this epoch or the next
    # (stat_dict starts empty every epoch, train.py:306)
    assert runner.meter.host_reads == 14
    means = [l for l in lines if l.startswith("mean ")]
    assert means[:6] == ["mean loss: 1.500000", "mean obj_acc: 0.500000", "mean loss: 3.500000",
                         "mean obj_acc: 0.500000", "mean loss: 2.500000", "mean obj_acc: 0.500000"]
    assert all(re.match(r"^mean [a-z_]+: -?\d+\.\d{6}$", l) for l in means)
    assert lines.count(" ---- batch: 002 ----") == 7 and lines.count(" ---- batch: 004 ----") == 7
    assert "eval mean detection_loss: 7.000000" in lines and "eval mAP: 0.300000" in lines
    assert open(tmp_path / "log_train.txt").read().splitlines() == lines
    with pytest.raises(ValueError):
        runner.meter = None
        V.Trainer(runner, None)


def _semi_runner(V, cfg, dev, seed):
    return V.SemiSupervisedStep(cfg, dev, num_proposal=K, seed=seed, graphs=False, meter=True, guard=True,
                                config_dict=_loose_filter(V, cfg))


def test_checkpoint_keys_and_bit_exact_resume(oracle_omp, monkeypatch, tmp_path):
    V, dev = _setup(False, oracle_omp, monkeypatch)
    cfg = V.scannet_config()
    batches = {e: V.make_semi_batch(1, 3, N, cfg, seed=20 + e, num_objects=5) for e in range(2)}
    epoch_batches = lambda epoch: [dict(batches[epoch])]  # noqa: E731

    def snapshot(runner):
        sd = runner.optimizer_state_dict()
        out = {"p": runner.flat_params.data.clone(), "t": runner.flat_teacher.clone()}
        for i, st in sd["state"].items():
            out["m%d" % i], out["v%d" % i], out["s%d" % i] = st["exp_avg"], st["exp_avg_sq"], st["step"]
        for name, net in (("net", runner.net), ("teacher", runner.teacher)):
            for k, b in net.named_buffers():
                out["%s.%s" % (name, k)] = b.clone()
        return out

    straight = _semi_runner(V, cfg, dev, 4)
    V.Trainer(straight, epoch_batches, log_dir=str(tmp_path / "a"), print_interval=1, log=None, seed=3).fit(2)
    first = _semi_runner(V, cfg, dev, 4)
    V.Trainer(first, epoch_batches, log_dir=str(tmp_path / "b"), print_interval=1, log=None, seed=3).fit(1)
    ckpt = torch.load(tmp_path / "b" / "checkpoint.tar", weights_only=False)
    assert sorted(ckpt) == sorted(["epoch", "optimizer_state_dict", "loss", "model_state_dict",
                                   "ema_model_state_dict"])  # train.py:570-579
    assert ckpt["epoch"] == 1 and ckpt["loss"] == 0
    assert sorted(ckpt["model_state_dict"]) == sorted(first.net.state_dict())
    assert len(ckpt["optimizer_state_dict"]["state"]) == len(list(first.net.parameters()))
    # the reference's optimizer takes the state as it is (train.py:218)
    torch.optim.Adam(_semi_runner(V, cfg, dev, 4).net.parameters(), lr=1e-3).load_state_dict(
        ckpt["optimizer_state_dict"])
    fresh = _semi_runner(V, cfg, dev, 9)  # other initial weights: everything comes from the file
    trainer = V.Trainer(fresh, epoch_batches, log_dir=str(tmp_path / "b"), print_interval=1, log=None, seed=3)
    assert trainer.resume(str(tmp_path / "b" / "checkpoint.tar")) == 1 and fresh.global_step == 1
    trainer.fit(2)
    a, b = snapshot(straight), snapshot(fresh)
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert float(a["s0"]) == 2.0
    # pretrain.py's checkpoint has no teacher
    sup = V.SupervisedStep(cfg, dev, num_proposal=K, meter=True)
    assert sorted(V.Trainer(sup, None).checkpoint(0)) == sorted(["epoch", "optimizer_state_dict", "loss",
                                                                  "model_state_dict"])


# ------------------------------------------------------------------ all-rank read-out
def _readout_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    load_pkg()
    T = importlib.import_module("3dioumatch_amd.votenet.train_meter")
    meter = T.TrainMeter(torch.device("cpu"))
    for s in range(2 + rank):  # rank 0: two steps, rank 1: three
        meter.add({"loss": torch.tensor(1.0 + rank + s), "pos_ratio": torch.tensor(0.25 * (rank + 1))})
    local = meter.result(reset=False)
    everyone = meter.result(group=dist.group.WORLD)
    with open(os.path.join(out_dir, "rank%d.json" % rank), "w") as f:
        json.dump({"local": local, "all": everyone, "reads": meter.host_reads}, f)
    dist.barrier()
    dist.destroy_process_group()


def test_all_rank_readout_two_ranks_gloo(tmp_path):
    world = 2
    port = 36500 + (os.getpid() % 2000)
    mp.spawn(_readout_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    r = [json.load(open(tmp_path / ("rank%d.json" % i))) for i in range(world)]
    assert r[0]["local"]["loss"] == 1.5 and r[1]["local"]["loss"] == 3.0
    want = {"loss": (1.0 + 2.0 + 2.0 + 3.0 + 4.0) / 5, "pos_ratio": (2 * 0.25 + 3 * 0.5) / 5, "steps": 5,
            "skipped_steps": 0}
    assert r[0]["all"] == want and r[1]["all"] == want
    assert r[0]["reads"] == 2  # one collective and one read per read-out, none per step


# ------------------------------------------------------------------ the front end
def _front_end():
    spec = importlib.util.spec_from_file_location("tools_train", os.path.join(ROOT, "tools", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_front_end_help_and_argument_wiring():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train.py"), "--help"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    for flag in ("--stage", "--synthetic", "--print_interval", "--eval_interval", "--save_interval", "--resume",
                 "--ema_decay", "--unlabeled_loss_weight", "--lr_decay_steps", "--clip_grad_norm", "--log_dir"):
        assert flag in out.stdout, flag
    fe = _front_end()
    flags = fe.parser().parse_args([])
    assert (flags.print_interval, flags.eval_interval, flags.save_interval, flags.max_epoch) == (25, 25, 200, 1001)
    semi = fe.settings(flags)  # train.py:46-70
    assert semi["semi"] and (semi["labeled_batch"], semi["unlabeled_batch"]) == (4, 8)
    assert semi["learning_rate"] == 2e-3 and semi["num_target"] == 128 and semi["guard"]
    assert semi["lr_decay_steps"] == [400, 600, 800, 900] and semi["lr_decay_rates"] == [0.3, 0.3, 0.1, 0.1]
    pre = fe.settings(fe.parser().parse_args(["--stage", "pretrain", "--no_guard", "--clip_grad_norm", "10"]))
    assert not pre["semi"] and (pre["labeled_batch"], pre["unlabeled_batch"]) == (8, 0)
    assert pre["learning_rate"] == 1e-3 and pre["num_target"] == 256 and pre["lr_decay_steps"] == [400, 600, 800]
    assert not pre["guard"] and pre["clip_grad_norm"] == 10.0
    with pytest.raises(SystemExit):
        fe.settings(fe.parser().parse_args(["--stage", "pretrain", "--batch_size", "4,8"]))
    with pytest.raises(SystemExit):
        fe.main(["--device", "cpu", "--synthetic", "4"])  # the loaders build on the GPU: said, not worked around
