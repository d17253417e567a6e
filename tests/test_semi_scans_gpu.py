"""Semi-supervised batches from label-free scans on the MI355X: scene_scan_semi_build (ScanLoader.semi_rows)
against its host restatement, the mixed batch of SceneLoader(unlabeled_scans=...) against the labeled
loader's device batch for the same scans, output reuse, the side-stream feed, poisoned allocations, and one
Trainer epoch of the semi-supervised step fed by a mixed loader.  Everything is compared bit for bit."""
import importlib

import numpy as np
import pytest
import torch

import dirty_memory
from conftest import load_pkg
from test_semi_scans import COMBOS, COUNTS, N, SPLITS, Data, explicit_draws, split_ids

load_pkg()
SC = importlib.import_module("3dioumatch_amd.votenet.scan_data")
SD = importlib.import_module("3dioumatch_amd.votenet.scannet_data")
SL = importlib.import_module("3dioumatch_amd.votenet.scene_loader")
V = importlib.import_module("3dioumatch_amd.votenet")
U = importlib.import_module("3dioumatch_amd.votenet.losses_unlabeled")

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def words(t):
    return t.contiguous().view(torch.int32)


def tensors(batch):
    return {k: v for k, v in batch.items() if torch.is_tensor(v)}


def assert_same_tensors(got, want):
    got, want = tensors(got), tensors(want)
    assert sorted(got) == sorted(want)
    for k, w in want.items():
        assert got[k].dtype == w.dtype and got[k].shape == w.shape, k
        assert torch.equal(words(got[k]), words(w)), k


def assert_is_host(got, want):
    assert sorted(got) == sorted(want)
    for k, w in want.items():
        g = got[k].cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), np.ascontiguousarray(w).view(np.uint32)
        differ = int((g != w).sum())
        print("%s: %d of %d words differ" % (k, differ, g.size))
        assert differ == 0, k


@pytest.fixture(scope="module", params=["scannet", "sunrgbd"])
def data(request, tmp_path_factory):
    return Data(request.param, str(tmp_path_factory.mktemp(request.param + "_semi_scans_gpu")))


# ------------------------------------------------------------------ the kernel against the host
@pytest.mark.parametrize("color,height", COMBOS)
def test_semi_rows_are_host_semi_rows(data, color, height):
    store = SC.ScanStore.from_files(data.files(), DEV, data.dataset)
    rows = SC.ScanLoader(store, N, use_color=color, use_height=height, seed=13)
    ids = [1, 2, 0]  # n == N, n > N, n < N
    for row0 in (1, 2, 61):
        counter = 1000 * row0 + 7
        got = rows.semi_rows(ids, counter, row0)
        assert got["point_clouds"].shape == (3, N, 3 + 3 * color + height)
        assert_is_host(got, rows.host_semi_rows(ids, counter, row0))
        draws = explicit_draws(data.dataset, [], ids, row0)
        assert_is_host(rows.semi_rows(ids, counter, row0, draws=draws),
                       rows.host_semi_rows(ids, counter, row0, draws=draws))
        part = {"ema_idx": draws["ema_idx"]}  # the rest drawn on the device
        assert_is_host(rows.semi_rows(ids, counter, row0, draws=part),
                       rows.host_semi_rows(ids, counter, row0, draws=part))
    # a row's draws are its place in the batch: the same scan at another row0 is another sample
    a, b = rows.semi_rows([2], 5, 1), rows.semi_rows([2], 5, 2)
    assert not torch.equal(a["point_clouds"], b["point_clouds"])
    assert not torch.equal(a["ema_point_clouds"], b["ema_point_clouds"])
    # the teacher's sample of a scan with n >= N is without replacement
    ema = rows.semi_rows([1, 2], 5, 1)["ema_point_clouds"].cpu().numpy()
    for r in range(2):
        assert len(np.unique(ema[r, :, 0:3], axis=0)) == N
    with pytest.raises(ValueError, match="out of range"):
        bad = explicit_draws(data.dataset, [], ids, 0)
        bad["ema_idx"][2, N - 1] = COUNTS[0]
        rows.semi_rows(ids, 0, 1, draws=bad)
    with pytest.raises(ValueError, match="row0"):
        rows.semi_rows(ids, 0, 62)


# ------------------------------------------------------------------ the mixed batch against the labeled loader
@pytest.mark.parametrize("color,height", COMBOS)
def test_mixed_semi_batch_is_the_labeled_loaders(data, color, height):
    both, mixed = data.pair(color, height, seed=21, device=DEV)
    for (nl, nu), counter in zip(SPLITS, (0, 3, 70000)):
        lab, unl = split_ids(nl, nu)
        want = both.semi_batch(lab, unl, counter)
        got = mixed.semi_batch(lab, unl, counter)
        assert_same_tensors(got, want)
        assert got["supervised_mask_host"] == want["supervised_mask_host"] == tuple([1] * nl + [0] * nu)
    lab, unl = split_ids(2, 3)
    draws = explicit_draws(data.dataset, lab, unl, 77)
    assert_same_tensors(mixed.semi_batch(lab, unl, 4, draws=draws), both.semi_batch(lab, unl, 4, draws=draws))
    # pretrain and eval batches are the plain loader's
    assert_same_tensors(mixed.pretrain_batch([0, 1], 2), both.pretrain_batch([0, 1], 2))
    assert_same_tensors(mixed.eval_batch([1, 0], 2), both.eval_batch([1, 0], 2))


def test_output_reuse_returns_the_same_tensors(data):
    _, mixed = data.pair(True, True, seed=2, device=DEV)
    lab, unl = split_ids(2, 3)
    out = mixed.allocate("semi", 2, 3)
    first = mixed.semi_batch(lab, unl, 1, out=out)
    for k, v in out[0].items():
        assert first[k] is v, k
    fresh = {k: v.clone() for k, v in tensors(mixed.semi_batch(lab, unl, 2)).items()}
    again = mixed.semi_batch(lab, unl, 2, out=out)
    for k, v in out[0].items():
        assert again[k] is v, k
    assert_same_tensors(again, fresh)
    rows = mixed._scan_rows
    tail = rows.allocate_semi(3)
    got = rows.semi_rows(unl, 2, 2, out=tail)
    for k, v in tail.items():
        assert got[k] is v and torch.equal(words(v), words(fresh[k][2:])), k
    with pytest.raises(ValueError, match="layout"):
        mixed.semi_batch(lab, unl[:2], 1, out=out)
    with pytest.raises(ValueError, match="layout"):
        rows.semi_rows(unl[:2], 0, 2, out=tail)


# ------------------------------------------------------------------ the side-stream feed
class StubRunner(object):
    """what scene_loader.feed asks of a runner"""

    def __init__(self):
        self.stream = torch.cuda.Stream(DEV)
        self.prefetched = 0

    def side_stream(self):
        return self.stream

    def prefetch_geometry(self, batch):
        self.prefetched += 1


def test_three_fed_batches_equal_direct_builds(data):
    _, mixed = data.pair(False, True, seed=6, device=DEV)
    plan = []
    for epoch in range(3):
        plan += list(SL.epoch_plan(len(mixed.labeled), 2, epoch, seed=1, num_unlabeled=len(mixed.unlabeled),
                                   unlabeled_batch_size=3))
    assert len(plan) == 3
    runner = StubRunner()
    fed = [{k: v.clone() for k, v in tensors(b).items()} for b in SL.feed(runner, mixed, plan, kind="semi")]
    torch.cuda.synchronize()
    assert len(fed) == 3 and runner.prefetched == 3
    for (counter, lab, unl), got in zip(plan, fed):
        assert sorted(unl.tolist()) == [0, 1, 2]
        assert_same_tensors(got, mixed.semi_batch(lab, unl, counter))


# ------------------------------------------------------------------ poisoned allocations
@pytest.mark.parametrize("fill", dirty_memory.FILLS, ids=dirty_memory.FILL_IDS)
def test_both_fills_on_poisoned_allocations(data, fill):
    _, mixed = data.pair(True, True, seed=3, device=DEV)
    lab, unl = split_ids(2, 3)

    def run():
        batch = tensors(mixed.semi_batch(lab, unl, 8))
        rows = mixed._scan_rows.semi_rows(unl, 8, 2)
        torch.cuda.synchronize()
        return batch, rows

    clean = run()
    with dirty_memory.poisoned(fill) as p:
        dirty = run()
    floats = [t for part in clean for t in part.values() if t.dtype == torch.float32]
    assert len(floats) == 15 and p.count >= len(floats)  # the float tensors of both are filled
    assert_same_tensors(dirty[0], clean[0])
    assert_same_tensors(dirty[1], clean[1])


# ------------------------------------------------------------------ end to end
def test_one_trainer_epoch_from_a_mixed_loader(tmp_path):
    """One epoch of the semi-supervised step (two steps of 2 labeled + 2 unlabeled rows) fed by a mixed
    loader: finite losses, and the logged statistics of the same epoch fed by the labeled loader that
    holds the unlabeled scans with their labels."""
    cfg = V.scannet_config()
    names = ["scene%04d_00" % i for i in range(8)]
    SD.write_synthetic_scans(str(tmp_path), names, num_points=4000, instances=12, boxes=6, seed=1)
    lab, unl = names[:4], names[4:]
    scenes = SD.ScanNetScenes(str(tmp_path), names, DEV, use_color=False, use_height=True)
    both = SD.ScanNetLoader(scenes, cfg, 3000, seed=0, labeled=lab, unlabeled=unl)
    store = SC.ScanStore.from_files([str(tmp_path / (s + "_vert.npy")) for s in unl], DEV, "scannet")
    mixed = SD.ScanNetLoader(SD.ScanNetScenes(str(tmp_path), lab, DEV, use_color=False, use_height=True), cfg,
                             3000, seed=0, unlabeled_scans=store)

    def epoch(loader):
        cd = U.default_config_dict(cfg, unlabeled_batch_size=2)
        runner = V.SemiSupervisedStep(cfg, DEV, num_proposal=64, seed=4, graphs=True, meter=True, guard=True,
                                      config_dict=cd)
        lines = []
        trainer = V.Trainer(runner, V.loader_epochs(runner, loader, "semi", 2, 2), print_interval=2,
                            log=lines.append, seed=5)
        assert trainer.train_one_epoch(0) == 2
        torch.cuda.synchronize()
        assert runner.meter.host_reads == 1 and runner.guard_report()["skipped_total"] == 0
        return trainer.last_stats, [l for l in lines if l.startswith("mean ")]

    got, got_lines = epoch(mixed)
    want, want_lines = epoch(both)
    assert got["steps"] == 2 and got["skipped_steps"] == 0
    assert "loss" in got and len(got) >= 10
    for k, v in got.items():
        assert np.isfinite(v), k
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], (k, got[k], want[k])
    assert got_lines == want_lines and len(got_lines) >= 10
