"""The training loop on the MI355X (votenet/trainer.py): the inference engine on a runner's own network
(its weights are views into one flat buffer), and a short supervised run on synthetic scans that trains,
logs, evaluates, checkpoints and resumes with one host read per print interval."""
import importlib
import os

import pytest
import torch

from conftest import load_pkg

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def test_engine_runs_on_a_flattened_detector():
    """InferenceEngine(runner.net.eval()) == the engine on a detector of its own holding the same weights:
    the one-pass kernels' weight images do not depend on where a weight starts."""
    load_pkg()
    V = importlib.import_module("3dioumatch_amd.votenet")
    I = importlib.import_module("3dioumatch_amd.votenet.inference")
    step_mod = importlib.import_module("3dioumatch_amd.votenet.step")
    data = importlib.import_module("3dioumatch_amd.votenet.data")
    cfg = V.scannet_config()
    runner = V.SupervisedStep(cfg, DEV, num_proposal=64, seed=4, graphs=False)
    weights = [layer.conv.weight for m in runner.net.modules() if hasattr(m, "mlp_module")
               for layer in m.mlp_module]
    assert any(w.data_ptr() % 16 for w in weights)  # the case: a weight off the 16-byte grid
    twin = step_mod.build_detector(cfg, num_proposal=64, seed=9).to(DEV)
    twin.load_state_dict(runner.net.state_dict())
    pc = data.make_batch(2, 20000, cfg, seed=3, num_objects=5)["point_clouds"].to(DEV)
    got = I.InferenceEngine(runner.net.eval(), graphs=False)(pc)
    want = I.InferenceEngine(twin.eval(), graphs=False)(pc)
    runner.net.train()
    for k in ("center", "objectness_scores", "sem_cls_scores", "iou_scores"):
        assert bool(torch.isfinite(got[k]).all()) and torch.equal(got[k], want[k]), k


def test_short_run_trains_logs_evaluates_checkpoints_and_resumes(tmp_path):
    load_pkg()
    V = importlib.import_module("3dioumatch_amd.votenet")
    SD = importlib.import_module("3dioumatch_amd.votenet.scannet_data")
    cfg = V.scannet_config()
    names = ["scene%04d_00" % i for i in range(6)]
    data_dir = tmp_path / "scans"
    os.makedirs(data_dir)
    SD.write_synthetic_scans(str(data_dir), names, num_points=4000, instances=12, boxes=6, seed=1)
    scenes = SD.ScanNetScenes(str(data_dir), names, DEV, use_color=False, use_height=True)
    loader = SD.ScanNetLoader(scenes, cfg, 3000, seed=0, labeled=names[:4])
    val_loader = SD.ScanNetLoader(scenes, cfg, 3000, seed=0, labeled=names[4:])
    config_dict = {"dataset_config": cfg, "remove_empty_box": False, "use_3d_nms": True, "nms_iou": 0.25,
                   "use_old_type_nms": False, "cls_nms": True, "use_iou_for_nms": False,
                   "per_class_proposal": True, "conf_thresh": 0.05}

    def make(seed):
        runner = V.SupervisedStep(cfg, DEV, num_proposal=64, seed=seed, graphs=True, meter=True, guard=True)
        lines = []
        trainer = V.Trainer(runner, V.loader_epochs(runner, loader, "pretrain", 2),
                            evaluate=V.engine_evaluator(lambda: SD.eval_batches(val_loader, 2), config_dict),
                            log_dir=str(tmp_path / "log"), print_interval=2, eval_interval=1, save_interval=2,
                            log=lines.append, seed=5)
        return runner, trainer, lines

    runner, trainer, lines = make(4)
    start = runner.flat_params.data.clone()
    trainer.fit(2)  # two epochs of two steps, evaluation behind the second
    torch.cuda.synchronize()
    assert runner.graphs and runner.net.training
    assert runner.meter.host_reads == 2  # one per print interval, none per step
    assert runner.guard_report()["skipped_total"] == 0
    assert float(runner.optimizer.state[runner.flat_params]["step"]) == 4.0
    assert bool(torch.isfinite(runner.flat_params.data).all()) and not torch.equal(runner.flat_params.data, start)
    assert lines.count(" ---- batch: 002 ----") == 2
    means = [l for l in lines if l.startswith("mean loss: ")]
    assert len(means) == 2 and all(float(l.split(": ")[1]) > 0 for l in means)
    assert any(l.startswith("mean grad_norm_value: ") for l in lines)
    assert any(l.startswith("eval mean detection_loss: ") for l in lines)
    assert sum(l.startswith("eval mAP: ") for l in lines) == 2  # both thresholds, once
    saved = sorted(f for f in os.listdir(tmp_path / "log") if f.endswith(".tar"))
    assert {"checkpoint.tar", "checkpoint_0.tar"} <= set(saved) <= {"checkpoint.tar", "checkpoint_0.tar",
                                                                      "best_checkpoint_sum.tar"}
    ckpt = torch.load(tmp_path / "log" / "checkpoint.tar", weights_only=False)
    assert sorted(ckpt) == ["epoch", "loss", "model_state_dict", "optimizer_state_dict"] and ckpt["epoch"] == 2
    assert ckpt["loss"] > 0  # the evaluation's mean loss (pretrain.py:306)

    fresh, trainer2, lines2 = make(9)
    assert trainer2.resume(str(tmp_path / "log" / "checkpoint.tar")) == 2 and fresh.global_step == 4
    assert torch.equal(fresh.flat_params.data, runner.flat_params.data)
    trainer2.fit(3)
    torch.cuda.synchronize()
    assert "**** EPOCH 002, STEP 4 ****" in lines2 and not any("EPOCH 001" in l for l in lines2)
    assert float(fresh.optimizer.state[fresh.flat_params]["step"]) == 6.0
    assert fresh.meter.host_reads == 1
    assert torch.load(tmp_path / "log" / "checkpoint.tar", weights_only=False)["epoch"] == 3
