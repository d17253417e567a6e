"""Host-side mirror of the VoteNet-IoU callers of the hot path (reference models/*.py), used
by bench.py and the train-step tests.  The reference's own model files also run unchanged on
top of `3dioumatch_amd/dropin`."""
from .backbone import Pointnet2Backbone  # noqa: F401
from .config import DatasetConfig, scannet_config, sunrgbd_config  # noqa: F401
from .detector import VoteNet  # noqa: F401
from .heads import GridConv, ProposalModule, VotingModule  # noqa: F401
from .losses import get_labeled_loss, get_loss  # noqa: F401
from .data import make_batch, make_semi_batch  # noqa: F401
from .step import (SemiSupervisedStep, SupervisedStep, update_ema_variables, lr_at,  # noqa: F401
                   bn_momentum_at)
from .eval_helper import (APCalculator, DeviceAPCalculator, EvalLossMeter, parse_groundtruths,  # noqa: F401
                          parse_groundtruths_device, parse_predictions, parse_predictions_device)
from .eval_det import eval_det, eval_det_cls, voc_ap  # noqa: F401
from .train_meter import TrainMeter, tb_name  # noqa: F401
from .trainer import Trainer, engine_evaluator, loader_epochs  # noqa: F401
from .scan_data import ScanLoader, ScanStore  # noqa: F401
from .detect import Detections, TiledDetections, detect, detect_tiled  # noqa: F401
from .detect import host_merge_nms, merge_nms_gpu, seam_reach, seam_settings  # noqa: F401
from .scan_tiles import TileStore, tile_grid  # noqa: F401
from .scan_voxels import VoxelStore, host_voxels  # noqa: F401
from .point_labels import PointLabels, host_label_points, label_points  # noqa: F401
from .point_index import PointIndex, host_point_index, point_index_gpu  # noqa: F401
from .mask_eval import MaskAPCalculator, MaskMatch, PointTruth, host_match_masks, match_masks  # noqa: F401
