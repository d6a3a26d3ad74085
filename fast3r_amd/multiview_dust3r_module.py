"""Inference-only shim of MultiViewDUSt3RLitModule (fast3r/models/multiview_dust3r_module.py:67-126).

The reference class is a LightningModule whose training / validation / metric machinery is outside the MI355X hot
path.  What inference callers use is kept with the same names:
    lit = MultiViewDUSt3RLitModule.load_for_inference(net)   (:119-123)
    lit.eval(); lit(views) == net(views)                     (:125-126)
`align_local_pts3d_to_global` (:427-549) runs on the GPU (fast3r_amd/align.py);
`estimate_focal` (:1081-1109) and `estimate_camera_poses` (:807-869) run on the GPU (fast3r_amd/focal.py, fast3r_amd/pose.py;
SURVEY.md section 8f rank 2; the PnP solver is not OpenCV's -- see pose.py); `evaluate_reconstruction` (:551-735) runs on the GPU
(fast3r_amd/recon_metric.py: nearest neighbours, normals and statistics in HIP; docs/rows_f.md); `evaluate_camera_poses` (:737-804)
and `correct_preds_orientation` (:871-938) run on the GPU too: the poses go from the PnP launch to the pairwise RRA / RTA / mAA counts
(fast3r_amd/cam_pose_metric.py, f3r_pose_metric.hip) without leaving the device.  The torchmetrics / Lightning logging of the reference
is replaced by plain per-epoch containers (`reconstruction_metrics_per_epoch`, `camera_pose_metrics_per_epoch`).
"""
import logging

import torch

from .align import align_local_pts3d_to_global as _align
from .focal import estimate_focal, estimate_focals  # noqa: F401  (module-level in the reference too, :1081)
from .cam_pose_metric import camera_pose_metrics as _camera_pose_metrics
from .pose import estimate_camera_poses as _estimate_camera_poses
from .pose import estimate_camera_poses_device as _estimate_camera_poses_device
from .recon_metric import reconstruction_metrics as _reconstruction_metrics

log = logging.getLogger(__name__)


class MultiViewDUSt3RLitModule(torch.nn.Module):
    def __init__(self, net, train_criterion=None, validation_criterion=None, optimizer=None, scheduler=None,
                 compile=False, pretrained=None, resume_from_checkpoint=None, eval_use_pts3d_from_local_head=True):
        super().__init__()
        self.net = net
        self.train_criterion, self.validation_criterion = train_criterion, validation_criterion
        self.pretrained, self.resume_from_checkpoint = pretrained, resume_from_checkpoint
        self.eval_use_pts3d_from_local_head = eval_use_pts3d_from_local_head
        self.reconstruction_metrics_per_epoch = {}
        self.RRA_thresholds = [5, 15, 30]  # :103-104
        self.RTA_thresholds = [5, 15, 30]
        self.camera_pose_metrics_per_epoch = []  # one dict per evaluated sample (the reference feeds torchmetrics MeanMetrics, :106-112)

    @classmethod
    def load_for_inference(cls, net):
        lit_module = cls(net=net, train_criterion=None, validation_criterion=None, optimizer=None, scheduler=None, compile=False)
        lit_module.eval()
        return lit_module

    def forward(self, views, **kw):
        return self.net(views, **kw)

    @staticmethod
    def estimate_camera_poses(preds, views=None, niter_PnP=10, focal_length_estimation_method="individual"):
        """Reference :807-869: returns (poses_c2w_all, estimated_focals_all), per sample and per view; preds must be on the GPU."""
        return _estimate_camera_poses(preds, views, niter_PnP, focal_length_estimation_method)

    @staticmethod
    def correct_preds_orientation(preds, views):
        """Reference :871-938, *in place*: the data loader hands portrait samples over transposed to landscape, so per view `conf` and
        `pts3d_in_other_view` (and, when the local head's outputs are present, `conf_local`, `pts3d_local` and
        `pts3d_local_aligned_to_global`) become lists over samples, each entry transposed back where `true_shape` (H, W) says portrait.
        Only views are taken: nothing is copied, and the samples of one view may end up with different shapes."""
        if views is None:
            return
        for pred, view in zip(preds, views):
            true_shape = view["true_shape"]
            portrait = [bool(true_shape[i][0] > true_shape[i][1]) for i in range(true_shape.shape[0])]
            keys = ["conf", "pts3d_in_other_view"]
            if "pts3d_local" in pred:
                keys += ["conf_local", "pts3d_local"]
                if "pts3d_local_aligned_to_global" in pred:
                    keys.append("pts3d_local_aligned_to_global")
            for key in keys:
                pred[key] = [pred[key][i].transpose(0, 1) if p else pred[key][i] for i, p in enumerate(portrait)]

    def evaluate_camera_poses(self, views, preds, niter_PnP=10, focal_length_estimation_method="individual"):
        """Reference :737-804: align first for 'first_view_from_local_head', correct the orientation of the preds in place, estimate
        the poses, and score them against `views[v]['camera_pose']` over all view pairs.  Returns the list of per-sample dicts
        {RRA_at_5, RRA_at_15, RRA_at_30, RTA_at_5, RTA_at_15, RTA_at_30, mAA_30} and appends them to
        `self.camera_pose_metrics_per_epoch`.  The predicted poses are cast to the ground truth's dtype, as in the reference, and stay
        on the device from the PnP launch to the counts.
        Deviation: the reference evaluates the pairs in the ground truth's dtype (normally fp32); here they are evaluated in fp64 on
        the same values, which differs only for pairs within fp32 rounding of a threshold or bin edge (fast3r_amd/cam_pose_metric.py).
        With fewer than two views the reference warns and then fails on an unbound name; here: warn and return []."""
        if focal_length_estimation_method == "first_view_from_local_head":
            self.align_local_pts3d_to_global(preds, views)
        self.correct_preds_orientation(preds, views)
        if len(preds) < 2:
            log.warning("Not enough camera poses to compute relative errors.")
            return []
        poses, _ = _estimate_camera_poses_device(preds, niter_PnP, focal_length_estimation_method)  # (B, n_views, 4, 4) fp32 on the device
        gt = torch.stack([view["camera_pose"] for view in views]).transpose(0, 1)  # (B, n_views, 4, 4)
        batch_results = _camera_pose_metrics(poses.to(gt.dtype), gt.to(poses.device), self.RRA_thresholds, self.RTA_thresholds, max_threshold=30)
        self.camera_pose_metrics_per_epoch.extend(batch_results)
        return batch_results

    def align_local_pts3d_to_global(self, preds, views, min_conf_thr_percentile=0):
        """Adds `pts3d_local_aligned_to_global` to every pred (reference :427-549); preds must be on the GPU."""
        _align(preds, views, min_conf_thr_percentile)

    def evaluate_reconstruction(self, views, preds, dataset_name, min_conf_thr_percentile_for_local_alignment_and_icp=0,
                                min_conf_thr_percentile_for_metric_cacluation=0, use_pts3d_from_local_head=True):
        """Reference :551-735: per sample, the confident predicted points (registered onto the GT by one weighted similarity) against
        the valid GT points -> accuracy / completion / normal consistency, stored under
        self.reconstruction_metrics_per_epoch[dataset_name][scene_name].  Also returns that dataset's dict."""
        if use_pts3d_from_local_head:
            self.align_local_pts3d_to_global(preds, views, min_conf_thr_percentile=min_conf_thr_percentile_for_local_alignment_and_icp)
        assert min_conf_thr_percentile_for_local_alignment_and_icp >= min_conf_thr_percentile_for_metric_cacluation
        results = _reconstruction_metrics(views, preds, min_conf_thr_percentile_for_local_alignment_and_icp,
                                          min_conf_thr_percentile_for_metric_cacluation, use_pts3d_from_local_head)
        for result in results:
            if dataset_name not in self.reconstruction_metrics_per_epoch:
                self.reconstruction_metrics_per_epoch[dataset_name] = {}
            self.reconstruction_metrics_per_epoch[dataset_name].update(result)
        return self.reconstruction_metrics_per_epoch.get(dataset_name)
