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
The validation path is complete with `model_step` (:169-188), `validation_step` (:239-306) and `on_validation_epoch_end` (:308-319): the
validation loss comes from the criterion's HIP kernels (fast3r_amd/losses.py, f3r_loss.hip) on the tensors the forward pass left on the
device, and is kept in `val_losses` / `val_loss_details_per_epoch`.  There is no training step and no backward.
"""
import logging
import re

import torch

from .align import align_local_pts3d_to_global as _align
from .focal import estimate_focal, estimate_focals  # noqa: F401  (module-level in the reference too, :1081)
from .cam_pose_metric import camera_pose_metrics as _camera_pose_metrics
from .depth_metric import evaluate_multiview_depth as _evaluate_multiview_depth
from .matching import match_views as _match_views
from .clean import clean_pointcloud as _clean_pointcloud
from .global_align import global_aligner as _global_aligner
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
        self.depth_metrics_per_epoch = {}  # dataset name -> {scene name -> the sample's dict of evaluate_multiview_depth}
        self.RRA_thresholds = [5, 15, 30]  # :103-104
        self.RTA_thresholds = [5, 15, 30]
        self.camera_pose_metrics_per_epoch = []  # one dict per evaluated sample (the reference feeds torchmetrics MeanMetrics, :106-112)
        self.current_epoch = 0  # Lightning's trainer sets it in the reference; here the caller's loop does
        self.val_losses = []  # one float per validation_step (the reference's MeanMetric val_loss, :250)
        self.val_loss_details_per_epoch = {}  # dataset name -> {logged key -> [one float per validation_step]}

    @classmethod
    def load_for_inference(cls, net):
        lit_module = cls(net=net, train_criterion=None, validation_criterion=None, optimizer=None, scheduler=None, compile=False)
        lit_module.eval()
        return lit_module

    def forward(self, views, **kw):
        return self.net(views, **kw)

    @property
    def device(self):
        """Where the net lives (Lightning's `self.device`); the CPU for a net without parameters."""
        params = self.net.parameters() if isinstance(self.net, torch.nn.Module) else iter(())
        p = next(params, None)
        return p.device if p is not None else torch.device("cpu")

    def model_step(self, batch, criterion):
        """Reference :169-188: move the batch's tensors to the net's device, run the forward pass and the criterion (any callable
        `criterion(views, preds) -> (loss, details)`; fast3r_amd.losses provides the reference's validation criterion on the GPU).
        -> (views, preds, loss, loss_details); loss and loss_details are None without a criterion (the reference fails to unpack there)."""
        device = self.device
        for view in batch:
            for name in "img pts3d valid_mask camera_pose camera_intrinsics F_matrix corres".split():
                if name in view:
                    view[name] = view[name].to(device, non_blocking=True)
        views = batch
        preds = self.forward(views)
        loss, loss_details = criterion(views, preds) if criterion is not None else (None, None)
        return views, preds, loss, loss_details

    def validation_step(self, batch, batch_idx, dataloader_idx=0):
        """Reference :239-306: the validation loss of the batch as a float, kept in `self.val_losses`; its details are kept under
        `self.val_loss_details_per_epoch[dataset_name]` with the reference's logged names, `val_detail_{dataset}_{key}` and the form
        without the view number, `val/{dataset}_{stripped key}`; then the camera-pose metrics for "Co3d_v2" and, in epoch 0 and every
        fifth epoch, the reconstruction metrics for dtu / 7scenes / nrgbd.  Raises ValueError without a validation criterion."""
        if self.validation_criterion is None:
            raise ValueError("validation_step needs a validation_criterion (fast3r_amd.losses.ConfLossMultiviewV2(...)); "
                             "load_for_inference() builds the module without one")
        views, preds, loss, loss_details = self.model_step(batch, self.validation_criterion)
        dataset_name = views[0]["dataset"][0]
        loss_value = float(loss.detach().cpu().item()) if torch.is_tensor(loss) else float(loss)
        self.val_losses.append(loss_value)
        if loss_details is not None:
            store = self.val_loss_details_per_epoch.setdefault(dataset_name, {})
            for key, value in loss_details.items():
                store.setdefault(f"val_detail_{dataset_name}_{key}", []).append(float(value))
                match = re.search(r"/(\d{1,2})$", key)
                if match:
                    store.setdefault(f"val/{dataset_name}_{key[:match.start()]}", []).append(float(value))
        if dataset_name == "Co3d_v2":
            self.evaluate_camera_poses(views, preds, niter_PnP=100, focal_length_estimation_method="first_view_from_global_head")
        if dataset_name in ("dtu", "7scenes", "nrgbd") and (self.current_epoch % 5 == 4 or self.current_epoch == 0):
            self.evaluate_reconstruction(views, preds, dataset_name=dataset_name, use_pts3d_from_local_head=self.eval_use_pts3d_from_local_head,
                                         min_conf_thr_percentile_for_local_alignment_and_icp=85, min_conf_thr_percentile_for_metric_cacluation=0)
        return loss_value

    def on_validation_epoch_end(self):
        """Reference :308-319 without a logger: -> {"val/loss": mean of the epoch's losses, every key of `val_loss_details_per_epoch`: its
        mean}, and clears both containers (NaN for "val/loss" without any step).  The metric containers are left to their readers."""
        mean = lambda xs: sum(xs) / len(xs) if xs else float("nan")  # noqa: E731
        out = {"val/loss": mean(self.val_losses)}
        for store in self.val_loss_details_per_epoch.values():
            for key, values in store.items():
                out[key] = mean(values)
        self.val_losses = []
        self.val_loss_details_per_epoch = {}
        return out

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

    def evaluate_multiview_depth(self, views, preds, dataset_name, **kw):
        """The reference's scripts/robustmvd_eval.py for the samples of a batch (fast3r_amd/depth_metric.py: median alignment, absrel,
        inlier ratios, optionally the sparsification curves, on the device): per sample the per-view metrics and their means, stored under
        self.depth_metrics_per_epoch[dataset_name][scene_name].  Also returns that dataset's dict.  `validation_step` does not call it."""
        for sample in _evaluate_multiview_depth(views, preds, **kw):
            self.depth_metrics_per_epoch.setdefault(dataset_name, {})[sample["scene"]] = sample
        return self.depth_metrics_per_epoch.get(dataset_name)

    def match_views(self, views, preds, **kw):
        """Reciprocal pointmap matches between view pairs of a forward pass (fast3r_amd/matching.py: the reference's find_reciprocal_matches
        over the pairs of make_pairs, batched on the device) -> ViewMatches.  The keywords of `fast3r_amd.match_views` pass through."""
        return _match_views(preds, views, **kw)

    @staticmethod
    def clean_pointcloud(preds, views=None, **kw):
        """The cross-view occlusion filter of the reference's BasePCOptimizer.clean_pointcloud (cloud_opt/base_opt.py:279-317) on a forward
        pass (fast3r_amd/clean.py) -> CleanedCloud.  The keywords of `fast3r_amd.clean_pointcloud` pass through."""
        return _clean_pointcloud(preds, views, **kw)

    @staticmethod
    def global_aligner(dust3r_output, device, **kw):
        """The reference's cloud_opt.global_aligner (fast3r_amd/global_align.py): pairwise observations -> a PointCloudOptimizer on `device`
        whose compute_global_alignment fuses them into one set of poses, focals and depth maps.  The keywords pass through."""
        return _global_aligner(dust3r_output, device, **kw)
