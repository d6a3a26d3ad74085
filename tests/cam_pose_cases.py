"""Seeded input recipes of the camera-pose metric fixture (tests/golden/cam_pose_cases.pt): tools/make_golden_cam_pose.py and the tests
both rebuild their inputs from here, so the fixture stores results only.

* pose sets: `pose_set(n_views, seed)` -> (pred, gt) fp32 (V, 4, 4) cam-to-world; pred = gt perturbed per view by a rotation of 3..25
  degrees about a random axis and a translation offset, so the pair errors spread over and beyond the [0, 30] degree histogram and
  stay clear of the small angles where fp32 acos loses digits;
* special sets: `special_set(name)`;
* evaluate scenes: pointmaps of known pinhole cameras (view 0 = the world frame, as in a Fast3R prediction), either a scene of
  tests/golden/pose_cases.pt by index or the mixed landscape / portrait batch built here.
"""
import math

import torch

RRA_THRESHOLDS = (5, 15, 30)
RTA_THRESHOLDS = (5, 15, 30)
MAX_THRESHOLD = 30
N_BINS = MAX_THRESHOLD + 1

# name: (n_views, seed).  The seeds are the first for which the margin conditions of tools/make_golden_cam_pose.py hold.
POSE_SETS = {"v2": (2, 0), "v3": (3, 0), "v8": (8, 0), "v12": (12, 0), "v64": (64, 0), "v1500": (1500, 0)}
EXACT_SETS = ("v2", "v3", "v8", "v12")     # fp32 reference, fp64 reference and the kernel must give identical counts
PER_PAIR_SETS = EXACT_SETS + ("v64",)      # per-pair arrays are stored
SPECIAL_SETS = ("pred_is_gt", "identity_pred", "opposite_translation", "half_turn", "trace_out_of_range", "nan_translation")
SPECIAL_VIEWS = 5

# evaluate cases: name -> ("fixture", index into tests/golden/pose_cases.pt) or ("mixed", seed)
EVAL_CASES = {"fixture_0": ("fixture", 0), "fixture_2": ("fixture", 2), "mixed_b2": ("mixed", 38)}
EVAL_NITER_PNP = 100
EVAL_MODES = ("first_view_from_global_head", "individual")
MIXED_SCENE = dict(n_views=3, H=40, W=56, focal=60.0, noise=0.002, n_out=150)  # sample 0 landscape (40, 56), sample 1 portrait (56, 40)


def random_rotation(g):
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
    if torch.det(q) < 0:
        q[:, 0] *= -1
    return q


def axis_angle(axis, angle):
    k = axis / axis.norm()
    K = torch.tensor([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]], dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def _se3(R, t):
    T = torch.eye(4, dtype=torch.float64)
    T[:3, :3], T[:3, 3] = R, t
    return T


def pose_set(n_views, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    pred, gt = [], []
    for _ in range(n_views):
        R, t = random_rotation(g), 2.0 * torch.randn(3, generator=g, dtype=torch.float64)
        ang = math.radians(3.0 + 22.0 * float(torch.rand(1, generator=g, dtype=torch.float64)))
        dR = axis_angle(torch.randn(3, generator=g, dtype=torch.float64), ang)
        dt = 0.6 * torch.randn(3, generator=g, dtype=torch.float64)
        gt.append(_se3(R, t))
        pred.append(_se3(dR @ R, t + dt))
    return torch.stack(pred).float(), torch.stack(gt).float()


def special_set(name):
    """(pred, gt) fp32 (SPECIAL_VIEWS, 4, 4)."""
    g = torch.Generator().manual_seed(77)
    gt = torch.stack([_se3(random_rotation(g), 2.0 * torch.randn(3, generator=g, dtype=torch.float64)) for _ in range(SPECIAL_VIEWS)])
    pred = gt.clone()
    if name == "pred_is_gt":
        pass
    elif name == "identity_pred":           # what a failed PnP returns for every view
        pred = torch.eye(4, dtype=torch.float64).repeat(SPECIAL_VIEWS, 1, 1)
    elif name == "opposite_translation":    # the translation measure is blind to sign
        pred[:, :3, 3] = -pred[:, :3, 3]
    elif name == "half_turn":               # every other view turned by 180 degrees: the lower extrapolation branch of acos
        pred[1::2, :3, :3] = pred[1::2, :3, :3] @ torch.diag(torch.tensor([1.0, -1.0, -1.0], dtype=torch.float64))
    elif name == "trace_out_of_range":      # a scaled rotation block: trace 4.5
        pred[2, :3, :3] = 1.5 * pred[2, :3, :3]
    elif name == "nan_translation":
        pred[2, 0, 3] = float("nan")
    else:
        raise KeyError(name)
    return pred.float(), gt.float()


def edges():
    """Every threshold and every histogram edge k * 30 / 31, as fp64."""
    e = [float(t) for t in RRA_THRESHOLDS + RTA_THRESHOLDS] + [k * MAX_THRESHOLD / N_BINS for k in range(N_BINS + 1)]
    return torch.tensor(sorted(set(e)), dtype=torch.float64)


def edge_distance(*errors):
    """Smallest |error - edge| over the given fp64 error tensors (non-finite and > 1e5 entries, the 1e6 rad default, are skipped)."""
    x = torch.cat([e.double().reshape(-1) for e in errors])
    x = x[torch.isfinite(x) & (x < 1e5)]
    if x.numel() == 0:
        return float("inf")
    return float((x[:, None] - edges()[None, :]).abs().min())


# ------------------------------------------------------------------------------------------------ evaluate scenes
def make_view(g, H, W, f, noise, n_out, anchor):
    """pointmap (H, W, 3) fp32 of a pinhole camera (focal f, principal point (W/2, H/2)) in the world frame, conf (H, W), cam_to_world"""
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    z = 2 + 3 * torch.rand(H, W, generator=g, dtype=torch.float64)
    Xc = torch.stack([(xs - W / 2) * z / f, (ys - H / 2) * z / f, z], -1)
    if anchor:
        R, t = torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
    else:
        R, t = random_rotation(g), torch.randn(3, generator=g, dtype=torch.float64)
    Xw = (Xc - t) @ R
    Xw = Xw + noise * torch.randn(Xw.shape, generator=g, dtype=torch.float64)
    if n_out:
        idx = torch.randperm(H * W, generator=g)[:n_out]
        Xw.view(-1, 3)[idx] += torch.randn(n_out, 3, generator=g, dtype=torch.float64)
    conf = 1.0 + torch.rand(H, W, generator=g) * 4 + 1e-3
    return Xw.float(), conf, _se3(R.t(), -R.t() @ t)


def mixed_scene(seed):
    """B = 2: sample 0 landscape, sample 1 portrait.  The portrait sample is stored transposed to landscape, the way the data loader
    delivers it, with `true_shape` = (H, W) of the image as taken.  -> (views, preds)."""
    m = MIXED_SCENE
    g = torch.Generator().manual_seed(seed)
    views, preds = [], []
    for v in range(m["n_views"]):
        land = make_view(g, m["H"], m["W"], m["focal"], m["noise"], m["n_out"], anchor=(v == 0))
        port = make_view(g, m["W"], m["H"], m["focal"], m["noise"], m["n_out"], anchor=(v == 0))
        preds.append({"pts3d_in_other_view": torch.stack([land[0], port[0].transpose(0, 1)]).contiguous(),
                      "conf": torch.stack([land[1], port[1].transpose(0, 1)]).contiguous()})
        # the "ground truth" is the scene's camera moved by 2..20 degrees and an offset, so that the pair errors spread over the histogram
        # instead of all falling into its first bin
        gt = []
        for T in (land[2], port[2]):
            ang = math.radians(2.0 + 18.0 * float(torch.rand(1, generator=g, dtype=torch.float64)))
            dR = axis_angle(torch.randn(3, generator=g, dtype=torch.float64), ang)
            gt.append(_se3(dR, 0.3 * torch.randn(3, generator=g, dtype=torch.float64)) @ T)
        views.append({"img": torch.zeros(2, 3, m["H"], m["W"]), "true_shape": torch.tensor([[m["H"], m["W"]], [m["W"], m["H"]]]),
                      "camera_pose": torch.stack(gt).float()})
    return views, preds


def fixture_scene(case):
    """views / preds of one case of tests/golden/pose_cases.pt (all samples landscape-shaped: true_shape = the stored shape)."""
    preds = [dict(p) for p in case["preds"]]
    views = []
    for p, T in zip(preds, case["gt_cam2world"]):
        B, H, W = p["conf"].shape
        views.append({"img": torch.zeros(B, 3, H, W), "true_shape": torch.tensor([[H, W]] * B), "camera_pose": T.float()})
    return views, preds


def eval_scene(name, pose_cases=None):
    kind, arg = EVAL_CASES[name]
    if kind == "mixed":
        return mixed_scene(arg)
    return fixture_scene(pose_cases[arg])
