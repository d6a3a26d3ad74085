"""What the post-processing front ends (scene.py, sky.py, mesh.py) share before they reach a kernel: unpacking what `inference()` returns,
bringing inputs to the work device, the input checks, and the read-back of packed bytes.  `who` is the caller's name, for the messages."""
import numpy as np
import torch

from ._lib import work_device


def preds_and_views(output_or_preds, views, who, needed_for):
    """{'preds', 'views'} (what `inference()` returns) or (preds, views) -> (preds, views)"""
    if isinstance(output_or_preds, dict):
        preds = output_or_preds["preds"]
        views = output_or_preds["views"] if views is None else views
    else:
        preds = output_or_preds
    if views is None:
        raise ValueError(f"{who}: views are needed for the {needed_for}")
    return preds, views


def fp32_on(t, dev, shape):
    """t as fp32 on dev, reshaped (as stored: nothing is permuted; the wrappers make a non-contiguous one contiguous)"""
    if t.device != dev or t.dtype != torch.float32:
        t = t.to(dev, torch.float32)
    return t.reshape(shape)


def as_tensor(x, what):
    """numpy or tensor -> (tensor, whether it was numpy)"""
    if isinstance(x, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(x)), True
    if not torch.is_tensor(x):
        raise ValueError(f"{what} must be a torch tensor or a numpy array, got {type(x).__name__}")
    return x, False


def on_work_device(x, who, name):
    """numpy or tensor -> (tensor on the work device, whether it was numpy)"""
    t, was_numpy = as_tensor(x, f"{who}: {name}")
    return t.to(work_device(t, name)), was_numpy


def read_back(rec):
    """the bytes of a packed uint8 device tensor: one copy through pinned memory"""
    host = torch.empty(rec.shape[0], dtype=torch.uint8, pin_memory=True)
    host.copy_(rec, non_blocking=True)
    torch.cuda.current_stream(rec.device).synchronize()
    return host.numpy().tobytes()


def check_inputs(preds, views, sample, not_sky, *, what, keys=None, mask_name="not_sky"):
    """The checks of (preds, views, sample) and of the per-view masks, under the caller's name `what`.  keys=None: the keys assemble_scene
    reads (both heads, the local one aligned); otherwise (points key, confidence key) of the one head the caller reads.  `not_sky`: None,
    "detect" or a list of per-view (H, W) masks, called `mask_name` in the messages (build_mesh passes its `valid` masks)."""
    if len(preds) == 0 or len(views) != len(preds):
        raise ValueError(f"{what}: need one view per pred and at least one (got {len(preds)} preds, {len(views)} views)")
    for i, pred in enumerate(preds):
        if keys is None and "pts3d_local_aligned_to_global" not in pred:
            raise KeyError(f"'pts3d_local_aligned_to_global' not in preds[{i}]: call align_local_pts3d_to_global(preds, views) first")
        for key in ("pts3d_in_other_view", "conf", "conf_local") if keys is None else keys:
            if key not in pred:
                raise KeyError(f"'{key}' not in preds[{i}]")
        if "img" not in views[i]:
            raise KeyError(f"'img' not in views[{i}]")
    B = preds[0]["conf" if keys is None else keys[1]].shape[0]
    if not 0 <= sample < B:
        raise ValueError(f"{what}: sample = {sample} outside [0, {B})")
    if isinstance(not_sky, str):
        if not_sky != "detect":
            raise ValueError(f"{what}: {mask_name} = {not_sky!r}; accepted values are None (no sky anywhere), 'detect' (detect_sky_masks "
                             "on the views' images) or a list of per-view (H, W) masks")
    elif not_sky is not None:
        if len(not_sky) != len(preds):
            raise ValueError(f"{what}: {mask_name} has {len(not_sky)} masks for {len(preds)} views")
        for i, m in enumerate(not_sky):
            m = torch.as_tensor(m)
            hw = tuple(preds[i]["conf" if keys is None else keys[1]].shape[1:3])
            if tuple(m.shape) != hw:
                raise ValueError(f"{what}: {mask_name}[{i}] has shape {tuple(m.shape)}; view {i} is {hw}")
            if m.dtype not in (torch.bool, torch.int8, torch.uint8):
                raise ValueError(f"{what}: {mask_name}[{i}] must be bool or int8, got {m.dtype}")
