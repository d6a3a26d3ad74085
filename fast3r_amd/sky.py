"""Sky detection on the GPU: the reference's `detect_sky_mask` (fast3r/viz/viser_visualizer.py:24-72, called per view at :348), which
decides `is_outdoor`, which decides whether "Mask Sky" is on, which decides what the exported PLY holds.  In the reference it is OpenCV
(8-bit HSV, `inRange`, a 7 x 7 dilation and a 7 x 7 opening) and scipy (`ndimage.label`) on the host, one view at a time; here it is one
batched call over all views of a scene, on a bit-packed bitmap (fast3r_amd/csrc/f3r_sky.hip, include/f3r.h "sky detection").

* `detect_sky_mask(img_rgb)`: the reference's signature, (H, W, 3) in [-1, 1] -> (H, W) int8, 1 = not sky.
* `detect_sky_masks(views, sample=0)`: all views at once from `view['img']` (B, 3, H, W) -> (list of (H, W) int8 device tensors, stats).
* `label_components(mask)`: 4-connected labelling of any (H, W) bitmap -> (roots int32 (H, W), count); a component's label is the
  smallest pixel index y * W + x in it, -1 marks the background.
* `morphology(mask)` / `classify(img)`: the two earlier stages on their own (what the tests pin them through).

The reference's quirks are kept: the 8-bit conversion is `trunc((img + 1) * 127.5)`, not the inverse of ImgNorm;
when no component touches row 0 the mask stays as it is.  Deviations: values outside [-1, 1] saturate where the reference's uint8 cast
wraps, and NaN reads as 0 (as in `assemble_scene`).
"""
import torch

from . import _lib, post_ops
from ._frontend import as_tensor, fp32_on
from ._lib import work_device

STAT_NAMES = ("sky_pixels", "components", "components_top", "components_kept", "branch")
BRANCH_NAMES = {_lib.F3R_SKY_EMPTY: "empty", _lib.F3R_SKY_NO_TOP: "no_top", _lib.F3R_SKY_TOP: "top"}
_ALL = _lib.F3R_SKY_CLASSIFY | _lib.F3R_SKY_MORPH | _lib.F3R_SKY_LABEL


def _bitmap_on_device(mask, name):
    """(H, W) bool / int8 / uint8 -> int8 on the work device (nonzero = set), the caller's device, and whether it was numpy"""
    m, was_numpy = as_tensor(mask, name)
    if m.dim() != 2 or m.dtype not in (torch.bool, torch.int8, torch.uint8):
        raise ValueError(f"{name} must be an (H, W) bool or int8 bitmap, got {tuple(m.shape)} {m.dtype}")
    home = m.device
    m = m.to(work_device(m, name))
    m = m.view(torch.int8) if m.dtype in (torch.bool, torch.uint8) else m   # any nonzero byte is set
    return m.contiguous(), home, was_numpy


def _give_back(t, home, was_numpy):
    t = t.to(home)
    return t.numpy() if was_numpy else t


def unpack_bits(words, H, W):
    """the (H, W) bool image of H * ceil(W / 64) bitmap words (int64 tensor, include/f3r.h f3r_sky_detect); for tests and debugging"""
    WW = post_ops.sky_row_words(W)
    shifts = torch.arange(64, device=words.device, dtype=torch.int64)
    bits = (words.reshape(H, WW, 1) >> shifts) & 1
    return bits.reshape(H, WW * 64)[:, :W].to(torch.bool)


def stats_dicts(stats):
    """the (V, 5) int32 stats of f3r_sky_detect as a list of dicts (branch by name); one small read-back"""
    out = []
    for row in stats.cpu().tolist():
        d = dict(zip(STAT_NAMES, row))
        d["branch"] = BRANCH_NAMES[d["branch"]]
        out.append(d)
    return out


def detect_sky_planes(planes, shapes):
    """all views at once from their (3, H * W) fp32 device planes -> (list of (H, W) int8 device tensors, (V, 5) int32 device stats).
    No host synchronisation: `assemble_scene(not_sky="detect")` calls this."""
    out = post_ops.sky_detect(planes, shapes, _ALL)
    return out["not_sky"], out["stats"]


def detect_sky_masks(views, sample=0):
    """`detect_sky_mask` for every view in one launch sequence.  views[i]['img']: (B, 3, H, W) in [-1, 1], on the host (uploaded here) or
    the device, as `inference()` or the device path provides them; H x W may differ between views.  -> (masks, stats): masks[i] an
    (H, W) int8 device tensor, 1 = not sky; stats[i] = {sky_pixels (entering the labelling), components, components_top,
    components_kept, branch: 'empty' | 'no_top' | 'top'}."""
    if len(views) == 0:
        raise ValueError("detect_sky_masks: no views")
    planes, shapes = [], []
    dev = None
    for i, view in enumerate(views):
        if "img" not in view:
            raise KeyError(f"'img' not in views[{i}]")
        img = view["img"]
        if not torch.is_tensor(img) or img.dim() != 4 or img.shape[1] != 3:
            raise ValueError(f"detect_sky_masks: views[{i}]['img'] must be a (B, 3, H, W) tensor, got {tuple(getattr(img, 'shape', ()))}")
        if not 0 <= sample < img.shape[0]:
            raise ValueError(f"detect_sky_masks: sample = {sample} outside [0, {img.shape[0]})")
        if dev is None:
            dev = work_device(img, "views")
        shapes.append((int(img.shape[2]), int(img.shape[3])))
        planes.append(fp32_on(img[sample], dev, (3, -1)))   # the (3, H, W) planes as stored: nothing is permuted
    masks, stats = detect_sky_planes(planes, shapes)
    return masks, stats_dicts(stats)


def detect_sky_mask(img_rgb):
    """The reference's `detect_sky_mask`: img_rgb (H, W, 3) in [-1, 1], numpy or torch, host or device -> (H, W) int8, 1 = not sky: a
    numpy array for numpy input, otherwise a tensor on the input's device."""
    t, was_numpy = as_tensor(img_rgb, "detect_sky_mask: img_rgb")
    if t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"detect_sky_mask: img_rgb must be (H, W, 3), got {tuple(t.shape)}")
    if t.dtype != torch.float32:   # the reference does `(img + 1) * 127.5` in the array's own type: only fp32 is reproduced here
        raise ValueError(f"detect_sky_mask: img_rgb must be float32 in [-1, 1], got {t.dtype}")
    home = t.device
    dev = work_device(t, "img_rgb")
    H, W = int(t.shape[0]), int(t.shape[1])
    planes = t.to(dev).permute(2, 0, 1).contiguous().reshape(3, H * W)   # the kernel reads planes
    masks, _ = detect_sky_planes([planes], [(H, W)])
    return _give_back(masks[0], home, was_numpy)


def label_components(mask):
    """4-connected components of an (H, W) bool / int8 bitmap (nonzero = set), numpy or torch.  -> (roots, count): roots (H, W) int32, for
    a set pixel the smallest pixel index y * W + x of its component, -1 for the background (numpy for numpy input, otherwise a tensor on
    the input's device); count = the number of components."""
    m, home, was_numpy = _bitmap_on_device(mask, "label_components: mask")
    out = post_ops.sky_detect([m], [tuple(m.shape)], _lib.F3R_SKY_LABEL, want_not_sky=False, want_roots=True)
    count = int(out["stats"][0, 1].item())
    return _give_back(out["roots"][0], home, was_numpy), count


def morphology(mask):
    """step 4 alone (dilate 7 x 7, open 7 x 7, pixels outside the image ignored) on an (H, W) bitmap -> (H, W) bool"""
    m, home, was_numpy = _bitmap_on_device(mask, "morphology: mask")
    H, W = m.shape
    out = post_ops.sky_detect([m], [(H, W)], _lib.F3R_SKY_MORPH)
    return _give_back(unpack_bits(out["bits"], H, W), home, was_numpy)


def classify(img_chw, bits=False):
    """steps 1-3 alone on a (3, H, W) image in [-1, 1] -> the (H, W) bool bitmap of sky-coloured pixels before any morphology (or, with
    bits=True, its H * ceil(W / 64) packed words as an int64 device tensor)"""
    t, was_numpy = as_tensor(img_chw, "classify: img")
    if t.dim() != 3 or t.shape[0] != 3:
        raise ValueError(f"classify: img must be (3, H, W), got {tuple(t.shape)}")
    home = t.device
    H, W = int(t.shape[1]), int(t.shape[2])
    out = post_ops.sky_detect([fp32_on(t, work_device(t, "img"), (3, -1))], [(H, W)], _lib.F3R_SKY_CLASSIFY)
    if bits:
        return out["bits"]
    return _give_back(unpack_bits(out["bits"], H, W), home, was_numpy)
