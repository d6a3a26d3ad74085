"""The numpy restatement of the map pictures (fast3r_amd/maps.py, include/f3r.h "map pictures"): what
matplotlib.pylab.imsave(path, a, cmap=...) writes for an fp32 map, step by step -- Normalize with vmin = a.min(), vmax = a.max(), then
Colormap.__call__(bytes=True) -- and the RGB line and the contact sheet of the plot functions.  tests/test_maps.py holds it against
matplotlib's own bytes (the golden file, and live matplotlib where it imports)."""
import json
import os

import numpy as np

F32 = np.float32
NPZ_KEYS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "maps_npz_keys.json")
DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fast3r_amd", "data")


def table(name):
    """the (256, 3) uint8 table of 'turbo' or 'Greys' from the package's data files"""
    if name == "Greys":   # pure grey: a text file of 256 levels, '#' starts a comment
        levels = [int(w) for line in open(os.path.join(DATA, "greys_lut_u8.txt")) for w in line.split("#", 1)[0].split()]
        return np.repeat(np.array(levels, dtype=np.uint8).reshape(256, 1), 3, axis=1)
    b = open(os.path.join(DATA, "turbo_lut_u8.bin"), "rb").read()
    return np.frombuffer(b, dtype=np.uint8).reshape(256, 3)


def value_range(a):
    """numpy's fp32 minimum and maximum: a NaN anywhere makes both NaN, infinities take part"""
    a = np.asarray(a, F32)
    with np.errstate(invalid="ignore"):
        return a.min(), a.max()


def normalize(a):
    """matplotlib.colors.Normalize on an fp32 array as numpy 2 runs it: vmin and vmax become Python floats, so `resdat -= vmin` and
    `resdat /= (vmax - vmin)` are fp64 operations whose results are rounded back into the fp32 array -- the divisor is the fp64 difference
    (finite where the fp32 one overflows, and not rounded to fp32)"""
    a = np.asarray(a, F32)
    vmin, vmax = (np.float64(v) for v in value_range(a))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if vmin == vmax:
            return np.zeros_like(a)
        t = (a.astype(np.float64) - vmin).astype(F32)
        return (t.astype(np.float64) / (vmax - vmin)).astype(F32)


def colorize(a, lut):
    """(H, W) fp32 -> (H, W, 4) uint8"""
    x = normalize(a)
    with np.errstate(invalid="ignore", over="ignore"):
        xa = x * F32(256)
        xa[xa == 256] = 255
        bad = np.isnan(xa)
        index = np.clip(np.where(bad, 0, xa), 0, 255).astype(np.int64)   # under and over take the end colours; truncation toward zero
    out = np.empty(x.shape + (4,), np.uint8)
    out[..., :3] = lut[index]
    out[..., 3] = 255
    out[bad] = 0
    return out


def rgb_picture(img):
    """(3, H, W) fp32 planes -> (H, W, 4) uint8: ((img + 1) * 127.5).astype(int).clip(0, 255), alpha 255"""
    img = np.asarray(img, F32)
    u = ((img + F32(1)) * F32(127.5)).astype(int).clip(0, 255).astype(np.uint8)
    out = np.empty(img.shape[1:] + (4,), np.uint8)
    out[..., :3] = u.transpose(1, 2, 0)
    out[..., 3] = 255
    return out


def sheet(cells, max_columns=8):
    """cells: per view a list over cell rows of None or an (H, W, 4) picture -> the contact sheet: cell = (largest H, largest W); view i
    in column i % cols of band i // cols, its k-th picture in the band's k-th cell row, top left; everything else 0"""
    shapes = [p.shape[:2] for row in cells for p in row if p is not None]
    Hc, Wc = max(s[0] for s in shapes), max(s[1] for s in shapes)
    n, per = len(cells), len(cells[0])
    cols = min(n, max_columns)
    bands = -(-n // cols)
    out = np.zeros((bands * per * Hc, cols * Wc, 4), np.uint8)
    for i, row in enumerate(cells):
        for k, p in enumerate(row):
            if p is not None:
                y, x = ((i // cols) * per + k) * Hc, (i % cols) * Wc
                out[y:y + p.shape[0], x:x + p.shape[1]] = p
    return out


def npz_spec():
    """the notebook's seven arrays as data: key, shape with N, H, W symbolic, dtype"""
    return json.load(open(NPZ_KEYS))


def check_npz(path, n, H, W):
    """the file against tests/golden/maps_npz_keys.json: keys in order, shapes with N, H, W bound, dtypes -> the loaded file"""
    spec = npz_spec()
    data = np.load(path)
    assert list(data.files) == [e["key"] for e in spec]
    bind = {"N": n, "H": H, "W": W}
    for e in spec:
        a = data[e["key"]]
        assert list(a.shape) == [bind.get(d, d) for d in e["shape"]] and str(a.dtype) == e["dtype"], e["key"]
    return data
