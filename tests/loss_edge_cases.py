"""Seeded cases of the validation loss (csrc/f3r_loss.hip, f3r_mv_conf_loss) at the edges of its indexing, a Python restatement of its tile
partition, and the guarded placement of its device buffers; shared by tests/test_loss_edge_cases.py (no GPU: the cases reach what they are
named for, the reference is stable on them, wrong restatements miss) and tests/test_loss_geometry_gpu.py (the kernels, through the C ABI).

Reference of every value comparison: loss_ref.multiview_conf_loss in float64.  `restate` below is a second, pixel-flat restatement that
follows the kernel's structure (moments per segment, factors per group, sums per segment, finish); it exists to carry the deliberately
wrong variants of test_loss_edge_cases.py and is itself checked against loss_ref there.

Families (ids are symbolic in nb = min(4 x CUs, 2048), the grid of the two streaming passes; the builders take nb):
  A  partition: T tiles of one-tile segments (1 .. 7 pixels) around nb and 2 nb, at least four segments per workgroup, and "crossing":
     multi-tile views among one-tile ones with all-invalid and zero-pixel views between them; V4, and V3 + avg_log1p + dist_clip
  B  counts: more than 4 groups, 64 members, 256 segments, 256 views; V4, V4 + local_scale_consistent, V3
  C  pixel counts around the 4 pixels of a thread and the 1024 of a tile, B = 3: samples 1 and 2 start at every residue of 4 pixels
  D  (run_loss(shifts=...)) one operand at a time off the 16-byte path
  E  poses whose 4 x 4 inverse needs row swaps; a general affine pose; fp64 poses
  F  mask bytes other than 0 / 1; NaN and +inf ground truth at a valid pixel, NaN at an invalid one
"""
import functools
import math
import os
import re

import torch

import loss_cases as C
import loss_ref
from post_cases import Bufs, _p, _stream

F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "fast3r_amd", "csrc", "f3r_loss.hip")

# f3r_loss.hip: THREADS * PX, MAX_BLOCKS, `const int nb = cus * 4` (pinned against the source text by test_loss_edge_cases.py)
THREADS, PX, MAX_BLOCKS, BLOCKS_PER_CU, WAVES, WAVE = 256, 4, 2048, 4, 4, 64
TILE = THREADS * PX


def source_constants():
    """the same constants read from the kernel's source text"""
    src = open(SOURCE).read()
    grab = lambda pat: int(re.search(pat, src).group(1))  # noqa: E731
    threads, px = grab(r"constexpr int THREADS = (\d+);"), grab(r"constexpr int PX = (\d+);")
    assert re.search(r"constexpr int TILE = THREADS \* PX;", src) and re.search(r"constexpr int WAVES = THREADS / 64;", src)
    assert re.search(r"return nb > MAX_BLOCKS \? MAX_BLOCKS : nb;", src)
    return dict(THREADS=threads, PX=px, TILE=threads * px, MAX_BLOCKS=grab(r"constexpr int MAX_BLOCKS = (\d+);"),
                BLOCKS_PER_CU=grab(r"const int nb = cus \* (\d+);"), WAVES=threads // 64)


def num_blocks(cus):
    return min(BLOCKS_PER_CU * cus, MAX_BLOCKS)


# ================================================================================================ the partition, restated
def first_tile(k, T, nb):
    return k * T // nb


def block_of_tile(t, T, nb):
    """f3r_loss.hip: block_of_tile, statement by statement -> (workgroup, correction steps taken)"""
    k = min(t * nb // T, nb - 1)
    steps = 0
    while k + 1 < nb and first_tile(k + 1, T, nb) <= t:
        k, steps = k + 1, steps + 1
    while k > 0 and first_tile(k, T, nb) > t:
        k, steps = k - 1, steps + 1
    return k, steps


class Partition:
    """npix: pixels per view; a segment is s = view * B + sample.  tile0 [nseg + 1], first [nb + 1], met[k]: the segments workgroup k sums a
    partial for, in order (from the tile intervals alone, not from the kernel's loop); slots: the (k, s, k + s) written"""

    def __init__(self, npix, B, nb):
        self.nb, self.B, self.nseg = nb, B, len(npix) * B
        self.seg_npix = [n for n in npix for _ in range(B)]
        self.tile0 = [0]
        for n in self.seg_npix:
            self.tile0.append(self.tile0[-1] + (-(-n // TILE) if n > 0 else 0))
        self.T = T = self.tile0[-1]
        self.first = [first_tile(k, T, nb) for k in range(nb + 1)]
        self.met, s = [], 0
        for k in range(nb):
            ta, tb = self.first[k], self.first[k + 1]
            row = []
            if ta < tb:
                while self.tile0[s + 1] <= ta:
                    s += 1
                q = s
                while q < self.nseg and self.tile0[q] < tb:
                    if self.tile0[q + 1] > self.tile0[q]:
                        row.append(q)
                    q += 1
            self.met.append(row)
        self.slots = [(k, s, k + s) for k, row in enumerate(self.met) for s in row]

    def owner(self):
        """[T]: the workgroup of every tile"""
        out = []
        for k in range(self.nb):
            out += [k] * (self.first[k + 1] - self.first[k])
        return out

    def gathered(self, s):
        """the workgroups gather_partials reads for segment s (empty for a segment without tiles)"""
        t0, t1 = self.tile0[s], self.tile0[s + 1]
        if t1 <= t0:
            return []
        kf, kl = block_of_tile(t0, self.T, self.nb)[0], block_of_tile(t1 - 1, self.T, self.nb)[0]
        return [k for k in range(kf, kl + 1) if self.first[k] < self.first[k + 1]]

    def meeting(self):
        """s -> the workgroups that meet it"""
        out = {}
        for k, s, _ in self.slots:
            out.setdefault(s, []).append(k)
        return out


def partition(npix, B, nb):
    return Partition(list(npix), B, nb)


# ================================================================================================ geometries of family A
A_T = {"1": lambda nb: 1, "nb/2+1": lambda nb: nb // 2 + 1, "nb-1": lambda nb: nb - 1, "nb": lambda nb: nb, "nb+1": lambda nb: nb + 1,
       "2nb-1": lambda nb: 2 * nb - 1, "2nb+1": lambda nb: 2 * nb + 1}
A_GEOMS = tuple(f"T={k}" for k in A_T) + ("four", "crossing")
ZERO_W = 3   # a zero-pixel view is (B, 0, ZERO_W)


def _short(i):
    return (1, 1 + (i * 3 + 4) % 7)   # 1 .. 7 pixels: one tile


def a_geometry(geom, nb):
    """-> dict(shapes, B, empty: views with every pixel invalid, zero: views without pixels, motifs: [(multi, empty, zero, multi) view indices])"""
    if geom.startswith("T="):
        return dict(shapes=[_short(i) for i in range(A_T[geom[2:]](nb))], B=1, empty=[], zero=[], motifs=[])
    if geom == "four":   # B = 2: T = 2 V >= 4 nb + 3
        return dict(shapes=[_short(i) for i in range((4 * nb + 3 + 1) // 2)], B=2, empty=[], zero=[], motifs=[])
    assert geom == "crossing" and nb >= 16
    # T = 4 nb exactly: workgroup k owns the tiles [4 k, 4 k + 4).  A motif is multi (last tile at 4 j), empty, zero-pixel, multi (first
    # tile at 4 j + 2) -- workgroup j ends the first, crosses the two and begins the second -- or with the two short views the other way round.
    shapes, empty, zero, motifs = [], [], [], []
    tiles = 0

    def add(shape):
        nonlocal tiles
        shapes.append(shape)
        n = shape[0] * shape[1]
        tiles += -(-n // TILE) if n else 0
        return len(shapes) - 1

    for i in range(3):
        add(_short(i))
    for multi_a, multi_b, zero_first in (((1, 4097), (1, 9217), False), ((3, 2049), (5, 1000), True)):
        while (tiles + -(-multi_a[0] * multi_a[1] // TILE) - 1) % 4 != 0:
            add(_short(len(shapes)))
        a = add(multi_a)
        if zero_first:
            z, e = add((0, ZERO_W)), add((1, 5))
        else:
            e, z = add((1, 5)), add((0, ZERO_W))
        b = add(multi_b)
        empty.append(e)
        zero.append(z)
        motifs.append((a, e, z, b))
        for i in range(5):
            add(_short(len(shapes)))
    add((2, 4096))            # a whole number of tiles: 8
    zero.append(add((0, ZERO_W)))
    while tiles < 4 * nb - 1:
        add(_short(len(shapes)))
    add(_short(len(shapes)))
    zero.append(add((0, ZERO_W)))   # the last view has no pixels
    assert tiles == 4 * nb
    return dict(shapes=shapes, B=1, empty=empty, zero=zero, motifs=motifs)


def crossing_workgroups(part, geo):
    """per motif, the workgroups that meet multi, empty and multi in a row, with the zero-pixel view's segment between the two multis"""
    out = []
    for a, e, z, b in geo["motifs"]:
        assert geo["B"] == 1 and a < min(e, z) and max(e, z) < b and part.tile0[z] == part.tile0[z + 1]
        out.append([k for k, row in enumerate(part.met) if any(row[i:i + 3] == [a, e, b] for i in range(len(row)))])
    return out


def check_a_preconditions(nb):
    """every geometry of family A has, at this nb, the property it is named for"""
    for key, fn in A_T.items():
        geo = a_geometry(f"T={key}", nb)
        p = partition([h * w for h, w in geo["shapes"]], geo["B"], nb)
        assert p.T == fn(nb) and all(1 <= n <= 7 for n in p.seg_npix)
        assert max(len(row) for row in p.met) == (1 if p.T <= nb else 2 if p.T < 2 * nb else 3)
        steps = sum(block_of_tile(t, p.T, nb)[1] for t in range(p.T))
        assert (steps > 0) == (p.T % nb != 0), (key, steps)    # the correction loop of block_of_tile runs unless nb divides T
    geo = a_geometry("four", nb)
    p = partition([h * w for h, w in geo["shapes"]], geo["B"], nb)
    assert p.T >= 4 * nb + 3 and all(1 <= n <= 7 for n in p.seg_npix) and min(len(row) for row in p.met) >= 4
    geo = a_geometry("crossing", nb)
    npix = [h * w for h, w in geo["shapes"]]
    p = partition(npix, geo["B"], nb)
    assert p.T >= 4 * nb and sum(npix) < 100_000
    multi = [n for n in npix if n > TILE]
    assert len(multi) >= 4 and all(4097 <= n <= 9217 for n in multi) and all(n <= 7 for n in npix if n <= TILE)
    assert all(npix[z] == 0 for z in geo["zero"]) and 0 not in geo["zero"] and geo["zero"][-1] == len(npix) - 1 and len(geo["zero"]) >= 3
    crossers = crossing_workgroups(p, geo)
    assert len(crossers) == 2 and all(len(ks) == 1 for ks in crossers), crossers
    for (a, e, z, b), (k,) in zip(geo["motifs"], crossers):   # k ends a, begins b: both are shared with a neighbour
        assert npix[a] > TILE and npix[b] > TILE and npix[z] == 0 and e in geo["empty"]
        assert k - 1 in p.meeting()[a] and k + 1 in p.meeting()[b]


# ================================================================================================ inputs
V4 = dict(version=4)
V4_LSC = dict(version=4, local_scale_consistent=True)
V3 = dict(version=3)
V3_CLIP = dict(version=3, norm_mode="avg_log1p", dist_clip=3.1)


def ref_kwargs(recipe):
    kw = dict(version=recipe["version"], norm_mode=recipe.get("norm_mode", "avg_dis"), gt_scale=recipe.get("gt_scale", False),
              dist_clip=recipe.get("dist_clip"), alpha=C.ALPHA)
    if recipe["version"] == 4:
        kw["local_scale_consistent"] = recipe.get("local_scale_consistent", False)
    return kw


def sample_scales(B):
    """one depth scale per sample in [1, 3), all different: a factor taken from another sample's group changes the output"""
    return tuple(1.0 + 2.0 * ((b * 0.6180339887) % 1.0) for b in range(B))


def _rotation(q):
    q = q / (((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]).sqrt()[:, None]
    w, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                        2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                        2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], dim=-1).reshape(-1, 3, 3)


# quarter and half turns about the axes (and their products): in the 4 x 4 elimination RZ90 swaps rows 0 and 1 at column 0, RY90 rows 0 and 2
# at column 0, RX90 rows 1 and 2 at column 1, CYCLE both columns; the half turns keep the rows and give negative pivots
TURNS = {"RZ90": [[0, -1, 0], [1, 0, 0], [0, 0, 1]], "RY90": [[0, 0, 1], [0, 1, 0], [-1, 0, 0]], "RX90": [[1, 0, 0], [0, 0, -1], [0, 1, 0]],
         "CYCLE": [[0, 0, 1], [1, 0, 0], [0, 1, 0]], "RX180": [[1, 0, 0], [0, -1, 0], [0, 0, -1]], "RZ180": [[-1, 0, 0], [0, -1, 0], [0, 0, 1]]}
E_TURNS = (("RZ90", "RX90"), ("RY90", "CYCLE"), ("RX180", "RZ180"))   # [view][sample]
SMALL = 1e-6    # the quaternion noise of the rotation that multiplies a turn: the would-be pivots are about 1e-6, not 0 -- an elimination
                # that does not swap still runs, and loses ten digits


def turned_poses(g, names, affine=False):
    """(B, 4, 4) fp64: turn x small rotation [x a stretch and shear], a translation"""
    B = len(names)
    R = torch.tensor([TURNS[n] for n in names], dtype=F64) @ _rotation(torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=F64) + SMALL * C._noise(g, B, 4))
    if affine:
        R = R @ (torch.diag(torch.tensor([1.5, 0.7, 1.2], dtype=F64)) + 0.1 * C._noise(g, B, 3, 3))
    P = torch.zeros(B, 4, 4, dtype=F64)
    P[:, :3, :3] = R
    P[:, :3, 3] = 0.3 * C._noise(g, B, 3)
    P[:, 3, 3] = 1.0
    return P


# Every factor is a sum over up to tens of thousands of pixels, so it carries a relative rounding error of about 1e-15, and L = |pred / n_pred -
# g / n_gt| inherits that as an ABSOLUTE error of about 1e-15 (its two terms are of size 1).  With loss_cases' predictions (the ground truth plus
# noise) views of 1 .. 7 pixels give terms arbitrarily close to 0, where the project's measure |got - ref| / max(|ref|, 1e-2) turns 2e-15 into
# 2e-13: two float64 evaluations of the reference then disagree beyond the bound.  A constant offset (times the sample's depth scale) keeps every L, and with conf >= 1 every
# confidence term, above 0.1 (asserted in test_loss_edge_cases.py), so the measure stays a relative one.
BIAS_GLOBAL = torch.tensor([4.0, -3.0, 2.5], dtype=F64)
BIAS_LOCAL = torch.tensor([-3.0, 4.0, 2.0], dtype=F64)


def build(shapes, B, seed, local=True, holes=0.2, depth_scale=None, poses=None, pose_fp64=False, empty=(), mask_bytes=False, gt_value=None):
    """-> (views, preds) on the CPU, built like loss_cases.build: float64 from uniforms, rounded to fp32 once.  poses: per view a function
    g -> (B, 4, 4) fp64 (default: loss_cases' moderate rotations); empty: views with every pixel invalid; mask_bytes: uint8 masks with the bytes
    {0, 1, 2, 128, 255}; gt_value: (view, sample, i, j, coordinate, value, valid) written into the ground truth and the mask after the build
    (value None: the mask alone).
    The predictions are loss_cases' plus a constant offset (BIAS_*): see there"""
    g = torch.Generator().manual_seed(7000 + seed)
    ps = [(poses[v](g) if poses else C._poses(g, B)) for v in range(len(shapes))]
    inv0 = torch.linalg.inv(ps[0])
    scale = torch.tensor(depth_scale or (1.0,) * B, dtype=F64)[:, None, None]
    views, preds = [], []
    for v, (H, W) in enumerate(shapes):
        z = (1.0 + 3.0 * torch.rand(B, H, W, generator=g, dtype=F64)) * scale
        xy = (torch.rand(B, H, W, 2, generator=g, dtype=F64) - 0.5) * 1.2 * z[..., None]
        cam = torch.cat([xy, z[..., None]], dim=-1)
        P = ps[v]
        world = C._apply(P[:, :3, :3], P[:, :3, 3], cam)
        anchor = C._apply(inv0[:, :3, :3], inv0[:, :3, 3], world)
        valid = torch.rand(B, H, W, generator=g, dtype=F64) >= holes
        if v in empty:
            valid[:] = False

        def conf():
            u = torch.rand(B, H, W, generator=g, dtype=F64)
            return (1.0 + 4.0 * (u * u)).float()

        pred = {"pts3d_in_other_view": (1.7 * anchor + BIAS_GLOBAL * scale[..., None] + 0.05 * C._noise(g, B, H, W, 3)).float(), "conf": conf()}
        if local:
            pred["pts3d_local"] = (0.6 * cam + BIAS_LOCAL * scale[..., None] + 0.05 * C._noise(g, B, H, W, 3)).float()
            pred["conf_local"] = conf()
        gt = world.float()
        if gt_value is not None and gt_value[0] == v:
            _, b, i, j, c, value, ok = gt_value
            valid[b, i, j] = ok
            if value is not None:
                gt[b, i, j, c] = value
        if mask_bytes:
            pick = torch.randint(0, 4, (B, H, W), generator=g)
            valid = torch.where(valid, torch.tensor([1, 2, 128, 255], dtype=torch.uint8)[pick], torch.zeros((), dtype=torch.uint8))
        P = P + 1e-9 * C._noise(g, B, 4, 4) * (P != 0) if pose_fp64 else P.float()
        views.append({"pts3d": gt, "valid_mask": valid, "camera_pose": P})
        preds.append(pred)
    return views, preds


class Case:
    def __init__(self, name, views, preds, recipe, empty=()):
        self.name, self.views, self.preds, self.recipe, self.empty = name, views, preds, recipe, tuple(empty)
        self.V, self.B = len(views), views[0]["pts3d"].shape[0]
        self.local = "pts3d_local" in preds[0]
        self.npix = [v["pts3d"].shape[1] * v["pts3d"].shape[2] for v in views]

    def with_recipe(self, name, recipe):
        return Case(name, self.views, self.preds, recipe, self.empty)


A_RECIPES = {"v4": V4, "v3clip": V3_CLIP}
B_SHAPES = ((2, 5), (2, 65), (65, 2), (129, 1), (300, 1), (3, 100))   # (V, B)
B_RECIPES = {"v4": V4, "v4lsc": V4_LSC, "v3": V3}
C_NPIX = (1, 2, 3, 4, 5, 63, 64, 65, 1022, 1023, 1024, 1025, 2047, 2048, 2049, 3073)
E_KINDS = ("turns", "affine", "fp64")
EF_SHAPES, EF_B = [(12, 16)] * 3, 2
GT_PIXEL = (1, 1, 5, 7, 1)   # view, sample, i, j, coordinate of the NaN / inf ground truth
F_KINDS = {"base": (V4, (None, False)), "maskbytes": (V4, None), "nan-v4": (V4, (math.nan, True)), "nan-v3": (V3, (math.nan, True)),
           "nan-v4-clip": (dict(V4, dist_clip=3.1), (math.nan, True)), "nan-v3-clip": (dict(V3, dist_clip=3.1), (math.nan, True)),
           "inf-v4": (V4, (math.inf, True)), "inf-v3": (V3, (math.inf, True)), "nan-invalid": (V4, (math.nan, False))}

A_NAMES = [f"A-{g}-{r}" for g in A_GEOMS for r in A_RECIPES]
B_NAMES = [f"B-V{v}-B{b}-{r}" for v, b in B_SHAPES for r in B_RECIPES]
C_NAMES = [f"C-n{n}" for n in C_NPIX]
E_NAMES = [f"E-{k}" for k in E_KINDS]
F_NAMES = [f"F-{k}" for k in F_KINDS]
NAMES = A_NAMES + B_NAMES + C_NAMES + E_NAMES + F_NAMES
D_BASE = "D-n1025-B1"
D_OPERANDS = ("gt", "pred", "conf", "pred_local", "conf_local", "mask")
D_SHIFT = {"gt": 4, "pred": 4, "conf": 4, "pred_local": 4, "conf_local": 4, "mask": 1}   # bytes


@functools.lru_cache(maxsize=None)
def _a_data(geom, nb):
    geo = a_geometry(geom, nb)
    return build(geo["shapes"], geo["B"], 100 + A_GEOMS.index(geom), depth_scale=sample_scales(geo["B"]), empty=geo["empty"]), geo


@functools.lru_cache(maxsize=None)
def _b_data(V, B):
    return build([(3, 5)] * V, B, 200 + V + 1000 * B, depth_scale=sample_scales(B))


@functools.lru_cache(maxsize=None)
def _f_data(gt):
    value, ok = gt
    return build(EF_SHAPES, EF_B, 500, gt_value=GT_PIXEL + (value, ok))


@functools.lru_cache(maxsize=64)
def case(name, nb=1024):
    """the case `name`; nb matters to family A only"""
    fam, rest = name.split("-", 1)
    if fam == "A":
        geom, r = rest.rsplit("-", 1)
        (views, preds), geo = _a_data(geom, nb)
        return Case(name, views, preds, A_RECIPES[r], sorted(geo["empty"] + geo["zero"]))
    if fam == "B":
        v, b, r = rest.split("-")
        return Case(name, *_b_data(int(v[1:]), int(b[1:])), B_RECIPES[r])
    if fam == "C":
        n = int(rest[1:])
        return Case(name, *build([(1, n)] * 2, 3, 300 + n, depth_scale=sample_scales(3)), V4)
    if fam == "D":
        return Case(name, *build([(1, 1025)] * 2, 1, 300 + 1025), V4)
    if fam == "E":
        g_turns = [functools.partial(turned_poses, names=n, affine=(rest == "affine")) for n in E_TURNS]
        return Case(name, *build(EF_SHAPES, EF_B, 400 + E_KINDS.index(rest), poses=g_turns, pose_fp64=(rest == "fp64")), V4)
    assert fam == "F"
    recipe, gt = F_KINDS[rest]
    if rest == "maskbytes":
        return Case(name, *build(EF_SHAPES, EF_B, 500, mask_bytes=True), recipe)
    if gt is None:
        return Case(name, *build(EF_SHAPES, EF_B, 500), recipe)
    return Case(name, *_f_data(gt), recipe)


def reference(c, **kw):
    """loss_ref.multiview_conf_loss -> {"loss": ..., **details}"""
    loss, details = loss_ref.multiview_conf_loss(c.views, c.preds, **ref_kwargs(c.recipe), **kw)
    return {"loss": loss, **details}


def reversed_pixels(c):
    """the same case with the pixels of every view in reversed order"""
    flip = lambda d: {k: (t if k == "camera_pose" else t.flip(1, 2)) for k, t in d.items()}  # noqa: E731
    return Case(c.name, [flip(v) for v in c.views], [flip(p) for p in c.preds], c.recipe, c.empty)


def solved_inverses(c):
    """inverse poses by a solve against the identity, not torch.linalg.inv"""
    eye = torch.eye(4, dtype=F64)
    return [torch.linalg.solve(v["camera_pose"].float().to(F64), eye.expand(c.B, 4, 4)) for v in c.views]


# ================================================================================================ Gauss-Jordan, as the kernel's invert4
def gauss_jordan(m, pivoting=True):
    """the 4 x 4 inverse by Gauss-Jordan elimination in float64 -> (inverse as nested lists, the pivot row chosen at every column)"""
    a = [[float(m[i][j]) for j in range(4)] + [1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    rows = []
    for c in range(4):
        piv = c
        if pivoting:
            for r in range(c + 1, 4):
                if abs(a[r][c]) > abs(a[piv][c]):
                    piv = r
        rows.append(piv)
        a[c], a[piv] = a[piv], a[c]
        d = a[c][c]
        a[c] = [x / d if d != 0.0 else math.nan for x in a[c]]
        for r in range(4):
            if r != c:
                f = a[r][c]
                a[r] = [x - f * y for x, y in zip(a[r], a[c])]
    return [row[4:] for row in a], rows


# ================================================================================================ the pixel-flat restatement and its wrong variants
WRONG = ("first64", "group_mod4", "mask_eq1", "no_pivot", "v3_nanmean", "clip_keeps_nan", "merged_partials")


def restate(c, wrong=None, nb=1024):
    """The criterion in float64 over all pixels of all views at once, in the kernel's order of steps.  wrong: one of WRONG --
    first64: V4's global factors from the first 64 views only; group_mod4: factor group i takes group i % 4's; mask_eq1: valid = (mask == 1);
    no_pivot: inverse poses by elimination without row swaps; v3_nanmean: V3's factors skip NaN; clip_keeps_nan: under dist_clip a pixel is
    dropped when |g| > clip (NaN stays); merged_partials: a workgroup that meets several segments does not reset its sums between them"""
    assert wrong is None or wrong in WRONG
    r = ref_kwargs(c.recipe)
    V, B, S = c.V, c.B, c.V * c.B
    cat = lambda key, src, w: torch.cat([d[key].reshape(-1, *w) for d in src])  # noqa: E731
    X = cat("pts3d", c.views, (3,)).to(F64)
    M = cat("valid_mask", c.views, ()).to(torch.uint8)
    seg = torch.cat([torch.arange(v * B, (v + 1) * B).repeat_interleave(n) for v, n in enumerate(c.npix)])
    pose = torch.cat([v["camera_pose"].float().to(F64) for v in c.views])   # [S][4][4]
    if wrong == "no_pivot":
        inv = torch.tensor([gauss_jordan(m.tolist(), pivoting=False)[0] for m in pose], dtype=F64)
    else:
        inv = torch.linalg.inv(pose)
    valid0 = (M == 1) if wrong == "mask_eq1" else (M != 0)
    log1p = r["norm_mode"] == "avg_log1p"
    sets = [("global", "pts3d_in_other_view", "conf", seg % B)] + ([("local", "pts3d_local", "conf_local", seg)] if c.local else [])

    part = partition(c.npix, B, nb) if wrong == "merged_partials" else None

    def seg_sums(x):
        """[N][K] -> [S][K]"""
        if part is None:
            return torch.zeros(S, x.shape[1], dtype=F64).index_add_(0, seg, x)
        start = torch.tensor([0] + part.seg_npix[:-1]).cumsum(0)
        tile = torch.tensor(part.tile0)[seg] + (torch.arange(len(seg)) - start[seg]) // TILE
        k = torch.tensor(part.owner())[tile]
        row = {(kk, s): i for i, (kk, s, _) in enumerate(part.slots)}
        idx = torch.tensor([row[p] for p in zip(k.tolist(), seg.tolist())]) if len(seg) else torch.zeros(0, dtype=torch.long)
        P = torch.zeros(len(part.slots), x.shape[1], dtype=F64).index_add_(0, idx, x)
        out = torch.zeros(S, x.shape[1], dtype=F64)
        for i, (kk, s, _) in enumerate(part.slots):
            if i and part.slots[i - 1][0] == kk:
                P[i] += P[i - 1]          # the sums of the segment before were not reset
            out[s] += P[i]
        return out

    geo, mom = {}, {}
    for kind, pkey, ckey, which in sets:
        m = inv[which]
        g = (m[:, :3, :3] * X[:, None, :]).sum(-1) + m[:, :3, 3]
        d = g.norm(dim=-1)
        ok = valid0
        if r["dist_clip"] is not None:
            ok = ok & (~(d > r["dist_clip"]) if wrong == "clip_keeps_nan" else (d <= r["dist_clip"]))
        pr = cat(pkey, c.preds, (3,)).to(F64)
        fg, fp = (torch.log1p(d), torch.log1p(pr.norm(dim=-1))) if log1p else (d, pr.norm(dim=-1))
        ng, npd = ok & ~torch.isnan(fg), ok & ~torch.isnan(fp)
        zero = torch.zeros_like(fg)
        mom[kind] = seg_sums(torch.stack([ok.to(F64), ng.to(F64), torch.where(ng, fg, zero), npd.to(F64), torch.where(npd, fp, zero)], 1)).view(V, B, 5)
        geo[kind] = (g, ok, pr, cat(ckey, c.preds, ()).to(F64))

    def factor(cnt, nn, s):
        if r["version"] == 4 or wrong == "v3_nanmean":
            f = s / nn
        else:
            f = torch.where(nn != cnt, torch.full_like(s, math.nan), s / cnt)
        return torch.where(f < 1e-8, torch.full_like(f, 1e-8), f)

    def mod4(f, dim):
        if wrong != "group_mod4":
            return f
        return f.index_select(dim, torch.arange(f.shape[dim]) % 4)

    def factors(kind, who):
        """[V][B]"""
        mm = mom[kind]
        cnt, nn, s = (mm[..., 0], mm[..., 1], mm[..., 2]) if who == "gt" else (mm[..., 0], mm[..., 3], mm[..., 4])
        if who == "gt" and r["gt_scale"]:
            return torch.ones(V, B, dtype=F64)
        if r["version"] == 4:
            if kind == "local" and r["local_scale_consistent"]:
                return factors("global", who)
            if kind == "global":
                top = 64 if wrong == "first64" else V
                return mod4(factor(cnt[:top].sum(0), nn[:top].sum(0), s[:top].sum(0)), 0).expand(V, B)
            return factor(cnt, nn, s)
        if kind == "global":
            return factor(cnt.sum(), nn.sum(), s.sum()).expand(V, B)
        return mod4(factor(cnt.sum(1), nn.sum(1), s.sum(1)), 0)[:, None].expand(V, B)

    pts, conf, terms = {}, {}, []
    for kind, _, _, _ in sets:
        g, ok, pr, cf = geo[kind]
        n_gt, n_pr = factors(kind, "gt").reshape(-1)[seg], factors(kind, "pred").reshape(-1)[seg]
        L = (pr / n_pr[:, None] - g / n_gt[:, None]).norm(dim=-1)
        zero = torch.zeros_like(L)
        sums = seg_sums(torch.stack([torch.where(ok, L, zero), torch.where(ok, L * cf - r["alpha"] * torch.log(cf), zero)], 1)).view(V, B, 2).sum(1)
        cnt = mom[kind][..., 0].sum(1)
        for v in range(V):
            pts[f"Regr3DMultiviewV3_pts3d_loss_{kind}/{v:02d}"] = float(sums[v, 0] / cnt[v])
            term = float(sums[v, 1] / cnt[v]) if cnt[v] > 0 else 0.0
            conf[f"ConfLossMultiviewV2_conf_loss_{kind}/{v:02d}"] = term
            terms.append(term)
    return {"loss": sum(terms) / len(terms), **pts, **conf}


# ================================================================================================ guarded placement and the launch
OPERANDS = ("gt", "mask", "pose", "pred", "conf", "pred_local", "conf_local")   # the order of the C ABI's tables
GAP, MARGIN = 256, 4096


def _arena(tensors, shift, dev):
    """every view's tensor inside ONE buffer of 0xFF bytes (NaN as fp32 / fp64, true as a mask byte), 16-byte aligned plus `shift` bytes,
    GAP bytes or more apart and MARGIN from the ends -> (device buffer, its host copy, device pointers)"""
    offs, at = [], MARGIN
    for t in tensors:
        offs.append(at + shift)
        at = (at + shift + t.numel() * t.element_size() + GAP + 15) // 16 * 16
    host = torch.full((at + MARGIN,), 0xFF, dtype=torch.uint8)
    for t, o in zip(tensors, offs):
        raw = t.contiguous().reshape(-1).view(torch.uint8)
        host[o:o + raw.numel()] = raw
    buf = host.to(dev)
    assert buf.data_ptr() % 16 == 0
    return buf, host, [buf.data_ptr() + o for o in offs]


def out_names(V, local):
    names = ["loss"]
    for prefix, kind in (("Regr3DMultiviewV3_pts3d_loss", "global"), ("Regr3DMultiviewV3_pts3d_loss", "local"),
                         ("ConfLossMultiviewV2_conf_loss", "global"), ("ConfLossMultiviewV2_conf_loss", "local")):
        names += [f"{prefix}_{kind}/{v:02d}" if local or kind == "global" else None for v in range(V)]
    return names


def run_loss(lib, dev, c, shifts=None, runs=1):
    """f3r_mv_conf_loss on guarded buffers -> per run the 1 + 4 V fp64 outputs (CPU) and the same as {"loss": ..., **details}.
    shifts: operand name (D_OPERANDS) -> bytes by which every view's tensor of that operand is moved inside its arena.  The workspace is exactly
    f3r_mv_conf_loss_workspace_bytes long, lies between sentinel words and holds 0xFF bytes before every run."""
    from fast3r_amd import _lib
    shifts = shifts or {}
    assert set(shifts) <= set(D_OPERANDS)
    V, B = c.V, c.B
    b = Bufs(dev)
    src = {"gt": [v["pts3d"] for v in c.views], "mask": [v["valid_mask"].to(torch.uint8) for v in c.views],
           "pose": [v["camera_pose"] for v in c.views], "pred": [p["pts3d_in_other_view"] for p in c.preds], "conf": [p["conf"] for p in c.preds]}
    if c.local:
        src.update(pred_local=[p["pts3d_local"] for p in c.preds], conf_local=[p["conf_local"] for p in c.preds])
    pose_dtype = src["pose"][0].dtype
    assert all(t.dtype == (pose_dtype if k == "pose" else torch.uint8 if k == "mask" else torch.float32) for k, ts in src.items() for t in ts)
    arenas, tables = {}, {}
    for k, ts in src.items():
        arenas[k] = _arena(ts, shifts.get(k, 0), dev)
        tables[k] = b.op(torch.tensor(arenas[k][2], dtype=torch.int64))
    npix = b.op(torch.tensor(c.npix, dtype=torch.int64))
    ws_bytes = lib.f3r_mv_conf_loss_workspace_bytes(V, B)
    assert ws_bytes > 0 and ws_bytes % 8 == 0
    ws, out = b.out(ws_bytes // 4), b.out(2 * (1 + 4 * V))
    r = ref_kwargs(c.recipe)
    results = []
    for _ in range(runs):
        ws.view.view(torch.int32).fill_(-1)
        out.view.view(torch.int32).fill_(-1)
        _lib.check(lib.f3r_mv_conf_loss(_p(tables["gt"]), _p(tables["mask"]), _p(tables["pose"]),
                                        _lib.F3R_REAL_F64 if pose_dtype == F64 else _lib.F3R_REAL_F32, _p(tables["pred"]), _p(tables["conf"]),
                                        _p(tables.get("pred_local")), _p(tables.get("conf_local")), _p(npix), V, B, r["version"],
                                        _lib.F3R_LOSS_LOG1P if r["norm_mode"] == "avg_log1p" else _lib.F3R_LOSS_DIS, int(r["gt_scale"]),
                                        int(r.get("local_scale_consistent", False)), int(r["dist_clip"] is not None),
                                        float(r["dist_clip"] or 0.0), float(r["alpha"]), _p(ws), ws_bytes, _p(out), _stream()), "f3r_mv_conf_loss")
        b.intact(c.name)
        for k, (buf, host, _) in arenas.items():
            assert torch.equal(buf.cpu(), host), f"{c.name}: the arena of {k} was written to"
        raw = out.view.cpu().contiguous().view(-1).view(F64).clone()
        results.append((raw, {k: float(x) for k, x in zip(out_names(V, c.local), raw) if k is not None}))
    return results
