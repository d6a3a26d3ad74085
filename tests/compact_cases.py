"""Seeded cases of the tile-compaction kernels at the edges of their walk -- tile_count / tile_compact, compact_rank, last_le and
exclusive_scan_rows_kernel of csrc/f3r_prims.h, as f3r_scene_collect_count / _write (csrc/f3r_scene.hip), f3r_cloud_combine_count / _write and
f3r_cloud_voxel_sort / _sums (csrc/f3r_cloud.hip), f3r_mesh_count / _write (csrc/f3r_mesh.hip), f3r_depth_medians + f3r_depth_sparsify
(csrc/f3r_depth.hip), f3r_recon_prepare (csrc/f3r_recon.hip) and f3r_match_count / _write (csrc/f3r_match.hip) use them -- with a Python
restatement of the partition and the walk, the references (numpy boolean indexing, cloud_ref, mesh_ref, depth_ref, recon_ref's registration), and
the guarded placement of every device buffer; shared by tests/test_compact_cases.py (no GPU: the cases reach their edges, the restatement agrees
with a boolean index, wrong restatements are caught) and tests/test_compact_geometry_gpu.py (the kernels, through the C ABI).  One list of lengths
and one list of keep patterns serve all seven families (`lengths`, `PATTERNS`, `pairings`).

Placement (the contract of every `run_*` function, asserted before it hands a value back):
  1. operands that feed a keep predicate (conf, mask bytes, thresholds) sit in arenas of 0x7F bytes: 0x7F7F7F7F reads as 3.39e38 (finite fp32),
     +127 (int8) and nonzero (uint8), so an element read past the end is KEPT and changes a count.  0xFF would read as NaN / -1: never kept.
  2. data operands (points, colours, image planes, the row tables) sit in arenas of 0xFF bytes (NaN / 255).
  3. every output -- the scan of n_tiles + 1 words and the count word included -- has exactly the size the count states and lies between
     sentinels; the byte outputs (3 M bytes, no multiple of 4) between sentinel bytes.
  4. a workspace is exactly f3r_*_workspace_bytes long, 256-byte aligned, between sentinel bytes, and 0xFF-filled before every run.
  5. after a launch: synchronise, sentinels, arenas, then values.
  6. a case named *-twice runs again on re-poisoned outputs and workspace: the same bits.
  7. nothing kept: the write entry is still called, with the pointers of zero-width guarded outputs, and must write nothing.
"""
import ctypes
import dataclasses
import functools

import numpy as np
import torch

import cloud_ref
from conv_cases import guarded_operand
from gemm_cases import SENTINEL32, Guarded
from post_cases import Bufs

from fast3r_amd import _lib

F32 = np.float32
WAVE = 64
T_COLLECT, T_CLOUD = _lib.COLLECT_TILE, _lib.CLOUD_TILE
SCAN_NT = 1024                               # f3r_prims.h: threads of exclusive_scan_rows_kernel's one workgroup per row
PRED_FILL, DATA_FILL, SENTINEL_BYTE = 0x7F, 0xFF, 0xC3
PATTERNS = ("all", "none", "first", "last", "lane0", "lane63", "alternate", "half", "straddle", "hole")


def lengths(T):
    """T-64 / T-63 / T-1: the variable-trip branch of tile_compact with 15 whole steps, 15 steps and one element, 16 steps less one lane;
    T and 2T: the unrolled full-tile branch"""
    return (1, 63, 64, 65, T - 65, T - 64, T - 63, T - 1, T, T + 1, 2 * T, 2 * T + 17)


def pairings(T):
    """(length, pattern): `half` at every length, every pattern at T-1, T and 2T+17, `last` and `lane63` at every length"""
    out = []
    for n in lengths(T):
        pats = PATTERNS if n in (T - 1, T, 2 * T + 17) else ("half", "last", "lane63")
        out += [(n, p) for p in pats]
    return out


def _rs(*key):
    s = 97531
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return np.random.RandomState(s)


def pattern(name, n, T, seed=0):
    """the keep flags of n elements"""
    i = np.arange(n)
    if name == "all":
        return np.ones(n, bool)
    if name == "none":
        return np.zeros(n, bool)
    if name == "first":
        return i == 0
    if name == "last":
        return i == n - 1
    if name == "lane0":                        # tiles start at multiples of T, a multiple of 64: the lane of element i is i % 64
        return i % WAVE == 0
    if name == "lane63":
        return i % WAVE == WAVE - 1
    if name == "alternate":
        return i % 2 == 1
    if name == "half":
        return _rs(1, n, T, seed).rand(n) < 0.5
    if name == "straddle":                     # 130 keepers centred on every multiple of T in [0, n]
        k = np.zeros(n, bool)
        for b in range(0, n + 1, T):
            k[max(b - 65, 0):min(b + 65, n)] = True
        return k
    if name == "hole":                         # tile 1 empty between full ones: the scan carries a zero
        return (i < T) | (i >= 2 * T)
    raise ValueError(name)


# ================================================================================================ the walk, restated
WRONG = ("stop", "rank_own", "inclusive_scan", "last_not_zeroed", "stream1_advances_0", "seg_lt", "passenger")
POISON32 = 0xFFFFFFFF


def tile_starts(lens, T):
    return np.concatenate([[0], np.cumsum([(n + T - 1) // T for n in lens])]).astype(np.int64)


def last_le(start, lo, hi, x, strict=False):
    """f3r_prims.h last_le; strict: `<` for `<=` (what it must NOT do)"""
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if (start[mid] < x) if strict else (start[mid] <= x):
            lo = mid
        else:
            hi = mid
    return lo


def walk(flags, T, K=1, wrong=None, over=None, zeroed_last=True):
    """Count kernel, scan, tile_compact on a table of segments.  flags[s] = the mask of every element of segment s (bit k: kept in stream k; bits K
    and up: the caller's passengers).  An element past a segment's end reads `over` (default: every stream bit -- the 0x7F arena).
    zeroed_last: the scan runs over n_tiles + 1 words of which the count kernel zeroes the last (cloud, voxel, mesh); else over n_tiles words with
    the total stored behind them (scene).  -> (scan uint32 [n_tiles + 1], out[k] = the (segment, element) stored at each slot, or -1, with
    `margin` spare slots behind the total; stray = stores outside even those)"""
    lens = [len(f) for f in flags]
    ts = tile_starts(lens, T)
    S, n_tiles = len(flags), int(ts[-1])
    over = (1 << K) - 1 if over is None else over
    lanes = np.arange(WAVE)

    def tile(t):
        seg = last_le(ts, 0, S, t, strict=wrong == "seg_lt")
        base, end = (t - int(ts[seg])) * T, lens[seg]
        return seg, base, (base + T if wrong == "stop" else min(base + T, end))

    def read(seg, i):
        f = flags[seg]
        ok = i < len(f)
        return np.where(ok, f[np.minimum(i, len(f) - 1)], over).astype(np.int64)

    cnt = np.zeros((n_tiles + 1, K), np.int64)
    for t in range(n_tiles):
        seg, base, stop = tile(t)
        if stop > base:
            m = read(seg, np.arange(base, stop))
            for k in range(K):
                cnt[t, k] = int(((m >> k) & 1).sum())
    if wrong == "last_not_zeroed":
        cnt[n_tiles] = POISON32
    words = n_tiles + 1 if zeroed_last else n_tiles
    inc = np.cumsum(cnt[:words], axis=0) % 2 ** 32
    scan = np.zeros((n_tiles + 1, K), np.int64)
    scan[:words] = inc if wrong == "inclusive_scan" else (inc - cnt[:words]) % 2 ** 32
    if not zeroed_last:
        scan[n_tiles] = inc[-1]
    total = [int(scan[n_tiles, k]) for k in range(K)]
    margin = 4 * T
    true_total = [int(sum(int(((np.asarray(f) >> k) & 1).sum()) for f in flags)) for k in range(K)]
    out = [np.full((true_total[k] + margin, 2), -1, np.int64) for k in range(K)]
    stray = 0
    for t in range(n_tiles):
        seg, base, stop = tile(t)
        run = [int(scan[t, k]) for k in range(K)]
        for c in range(base, stop, WAVE):
            i = c + lanes
            m = np.where(i < stop, read(seg, i), 0)
            slots = []
            for k in range(K):
                bit = (m >> k) & 1
                below = np.cumsum(bit) - (0 if wrong == "rank_own" else bit)
                slots.append(run[k] + below)
                run[0 if wrong == "stream1_advances_0" else k] += int(bit.sum())
            emit = (m != 0) if wrong == "passenger" else ((m & ((1 << K) - 1)) != 0)
            for k in range(K):
                # emit stores stream k's record where bit k is set; the passenger variant also stores stream 0's record for a passenger-only lane
                sel = emit & ((((m >> k) & 1) == 1) | ((m >> K != 0) if (wrong == "passenger" and k == 0) else False))
                for lane in np.flatnonzero(sel):
                    s = int(slots[k][lane])
                    if 0 <= s < len(out[k]):
                        out[k][s] = (seg, int(i[lane]))
                    else:
                        stray += 1
    return scan.astype(np.uint32), out, stray, total


def walk_ref(flags, K=1):
    """a plain boolean index: per stream the (segment, element) pairs kept, in table order"""
    out = []
    for k in range(K):
        rows = [np.stack([np.full(int(sel.sum()), s), np.flatnonzero(sel)], 1) for s, f in enumerate(flags) for sel in [((np.asarray(f) >> k) & 1) == 1]]
        out.append(np.concatenate(rows).astype(np.int64) if rows else np.zeros((0, 2), np.int64))
    return out


def walk_agrees(flags, T, K=1, wrong=None, **kw):
    """the restated walk stores exactly the boolean index, states its length as the total, and nothing else"""
    scan, out, stray, total = walk(flags, T, K, wrong, **kw)
    ref = walk_ref(flags, K)
    for k in range(K):
        if total[k] != len(ref[k]) or stray or not np.array_equal(out[k][:len(ref[k])], ref[k]) or (out[k][len(ref[k]):] != -1).any():
            return False
    return True


def scan_words_per_thread(words):
    """exclusive_scan_rows_kernel: per = ceil(len / NT)"""
    return (words + SCAN_NT - 1) // SCAN_NT


# ================================================================================================ table cases shared by the families
def ragged_lens(T):
    """one segment ends inside a step, one exactly on a tile, one owns a single-element tile"""
    return (65, T, 1)


def scan_lens(n_tiles, T, parts=5):
    """`parts` segments with n_tiles tiles in all; their last tiles end 0, 1, 63, 64 and 65 elements short"""
    tiles = [n_tiles // parts + (1 if p < n_tiles % parts else 0) for p in range(parts)]
    short = (0, 1, 63, 64, 65)
    return tuple(t * T - short[p % 5] for p, t in enumerate(tiles))


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    lens: tuple            # elements per segment
    pat: str = "half"
    extra: str = ""

    @property
    def twice(self):
        return self.name.endswith("-twice")


def table_cases(T, multi=("three-ragged",)):
    out = [Case(f"{p}@{n}" + ("-twice" if (n, p) == (2 * T + 17, "half") else ""), (n,), p) for n, p in pairings(T)]
    if "three-ragged" in multi:
        out.append(Case("three-ragged-twice", ragged_lens(T), "half"))
    if "scan" in multi:
        out += [Case("scan-1025", scan_lens(1025, T), "lane63"), Case("scan-2049", scan_lens(2049, T), "lane63")]
    return out


def case_flags(c, T):
    return [pattern(c.pat, n, T, seed=s) for s, n in enumerate(c.lens)]


# ================================================================================================ scene collect
SCENE_EXTRA = ("num-short", "null-mask", "const-colour", "null-mask-const-colour")
SCENE = table_cases(T_COLLECT, multi=("three-ragged", "scan")) + [Case(f"{e}@{n}", (n,), "half", e) for e in SCENE_EXTRA for n in (T_COLLECT - 1, 2 * T_COLLECT + 17)]
SCENE_SHORT_TAIL = 300                       # entries behind `num` in the num-short cases, all of them "keep"
CONST_COLOUR = 0x0A8040                      # r = 0x40, g = 0x80, b = 0x0A


def by_name(cases, name):
    return next(c for c in cases if c.name == name)


@functools.lru_cache(maxsize=None)
def scene_data(name):
    """per segment: pts [L][3] fp32, col [L][3] u8 | None, mask [L] int8 | None, num <= L"""
    c = by_name(SCENE, name)
    segs = []
    for s, (n, keep) in enumerate(zip(c.lens, case_flags(c, T_COLLECT))):
        rs = _rs(2, n, s, len(c.name))
        L = n + (SCENE_SHORT_TAIL if c.extra == "num-short" else 0)
        mask = np.where(keep, rs.randint(1, 128, n), rs.choice([0, -1, -128], n)).astype(np.int8)   # kept: > 0
        mask = np.concatenate([mask, np.full(L - n, 1, np.int8)])
        segs.append(dict(pts=rs.randn(L, 3).astype(F32), col=None if "const-colour" in c.extra else rs.randint(0, 256, (L, 3)).astype(np.uint8),
                         mask=None if "null-mask" in c.extra else mask, num=n, const=CONST_COLOUR + s))
    return segs


def scene_flags(segs):
    return [np.ones(d["num"], np.int64) if d["mask"] is None else (d["mask"][:d["num"]] > 0).astype(np.int64) for d in segs]


def tile_scan(flags, T):
    """exclusive scan of the kept elements per tile, the total in the last word"""
    cnt = [int(f[b:b + T].sum()) for f in flags for b in range(0, len(f), T)]
    return np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def scene_ref(name):
    """numpy boolean index -> (scan [n_tiles + 1] uint32, pts [M][3] fp32, rgb [M][3] u8)"""
    segs = scene_data(name)
    flags = scene_flags(segs)
    pts, rgb = [], []
    for d, f in zip(segs, flags):
        k = f.astype(bool)
        pts.append(d["pts"][:d["num"]][k])
        const = np.array([(d["const"] >> (8 * ch)) & 255 for ch in range(3)], np.uint8)
        rgb.append(d["col"][:d["num"]][k] if d["col"] is not None else np.broadcast_to(const, (int(k.sum()), 3)))
    return tile_scan(flags, T_COLLECT), np.concatenate(pts), np.concatenate(rgb).astype(np.uint8)


# ================================================================================================ cloud combine
CLOUD_EXTRA = ("mask-carrier", "both", "nan-conf", "u8-img", "flip", "null-thresholds")
CLOUD = (table_cases(T_CLOUD) + [Case(f"mask-carrier-{p}@{n}", (n,), p, "mask-carrier") for n in (T_CLOUD - 1, 2 * T_CLOUD + 17) for p in PATTERNS]
         + [Case(f"{e}@{n}", (n,), "half", e) for e in CLOUD_EXTRA[1:] for n in (T_CLOUD - 1, 2 * T_CLOUD + 17)]
         + [Case("three-ragged-u8-flip", ragged_lens(T_CLOUD), "half", "u8-img flip")])


@functools.lru_cache(maxsize=None)
def cloud_data(name):
    """per view: conf [n] fp32 | None, pts [n][3], img (fp32 planes [3][n] in [-1.2, 1.2] with a NaN, or u8 [n][3]), mask [n] u8 | None, thr.
    A pixel that the confidence drops holds EXACTLY the threshold (every other one), a smaller value, or in nan-conf a NaN: `>=` keeps too many"""
    c = by_name(CLOUD, name)
    views = []
    for s, (n, keep) in enumerate(zip(c.lens, case_flags(c, T_CLOUD))):
        rs = _rs(3, n, s, len(c.name))
        thr = F32(1.5 + s)
        by_conf, by_mask = keep, np.ones(n, bool)
        if "mask-carrier" in c.extra or "null-thresholds" in c.extra:
            by_conf, by_mask = np.ones(n, bool), keep
        if "both" in c.extra:                   # the pattern is the AND of two halves
            by_conf, by_mask = pattern("half", n, T_CLOUD, seed=11), pattern("half", n, T_CLOUD, seed=12)
        low = np.where(np.arange(n) % 2 == 0, thr, thr - F32(0.25) * rs.rand(n).astype(F32) - F32(0.01)).astype(F32)
        if "nan-conf" in c.extra:
            low[np.arange(n) % 3 == 0] = np.nan
        conf = np.where(by_conf, thr + F32(0.01) + rs.rand(n).astype(F32), low).astype(F32)
        if "null-thresholds" in c.extra:       # a confidence that would drop everything, were it tested
            conf = np.full(n, thr - 1, F32)
        mask = np.where(by_mask, rs.randint(1, 256, n), 0).astype(np.uint8)
        img = rs.randint(0, 256, (n, 3)).astype(np.uint8) if "u8-img" in c.extra else (rs.rand(3, n) * 2.4 - 1.2).astype(F32)
        if img.dtype == F32 and n > 2:
            img[1, n // 2] = np.nan
        views.append(dict(conf=None if "mask-carrier" in c.extra else conf, pts=rs.randn(n, 3).astype(F32), img=img,
                          mask=mask if ("mask-carrier" in c.extra or "both" in c.extra or "null-thresholds" in c.extra) else None, thr=float(thr), n=n))
    return dict(views=views, flip="flip" in c.extra, thresholds="null-thresholds" not in c.extra)


def cloud_flags(d):
    out = []
    for v in d["views"]:
        k = np.ones(v["n"], bool)
        if d["thresholds"] and v["conf"] is not None:
            with np.errstate(invalid="ignore"):
                k &= v["conf"] > F32(v["thr"])
        if v["mask"] is not None:
            k &= v["mask"] != 0
        out.append(k.astype(np.int64))
    return out


@functools.lru_cache(maxsize=None)
def cloud_ref_of(name):
    """cloud_ref.combine's pieces on the explicit thresholds -> (scan, points [M][3], colors [M][3])"""
    d = cloud_data(name)
    flags = cloud_flags(d)
    pts, col = [], []
    for v, f in zip(d["views"], flags):
        k = f.astype(bool)
        p = v["pts"][k].copy()
        if d["flip"]:
            p = p[:, [0, 2, 1]]
            p[:, 2] = -p[:, 2]
        pts.append(p)
        col.append(v["img"][k] if v["img"].dtype == np.uint8 else cloud_ref.color_u8(v["img"].T[k]))
    return tile_scan(flags, T_CLOUD), np.concatenate(pts).astype(F32), np.concatenate(col).astype(np.uint8)


# ================================================================================================ voxel heads
VOXEL = ([Case(f"{p}@{n}" + ("-twice" if (n, p) == (2 * T_CLOUD + 17, "half") else ""), (n,), p) for n, p in pairings(T_CLOUD)]
         + [Case("head-at-T", (2 * T_CLOUD,), "runs", "500 524 300 724"), Case("run-across-T", (2 * T_CLOUD,), "runs", "500 600 300 648"),
            Case("no-colours@2065", (2 * T_CLOUD + 17,), "half", "no-colours")])


def voxel_heads(c):
    """is_head of every sorted position: the pattern with position 0 a head (it always is), or the starts of the listed runs"""
    n = c.lens[0]
    if c.pat == "runs":
        runs = [int(x) for x in c.extra.split()]
        assert sum(runs) == n
        h = np.zeros(n, bool)
        h[np.cumsum([0] + runs[:-1])] = True
        return h
    h = pattern(c.pat, n, T_CLOUD).copy()
    h[0] = True
    return h


@functools.lru_cache(maxsize=None)
def voxel_data(name):
    """points whose voxel (size 1) is (id, 0, 0), id = the heads before the sorted position, shuffled; colours u8 | None"""
    c = by_name(VOXEL, name)
    n = c.lens[0]
    rs = _rs(4, n, len(c.name), PATTERNS.index(c.pat) if c.pat in PATTERNS else 99)
    vid = np.cumsum(voxel_heads(c)) - 1
    p = np.stack([vid + 0.4 * rs.rand(n), 0.4 * rs.rand(n), 0.4 * rs.rand(n)], 1).astype(F32)
    p[0] = (0.0, 0.0, 0.0)                       # pins the minimum: index = floor(coordinate + 0.5)
    perm = rs.permutation(n)
    col = None if c.extra == "no-colours" else rs.randint(0, 256, (n, 3)).astype(np.uint8)
    return p[perm], col, 1.0


def voxel_sorted_keys(name):
    """the x index of every sorted position, from cloud_ref's index arithmetic alone"""
    p, _, vs = voxel_data(name)
    idx = cloud_ref.voxel_indices(p, vs)
    assert not idx[:, 1:].any()
    return np.sort(idx[:, 0], kind="stable")


def head_flags(keys, i0_clause=True, before=None):
    """is_head of f3r_cloud.hip over sorted keys: i == 0 or keys[i] != keys[i - 1].  i0_clause=False is what it must NOT do: position 0 then
    compares with `before`, whatever lies in front of the keys (a voxel is lost when that happens to equal keys[0])"""
    keys = np.asarray(keys)
    prev = np.concatenate([[keys[0] if before is None else before], keys[:-1]])
    h = keys != prev
    if i0_clause:
        h[0] = True
    return h


@functools.lru_cache(maxsize=None)
def voxel_ref(name):
    p, col, vs = voxel_data(name)
    return cloud_ref.voxel_down_sample(p, col, vs)


# ================================================================================================ guarded placement and the launches
def _arena(t, dev, fill, margin):
    """conv_cases.guarded_operand with a fill of the caller's"""
    nb = t.numel() * t.element_size()
    off = (margin + 15) // 16 * 16 + 16
    buf = torch.full((off + nb + off,), fill, dtype=torch.uint8, device=dev)
    view = buf[off:off + nb].view(t.dtype).view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    return view, buf


@dataclasses.dataclass
class ByteRegion:
    """nbytes at a 256-byte aligned address between sentinel bytes"""
    buf: torch.Tensor
    lead: int
    nbytes: int

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.lead

    @property
    def view(self):
        return self.buf[self.lead:self.lead + self.nbytes]

    def fill(self, byte):
        self.view.fill_(byte)

    def intact(self):
        return bool((self.buf[:self.lead] == SENTINEL_BYTE).all()) and bool((self.buf[self.lead + self.nbytes:] == SENTINEL_BYTE).all())


def byte_region(nbytes, dev, fill=SENTINEL_BYTE):
    """the byte-sentinel helper: out_rgb / colors of 3 M bytes, and the workspaces"""
    margin = max(4096, (nbytes + 255) // 256 * 256)
    buf = torch.full((margin + nbytes + margin + 256,), SENTINEL_BYTE, dtype=torch.uint8, device=dev)
    lead = margin + (-(buf.data_ptr() + margin)) % 256
    r = ByteRegion(buf, lead, nbytes)
    assert r.ptr % 256 == 0 and lead + nbytes + margin <= buf.numel()
    r.fill(fill)
    return r


class Placed(Bufs):
    """post_cases.Bufs with the predicate arenas, the byte outputs, the workspaces and the arena check of this family"""

    def __init__(self, dev):
        super().__init__(dev)
        self.arenas, self.regions = [], []

    def _keep(self, view, buf):
        self.arenas.append((buf, buf.clone()))
        return view

    def data(self, a):
        """a data operand inside 0xFF bytes"""
        if a is None:
            return None
        view, buf = guarded_operand(torch.from_numpy(np.ascontiguousarray(a)), self.dev, 4096)
        return self._keep(view, buf)

    def pred(self, a):
        """an operand that feeds a keep predicate inside 0x7F bytes"""
        if a is None:
            return None
        return self._keep(*_arena(torch.from_numpy(np.ascontiguousarray(a)), self.dev, PRED_FILL, 4096))

    def out(self, n, dtype=torch.float32, want=True):
        """Bufs.out; zero words wide: 4096 sentinel words and no output between them"""
        if n > 0 or not want:
            return super().out(n, dtype, want)
        lead = 2048
        buf = torch.full((2 * lead,), SENTINEL32, dtype=torch.int32, device=self.dev)
        g = Guarded(buf[lead:lead].view(dtype).view(1, 0), buf, lead, 1, 0, 0)
        self.outs.append(g)
        return g

    def bytes_out(self, n):
        r = byte_region(n, self.dev)
        self.regions.append(r)
        return r

    def workspace(self, nbytes):
        r = byte_region(nbytes, self.dev, fill=0xFF)
        self.regions.append(r)
        return r

    def check(self, what):
        self.intact(what)
        for r in self.regions:
            assert r.intact(), f"{what}: a store outside a byte region of {r.nbytes} bytes"
        for buf, snap in self.arenas:
            assert torch.equal(buf, snap), f"{what}: an operand arena was written to"


def out_ptr(g):
    """the address of a guarded 32-bit output, also when it is zero words wide (an empty view has no data_ptr)"""
    return g.buf.data_ptr() + g.lead * g.buf.element_size()


def out_np(g, dtype):
    return g.view.reshape(-1).cpu().numpy().view(dtype)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _table(rows, starts):
    return np.concatenate([np.asarray(rows, np.int64).reshape(-1), np.asarray(starts, np.int64)])


def run_scene(lib, dev, name, runs=1):
    """f3r_scene_collect_count / _write on guarded buffers -> per run (scan [n_tiles + 1] uint32, pts [M][3] fp32, rgb [M][3] u8)"""
    segs = scene_data(name)
    ts = tile_starts([d["num"] for d in segs], T_COLLECT)
    S, n_tiles = len(segs), int(ts[-1])
    b = Placed(dev)
    rows = []
    for d in segs:
        pts, col, mask = b.data(d["pts"]), b.data(d["col"]), b.pred(d["mask"])
        rows.append([pts.data_ptr(), 0 if col is None else col.data_ptr(), 0 if mask is None else mask.data_ptr(), d["num"], d["const"]])
    table = b.data(_table(rows, ts))
    got = []
    for r in range(runs):
        what = f"scene collect {name} run {r}"
        scan = b.out(n_tiles + 1, torch.int32)
        _lib.check(lib.f3r_scene_collect_count(table.data_ptr(), S, n_tiles, out_ptr(scan), _stream()), "f3r_scene_collect_count")
        b.check(what + " count")
        sc = out_np(scan, np.uint32)
        M = int(sc[n_tiles])
        assert M <= sum(d["num"] for d in segs), f"{what}: the total {M} exceeds the entries"
        pts, rgb = b.out(3 * M), b.bytes_out(3 * M)
        _lib.check(lib.f3r_scene_collect_write(table.data_ptr(), S, n_tiles, out_ptr(scan), out_ptr(pts), rgb.ptr, _stream()), "f3r_scene_collect_write")
        b.check(what + " write")
        got.append((sc, out_np(pts, F32).reshape(M, 3), rgb.view.cpu().numpy().reshape(M, 3)))
    return got


def run_cloud(lib, dev, name, runs=1):
    """f3r_cloud_combine_count / _write with explicit thresholds on guarded buffers -> per run (scan, points [M][3], colors [M][3])"""
    d = cloud_data(name)
    views = d["views"]
    ts = tile_starts([v["n"] for v in views], T_CLOUD)
    V, n_tiles = len(views), int(ts[-1])
    b = Placed(dev)
    rows, vbase = [], 0
    for v in views:
        conf, pts, img, mask = b.pred(v["conf"]), b.data(v["pts"]), b.data(v["img"]), b.pred(v["mask"])
        rows.append([0 if conf is None else conf.data_ptr(), pts.data_ptr(), img.data_ptr(), 0 if mask is None else mask.data_ptr(), 1, v["n"], vbase,
                     int(v["img"].dtype == np.uint8), 0, 0, 0, 0])
        vbase += v["n"]
    table = b.data(_table(rows, ts))
    thr = b.pred(np.array([v["thr"] for v in views], F32)) if d["thresholds"] else None
    thr_ptr = None if thr is None else thr.data_ptr()
    got = []
    for r in range(runs):
        what = f"cloud combine {name} run {r}"
        scan = b.out(n_tiles + 1, torch.int32)
        _lib.check(_lib.entry("f3r_cloud_combine_count")(table.data_ptr(), V, n_tiles, thr_ptr, out_ptr(scan), _stream()), "f3r_cloud_combine_count")
        b.check(what + " count")
        sc = out_np(scan, np.uint32)
        M = int(sc[n_tiles])
        assert M <= vbase, f"{what}: the total {M} exceeds the pixels"
        pts, col = b.out(3 * M), b.bytes_out(3 * M)
        _lib.check(_lib.entry("f3r_cloud_combine_write")(table.data_ptr(), V, n_tiles, thr_ptr, out_ptr(scan), int(d["flip"]), out_ptr(pts), col.ptr, _stream()),
                   "f3r_cloud_combine_write")
        b.check(what + " write")
        got.append((sc, out_np(pts, F32).reshape(M, 3), col.view.cpu().numpy().reshape(M, 3)))
    return got


def run_voxel(lib, dev, name, runs=1):
    """f3r_cloud_voxel_sort, then f3r_cloud_voxel_sums, on guarded buffers and a workspace of exactly f3r_cloud_voxel_workspace_bytes, 0xFF-filled
    before every run -> per run (n_voxels, points [m][3] fp32, colors [m][3] u8 | None, counts [m] int32)"""
    p, col, vs = voxel_data(name)
    n = len(p)
    b = Placed(dev)
    pts, colors = b.data(p), b.data(col)
    lo = p.astype(np.float64).min(axis=0)
    min_bound = (ctypes.c_double * 3)(*lo)
    bits = (ctypes.c_int * 3)(*cloud_ref.key_bits(p, vs))
    ws_bytes = _lib.entry("f3r_cloud_voxel_workspace_bytes")(n)
    assert ws_bytes > 0
    ws = b.workspace(ws_bytes)
    got = []
    for r in range(runs):
        what = f"voxel {name} run {r}"
        ws.fill(0xFF)
        nv = b.out(1, torch.int32)
        _lib.check(_lib.entry("f3r_cloud_voxel_sort")(pts.data_ptr(), n, min_bound, float(vs), bits, ws.ptr, ws_bytes, out_ptr(nv), _stream()), "f3r_cloud_voxel_sort")
        b.check(what + " sort")
        m = int(out_np(nv, np.uint32)[0])
        assert 1 <= m <= n, f"{what}: {m} voxels of {n} points"
        out_p, out_c, counts = b.out(3 * m), b.bytes_out(3 * m if col is not None else 0), b.out(m, torch.int32)
        _lib.check(_lib.entry("f3r_cloud_voxel_sums")(pts.data_ptr(), None if col is None else colors.data_ptr(), n, m, ws.ptr, ws_bytes, out_ptr(out_p),
                                                      None if col is None else out_c.ptr, out_ptr(counts), _stream()), "f3r_cloud_voxel_sums")
        b.check(what + " sums")
        got.append((m, out_np(out_p, F32).reshape(m, 3), None if col is None else out_c.view.cpu().numpy().reshape(m, 3), out_np(counts, np.int32)))
    return got


# ================================================================================================ mesh
T_MESH = _lib.MESH_TILE
MESH_SHAPES = {1: (1, 1), 63: (7, 9), 64: (8, 8), 65: (5, 13), 959: (7, 137), 960: (30, 32), 961: (31, 31), 1023: (31, 33), 1024: (32, 32), 1025: (25, 41),
               2048: (32, 64), 2065: (35, 59)}                 # H W in lengths(T); (H - 1)(W - 1) = 960 = T - 64 and 961 = T - 63 among them
MESH_CFG = ((0, 1, 0, 0), (1, 1, 1, 0), (0, 0, 1, 1), (1, 0, 0, 1))   # drop_unreferenced, double_sided, int64 indices, flip_axes
QUAD_PATTERNS = ("all", "none", "first", "last", "lane0", "lane63", "straddle", "hole")   # keepers in runs or at least two quads apart


@dataclasses.dataclass(frozen=True)
class MeshCase:
    name: str
    views: tuple           # (H, W, pattern, "pixels" | "quads")
    cfg: tuple = MESH_CFG[0]
    carrier: str = "conf"

    @property
    def twice(self):
        return self.name.endswith("-twice")


def _mesh_cases():
    assert sorted(MESH_SHAPES) == sorted(lengths(T_MESH)) and all(h * w == n for n, (h, w) in MESH_SHAPES.items())
    out = []
    for k, (n, p) in enumerate(pairings(T_MESH)):              # the pattern over the PIXELS: the validity, used and vertex kernels
        out.append(MeshCase(f"pixels-{p}@{n}" + ("-twice" if (n, p) == (2 * T_MESH + 17, "half") else ""), (MESH_SHAPES[n] + (p, "pixels"),), MESH_CFG[k % 4],
                            ("conf", "mask")[k // 4 % 2]))
    k = 0
    for q in lengths(T_MESH):                                  # the pattern over the QUADS of a view two pixels wide: the count and face kernels
        for p in (QUAD_PATTERNS if q in (T_MESH - 1, T_MESH, 2 * T_MESH + 17) else ("all", "last", "lane63")):
            out.append(MeshCase(f"quads-{p}@{q}", ((q + 1, 2, p, "quads"),), MESH_CFG[k % 4], ("mask", "conf")[k // 4 % 2]))
            k += 1
    out += [MeshCase("three-ragged-twice", tuple(MESH_SHAPES[n] + ("half", "pixels") for n in ragged_lens(T_MESH)), MESH_CFG[1]),
            MeshCase("three-ragged-quads", tuple((q + 1, 2, "all", "quads") for q in ragged_lens(T_MESH)), MESH_CFG[3], "mask"),
            MeshCase("row-and-column", ((1, T_MESH + 1, "all", "pixels"), (T_MESH + 1, 1, "half", "pixels"), (8, 8, "all", "pixels")), MESH_CFG[1]),
            MeshCase("row-and-column-keep-all", ((T_MESH + 1, 1, "all", "pixels"), (1, 65, "half", "pixels"), (8, 8, "half", "pixels")), MESH_CFG[2], "mask")]
    return out


MESH = _mesh_cases()


def quad_validity(H, keep):
    """the pixel validity [H][2] that keeps exactly the quads of `keep` (length H - 1): a keeper next to a keeper keeps both triangles; a lone one
    keeps only A, only B or both, in turn"""
    v = np.zeros((H, 2), bool)
    lone = 0
    for y in np.flatnonzero(keep):
        run = (y > 0 and keep[y - 1]) or (y + 1 < len(keep) and keep[y + 1])
        kind = 2 if run else lone % 3
        lone += 0 if run else 1
        if kind == 0:
            v[y, 0] = v[y, 1] = v[y + 1, 0] = True
        elif kind == 1:
            v[y, 1] = v[y + 1, 0] = v[y + 1, 1] = True
        else:
            v[y] = v[y + 1] = True
    return v


def quad_flags(valid):
    """bit 0: triangle A (i, i+1, i+W) kept, bit 1: triangle B (i+1, i+W, i+W+1), per quad in row-major order"""
    v = np.asarray(valid, bool)
    if v.shape[0] < 2 or v.shape[1] < 2:
        return np.zeros(0, np.int64)
    a = v[:-1, :-1] & v[:-1, 1:] & v[1:, :-1]
    b = v[:-1, 1:] & v[1:, :-1] & v[1:, 1:]
    return (a.astype(np.int64) | (b.astype(np.int64) << 1)).reshape(-1)


def mesh_valid(c):
    out = []
    for s, (H, W, pat, kind) in enumerate(c.views):
        if kind == "quads":
            assert W == 2 and pat in QUAD_PATTERNS
            out.append(quad_validity(H, pattern(pat, H - 1, T_MESH)))
        else:
            out.append(pattern(pat, H * W, T_MESH, seed=s).reshape(H, W))
    return out


@functools.lru_cache(maxsize=None)
def mesh_data(name):
    """per view: H, W, valid [H][W], conf [n] | None, mask [n] | None, thr, pts [n][3], img fp32 planes [3][n]"""
    c = by_name(MESH, name)
    views = []
    for s, ((H, W, _, _), valid) in enumerate(zip(c.views, mesh_valid(c))):
        n = H * W
        rs = _rs(5, n, s, len(c.name))
        k = valid.reshape(-1)
        thr = F32(2.0 + s)
        low = np.where(np.arange(n) % 2 == 0, thr, thr - F32(0.5) * rs.rand(n).astype(F32) - F32(0.01)).astype(F32)
        conf = np.where(k, thr + F32(0.01) + rs.rand(n).astype(F32), low).astype(F32)
        mask = np.where(k, rs.randint(1, 256, n), 0).astype(np.uint8)
        views.append(dict(H=H, W=W, valid=valid, conf=conf if c.carrier == "conf" else None, mask=mask if c.carrier == "mask" else None, thr=float(thr),
                          pts=rs.randn(n, 3).astype(F32), img=(rs.rand(3, n) * 2.2 - 1.1).astype(F32)))
    return views


@functools.lru_cache(maxsize=None)
def mesh_ref_of(name):
    """mesh_ref.build on the validity as a mask -> (counts [V][3] uint32 = kept A, kept B, vertices written; vertices; faces int64; face_colors)"""
    import mesh_ref
    c = by_name(MESH, name)
    drop, ds, _, flip = c.cfg
    views = mesh_data(name)
    m = mesh_ref.build([(v["img"].reshape(3, v["H"], v["W"]), v["pts"].reshape(v["H"], v["W"], 3), None) for v in views], None, masks=[v["valid"] for v in views],
                       double_sided=bool(ds), drop_unreferenced=bool(drop), flip_axes=bool(flip))
    counts = np.array([[int((quad_flags(v["valid"]) & 1).sum()), int((quad_flags(v["valid"]) >> 1).sum()), nv] for v, nv in zip(views, m["vertices_per_view"])], np.uint32)
    assert (m["faces_per_view"] == (2 if ds else 1) * (counts[:, 0].astype(np.int64) + counts[:, 1])).all()
    return counts, m["vertices"], m["faces"], m["face_colors"]


def mesh_tiles(views):
    tsv = tile_starts([v["H"] * v["W"] for v in views], T_MESH)
    tsq = np.concatenate([[0], np.cumsum([max(1, ((v["H"] - 1) * (v["W"] - 1) + T_MESH - 1) // T_MESH) for v in views])]).astype(np.int64)
    return tsv, tsq


def run_mesh(lib, dev, name, runs=1):
    """f3r_mesh_count / _write with explicit thresholds on guarded buffers and a workspace of exactly f3r_mesh_workspace_bytes, 0xFF-filled before
    every run -> per run (counts [V][3] uint32, vertices [nv][3] fp32, faces [nf][3] int32 | int64, face_colors [nf][3] u8)"""
    c = by_name(MESH, name)
    drop, ds, i64, flip = c.cfg
    views = mesh_data(name)
    V = len(views)
    tsv, tsq = mesh_tiles(views)
    nvt, nqt = int(tsv[-1]), int(tsq[-1])
    b = Placed(dev)
    rows, vbase = [], 0
    for v in views:
        conf, pts, img, mask = b.pred(v["conf"]), b.data(v["pts"]), b.data(v["img"]), b.pred(v["mask"])
        rows.append([0 if conf is None else conf.data_ptr(), pts.data_ptr(), img.data_ptr(), 0 if mask is None else mask.data_ptr(), v["H"], v["W"], vbase, 0, 0, 0, 0, 0])
        vbase += v["H"] * v["W"]
    table = b.data(_table(rows, np.concatenate([tsv, tsq])))
    thr = b.pred(np.array([v["thr"] for v in views], F32)) if c.carrier == "conf" else None
    thr_ptr = None if thr is None else thr.data_ptr()
    host_hw = (ctypes.c_int64 * (2 * V))(*[x for v in views for x in (v["H"], v["W"])])
    ws_bytes = lib.f3r_mesh_workspace_bytes(nvt, nqt, vbase, drop)
    assert ws_bytes > 0
    ws = b.workspace(ws_bytes)
    got = []
    for r in range(runs):
        what = f"mesh {name} run {r}"
        ws.fill(0xFF)
        counts = b.out(3 * V, torch.int32)
        _lib.check(lib.f3r_mesh_count(table.data_ptr(), host_hw, V, nvt, nqt, vbase, thr_ptr, drop, ws.ptr, ws_bytes, out_ptr(counts), _stream()), "f3r_mesh_count")
        b.check(what + " count")
        cn = out_np(counts, np.uint32).reshape(V, 3)
        nv, nf = int(cn[:, 2].sum()), (2 if ds else 1) * int(cn[:, 0].sum() + cn[:, 1].sum())
        assert nv <= vbase and nf <= 4 * sum((v["H"] - 1) * (v["W"] - 1) for v in views), f"{what}: counts {cn.tolist()} exceed the views"
        vert, faces, cols = b.out(3 * nv), b.out(3 * nf * (2 if i64 else 1), torch.int32), b.bytes_out(3 * nf)
        _lib.check(lib.f3r_mesh_write(table.data_ptr(), host_hw, V, nvt, nqt, vbase, ds, drop, flip, _lib.F3R_INDEX_I64 if i64 else _lib.F3R_INDEX_I32, ws.ptr, ws_bytes,
                                      out_ptr(vert), out_ptr(faces), cols.ptr, _stream()), "f3r_mesh_write")
        b.check(what + " write")
        got.append((cn, out_np(vert, F32).reshape(nv, 3), out_np(faces, np.int64 if i64 else np.int32).reshape(nf, 3), cols.view.cpu().numpy().reshape(nf, 3)))
    return got


# ================================================================================================ depth sparsify
T_DEPTH = _lib.DEPTH_TILE
DEPTH_BINS = 10
DEPTH_SEGS = (1, 2, 256, 257)
DEPTH = (table_cases(T_DEPTH) + [Case("empty-between", (65, 70, T_DEPTH), "half", "empty-middle"), Case("segs-2", (T_DEPTH + 1, 65), "half"),
                                 Case("segs-256", tuple(1 + (s * 7) % 3 for s in range(256)), "alternate", "few"),
                                 Case("segs-257-twice", tuple(1 + (s * 5) % 3 for s in range(257)), "alternate", "few")])


def depth_passes(n_seg):
    """f3r_depth_sparsify: (32 + seg_bits + 7) / 8 passes of the sort, seg_bits = ceil(log2(n_seg))"""
    return (32 + (n_seg - 1).bit_length() + 7) // 8


@functools.lru_cache(maxsize=None)
def depth_data(name):
    """per segment g, p, conf [n] fp32 and mask [n] u8: distinct confidences and distinct errors; an invalid pixel is so by its mask byte, by g = 0,
    g < 0, a NaN p or an infinite p in turn"""
    c = by_name(DEPTH, name)
    segs = []
    for s, n in enumerate(c.lens):
        rs = _rs(6, n, s, len(c.name))
        keep = pattern(c.pat, n, T_DEPTH, seed=s)
        if c.extra == "few":                     # 1 to 3 pixels: every fourth segment has no valid pixel, the others keep their first or all
            keep = np.zeros(n, bool) if s % 4 == 1 else (np.ones(n, bool) if s % 2 else np.arange(n) == 0)
        if c.extra == "empty-middle" and s == 1:
            keep = np.zeros(n, bool)
        g = (1.0 + 4.0 * rs.rand(n)).astype(F32)
        p = (g * (0.5 + rs.rand(n))).astype(F32)
        conf = (1.0 + rs.permutation(n) / F32(n)).astype(F32)
        mask = rs.randint(1, 256, n).astype(np.uint8)
        why = np.arange(n) % 5
        bad = ~keep
        mask[bad & (why == 0)] = 0
        g[bad & (why == 1)] = 0.0
        g[bad & (why == 2)] = -1.5
        p[bad & (why == 3)] = np.nan
        p[bad & (why == 4)] = np.inf
        segs.append(dict(g=g, p=p, conf=conf, mask=mask, keep=keep))
    return segs


@functools.lru_cache(maxsize=None)
def depth_ref_of(name):
    import depth_ref
    return tuple(depth_ref.segment(s["g"], s["p"], s["conf"], s["mask"], alignment="median", uncertainty=True, n_bins=DEPTH_BINS) for s in depth_data(name))


def run_depth(lib, dev, name, runs=1):
    """f3r_depth_medians, then f3r_depth_sparsify, on guarded buffers (g, p, conf and mask all feed the validity: 0x7F arenas) and a workspace of
    exactly f3r_depth_workspace_bytes(.., 1, n_bins), 0xFF-filled before every run -> per run (out [S][16 + 2 K] float64, order_conf, order_err
    [total] uint32, starts [S + 1] uint32)"""
    segs = depth_data(name)
    S, K = len(segs), DEPTH_BINS
    b = Placed(dev)
    rows, base = [], 0
    for s in segs:
        g, p, conf, mask = b.pred(s["g"]), b.pred(s["p"]), b.pred(s["conf"]), b.pred(s["mask"])
        rows.append([g.data_ptr(), p.data_ptr(), 1, 0, conf.data_ptr(), mask.data_ptr(), len(s["g"]), base])
        base += len(s["g"])
    ts = tile_starts([len(s["g"]) for s in segs], T_DEPTH)
    words = _table(rows, ts)
    host = (ctypes.c_int64 * len(words))(*words.tolist())
    table = b.data(words)
    nt, ld = int(ts[-1]), _lib.DEPTH_OUT_WORDS + 2 * K
    ws_bytes = lib.f3r_depth_workspace_bytes(S, nt, base, 1, K)
    assert ws_bytes > 0
    ws = b.workspace(ws_bytes)
    got = []
    for r in range(runs):
        what = f"depth {name} run {r}"
        ws.fill(0xFF)
        out, oc, oe, st = b.out(2 * S * ld, torch.int32), b.out(base, torch.int32), b.out(base, torch.int32), b.out(S + 1, torch.int32)
        _lib.check(lib.f3r_depth_medians(table.data_ptr(), host, S, nt, _lib.F3R_DEPTH_ALIGN_MEDIAN, 0, 0.0, out_ptr(out), ld, _stream()), "f3r_depth_medians")
        b.check(what + " medians")
        _lib.check(lib.f3r_depth_sparsify(table.data_ptr(), host, S, nt, 0, 0, 0.0, 0.0, K, ws.ptr, ws_bytes, out_ptr(oc), out_ptr(oe), out_ptr(st), out_ptr(out), ld,
                                          _stream()), "f3r_depth_sparsify")
        b.check(what + " sparsify")
        got.append((out_np(out, np.float64).reshape(S, ld), out_np(oc, np.uint32), out_np(oe, np.uint32), out_np(st, np.uint32)))
    return got


# ================================================================================================ recon prepare
T_RECON = 2048                               # f3r_recon.hip: TILE
Q_ICP = 0.75
RECON_FLOOR = 2.0 ** -20


@dataclasses.dataclass(frozen=True)
class ReconCase:
    name: str
    B: int
    bounds: tuple          # the view boundaries inside a sample: 0 .. L
    pat: str
    q_metric: float

    @property
    def L(self):
        return self.bounds[-1]

    @property
    def twice(self):
        return self.name.endswith("-twice")


RECON = ([ReconCase(f"{p}@{n}" + ("-twice" if (n, p) == (2 * T_RECON + 17, "half") else ""), 1, (0, n), p, (0.0, 0.5)[k % 2]) for k, (n, p) in enumerate(pairings(T_RECON))]
         + [ReconCase("views-3", 1, (0, 1000, 2500, 2 * T_RECON + 17), "half", 0.5), ReconCase("views-3-lane63", 1, (0, 100, T_RECON + 33, 2 * T_RECON), "lane63", 0.0),
            ReconCase("two-samples-twice", 2, (0, 333, T_RECON + 1), "half", 0.5), ReconCase("two-samples-last", 2, (0, 65, T_RECON - 1), "last", 0.0)])


@functools.lru_cache(maxsize=None)
def recon_data(name):
    """conf [B L] (distinct inside a view), valid [B L] bytes = the pattern over each sample, pred, gt [B L][3] with gt a similarity of pred and noise"""
    c = by_name(RECON, name)
    B, L = c.B, c.L
    rs = _rs(7, L, B, len(c.name))
    conf = np.concatenate([(1.0 + rs.permutation(hi - lo) / F32(hi - lo)).astype(F32) for _ in range(B) for lo, hi in zip(c.bounds[:-1], c.bounds[1:])])
    keep = np.concatenate([pattern(c.pat, L, T_RECON, seed=i) for i in range(B)])
    valid = np.where(keep, rs.randint(1, 256, B * L), 0).astype(np.uint8)
    pred = rs.randn(B * L, 3)
    q, _ = np.linalg.qr(rs.randn(3, 3))
    q *= np.sign(np.linalg.det(q))
    gt = 1.7 * pred @ q.T + np.array([0.3, -1.0, 2.0]) + 0.01 * rs.randn(B * L, 3)
    seg = np.array([i * L + x for i in range(B) for x in c.bounds[:-1]] + [B * L], np.int64)
    return dict(conf=conf, valid=valid, pred=pred.astype(F32), gt=gt.astype(F32), seg=seg, keep=keep)


def recon_masks(name):
    """bit 0: valid and conf >= thr_metric, bit 1: valid, bit 2 (the passenger): conf >= thr_icp -- per pixel, the thresholds per (sample, view)"""
    import depth_ref
    c, d = by_name(RECON, name), recon_data(name)
    m = np.zeros(c.B * c.L, np.int64)
    for lo, hi in zip(d["seg"][:-1], d["seg"][1:]):
        cf = d["conf"][lo:hi]
        tm, ti = depth_ref.quantile_rule(cf, np.float32(c.q_metric)), depth_ref.quantile_rule(cf, np.float32(Q_ICP))
        v = d["valid"][lo:hi] != 0
        m[lo:hi] = (v & (cf >= tm)).astype(np.int64) | (v.astype(np.int64) << 1) | ((cf >= ti).astype(np.int64) << 2)
    return m


def umeyama(x, y, w, dtype):
    """recon_ref.rigid_points_registration(compute_scaling=True), operation for operation, in `dtype` throughout"""
    X, Y, w = x.to(dtype), y.to(dtype), w.to(dtype)
    wn = w / w.sum()
    mx, my = (wn[:, None] * X).sum(0), (wn[:, None] * Y).sum(0)
    Xc, Yc = X - mx, Y - my
    M = (wn[:, None] * Yc).T @ Xc
    U, S, Vt = torch.linalg.svd(M)
    d = torch.sign(torch.det(U) * torch.det(Vt))
    one = torch.ones((), dtype=dtype)
    D = torch.diag(torch.stack([one, one, d]))
    R = U @ D @ Vt
    s = (S * torch.diagonal(D)).sum() / (wn * (Xc * Xc).sum(1)).sum()
    return R, my - s * (R @ mx), s


@functools.lru_cache(maxsize=None)
def recon_ref_of(name, dtype=torch.float64):
    """-> (counts [2][B] int32, gt_out rows per sample, rts [B][13] and the transformed kept predictions per sample in `dtype`, as float64)"""
    c, d = by_name(RECON, name), recon_data(name)
    m = recon_masks(name)
    counts, gts, rts, preds = np.zeros((2, c.B), np.int32), [], [], []
    for i in range(c.B):
        sl = slice(i * c.L, (i + 1) * c.L)
        k0, k1, w = (m[sl] & 1) == 1, (m[sl] & 2) == 2, (m[sl] & 4) == 4
        counts[:, i] = k0.sum(), k1.sum()
        gts.append(d["gt"][sl][k1])
        x, y, wk = torch.from_numpy(d["pred"][sl][k0]), torch.from_numpy(d["gt"][sl][k0]), torch.from_numpy(w[k0])
        if int(wk.sum()) < 3:
            R, t, s = torch.eye(3, dtype=dtype), torch.zeros(3, dtype=dtype), torch.ones((), dtype=dtype)
        else:
            R, t, s = umeyama(x, y, wk, dtype)
        rts.append(torch.cat([R.reshape(-1), t, s.reshape(1)]).double().numpy())
        preds.append((s * (x.to(dtype) @ R.T) + t).double().numpy())
    return counts, gts, np.stack(rts), preds


def rel_err(a, b):
    """max |a - b| / max |b| (0 for empty tensors)"""
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.abs(a - b).max() / np.abs(b).max()) if b.size else 0.0


def run_recon(lib, dev, name, runs=1):
    """f3r_recon_prepare on guarded buffers and a workspace of exactly f3r_recon_prepare_workspace_bytes, 0xFF-filled before every run.  pred_out and
    gt_out are [B L][3] by the ABI; the rows past a sample's count must keep their sentinel words (asserted here)
    -> per run (counts [2][B] int32, gt rows per sample, rts [B][13] fp32, pred rows per sample)"""
    c, d = by_name(RECON, name), recon_data(name)
    B, V, L = c.B, len(c.bounds) - 1, c.L
    b = Placed(dev)
    conf, valid, pred, gt, seg = b.pred(d["conf"]), b.pred(d["valid"]), b.data(d["pred"]), b.data(d["gt"]), b.data(d["seg"])
    ws_bytes = lib.f3r_recon_prepare_workspace_bytes(B, V, L)
    assert ws_bytes > 0
    ws = b.workspace(ws_bytes)
    got = []
    for r in range(runs):
        what = f"recon {name} run {r}"
        ws.fill(0xFF)
        pred_out, gt_out, counts, rts = b.out(3 * B * L), b.out(3 * B * L), b.out(2 * B, torch.int32), b.out(13 * B)
        _lib.check(lib.f3r_recon_prepare(conf.data_ptr(), pred.data_ptr(), gt.data_ptr(), valid.data_ptr(), seg.data_ptr(), B, V, L, float(c.q_metric), Q_ICP,
                                         out_ptr(pred_out), out_ptr(gt_out), out_ptr(counts), out_ptr(rts), ws.ptr, ws_bytes, _stream()), "f3r_recon_prepare")
        b.check(what)
        cn = out_np(counts, np.int32).reshape(2, B)
        assert ((0 <= cn) & (cn <= L)).all(), f"{what}: counts {cn.tolist()}"
        po, go = out_np(pred_out, np.int32).reshape(B, L, 3), out_np(gt_out, np.int32).reshape(B, L, 3)
        for i in range(B):
            assert (po[i, cn[0, i]:] == SENTINEL32).all() and (go[i, cn[1, i]:] == SENTINEL32).all(), f"{what}: a row past the count of sample {i} was written"
        got.append((cn, [go[i, :cn[1, i]].view(F32) for i in range(B)], out_np(rts, F32).reshape(B, 13), [po[i, :cn[0, i]].view(F32) for i in range(B)]))
    return got


# ================================================================================================ match write
T_MATCH = _lib.MATCH_TILE
MATCH_WIDTHS = (37, 64, 5)


@dataclasses.dataclass(frozen=True)
class MatchCase:
    name: str
    n: int                 # candidates of view 1, the pair's second view; view 0 has as many, view 2 none
    pat: str
    cut: int = 0           # n_matches = the total less this many

    @property
    def twice(self):
        return self.name.endswith("-twice")


MATCH = ([MatchCase(f"{p}@{n}" + ("-twice" if (n, p) == (2 * T_MATCH + 17, "half") else ""), n, p) for n, p in pairings(T_MATCH)]
         + [MatchCase("cut-5@4113", 2 * T_MATCH + 17, "half", 5), MatchCase("cut-all-but-one@2047", T_MATCH - 1, "all", T_MATCH - 2), MatchCase("cut-1@2048", T_MATCH, "lane63", 1)])
MATCH_DIRECTED = ((0, 1), (1, 0), (0, 2), (2, 0), (2, 1), (1, 2))
MATCH_PAIRS = ((0, 2, 2, 3), (0, 1, 0, 1), (2, 1, 4, 5), (1, 0, 1, 0))     # (i, j, row of i -> j, row of j -> i): an empty j, the pattern, an empty i, the mirror


@functools.lru_cache(maxsize=None)
def match_data(name):
    """hand-built neighbours: candidate q of view 1 is reciprocal with view 0 iff the pattern keeps it.  A dropped q names -1, n (out of range) or
    a candidate of view 0 whose own neighbour is someone else, in turn."""
    c = by_name(MATCH, name)
    n = c.n
    rs = _rs(8, n, len(c.name))
    keep = pattern(c.pat, n, T_MATCH)
    counts = (n, n, 0)
    seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    qoff = np.concatenate([[0], np.cumsum([counts[a] for a, _ in MATCH_DIRECTED])]).astype(np.int64)
    nn = np.zeros(int(qoff[-1]), np.int32)
    perm = rs.permutation(n).astype(np.int32)                  # a(q): q's neighbour in view 0, all distinct
    n10 = perm.copy()
    n01 = np.full(n, n, np.int32)                              # view 0's candidates: no neighbour, unless a kept q names them
    n01[perm[keep]] = np.flatnonzero(keep)
    dropped = np.flatnonzero(~keep)
    why = np.arange(len(dropped)) % 3
    n10[dropped[why == 0]] = -1
    n10[dropped[why == 1]] = n
    other = dropped[why == 2]                                  # a valid candidate of view 0 that answers with another q (or with none)
    n01[perm[other]] = (other + 1) % n
    fix = n01[perm[other]] == other
    n01[perm[other][fix]] = n
    nn[qoff[0]:qoff[1]], nn[qoff[1]:qoff[2]] = n01, n10
    nn[qoff[5]:qoff[6]] = 0                                    # view 1 -> the empty view 2: "0 for an empty b"
    dist = rs.rand(int(qoff[-1])).astype(np.float64)
    pix = np.concatenate([rs.permutation(m).astype(np.int32) for m in counts])
    pts = rs.randn(int(seg[-1]), 3).astype(F32)
    tile_off = np.concatenate([[0], np.cumsum([(counts[j] + T_MATCH - 1) // T_MATCH for _, j, _, _ in MATCH_PAIRS])]).astype(np.int64)
    return dict(counts=counts, seg=seg, qoff=qoff, nn=nn, dist=dist, pix=pix, pts=pts, tile_off=tile_off, keep=keep)


def match_flags(d):
    """`reciprocal` restated per pair: the candidates q of view j with nn_ij[nn_ji[q]] == q, and their a"""
    out = []
    for i, j, f, bk in MATCH_PAIRS:
        ni, nj = d["counts"][i], d["counts"][j]
        a = d["nn"][d["qoff"][bk]:d["qoff"][bk] + nj].astype(np.int64)
        ok = (ni > 0) & (a >= 0) & (a < ni)
        back = d["nn"][d["qoff"][f]:d["qoff"][f] + ni]
        ok[ok] = back[a[ok]] == np.flatnonzero(ok)
        out.append((ok, a))
    return out


@functools.lru_cache(maxsize=None)
def match_ref_of(name):
    """-> (tile_counts [tiles + 1] uint32 scanned, offsets [P + 2] int64, xy_i, xy_j [M][2] int32, dist [M]) with M the total less the case's cut"""
    c, d = by_name(MATCH, name), match_data(name)
    flags = match_flags(d)
    per_tile = [int(ok[b:b + T_MATCH].sum()) for ok, _ in flags for b in range(0, len(ok), T_MATCH)]
    scan = np.concatenate([[0], np.cumsum(per_tile)]).astype(np.uint32)
    offsets = np.array([int(scan[t]) for t in d["tile_off"]] + [0], np.int64)
    xi, xj, ds = [], [], []
    for (i, j, f, bk), (ok, a) in zip(MATCH_PAIRS, flags):
        q = np.flatnonzero(ok)
        pj, pi = d["pix"][d["seg"][j] + q], d["pix"][d["seg"][i] + a[q]]
        xj.append(np.stack([pj % MATCH_WIDTHS[j], pj // MATCH_WIDTHS[j]], 1))
        xi.append(np.stack([pi % MATCH_WIDTHS[i], pi // MATCH_WIDTHS[i]], 1))
        ds.append(d["dist"][d["qoff"][bk] + q])
    M = int(scan[-1]) - c.cut
    assert M >= 0
    return scan, offsets, np.concatenate(xi).astype(np.int32)[:M], np.concatenate(xj).astype(np.int32)[:M], np.concatenate(ds)[:M]


def run_match(lib, dev, name, runs=1):
    """f3r_match_count / _write on an index from post_ops.match_index and hand-built neighbours, every buffer of the two entries guarded; the
    outputs hold n_matches = total - cut rows: nothing may be stored at or past them
    -> per run (tile_counts, offsets, xy_i, xy_j int32 [M][2], dist float64 [M])"""
    from fast3r_amd import post_ops
    c, d = by_name(MATCH, name), match_data(name)
    V, P, D = 3, len(MATCH_PAIRS), len(MATCH_DIRECTED)
    ix = post_ops.match_index(torch.from_numpy(d["pts"]).to(dev), d["counts"])
    b = Placed(dev)
    seg, qoff, toff, pairs = b.data(d["seg"]), b.data(d["qoff"]), b.data(d["tile_off"]), b.data(np.asarray(MATCH_PAIRS, np.int32))
    nn, dist, pix, widths = b.pred(d["nn"]), b.data(d["dist"]), b.data(d["pix"]), b.data(np.asarray(MATCH_WIDTHS, np.int32))
    seg_h, qoff_h, toff_h = ((ctypes.c_int64 * len(a))(*a.tolist()) for a in (d["seg"], d["qoff"], d["tile_off"]))
    pairs_h = (ctypes.c_int32 * (4 * P))(*[x for p in MATCH_PAIRS for x in p])
    T = int(d["tile_off"][-1])
    count, write = _lib.entry("f3r_match_count"), _lib.entry("f3r_match_write")
    got = []
    for r in range(runs):
        what = f"match {name} run {r}"
        tc, off = b.out(T + 1, torch.int32), b.out(2 * (P + 2), torch.int32)
        _lib.check(count(ix["index"].data_ptr(), seg.data_ptr(), seg_h, V, pairs.data_ptr(), pairs_h, toff.data_ptr(), toff_h, P, qoff.data_ptr(), qoff_h, D,
                         nn.data_ptr(), out_ptr(tc), out_ptr(off), _stream()), "f3r_match_count")
        b.check(what + " count")
        offsets = out_np(off, np.int64)
        total = int(offsets[P])
        assert 0 <= total <= 2 * c.n and offsets[P + 1] == 0, f"{what}: offsets {offsets.tolist()}"
        M = max(total - c.cut, 0)
        xi, xj, ds = b.out(2 * M, torch.int32), b.out(2 * M, torch.int32), b.out(2 * M, torch.int32)
        _lib.check(write(seg.data_ptr(), seg_h, V, pairs.data_ptr(), pairs_h, toff.data_ptr(), toff_h, P, qoff.data_ptr(), qoff_h, D, nn.data_ptr(), dist.data_ptr(),
                         out_ptr(tc), pix.data_ptr(), widths.data_ptr(), out_ptr(xi), out_ptr(xj), out_ptr(ds), M, _stream()), "f3r_match_write")
        b.check(what + " write")
        got.append((out_np(tc, np.uint32), offsets, out_np(xi, np.int32).reshape(M, 2), out_np(xj, np.int32).reshape(M, 2), out_np(ds, np.float64)))
    return got
