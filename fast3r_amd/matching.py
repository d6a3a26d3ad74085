"""Pixel correspondences between views on the GPU: the reference's `find_reciprocal_matches` (fast3r/dust3r/utils/geometry.py:381-397: two
cKDTrees, mutual nearest neighbours) and the pair lists of `make_pairs` (fast3r/dust3r/image_pairs.py:17-47), for every view pair of a scene
in one batched call.  Fast3R puts every view's pointmap in one frame, so reciprocal 3D neighbours between two views are 2D-2D matches.

The kernels (fast3r_amd/csrc/f3r_match.hip, include/f3r.h "view matching", docs/rows_f.md) index the candidates of all views in one call, search
all directed pairs in one launch and write the matches of all pairs in order; the host reads one small table back per chunk of pairs.

* `find_reciprocal_matches(P1, P2)`: the reference's name and returns, on device tensors.
* `scene_graph_pairs(n_views, scene_graph, prefilter, symmetrize)`: the index pairs `make_pairs` forms.
* `match_views(preds, ...)` -> `ViewMatches`: candidates per view (subsampling, confidence percentile, masks), matches per pair.
"""
import dataclasses

import numpy as np
import torch

from . import _lib, post_ops
from ._lib import work_device

QUERY_BYTES = 12  # workspace per directed query: the neighbour's int32 index and the fp64 distance
MAX_CHUNK_QUERIES = (1 << 31) - 1  # directed queries of one chunk: one thread each in one launch (f3r_match_search refuses more)
MAX_CHUNK_TILES = (1 << 21) - 1    # tiles of the second views of one chunk's pairs (f3r_match_count refuses more)


# ------------------------------------------------------------------------------------------------------------------- pair graphs
def _graph_arg(scene_graph, name, default):
    """'swin-3' -> 3, 'swin' -> default"""
    if scene_graph == name:
        return default
    try:
        k = int(scene_graph[len(name) + 1:])
    except ValueError:
        k = -1
    if not scene_graph.startswith(name + "-") or k < 0:
        raise ValueError(f"scene_graph_pairs: cannot read the number in scene graph {scene_graph!r} (expected {name!r} or '{name}-K')")
    return k


def _prefilter_arg(prefilter, name):
    try:
        return int(prefilter[len(name):])
    except ValueError:
        raise ValueError(f"scene_graph_pairs: cannot read the number in prefilter {prefilter!r} (expected '{name}K')") from None


def scene_graph_pairs(n_views, scene_graph="complete", prefilter=None, symmetrize=True):
    """The index pairs `make_pairs(imgs, scene_graph, prefilter, symmetrize)` forms over n_views images: int64 numpy [P, 2].
    scene_graph: 'complete' (every (i, j) with j < i), 'swin' / 'swin-K' (each view with its next K, cyclically; K = 3), 'oneref' / 'oneref-K' (view K
    with every other; K = 0).  prefilter: None, 'seqK' (keep |i - j| <= K) or 'cycK' (the same on a circle).  Every graph comes out in ascending
    (i, j) order of the unsymmetrised pairs, followed by their reverses with symmetrize (the reference walks a set for 'swin': its order there is
    no contract).  An unknown name is a ValueError (the reference returns no pairs)."""
    n = int(n_views)
    if n < 0:
        raise ValueError(f"scene_graph_pairs: n_views = {n_views} is negative")
    if not isinstance(scene_graph, str):
        raise ValueError(f"scene_graph_pairs: scene_graph must be a string, got {scene_graph!r}")
    if scene_graph == "complete":
        pairs = [(i, j) for i in range(n) for j in range(i)]
    elif scene_graph.startswith("swin"):
        k = _graph_arg(scene_graph, "swin", 3)
        s = set()
        for i in range(n):
            for j in range(1, k + 1):
                a, b = i, (i + j) % n  # the loop closes; a window that wraps onto its own view gives (i, i), as in the reference
                s.add((a, b) if a < b else (b, a))
        pairs = list(s)
    elif scene_graph.startswith("oneref"):
        ref = _graph_arg(scene_graph, "oneref", 0)
        if n and not 0 <= ref < n:
            raise ValueError(f"scene_graph_pairs: the reference view of {scene_graph!r} is not one of the {n} views")
        pairs = [(ref, j) for j in range(n) if j != ref]
    else:
        raise ValueError(f"scene_graph_pairs: unknown scene graph {scene_graph!r} (complete, swin, swin-K, oneref, oneref-K)")
    pairs = sorted(pairs)
    if prefilter is not None:
        if not isinstance(prefilter, str) or not (prefilter.startswith("seq") or prefilter.startswith("cyc")):
            raise ValueError(f"scene_graph_pairs: unknown prefilter {prefilter!r} (seqK, cycK)")
        if prefilter.startswith("seq"):
            w = _prefilter_arg(prefilter, "seq")
            pairs = [(i, j) for i, j in pairs if abs(i - j) <= w]
        else:
            w = _prefilter_arg(prefilter, "cyc")
            pairs = [(i, j) for i, j in pairs if min(abs(i - j), abs(i - j + n), abs(i - j - n)) <= w]
    if symmetrize:
        pairs = pairs + [(j, i) for i, j in pairs]
    return np.asarray(pairs, dtype=np.int64).reshape(-1, 2)


def _pair_list(pairs, n_views):
    """`pairs` of match_views -> int64 numpy [P, 2]: a graph string, or explicit rows (i, j) (repeats and i == j allowed, P = 0 allowed)"""
    if isinstance(pairs, str):
        return scene_graph_pairs(n_views, pairs, symmetrize=False)
    if torch.is_tensor(pairs):
        pairs = pairs.detach().cpu().numpy()
    arr = np.asarray(pairs)
    if arr.size == 0:
        return np.zeros((0, 2), dtype=np.int64)
    if arr.ndim != 2 or arr.shape[1] != 2 or arr.dtype.kind not in "iu":
        raise ValueError(f"match_views: pairs must be a scene-graph string or integer rows (i, j), got an array of shape {arr.shape} and type {arr.dtype}")
    arr = arr.astype(np.int64)
    if arr.min() < 0 or arr.max() >= n_views:
        raise ValueError(f"match_views: pairs name views outside 0 .. {n_views - 1}")
    return arr


# ------------------------------------------------------------------------------------------------------------------- chunks
def plan_chunks(counts, pairs, index_bytes, max_workspace_bytes, max_queries=MAX_CHUNK_QUERIES, max_tiles=MAX_CHUNK_TILES):
    """Split the pair list so that every chunk's workspace -- the index plus QUERY_BYTES per directed query, each directed pair (a -> b) once per
    chunk -- stays within max_workspace_bytes, and its directed queries and tiles within what one launch takes.  -> a list of dicts(start, stop: the rows of `pairs`, directed: the chunk's directed pairs in
    first-use order, rows: per pair the (forward, backward) rows of `directed`, queries, bytes).  A pair that does not fit alone is a ValueError."""
    budget = int(max_workspace_bytes) - int(index_bytes)
    chunks, cur = [], None
    for p, (i, j) in enumerate(np.asarray(pairs, dtype=np.int64).reshape(-1, 2).tolist()):
        need = [(i, j)] if i == j else [(i, j), (j, i)]
        alone = QUERY_BYTES * sum(counts[a] for a, _ in need)
        tiles = -(-counts[j] // _lib.MATCH_TILE)
        if alone > budget:
            raise ValueError(f"match_views: pair ({i}, {j}) alone needs {int(index_bytes) + alone} bytes of workspace ({counts[i]} and {counts[j]} "
                             f"candidates; the index takes {int(index_bytes)}), more than max_workspace_bytes = {int(max_workspace_bytes)}: raise the "
                             "budget, or take fewer candidates with a larger `subsample`")
        if cur is not None:
            extra = QUERY_BYTES * sum(counts[a] for a, b in need if (a, b) not in cur["_rows"])
            if (cur["bytes"] + extra > int(max_workspace_bytes) or cur["queries"] + extra // QUERY_BYTES > max_queries
                    or cur["tiles"] + tiles > max_tiles):
                chunks.append(cur)
                cur = None
        if cur is None:
            cur = {"start": p, "stop": p, "directed": [], "_rows": {}, "rows": [], "queries": 0, "tiles": 0, "bytes": int(index_bytes)}
        for d in need:
            if d not in cur["_rows"]:
                cur["_rows"][d] = len(cur["directed"])
                cur["directed"].append(d)
                cur["queries"] += counts[d[0]]
                cur["bytes"] += QUERY_BYTES * counts[d[0]]
        cur["rows"].append((cur["_rows"][(i, j)], cur["_rows"][(j, i)]))
        cur["tiles"] += tiles
        cur["stop"] = p + 1
    if cur is not None:
        chunks.append(cur)
    for c in chunks:
        del c["_rows"]
    return chunks


# ------------------------------------------------------------------------------------------------------------------- results
@dataclasses.dataclass
class ViewMatches:
    """Matches of P view pairs, as device tensors.  pairs int64 [P, 2]; offsets int64 [P + 1]; xy_i, xy_j int32 [M, 2] as (x, y), like the
    reference's xy_grid; dist fp64 [M]; counts int64 [P].  The matches of pair p are rows offsets[p] .. offsets[p + 1], in ascending candidate
    order of view j: the order `pts2d[1][reciprocal_in_P2]`, `pts2d[0][nn2_in_P1][reciprocal_in_P2]` has with the reference function."""
    pairs: torch.Tensor
    offsets: torch.Tensor
    xy_i: torch.Tensor
    xy_j: torch.Tensor
    dist: torch.Tensor
    counts: torch.Tensor
    n_chunks: int = 1
    workspace_bytes: int = 0

    def pair(self, p):
        """(xy_i, xy_j, dist) of pair p"""
        P = self.pairs.shape[0]
        if not -P <= p < P:
            raise IndexError(f"ViewMatches.pair: {p} is not one of the {P} pairs")
        a, b = self.offsets[p % P:p % P + 2].tolist()
        return self.xy_i[a:b], self.xy_j[a:b], self.dist[a:b]

    def covisibility(self, n_views=None, max_dist=None):
        """int64 [N, N]: the match counts of every pair summed into [i, j] and [j, i] (a pair (i, i) into [i, i] once); matches farther apart
        than max_dist are not counted."""
        P = self.pairs.shape[0]
        N = int(n_views) if n_views is not None else (int(self.pairs.max()) + 1 if P else 0)
        out = torch.zeros((N, N), dtype=torch.int64, device=self.pairs.device)
        if P == 0:
            return out
        if max_dist is None:
            cnt = self.counts
        else:
            owner = torch.repeat_interleave(torch.arange(P, device=self.pairs.device), self.counts)
            cnt = torch.zeros(P, dtype=torch.int64, device=self.pairs.device).index_add_(0, owner, (self.dist <= float(max_dist)).long())
        i, j = self.pairs[:, 0], self.pairs[:, 1]
        out.index_put_((i, j), cnt, accumulate=True)
        off = i != j
        out.index_put_((j[off], i[off]), cnt[off], accumulate=True)
        return out


# ------------------------------------------------------------------------------------------------------------------- matching
def _points(x, what):
    t = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x)
    if t.ndim != 2 or t.shape[-1] != 3:
        raise ValueError(f"{what}: expected an (n, 3) point array, got shape {tuple(t.shape)}")
    if not t.dtype.is_floating_point:
        raise ValueError(f"{what}: expected floating-point coordinates, got {t.dtype}")
    return t


def _raise_non_finite(flag, who):
    if flag:
        raise ValueError(f"{who}: {flag} view(s) have NaN or inf coordinates among their candidates (cKDTree raises on those too); mask them out")


def find_reciprocal_matches(P1, P2):
    """The reference's find_reciprocal_matches on (n1, 3) and (n2, 3) points -> (reciprocal_in_P2 bool [n2], nn2_in_P1 int64 [n2],
    num_matches int).  Exact nearest neighbours by the fp64 distance of the fp32 coordinates, ties to the smaller index;
    reciprocal_in_P2[j] = (nn1_in_P2[nn2_in_P1[j]] == j).  NaN / inf coordinates are a ValueError.  An empty P1 or P2 gives no matches (with
    P1 empty nn2_in_P1 is all 0)."""
    a, b = _points(P1, "find_reciprocal_matches: P1"), _points(P2, "find_reciprocal_matches: P2")
    dev = a.device if a.is_cuda else (b.device if b.is_cuda else work_device(a, "points"))
    a, b = (t.to(device=dev, dtype=torch.float32).contiguous() for t in (a, b))
    n1, n2 = a.shape[0], b.shape[0]
    ix = post_ops.match_index(torch.cat([a, b]), [n1, n2])
    found = post_ops.match_search(ix, [(0, 1), (1, 0)])
    counted = post_ops.match_count(ix, found, [(0, 1, 0, 1)])
    offsets = counted["offsets"].cpu().tolist()  # the one read-back: the count and the flag word
    _raise_non_finite(offsets[2], "find_reciprocal_matches")
    nn1, nn2 = found["nn_idx"][:n1].long(), found["nn_idx"][n1:].long()
    if n1 == 0 or n2 == 0:
        return torch.zeros(n2, dtype=torch.bool, device=dev), nn2, 0
    reciprocal = nn1[nn2] == torch.arange(n2, device=dev)
    return reciprocal, nn2, int(offsets[1])


def _preds_of(output_or_preds, views):
    if isinstance(output_or_preds, dict):
        if "preds" not in output_or_preds:
            raise ValueError("match_views: a dict must be the output of inference(): {'preds': [...], 'views': [...]}")
        return list(output_or_preds["preds"]), output_or_preds.get("views", views)
    return list(output_or_preds), views


def _sample_of(t, sample, trailing, what):
    """(B, H, W, ...) -> (H, W, ...) of one sample; a map without the batch dimension passes"""
    if t.dim() == 3 + trailing:
        if not 0 <= sample < t.shape[0]:
            raise ValueError(f"match_views: sample = {sample} outside the batch of {t.shape[0]} ({what})")
        t = t[sample]
    if t.dim() != 2 + trailing or (trailing and t.shape[-1] != 3):
        raise ValueError(f"match_views: {what} must be (H, W{', 3' if trailing else ''}) with or without a batch dimension, got {tuple(t.shape)}")
    return t


def _threshold(c, q):
    """torch.quantile(c, q) ('linear') of an fp32 vector by the project's rule (f3r_post_common.h block_quantile): the rank q (n - 1) in fp32,
    at::lerp between the two order statistics with every operation rounded on its own; NaN with any NaN.  A 0-dim tensor, no read-back."""
    if q == 0.0:
        return c.amin()  # the smallest value, NaN with any NaN
    srt = torch.sort(c).values  # NaNs last
    rank = np.float32(q) * np.float32(c.numel() - 1)
    lo = np.floor(rank)
    w = np.float32(rank - lo)
    vlo, vhi = srt[int(lo)], srt[int(np.ceil(rank))]
    d = vhi - vlo
    thr = vlo + d * float(w) if w < np.float32(0.5) else vhi - d * float(np.float32(1.0) - w)
    return torch.where(torch.isnan(srt[-1]), srt[-1], thr)


def view_candidates(pts, confs, masks, min_conf_thr_percentile, subsample):
    """The candidates of every view: lists of (H, W, 3) fp32 pointmaps, (H, W) fp32 confidences or None, (H, W) bool masks or None, all on one
    GPU.  Pixel (y, x) is a candidate iff y % subsample == 0 and x % subsample == 0, conf >= torch.quantile(conf.flatten(), pct / 100) (_threshold; over the
    whole map: a NaN confidence keeps nothing) and its mask is true.  -> (points fp32 [total, 3], pix int32 [total] row-major pixel indices,
    counts: a list, widths int32 [V]); candidates in row-major order.  One read-back (the counts)."""
    dev, V, s, q = pts[0].device, len(pts), int(subsample), float(min_conf_thr_percentile) / 100.0
    keeps, sub_sizes = [], []
    for v in range(V):
        H, W = pts[v].shape[:2]
        c, m = confs[v], masks[v]
        if c is not None:
            k = c[::s, ::s] >= _threshold(c.reshape(-1), q)
        else:
            k = torch.ones((-(-H // s), -(-W // s)), dtype=torch.bool, device=dev)
        if m is not None:
            k = k & m[::s, ::s]
        keeps.append(k.reshape(-1))
        sub_sizes.append(k.numel())
    sub_off = np.concatenate([[0], np.cumsum(sub_sizes)]).astype(np.int64)
    idx = torch.cat(keeps).nonzero().squeeze(1)
    off_dev = torch.from_numpy(sub_off).to(dev)
    view_of = torch.bucketize(idx, off_dev[1:], right=True)
    counts = torch.bincount(view_of, minlength=V).cpu().tolist()
    widths = torch.tensor([p.shape[1] for p in pts], dtype=torch.int64, device=dev)
    sub_w = torch.tensor([-(-p.shape[1] // s) for p in pts], dtype=torch.int64, device=dev)
    local = idx - off_dev[view_of]
    wv, swv = widths[view_of], sub_w[view_of]
    pix = ((local // swv) * s * wv + (local % swv) * s)
    seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    parts = [pts[v].reshape(-1, 3)[pix[seg[v]:seg[v + 1]]] for v in range(V) if counts[v]]
    points = torch.cat(parts) if parts else torch.zeros((0, 3), dtype=torch.float32, device=dev)
    return points.contiguous(), pix.to(torch.int32), counts, widths.to(torch.int32)


def match_views(output_or_preds, views=None, *, pairs="complete", pts3d_key="pts3d_in_other_view", conf_key="conf", min_conf_thr_percentile=0,
                masks=None, subsample=1, sample=0, max_workspace_bytes=2 << 30):
    """Reciprocal matches between the pointmaps of view pairs.  output_or_preds: the output dict of inference() or its preds list (per view
    pts3d_key (B, H, W, 3) and conf_key (B, H, W); `sample` picks the batch entry; views may differ in size).  pairs: a graph string for
    scene_graph_pairs(n_views, pairs, symmetrize=False), or explicit rows (i, j).  Candidates per view: see view_candidates (masks: optional bool
    (H, W) per view).  For pair (i, j) the result is what find_reciprocal_matches(cand_i, cand_j) gives, as pixel coordinates.  When the
    workspace (the index plus 12 bytes per directed query) would exceed max_workspace_bytes the pair list is split into chunks.  -> ViewMatches."""
    preds, views = _preds_of(output_or_preds, views)
    V = len(preds)
    if V < 1:
        raise ValueError("match_views: need at least one view")
    s = int(subsample)
    if s != subsample or s < 1:
        raise ValueError(f"match_views: subsample must be a positive integer, got {subsample!r}")
    pct = float(min_conf_thr_percentile)
    if not 0.0 <= pct <= 100.0:
        raise ValueError(f"match_views: min_conf_thr_percentile must lie in [0, 100], got {min_conf_thr_percentile!r}")
    if masks is not None and len(masks) != V:
        raise ValueError(f"match_views: masks must have one entry per view ({V}), got {len(masks)}")
    pair_rows = _pair_list(pairs, V)
    for v, p in enumerate(preds):
        if pts3d_key not in p:
            raise KeyError(f"match_views: preds[{v}] has no '{pts3d_key}'")
    dev = work_device(preds[0][pts3d_key], "preds")
    to = lambda t: t.to(dev) if t.device != dev else t  # noqa: E731
    pts_l, conf_l, mask_l = [], [], []
    for v, p in enumerate(preds):
        x = _sample_of(to(p[pts3d_key]), sample, 1, f"preds[{v}]['{pts3d_key}']").to(torch.float32)
        c = None
        if conf_key is not None and conf_key in p:
            c = _sample_of(to(p[conf_key]), sample, 0, f"preds[{v}]['{conf_key}']").to(torch.float32)
            if c.shape != x.shape[:2]:
                raise ValueError(f"match_views: view {v}: the confidence {tuple(c.shape)} must have the pointmap's size {tuple(x.shape[:2])}")
        elif pct > 0:
            raise ValueError(f"match_views: min_conf_thr_percentile > 0 needs '{conf_key}' in every pred (view {v} has none)")
        m = None
        if masks is not None and masks[v] is not None:
            m = to(torch.as_tensor(masks[v]))
            if m.dtype != torch.bool or m.shape != x.shape[:2]:
                raise ValueError(f"match_views: masks[{v}] must be bool {tuple(x.shape[:2])}, got {m.dtype} {tuple(m.shape)}")
        pts_l.append(x)
        conf_l.append(c)
        mask_l.append(m)
    points, pix, counts, widths = view_candidates(pts_l, conf_l, mask_l, pct, s)
    ix = post_ops.match_index(points, counts)
    chunks = plan_chunks(counts, pair_rows, ix["index"].numel(), max_workspace_bytes)
    P = pair_rows.shape[0]
    out = {"xy_i": [], "xy_j": [], "dist": [], "counts": []}
    for ch in chunks:
        found = post_ops.match_search(ix, ch["directed"])
        rows = [(i, j, f, b) for (i, j), (f, b) in zip(pair_rows[ch["start"]:ch["stop"]].tolist(), ch["rows"])]
        counted = post_ops.match_count(ix, found, rows)
        offsets = counted["offsets"].cpu().numpy()  # the chunk's one read-back: the match counts and the flag word
        _raise_non_finite(int(offsets[-1]), "match_views")
        xy_i, xy_j, dist = post_ops.match_write(ix, found, counted, int(offsets[-2]), pix, widths)
        out["xy_i"].append(xy_i)
        out["xy_j"].append(xy_j)
        out["dist"].append(dist)
        out["counts"].append(np.diff(offsets[:-1]))
    if not chunks:  # no pair: the index still says whether a candidate is NaN / inf
        found = post_ops.match_search(ix, [])
        _raise_non_finite(int(post_ops.match_count(ix, found, [])["offsets"].cpu()[-1]), "match_views")
    cnt = np.concatenate(out["counts"]).astype(np.int64) if chunks else np.zeros(0, dtype=np.int64)
    cat = lambda parts, shape, dt: torch.cat(parts) if parts else torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    return ViewMatches(pairs=torch.from_numpy(pair_rows).to(dev), offsets=torch.from_numpy(np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)).to(dev),
                       xy_i=cat(out["xy_i"], (0, 2), torch.int32), xy_j=cat(out["xy_j"], (0, 2), torch.int32), dist=cat(out["dist"], (0,), torch.float64),
                       counts=torch.from_numpy(cnt).to(dev), n_chunks=max(len(chunks), 1),
                       workspace_bytes=max((c["bytes"] for c in chunks), default=ix["index"].numel()))
