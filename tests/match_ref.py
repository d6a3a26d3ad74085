"""Plain numpy restatement of view matching (fast3r_amd/matching.py): the yardstick of tests/test_matching.py (against the reference's own
find_reciprocal_matches / make_pairs through tests/golden/matches_cases.npz) and of tests/test_matching_gpu.py (against the kernels).
Brute force: fp64 distances of the fp32 coordinates in the order ((dx^2 + dy^2) + dz^2), argmin with ties to the smaller index, the
reciprocity rule, the candidate rule, the pair graphs and the output order.  No library, no GPU."""
import numpy as np

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------------------- nearest neighbours
def sq_dists(Q, D):
    """[nq, nd] fp64: ((dx^2 + dy^2) + dz^2), every operation rounded on its own, of fp32 coordinates widened exactly"""
    Q, D = np.asarray(Q, F32).astype(F64), np.asarray(D, F32).astype(F64)
    dx = Q[:, None, 0] - D[None, :, 0]
    dy = Q[:, None, 1] - D[None, :, 1]
    dz = Q[:, None, 2] - D[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def nearest(Q, D, block=512):
    """(idx int64 [nq], d2 fp64 [nq]) of the nearest row of D for every row of Q; ties to the smaller index (np.argmin takes the first);
    an empty D gives index 0 and an infinite distance"""
    Q, D = np.asarray(Q, F32).reshape(-1, 3), np.asarray(D, F32).reshape(-1, 3)
    nq = Q.shape[0]
    if D.shape[0] == 0:
        return np.zeros(nq, np.int64), np.full(nq, np.inf)
    idx, d2 = np.zeros(nq, np.int64), np.zeros(nq, F64)
    for s in range(0, nq, block):
        m = sq_dists(Q[s:s + block], D)
        i = np.argmin(m, axis=1)
        idx[s:s + block] = i
        d2[s:s + block] = m[np.arange(m.shape[0]), i]
    return idx, d2


def best_two(Q, D, block=512):
    """(best, second best) squared distances per query (second = inf for a one-point D): the margin the golden inputs are conditioned on"""
    Q, D = np.asarray(Q, F32).reshape(-1, 3), np.asarray(D, F32).reshape(-1, 3)
    b, s2 = np.zeros(Q.shape[0]), np.full(Q.shape[0], np.inf)
    for s in range(0, Q.shape[0], block):
        m = np.sort(sq_dists(Q[s:s + block], D), axis=1)
        b[s:s + block] = m[:, 0]
        if m.shape[1] > 1:
            s2[s:s + block] = m[:, 1]
    return b, s2


def check_finite(*clouds):
    for c in clouds:
        if not np.isfinite(np.asarray(c, F32)).all():
            raise ValueError("match_ref: NaN or inf coordinates")


def find_reciprocal_matches(P1, P2):
    """(reciprocal_in_P2 bool [n2], nn2_in_P1 int64 [n2], num_matches, d2 fp64 [n2] of P2's points to their neighbours)"""
    P1, P2 = np.asarray(P1, F32).reshape(-1, 3), np.asarray(P2, F32).reshape(-1, 3)
    check_finite(P1, P2)
    nn1_in_P2, _ = nearest(P1, P2)
    nn2_in_P1, d2 = nearest(P2, P1)
    if P1.shape[0] == 0 or P2.shape[0] == 0:
        return np.zeros(P2.shape[0], bool), nn2_in_P1, 0, d2
    reciprocal_in_P2 = nn1_in_P2[nn2_in_P1] == np.arange(P2.shape[0])
    return reciprocal_in_P2, nn2_in_P1, int(reciprocal_in_P2.sum()), d2


# ------------------------------------------------------------------------------------------------------------------- pair graphs
def scene_graph_pairs(n, scene_graph="complete", prefilter=None, symmetrize=True):
    """the index pairs of the reference's make_pairs, in ascending (i, j) order of the unsymmetrised pairs, then their reverses"""
    if scene_graph == "complete":
        pairs = [(i, j) for i in range(n) for j in range(i)]
    elif scene_graph.startswith("swin"):
        k = int(scene_graph.split("-")[1]) if "-" in scene_graph else 3
        pairs = list({(min(i, (i + j) % n), max(i, (i + j) % n)) for i in range(n) for j in range(1, k + 1)})
    elif scene_graph.startswith("oneref"):
        r = int(scene_graph.split("-")[1]) if "-" in scene_graph else 0
        pairs = [(r, j) for j in range(n) if j != r]
    else:
        raise ValueError(scene_graph)
    pairs = sorted(pairs)
    if prefilter is not None:
        w, cyc = int(prefilter[3:]), prefilter.startswith("cyc")
        dis = lambda i, j: min(abs(i - j), abs(i + n - j), abs(i - n - j)) if cyc else abs(i - j)  # noqa: E731
        pairs = [(i, j) for i, j in pairs if dis(i, j) <= w]
    if symmetrize:
        pairs = pairs + [(j, i) for i, j in pairs]
    return np.asarray(pairs, np.int64).reshape(-1, 2)


# ------------------------------------------------------------------------------------------------------------------- candidates
def quantile_f32(values, q):
    """torch.quantile(values, q) ('linear') of an fp32 array by the project's rule: rank = q (n - 1) in fp32, at::lerp of the two order statistics
    with every operation rounded on its own; NaN with any NaN"""
    v = np.asarray(values, F32).reshape(-1)
    if np.isnan(v).any():
        return F32(np.nan)
    v = np.sort(v)
    rank = F32(q) * F32(v.size - 1)
    lo = np.floor(rank)
    a, b = v[int(lo)], v[int(np.ceil(rank))]
    w = F32(rank - lo)
    d = F32(b - a)
    return F32(a + w * d) if w < F32(0.5) else F32(b - d * F32(F32(1.0) - w))


def candidates(pts, conf=None, mask=None, pct=0, subsample=1):
    """row-major pixel indices (int64) of the candidates of one (H, W, 3) pointmap"""
    H, W = pts.shape[:2]
    keep = np.zeros((H, W), bool)
    keep[::subsample, ::subsample] = True
    if conf is not None:
        with np.errstate(invalid="ignore"):
            keep &= np.asarray(conf, F32) >= quantile_f32(conf, pct / 100.0)
    if mask is not None:
        keep &= np.asarray(mask, bool)
    return np.flatnonzero(keep.reshape(-1))


def match_views(pts, confs=None, masks=None, pairs="complete", pct=0, subsample=1):
    """dict(pairs [P, 2], offsets [P + 1], counts [P], xy_i, xy_j int32 [M, 2] as (x, y), d2 fp64 [M]): per pair what find_reciprocal_matches
    gives on the two candidate sets, matches in ascending candidate order of view j"""
    V = len(pts)
    confs = [None] * V if confs is None else confs
    masks = [None] * V if masks is None else masks
    pix = [candidates(pts[v], confs[v], masks[v], pct, subsample) for v in range(V)]
    cand = [np.asarray(pts[v], F32).reshape(-1, 3)[pix[v]] for v in range(V)]
    if isinstance(pairs, str):
        pairs = scene_graph_pairs(V, pairs, symmetrize=False)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    check_finite(*cand)
    cache, xy_i, xy_j, d2s, counts = {}, [], [], [], []
    for i, j in pairs.tolist():
        if (i, j) not in cache:
            cache[(i, j)] = find_reciprocal_matches(cand[i], cand[j])
        rec, nn2, n, d2 = cache[(i, j)]
        Wi, Wj = pts[i].shape[1], pts[j].shape[1]
        pj, pi = pix[j][rec], (pix[i][nn2[rec]] if n else np.zeros(0, np.int64))
        xy_j.append(np.stack([pj % Wj, pj // Wj], 1))
        xy_i.append(np.stack([pi % Wi, pi // Wi], 1))
        d2s.append(d2[rec])
        counts.append(n)
    cat = lambda parts, shape: np.concatenate(parts) if parts else np.zeros(shape)  # noqa: E731
    return {"pairs": pairs, "offsets": np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), "counts": np.asarray(counts, np.int64),
            "xy_i": cat(xy_i, (0, 2)).astype(np.int32), "xy_j": cat(xy_j, (0, 2)).astype(np.int32), "d2": cat(d2s, (0,)).astype(F64),
            "n_candidates": [len(p) for p in pix]}


def covisibility(res, n_views, max_dist=None):
    out = np.zeros((n_views, n_views), np.int64)
    for p, (i, j) in enumerate(res["pairs"].tolist()):
        d = np.sqrt(res["d2"][res["offsets"][p]:res["offsets"][p + 1]])
        c = len(d) if max_dist is None else int((d <= max_dist).sum())
        out[i, j] += c
        if i != j:
            out[j, i] += c
    return out
