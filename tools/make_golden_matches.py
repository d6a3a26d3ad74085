"""Writes tests/golden/matches_cases.npz (CPU only; needs the reference checkout and scipy).  `--check` regenerates it in memory and compares
it with the committed file array for array.

The golden is what the reference's own `find_reciprocal_matches` (fast3r/dust3r/utils/geometry.py:381-397, two cKDTrees) returns on seeded
inputs -- three noisy surface patches seen from shifted poses and two unrelated random clouds (tests/match_cases.py) -- and the index pairs
its `make_pairs` (fast3r/dust3r/image_pairs.py:17-47) forms for every graph string and prefilter at n = 1, 2, 5, 8.  Only data: arrays and
index lists.

Condition on the inputs, asserted here: for every query the second-best squared distance exceeds the best by a relative 1e-9 (brute force,
fp64), which keeps cKDTree's tree-order tie-breaking and last-bit differences out of an index comparison.  A seed that fails is replaced by
the next one, never dropped; the file stores the seed used and `margins_ok`.  Also asserted: tests/match_ref.py reproduces every stored
array exactly (`restatement_matches`)."""
import argparse
import contextlib
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import match_cases as C  # noqa: E402
import match_ref as R  # noqa: E402
from oracle import ref_loader  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "matches_cases.npz")
MARGIN = 1e-9


def margins_ok(A, B):
    """every query of A in B and of B in A has a second-best squared distance beyond (1 + MARGIN) x the best"""
    for Q, D in ((A, B), (B, A)):
        best, second = R.best_two(Q.reshape(-1, 3), D.reshape(-1, 3))
        if not (second > best * (1.0 + MARGIN)).all():
            return False
    return True


def cloud_pairs(patches, clouds):
    return [("patch01", patches[0], patches[1]), ("patch12", patches[1], patches[2]), ("patch20", patches[2], patches[0]),
            ("clouds", clouds[0], clouds[1])]


def generate():
    ref_loader.install()
    with contextlib.redirect_stdout(io.StringIO()):
        from fast3r.dust3r.image_pairs import make_pairs
        from fast3r.dust3r.utils.geometry import find_reciprocal_matches
    seed = 1
    while True:
        patches, clouds = C.golden_inputs(seed)
        if all(margins_ok(a, b) for _, a, b in cloud_pairs(patches, clouds)):
            break
        seed += 1  # reseeded, never dropped
    data = {"seed": np.int64(seed), "margins_ok": np.bool_(True), "margin": np.float64(MARGIN)}
    for k, p in enumerate(patches):
        data[f"patch{k}"] = p
    for k, c in enumerate(clouds):
        data[f"cloud{k}"] = c
    for name, a, b in cloud_pairs(patches, clouds):
        P1, P2 = a.reshape(-1, 3), b.reshape(-1, 3)
        rec, nn2, num = find_reciprocal_matches(P1, P2)
        data[f"{name}_reciprocal_in_P2"] = np.asarray(rec, bool)
        data[f"{name}_nn2_in_P1"] = np.asarray(nn2, np.int64)
        data[f"{name}_num_matches"] = np.int64(num)
        mine = R.find_reciprocal_matches(P1, P2)
        assert np.array_equal(mine[0], data[f"{name}_reciprocal_in_P2"]) and np.array_equal(mine[1], data[f"{name}_nn2_in_P1"]) and mine[2] == num, name
    for n in C.GRAPH_SIZES:
        imgs = [{"idx": i} for i in range(n)]
        for g in C.GRAPHS:
            for f in C.PREFILTERS:
                for sym in (False, True):
                    if g.startswith("oneref-") and int(g.split("-")[1]) >= n:
                        continue  # the reference indexes imgs[refid]
                    if f is not None and not make_pairs(imgs, g, None, sym):
                        continue  # the reference's prefilter takes max() over the edges: no pair list to record for an empty graph
                    got = np.asarray([(a["idx"], b["idx"]) for a, b in make_pairs(imgs, g, f, sym)], np.int64).reshape(-1, 2)
                    data[f"pairs_n{n}_{g}_{f}_{int(sym)}"] = got
                    mine = R.scene_graph_pairs(n, g, f, sym)
                    if g.startswith("swin"):  # the reference walks a set: compared as sets, and the symmetrised half as the mirrored set
                        assert sorted(map(tuple, got.tolist())) == sorted(map(tuple, mine.tolist())), (n, g, f, sym)
                    else:
                        assert np.array_equal(got, mine), (n, g, f, sym, got, mine)
    data["restatement_matches"] = np.bool_(True)
    return data


def same(a, b):
    return sorted(a) == sorted(b) and all(np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.array_equal(a[k], b[k]) for k in a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="regenerate in memory and compare with the committed file array for array")
    args = ap.parse_args()
    data = generate()
    n_pairs = sum(k.startswith("pairs_") for k in data)
    print(f"seed {int(data['seed'])}: margins hold; tests/match_ref.py reproduces the reference on 4 cloud pairs and {n_pairs} pair lists")
    if args.check:
        with np.load(OUT) as f:
            ok = same(data, {k: f[k] for k in f.files})
        print("matches_cases.npz reproduced array for array" if ok else "matches_cases.npz DIFFERS from a fresh generation")
        sys.exit(0 if ok else 1)
    np.savez_compressed(OUT, **data)
    size = os.path.getsize(OUT)
    assert size < 1000 * 1000, size
    print(f"wrote {OUT} ({size} bytes)")


if __name__ == "__main__":
    main()
