"""Records what every workspace-sizing function of libf3r_hip.so returns, `args -> bytes`, into tests/golden/workspace_bytes.json.
These functions are pure host code (no GPU needed).  tests/test_workspace_bytes.py asserts that the built library still returns the
recorded numbers: a sizing function and the layout that carves the workspace must not drift apart unnoticed.

    python tools/record_workspace_bytes.py [path/to/libf3r_hip.so]      # default: the in-tree library

Re-record only when a workspace layout changes on purpose.
"""
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "workspace_bytes.json")

COUNTS = [1, 63, 64, 65, 255, 256, 257, 4096, 4097, 2 ** 20]   # both sides of every alignment and tile boundary
BAD = [0, -1]                                                  # must give 0
SMALL = [1, 2, 3, 8, 31, 32, 33, 64, 65]                       # views / samples / problems


def cases():
    """{function: [argument tuples]}"""
    one = [(n,) for n in COUNTS + BAD]
    tiles = [1, 2, 257]
    out = {
        "f3r_scene_sort_workspace_bytes": [(n, t) for n in COUNTS for t in tiles] + [(0, 1), (-1, 1), (1, 0), (1, -1)],
        "f3r_scene_extent_workspace_bytes": [()],
        "f3r_nn_index_bytes": one,
        "f3r_nn_workspace_bytes": one,
        "f3r_recon_stats_workspace_bytes": one,
        "f3r_recon_prepare_workspace_bytes": [(b, v, n) for b in (1, 3) for v in (1, 2, 33) for n in COUNTS]
        + [(0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1), (1, -1, 1), (1, 1, -1)],
        "f3r_sky_workspace_bytes": [(w, 64 * w - 1, max(1, w // 2), st) for w in COUNTS for st in (1, 2, 3, 4, 6, 7)]
        + [(0, 1, 1, 7), (-1, 1, 1, 7), (1, 0, 1, 7), (1, -1, 1, 7), (1, 1, 0, 7), (1, 1, -1, 7), (1, 1, 1, 0), (1, 1, 1, 8)],
        "f3r_mesh_workspace_bytes": [(max(1, n // 1024), t, n, d) for n in COUNTS for t in tiles for d in (0, 1)]
        + [(n, 3, 1024 * n, d) for n in COUNTS[:9] for d in (0, 1)]
        + [(0, 1, 1, 0), (-1, 1, 1, 0), (1, 0, 1, 1), (1, -1, 1, 1), (1, 1, 0, 0), (1, 1, -1, 1)],
        "f3r_mv_conf_loss_workspace_bytes": list(itertools.product(SMALL, SMALL)) + [(1, n) for n in COUNTS] + [(n, 1) for n in COUNTS]
        + [(2048, 2048), (2049, 2048), (0, 1), (-1, 1), (1, 0), (1, -1)],   # 2^22 segments is the most the loss takes
        "f3r_align_workspace_bytes": one + [(n,) for n in SMALL],
        "f3r_focal_workspace_bytes": [(v, h, w) for v in (1, 2, 33) for h, w in ((1, 1), (7, 9), (63, 65), (224, 224), (512, 384))]
        + [(n, 7, 9) for n in COUNTS] + [(1, n, 1) for n in COUNTS] + [(1, 1, n) for n in COUNTS]
        + [(0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, 0), (1, -1, 8), (1, 8, -1)],
    }
    return out


def measure(lib):
    return {name: [[list(a), int(getattr(lib, name)(*a))] for a in args] for name, args in cases().items()}


def main():
    from fast3r_amd import _lib
    if len(sys.argv) > 1:
        _lib.LIB_PATH = os.path.abspath(sys.argv[1])
    rec = measure(_lib.lib())
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(f'"{k}": {json.dumps(v, separators=(",", ":"))}' for k, v in rec.items()) + "\n}\n")
    print(f"wrote {GOLDEN}: {sum(len(v) for v in rec.values())} cases of {len(rec)} functions")


if __name__ == "__main__":
    main()
