"""Writes fast3r_amd/data/greys_lut_u8.txt (256 grey levels as text: the table is pure grey) and tests/golden/map_cases.npz, and re-checks fast3r_amd/data/turbo_lut_u8.bin (CPU only; needs
matplotlib and PIL -- tool-time dependencies: nothing under fast3r_amd/ imports matplotlib).  `--check` regenerates everything in memory and
compares it with the committed files byte for byte.

The golden is what the reference notebook's plot functions save: matplotlib.pylab.imsave(path, map, cmap='turbo' | 'Greys') on the maps
of tests/map_cases.py, and imsave(path, uint8 image) on its images, each file decoded again to its RGBA bytes.  Stored per picture: the
fp32 input and the (H, W, 4) uint8 bytes.  Asserted here: tests/maps_ref.py reproduces every picture exactly.
Keys: s/<case>/<i>/in, s/<case>/<i>/<cmap>; z/in, z/<cmap> (the z channel of the pointmap); v/<view>/<key>/in (both batch rows) and
v/<view>/<key>/<sample> with key in conf, conf_local, depth_local, img."""
import argparse
import io
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import map_cases as C  # noqa: E402
import maps_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "map_cases.npz")
GREYS = os.path.join(ROOT, "fast3r_amd", "data", "greys_lut_u8.txt")
TURBO = os.path.join(ROOT, "fast3r_amd", "data", "turbo_lut_u8.bin")


def table_bytes(name):
    from matplotlib import colormaps
    cmap = colormaps[name]
    cmap._init()
    return (cmap._lut[:256, :3] * 255).astype(np.uint8).tobytes()


def imsave_rgba(array, **kw):
    """what imsave writes, read back: (H, W, 4) uint8"""
    from matplotlib import pylab
    from PIL import Image
    buf = io.BytesIO()
    pylab.imsave(buf, array, format="png", **kw)
    buf.seek(0)
    out = np.asarray(Image.open(buf).convert("RGBA"))
    assert out.shape == array.shape[:2] + (4,) and out.dtype == np.uint8
    return out


def generate():
    tables = {name: np.frombuffer(table_bytes(name), np.uint8).reshape(256, 3) for name in C.CMAPS}
    out = {}

    def scalar(prefix, a):
        for cmap in C.CMAPS:
            got = imsave_rgba(a, cmap=cmap)
            assert np.array_equal(R.colorize(a, tables[cmap]), got), (prefix, cmap)
            out[f"{prefix}/{cmap}"] = got

    for name, maps in C.scalar_cases().items():
        for i, a in enumerate(maps):
            out[f"s/{name}/{i}/in"] = a
            scalar(f"s/{name}/{i}", a)
    p = C.pointmap_case()
    out["z/in"] = p
    scalar("z", p[..., 2])
    preds, views = C.views_case()
    for v, (pred, view) in enumerate(zip(preds, views)):
        for key, cmap in (("conf", "turbo"), ("conf_local", "turbo"), ("depth_local", "Greys"), ("img", None)):
            src = view["img"] if key == "img" else pred.get("pts3d_local" if key == "depth_local" else key)
            if src is None:
                continue
            out[f"v/{v}/{key}/in"] = src
            for b in range(src.shape[0]):
                if key == "img":    # the notebook's line, then imsave of the uint8 image
                    u8 = ((src[b].transpose(1, 2, 0) + 1) * 127.5).astype(int).clip(0, 255).astype(np.uint8)
                    got = imsave_rgba(u8)
                    assert np.array_equal(R.rgb_picture(src[b]), got), (v, b)
                else:
                    a = src[b][..., 2] if key == "depth_local" else src[b]
                    got = imsave_rgba(a, cmap=cmap)
                    assert np.array_equal(R.colorize(a, tables[cmap]), got), (v, key, b)
                out[f"v/{v}/{key}/{b}"] = got
    return out, tables


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # matplotlib's own lines overflow and meet NaN on the cases made for that
        out, tables = generate()
    turbo = tables["turbo"].tobytes()
    g = tables["Greys"].astype(int)
    assert (g[:, 0] == g[:, 1]).all() and (g[:, 0] == g[:, 2]).all() and g[0, 0] == 255 and g[-1, 0] == 0 and (np.diff(g[:, 0]) <= 0).all()   # pure grey, 255 down to 0
    greys_text = ("# trunc(matplotlib.cm.Greys' 256 table rows * 255): one grey level per entry (R = G = B), 16 entries per line; "
                  "tools/make_golden_maps.py writes and checks it\n"
                  + "".join(" ".join(str(v) for v in g[i:i + 16, 0]) + "\n" for i in range(0, 256, 16)))
    ok = open(TURBO, "rb").read() == turbo
    if args.check:
        ok = ok and os.path.exists(GREYS) and open(GREYS).read() == greys_text
        old = np.load(OUT)
        ok = ok and sorted(old.files) == sorted(out) and all(old[k].dtype == out[k].dtype and old[k].tobytes() == out[k].tobytes() for k in out)
        print("map_cases.npz and both tables reproduced byte for byte" if ok else "map_cases.npz or a table DIFFERS from a fresh generation")
        sys.exit(0 if ok else 1)
    assert ok, "fast3r_amd/data/turbo_lut_u8.bin is not matplotlib's turbo table"
    with open(GREYS, "w") as f:
        f.write(greys_text)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(out)} arrays) and {GREYS}")


if __name__ == "__main__":
    main()
