"""Writes tests/golden/scene_cases.pt and fast3r_amd/data/turbo_lut_u8.bin (CPU only; needs the reference checkout and matplotlib).
`--check` regenerates both in memory and compares them with the committed files bit for bit.

The golden is what the reference's own `start_visualization` (fast3r/viz/viser_visualizer.py), unmodified, does to the scenes of
tests/scene_cases.py, with
* `viser` resolving to the recording stand-in tests/viser_stub.py;
* `threading.Thread` in that module replaced by a no-op (the playback loop never starts);
* `detect_sky_mask` replaced by the recipe's seeded mask (all ones where the recipe has none);
* `np.argsort` in that module wrapped to pass kind='stable';
* `MultiViewDUSt3RLitModule` in that module replaced by a stand-in whose `estimate_camera_poses` returns identity poses and unit focals:
  the scenes include views of a few pixels on which a PnP solve has no meaning, and no pose is recorded;
* real matplotlib; `cv2` resolving to oracle/cv2_stub.py; `imageio` to a permissive stub (GIF rendering is out of scope).
It then fires the GUI handlers to reach each state of scene_cases.STATES and presses "Download PLY".

Stored per scene: the input checksum, the per-view orders (int16 / int32), max_conf_global, is_high_confidence, scene_extent,
is_outdoor, and per state the per-node counts and visibilities and the length and SHA-256 of the PLY (None: nothing to save).  Asserted
here and stored as `restatement_matches`: tests/scene_ref.py reproduces all of it bit for bit, and its extent interpolation equals
np.percentile.  The turbo table is matplotlib's data: trunc(cm.turbo's 256 rows * 255)."""
import argparse
import contextlib
import io
import os
import sys
import types
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import scene_cases as C  # noqa: E402
import scene_ref as R  # noqa: E402
import viser_stub  # noqa: E402
from oracle import cv2_stub, ref_loader  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "scene_cases.pt")
LUT = os.path.join(ROOT, "fast3r_amd", "data", "turbo_lut_u8.bin")


def turbo_bytes():
    from matplotlib import cm
    lut = cm.turbo(np.arange(256))[:, :3]
    return (lut * 255).astype(np.uint8).tobytes()


def load_reference():
    sys.modules["cv2"] = cv2_stub
    v, t = viser_stub.modules()
    sys.modules["viser"], sys.modules["viser.transforms"] = v, t
    ref_loader._STUB_ROOTS = tuple(r for r in ref_loader._STUB_ROOTS if r != "cv2") + (
        "roma", "torchmetrics", "pl_bolts", "open3d", "rerun", "trimesh", "wandb", "imageio")
    ref_loader.install()
    with contextlib.redirect_stdout(io.StringIO()):
        import fast3r.viz.viser_visualizer as vv
    assert vv.viser is v and vv.cv2 is cv2_stub
    real_np = vv.np

    class _Np:
        """the module's `np`, with argsort made stable"""

        def __getattr__(self, name):
            return getattr(real_np, name)

        @staticmethod
        def argsort(a, *args, **kw):
            kw.setdefault("kind", "stable")
            return real_np.argsort(a, *args, **kw)
    vv.np = _Np()
    vv.threading = types.SimpleNamespace(Thread=lambda *a, **k: types.SimpleNamespace(start=lambda: None))

    class _Module:
        @staticmethod
        def estimate_camera_poses(preds, niter_PnP=10, focal_length_estimation_method="individual"):
            n = len(preds)
            return [[np.eye(4) for _ in range(n)]], [[1.0 for _ in range(n)]]
    vv.MultiViewDUSt3RLitModule = _Module
    vv.tqdm = lambda x, *a, **k: x
    return vv


def set_state(server, st, is_outdoor, num_frames):
    """fire the reference's handlers so that the GUI ends in state `st` (scene_cases.STATE_KEYS)"""
    g = server.gui.handles
    g["High/Low Conf Threshold"].value = st["threshold"]
    g["Global"].value = st["show_global"]
    g["Local"].value = st["show_local"]
    if st["color"] == "rgb":
        g["Show Confidence"].value = False
        g["Color by View"].value = False
    elif st["color"] == "confidence":
        g["Color by View"].value = False
        g["Show Confidence"].value = True
    else:
        g["Show Confidence"].value = False
        g["Color by View"].value = True
    g["Mask Sky"].value = is_outdoor if st["mask_sky"] is None else st["mask_sky"]
    g["Per-View Conf Percentile"].value = st["percentile"]
    g["Timestep"].value = num_frames - 1 - st["back"]
    assert not (st["show_high_conf"] and st["show_low_conf"])
    if st["show_low_conf"]:
        g["Show High-Conf Views"].value = False
        g["Show Low-Conf Views"].value = True
    else:
        g["Show Low-Conf Views"].value = False
        g["Show High-Conf Views"].value = st["show_high_conf"]


def record(server, num_frames):
    nodes = server.scene.nodes
    client = viser_stub.Client()
    with contextlib.redirect_stdout(io.StringIO()):
        server.gui.handles["Download PLY"].click(client)
    ply = client.downloads[-1][1] if client.downloads else None
    counts, visible = [], []
    for i in range(num_frames):
        for head in ("global", "local"):
            n = nodes[f"/pts3d_{head}/t{i}"]
            counts.append(len(n.points))
            visible.append(bool(n.visible))
    return {"counts": counts, "visible": visible, "ply": R.digest(ply)}


def run_scene(vv, name, lut_u8):
    scene = C.build(name)
    V = len(scene["preds"])
    masks = scene["masks"] or [np.ones(s, np.int8) for s in scene["shapes"]]
    use_ref = C.SCENES[name].get("reference", True)
    server = None
    if use_ref:
        it = iter(masks)
        vv.detect_sky_mask = lambda img: next(it)
        with contextlib.redirect_stdout(io.StringIO()):
            server = vv.start_visualization(C.single_sample(scene))
        nodes = server.scene.nodes
    # the orders: the reference keeps only the sorted arrays, so they come from the restatement, which the PLY hashes below pin on it
    s = scene["sample"]
    out = {"checksum": C.checksum(scene), "shapes": scene["shapes"], "orders": [], "max_conf_global": [], "is_high_confidence": [], "states": {}}
    frames = []
    for i in range(V):
        pred = {k: v[s].numpy() for k, v in scene["preds"][i].items()}
        view = {"img": scene["views"][i]["img"][s].numpy()}
        fd = R.frame_data(pred, view, masks[i], i, V, C.DEFAULT_THRESHOLD, lut_u8)
        frames.append(fd)
        n = len(fd["order_global"])
        dt = torch.int16 if n <= 32767 else torch.int32
        out["orders"].append({h: torch.from_numpy(fd[f"order_{h}"].astype(np.int64)).to(dt) for h in ("global", "local")})
    # the initial state: every view shown whatever its confidence, no percentile cut, the sky mask where the scene is outdoor
    outdoor = bool(server.gui.handles["Mask Sky"].value) if use_ref else bool(R.is_outdoor(frames))
    assert outdoor == R.is_outdoor(frames), name
    # the reference's frame_data is not reachable from outside; its nodes are: in the initial state (mask off) they hold the sorted arrays
    if use_ref and not outdoor:
        for i in range(V):
            for h in ("global", "local"):
                n = nodes[f"/pts3d_{h}/t{i}"]
                assert np.array_equal(n.points, frames[i][f"sorted_pts3d_{h}"], equal_nan=True), (name, i, h)
                assert np.array_equal((np.asarray(n.colors) * 255).astype(np.uint8), frames[i][f"colors_rgb_{h}"]), (name, i, h)
    out["is_outdoor"] = outdoor
    states = {"initial": dict(zip(C.STATE_KEYS, (0, None, "rgb", False, True, True, True, 0, C.DEFAULT_THRESHOLD)))}
    for j, st in enumerate(C.STATES):
        states[f"s{j:02d}"] = dict(zip(C.STATE_KEYS, st))
    ok = True
    for key, st in states.items():
        if use_ref:
            if key != "initial":
                set_state(server, st, outdoor, V)
            rec = record(server, V)
        mask_sky = outdoor if st["mask_sky"] is None else st["mask_sky"]
        p, c, counts = R.collect(frames, percentile=st["percentile"], mask_sky=mask_sky, color=st["color"], show_global=st["show_global"],
                                 show_local=st["show_local"], show_high_conf=st["show_high_conf"], show_low_conf=st["show_low_conf"],
                                 upto=V - 1 - st["back"], threshold=st["threshold"])
        mine = R.digest(None if p is None else R.ply_bytes(p, c))
        if not use_ref:
            rec = {"counts": counts, "visible": None, "ply": mine}
        assert mine == rec["ply"], (name, key, mine, rec["ply"])
        assert counts == rec["counts"], (name, key)
        ok = ok and mine == rec["ply"] and counts == rec["counts"]
        out["states"][key] = dict(rec, state=st)
    # max_conf_global is np.max of the input; the states that show one confidence class alone pin is_high_confidence on the reference
    for i in range(V):
        with np.errstate(invalid="ignore"):
            out["max_conf_global"].append(float(scene["preds"][i]["conf"][s].numpy().max()))
        assert np.float64(out["max_conf_global"][-1]).tobytes() == np.float64(frames[i]["max_conf_global"]).tobytes()
        out["is_high_confidence"].append(bool(out["max_conf_global"][-1] >= C.DEFAULT_THRESHOLD))
    allp = np.concatenate([scene["preds"][i]["pts3d_in_other_view"][s].numpy().reshape(-1, 3) for i in range(V)], axis=0)
    with np.errstate(invalid="ignore"):
        ext = np.percentile(allp, 80, axis=0) - np.percentile(allp, 20, axis=0)
    mine = R.scene_extent([f["sorted_pts3d_global"] for f in frames])
    assert ext.dtype == mine.dtype == np.float32 and ext.tobytes() == mine.tobytes(), (name, ext, mine)
    out["scene_extent"] = torch.from_numpy(ext.copy())
    out["reference"] = use_ref
    out["restatement_matches"] = ok
    out["extent_matches_np_percentile"] = True
    return out


def run_ply_cases(vv):
    out = {}
    for name in C.PLY_CASES:
        pts, col = C.ply_case(name)
        ref = vv.generate_ply_bytes(pts, col)
        assert ref == R.ply_bytes(pts, col), name
        out[name] = R.digest(ref)
    # the rgb round trip: uint8 -> / 255.0 -> safe_color_conversion is the identity for all 256 values
    u = np.arange(256, dtype=np.uint8)
    assert np.array_equal(vv.safe_color_conversion(u / 255.0), u)
    return out


def generate():
    warnings.filterwarnings("ignore")
    vv = load_reference()
    lut = turbo_bytes()
    lut_u8 = np.frombuffer(lut, np.uint8).reshape(256, 3)
    data = {"tile": C.T, "scenes": {name: run_scene(vv, name, lut_u8) for name in C.SCENES}, "ply": run_ply_cases(vv), "rgb_round_trip": True}
    return data, lut


def same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and bool(
            (a.contiguous().view(-1).view(torch.uint8) == b.contiguous().view(-1).view(torch.uint8)).all())
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, float):
        return isinstance(b, float) and np.float64(a).tobytes() == np.float64(b).tobytes()
    return a == b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="regenerate in memory and compare with the committed files bit for bit")
    args = ap.parse_args()
    data, lut = generate()
    if args.check:
        ok = same(data, torch.load(OUT, weights_only=False)) and open(LUT, "rb").read() == lut
        print("scene_cases.pt and turbo_lut_u8.bin reproduced bit for bit" if ok else "scene_cases.pt or turbo_lut_u8.bin DIFFERS from a fresh generation")
        sys.exit(0 if ok else 1)
    os.makedirs(os.path.dirname(LUT), exist_ok=True)
    with open(LUT, "wb") as f:
        f.write(lut)
    torch.save(data, OUT)
    size = os.path.getsize(OUT)
    assert size < 500 * 1000, size
    print(f"wrote {OUT} ({size} bytes) and {LUT} ({len(lut)} bytes)")


if __name__ == "__main__":
    main()
