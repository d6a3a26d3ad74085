"""The workspaces of the post-processing entry points: what the sizing functions return is pinned (tests/golden/workspace_bytes.json,
recorded by tools/record_workspace_bytes.py before the sizes and the layouts were made one function each), and the carver they are
built on (fast3r_amd/csrc/f3r_carve.h) is run on the host under AddressSanitizer and UBSan.  No GPU needed: all of it is host code."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_every_sizing_function_returns_the_recorded_bytes(built_lib):
    import record_workspace_bytes as R
    want = json.load(open(R.GOLDEN))
    assert set(want) == set(R.cases()) and len(want) == 11
    got = R.measure(built_lib)
    for name in want:
        assert len(want[name]) == len(R.cases()[name]) >= 1
        for (args, expect), (args_now, now) in zip(want[name], got[name]):
            assert args == args_now and now == expect, (name, args, now, expect)
    # the recording covers what it is there for: both sides of every boundary, both sky layouts, both mesh layouts, the refusals
    assert {a[0] for a, _ in want["f3r_recon_stats_workspace_bytes"]} >= {1, 63, 64, 65, 255, 256, 257, 4096, 4097, 2 ** 20, 0, -1}
    assert {a[3] & 4 for a, _ in want["f3r_sky_workspace_bytes"]} == {0, 4} and {a[3] for a, _ in want["f3r_mesh_workspace_bytes"]} == {0, 1}
    for name in want:
        if name != "f3r_scene_extent_workspace_bytes":
            assert any(b == 0 for _, b in want[name]) and any(b > 0 for _, b in want[name]), name


def test_carver_sizes_and_carves_alike_under_sanitizers(tmp_path):
    """tests/csrc/carve_host.cpp: for region lists with zero-sized regions and alignments 8 and 256, the carve pass ends at the sized total,
    every pointer is aligned, and writing every byte of every region of a block of exactly that size trips neither sanitizer"""
    exe = str(tmp_path / "carve_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "csrc", "carve_host.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "regions ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
