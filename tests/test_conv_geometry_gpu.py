"""The 3x3 implicit-GEMM convolution at the edges of its geometry, on a real MI355X through the C ABI: images narrower or shorter than the kernel,
output tiles that hold many whole images and a ragged end, stride 2 at both parities, channel tails of the 128-tile kernel, persistent
workgroups that walk a second tile, and the K-tile table guard of the 256-tile kernel (cases and float64 references: tests/conv_cases.py).

Every case runs on every kernel form that accepts it and is held to the tolerance the project already uses for that kind of output: lowp outputs
lp_tol, hi + lo planes of x3 split_tol, x3f8 against its decoded planes 2e-6, the fused tail against float64 as in
test_fused_head_tail_matches_the_separate_kernels.  Every operand plane lies inside a larger buffer of NaN patterns and every output inside a
buffer of sentinel words: a load before or behind a plane poisons the result, a store outside the M x N outputs changes a sentinel.
"""
import pytest
import torch

import conv_cases as cc
from conv_cases import H16
from fast3r_amd import ops
from test_gemm256_gpu import split_tol
from test_kernels_gpu import DEV, lp_tol

pytestmark = pytest.mark.gpu


def check(kind, got, ref, tol, what):
    """test_kernels_gpu.assert_close, with the figure printed before it is asserted"""
    got, ref = got.detach().double().cpu(), ref.double()
    scale = float(ref.abs().max().clamp_min(1e-6))
    err = float((got - ref).abs().max())
    print(f"[conv-geometry] kind={kind} rel_err={err / scale:.3e} tol={tol:.1e} {what}")
    assert err == err and err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (tol {tol:.1e})"


class Launcher:
    """the device tensors of a case, in guarded placement, and its launches"""

    def __init__(self, c):
        self.c, self.d = c, cc.build(c)
        d, B = self.d, c.B
        margin = (c.W + 2) * c.Ci * 2   # an image row and two pixels of a plane, in bytes (a pixel of the fp8 planes is 2 C bytes as well)
        self.keep = []

        def place(t):
            if t is None:
                return None
            view, buf = cc.guarded_operand(cc.periodic(t, B), DEV, margin)
            self.keep.append(buf)
            return view

        self.x, self.x_lo, self.x_f8 = place(d["x"]), place(d["x_lo"]), place(d["x_f8"])
        self.w = d["w"].to(DEV)
        self.kw = dict(stride=c.stride, bias=None if d["bias"] is None else d["bias"].to(DEV), a_relu="a_relu" in c.extras)
        if c.split == "x3":
            self.kw.update(split="x3", x_lo=self.x_lo)
        elif c.split == "x3f8":
            self.kw.update(split="x3f8", x_f8=self.x_f8, w_scale=d["w_scale"].to(DEV))
        if d["res"] is not None:
            (r1, r1lo), (r2, r2lo) = [[None if t is None else cc.periodic(t, B).to(DEV) for t in pair] for pair in d["res"]]
            self.kw.update(res_lp=r1, res_lp2=r2, res_lp_lo=r1lo, res_lp2_lo=r2lo, want_relu=True)
        self.fin = None
        if d["fin"] is not None:
            w4, b4, conf_mode = d["fin"]
            self.fin = ops.dpt_fin_args(w4.to(DEV), b4.to(DEV), conf_mode)
        self.ref = {k: cc.periodic(v, B) for k, v in d["ref"].items()}

    def run(self, sel):
        """-> {"out": the output planes summed in float64 [, "relu"]} or {"pts", "conf"}, and the raw tensors for bit comparisons"""
        c = self.c
        if self.fin is not None:
            pts, conf = ops.conv3x3(self.x, self.w, act="relu", fin=self.fin, kernel_sel=sel, **self.kw)
            return dict(pts=pts, conf=conf), [pts, conf]
        oh, ow = c.out_hw
        out, buf, lo, hi = cc.guarded_out((c.B, oh, ow, c.Co), c.dtype, DEV)
        r = ops.conv3x3(self.x, self.w, out=out, want_lo=c.split is not None, kernel_sel=sel, **self.kw)
        torch.cuda.synchronize()
        assert cc.guards_intact(buf, lo, hi), f"{c.id} sel={sel}: a store outside the {c.M} x {c.Co} outputs"
        if not isinstance(r, dict):
            r = dict(out=r)
        assert r["out"].data_ptr() == out.data_ptr()
        got = {}
        for name in ("out", "relu"):
            if name in r:
                got[name] = r[name].double() + r[name + "_lo"].double() if name + "_lo" in r else r[name].double()
        return got, [r[k] for k in sorted(r)]

    def tol(self, name):
        c = self.c
        if name in ("pts", "conf"):   # as test_fused_head_tail_matches_the_separate_kernels; x3f8 against its planes: the fp16 figure
            if c.split == "x3":
                return 2e-4 if c.dtype == torch.bfloat16 else 3e-5
            return 3e-5 if (c.split == "x3f8" or name == "conf") else 2e-5
        return {None: lp_tol(c.dtype), "x3": split_tol(c.dtype), "x3f8": 2e-6}[c.split]

    def kind(self, name):
        dt = "f16" if self.c.dtype == H16 else "bf16"
        return f"{'fin' if name in ('pts', 'conf') else 'conv'}-{self.c.split or 'one'}-{dt}"


def _run_forms(L, sels):
    """every form runs and prints its figures -> (raw outputs by form, the misses)"""
    raws, missed = {}, []
    for sel in sels:
        got, raws[sel] = L.run(sel)
        for name, g in got.items():
            if g is not None:
                try:
                    check(L.kind(name), g, L.ref[name], L.tol(name), f"{L.c.id} {name} sel={sel}")
                except AssertionError as e:
                    missed.append(str(e).splitlines()[0])
    return raws, missed


def _run_all_forms(c):
    _, missed = _run_forms(Launcher(c), cc.kernel_sels(c))
    assert not missed, "; ".join(missed)


@pytest.mark.parametrize("c", cc.TINY, ids=lambda c: c.id)
def test_tiny_images(built_lib, c):
    """H, W of 1 .. 5: the tap offsets alias the centre pixel or another row and only the mask keeps them out; tiles of many whole images, rows
    past M"""
    _run_all_forms(c)


@pytest.mark.parametrize("c", cc.STRIDE2, ids=lambda c: c.id)
def test_stride_2_parities(built_lib, c):
    _run_all_forms(c)


@pytest.mark.parametrize("c", cc.TAILS, ids=lambda c: c.id)
def test_128_tile_channel_tails(built_lib, c):
    _run_all_forms(c)


N_SECOND = len(cc.second_tile_cases(cc.CU_NOMINAL))


@pytest.mark.parametrize("i", range(N_SECOND), ids=[c.id for c in cc.second_tile_cases(cc.CU_NOMINAL)])   # (ids: at the nominal CU count)
def test_second_tile_of_a_persistent_workgroup(built_lib, i):
    """more tiles than CUs: the first workgroups compute a second tile whose opening loads were issued before the first one's epilogue (and, with
    the fused tail, beside its partials parked in K-tile buffer 2).  The one-tile-per-workgroup grid (kernel_sel 5) runs the same instructions per
    tile: its output must be the same bits."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    c = cc.second_tile_cases(n_cu)[i]
    if cc.period_hides_a_stale_tile(c, n_cu):
        pytest.skip(f"content of period {c.P} on {n_cu} CUs: a stale tile would carry identical content")
    assert cc.tiles(c, 256 if c.Co == 256 else 128) >= n_cu + 4
    L = Launcher(c)
    one_tile = c.split != "x3f8"   # (kernel_sel 5 on the fused-tail x3f8 launch is another schedule, a measurement form)
    raws, missed = _run_forms(L, cc.kernel_sels(c) + ([5] if one_tile else []))
    if one_tile:
        for a, b in zip(raws[2] if 2 in raws else raws[0], raws[5]):
            assert (a is None and b is None) or torch.equal(a, b), f"{c.id}: the persistent grid and one tile per workgroup differ"
    assert not missed, "; ".join(missed)


def _needs_guard(lib):
    """(host side) the library under test has the K-tile table guard: without it the launches below would read table records nobody wrote"""
    assert lib._Z28f3r_gemm256_max_conv_k_tilesv() == cc.TAB_ENTRIES


def test_k_tile_table_guard_falls_back_or_raises(built_lib):
    _needs_guard(built_lib)
    c = cc.GUARD_OVER_X3   # 513 records
    assert cc.k_tiles(c) == cc.TAB_ENTRIES + 1
    L = Launcher(c)
    _, missed = _run_forms(L, [0, 1])   # 0 = by shape: the 128-tile kernel
    assert not missed, "; ".join(missed)
    for sel in (2, 3, 4, 5):
        with pytest.raises(ValueError, match="not eligible"):
            L.run(sel)
    f8 = Launcher(cc.GUARD_OVER_F8)
    with pytest.raises(ValueError, match="K-tiles"):
        f8.run(0)
    fin = Launcher(cc.ConvCase(1, 8, 8, 1216, 128, 1, "x3", H16, ("bias", "fin")))
    with pytest.raises(ValueError, match="K-tiles"):
        fin.run(0)


@pytest.mark.parametrize("sel", [1, 2, 3, 4, 0])
def test_k_tile_table_full(built_lib, sel):
    _needs_guard(built_lib)
    """x3 at C = 1152: 486 of the 512 records, the largest x3 shape the 256-tile kernel takes, and the longest sum it forms (3 x 10 368 products).
    fp32-class only because the kernel adds the bias behind the K loop: started at the bias the same sum ended at 3.6e-6 of the output scale,
    above split_tol; summed from zero it gives the 128-tile kernel's 2.4e-6 (of which 1.4e-6 are the planes: the fp16 low plane of weights of size
    (9 C)^-1/2 is subnormal)."""
    c = cc.GUARD_FITS_X3
    assert sel in cc.kernel_sels(c)
    _, missed = _run_forms(Launcher(c), [sel])
    assert not missed, "; ".join(missed)
