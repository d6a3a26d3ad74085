"""The grouped-barrier form of the hand-scheduled attention kernel without a GPU: AttnGen(tiles_per_barrier=G, pf=..., nslot=8) of
fast3r_amd/csrc/asm/attn_gen.py meets at one s_barrier per G key tiles instead of one per tile.  The arithmetic per wave is unchanged, so on the
same operands its output must be BIT-IDENTICAL to the G = 1 kernel's.  tools/gfx950_emu.py runs the waves of a workgroup one after the other
between barriers and lands LDS-DMA data only at the issuing wave's vmcnt wait -- the largest skew the grouped form allows -- so a wait count or a
ring rule that is off shows as different numbers (the negative control below removes one tile from the wait and sees them).

The ring rules themselves (attn_gen.py header, "The LDS ring") are restated here as a model: waves anywhere between two barriers, a tile live from
the barrier after which it may be read to the last read of it.  The constructor must accept a (G, pf, nslot) triple exactly when the model finds
neither an overwrite of a live slot nor a read of a tile some wave has not waited for."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "fast3r_amd", "csrc", "asm"))

# every (G, pf) on the 8-slot ring that profiles/attn_grouped_barrier_ab.jsonl measures; the library ships attn_gen.GROUPED_RING
SETTINGS = [(2, 3), (2, 4), (2, 5), (2, 6), (3, 4), (3, 5)]
TOL = {"f16": 6e-4, "bf16": 5e-3}   # the bars of tests/test_attn_asm_emu.py against the float64 softmax

_plain = {}   # the G = 1 kernel's output per case, computed once


def _run(gen, dtype="f16", **kw):
    import emu_attn
    outs = []
    kw.setdefault("n_heads", 1)
    kw.setdefault("wgs", ((0, 0, 0),))
    err = emu_attn.run_case(dtype, gen_kwargs=gen, outs=outs, **kw)
    return err, outs


def _same_bits(G, pf, dtype="f16", **kw):
    key = (dtype, repr(sorted(kw.items())))
    if key not in _plain:
        _plain[key] = _run(None, dtype, **kw)
    err1, plain = _plain[key]
    err, got = _run(dict(tiles_per_barrier=G, pf=pf, nslot=8), dtype, **kw)
    assert err1 < TOL[dtype] and err < TOL[dtype], (err1, err)
    assert len(got) == len(plain) and len(got) > 0
    for a, b in zip(plain, got):
        assert a.dtype == np.uint16 and np.array_equal(a, b), f"G={G} pf={pf}: {int((a != b).sum())} of {a.size} output words differ from the G = 1 kernel"


def _shipped():
    import attn_gen
    r = attn_gen.GROUPED_RING
    assert r["nslot"] == 8 and (r["tiles_per_barrier"], r["pf"]) in SETTINGS
    return r["tiles_per_barrier"], r["pf"]


# ---------------------------------------------------------------------------------------------- bit identity with the G = 1 kernel
@pytest.mark.parametrize("tiles", [1, 2, 3, 5, 8, 9, 11, 19])
@pytest.mark.parametrize("G,pf", SETTINGS)
def test_grouped_kernel_is_bit_identical_over_tile_counts(G, pf, tiles):
    """every remainder mod G (2 and 3), fewer tiles than one group, than the ring fill, and 19 >= 2 * 8 + G: the 8-slot ring wraps more than twice"""
    _same_bits(G, pf, n_tiles=tiles, spike=True)


@pytest.mark.parametrize("G,pf", SETTINGS)
@pytest.mark.parametrize("tiles", [(1, 2, 1), (1, 1, 1, 1, 1, 1, 1, 1)])
def test_grouped_kernel_walks_segments(G, pf, tiles):
    """segment hops in the LDS-DMA stream fall on every position inside a group"""
    _same_bits(G, pf, n_tiles=list(tiles), spike=True)


@pytest.mark.parametrize("G,pf", SETTINGS)
def test_grouped_kernel_parks_and_resumes_its_state(G, pf):
    """two launches of 3 and 6 tiles with the online-softmax state parked in between: the tile count, and with it the group, starts again per launch"""
    _same_bits(G, pf, n_tiles=[3, 6], split_state=True, spike=True)


@pytest.mark.parametrize("G,pf", SETTINGS)
@pytest.mark.parametrize("tq,wg", [(600, (1, 0, 0)), (1000, (1, 0, 0))])
def test_grouped_kernel_partial_last_workgroup(G, pf, tq, wg):
    """waves re-aimed at the last query rows still walk every tile: the barrier of every G-th tile stays uniform over the workgroup (a wave that left
    would leave the others at a barrier nobody else reaches: the emulator's deadlock, or rows nobody wrote)"""
    _same_bits(G, pf, n_tiles=5, tq=tq, wgs=(wg,), spike=True)


def test_grouped_kernel_work_stealing_form():
    """steal = 2: a persistent workgroup re-enters the prologue per item (every item enters the unrolled loop at tile 0) and the FETCH block's barriers stand
    between two items' rings"""
    G, pf = _shipped()
    _same_bits(G, pf, n_tiles=5, tq=1024, n_heads=2, wgs=((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)), steal=2)
    _same_bits(3, 4, n_tiles=4, tq=700, n_heads=1, wgs=((0, 0, 0), (1, 0, 0)), steal=2)


@pytest.mark.parametrize("G,pf", SETTINGS)
@pytest.mark.parametrize("tiles", [3, 10])
def test_grouped_kernel_bf16(G, pf, tiles):
    _same_bits(G, pf, dtype="bf16", n_tiles=tiles, spike=True)


def test_grouped_kernel_batch_gqa_and_second_query_block():
    G, pf = _shipped()
    _same_bits(G, pf, n_tiles=4, n_heads=4, wgs=((1, 3, 1), (0, 0, 0)), batch=2, kv_shift=1, q_blocks=2)


def test_emulator_sees_a_wait_that_is_one_tile_short(monkeypatch):
    """negative control: the grouped kernel with NP added to the vmcnt in front of its loop barrier (one tile fewer waited for) must NOT reproduce
    the G = 1 kernel's output -- what makes the bit comparisons above a test of the wait counts"""
    import attn_gen
    import isa
    build = attn_gen.AttnGen.build

    def short(self):
        p = build(self)
        if self.G > 1:
            at = [i for i, it in enumerate(p.items) if isinstance(it, isa.Ins) and it.op == "s_barrier" and isinstance(p.items[i - 1], isa.Ins)
                  and p.items[i - 1].op == "s_waitcnt" and str(p.items[i - 1].args[0]).startswith("vmcnt") and "pieces of tiles" in (p.items[i - 1].comment or "")]
            assert len(at) == 1
            w = p.items[at[0] - 1]
            p.items[at[0] - 1] = isa.Ins("s_waitcnt", (f"vmcnt({self.NP * (self.pf - self.G)})",), {}, w.comment)
        return p
    monkeypatch.setattr(attn_gen.AttnGen, "build", short)
    with pytest.raises(AssertionError):
        _same_bits(2, 4, n_tiles=9, spike=True)


# ---------------------------------------------------------------------------------------------- the ring rules as a model
def ring_violations(G, pf, nslot, wait, n_tiles, strict=False):
    """Tiles 0 .. n_tiles - 1; a barrier at the boundary of every tile b that is a multiple of G (the prologue's is b = 0).  A wave issues the LDS-DMA of
    tile x (slot x % nslot) while it computes tile x - pf, tiles < pf before the first barrier, and keeps issuing past the last tile (the re-issued
    tail).  In front of a barrier it waits until at most `wait` of the tiles it has issued are outstanding.  Between the barrier of tile b and the next
    one a wave may be in any tile ts of the group and any other wave in any tile tf >= ts of it.
      * the slow wave reads tile ts and K half 0 of tile ts + 1 (strict: and still has reads of tile ts - 1 in flight);
      * a tile is certainly in LDS for everyone only if EVERY wave waited for its quarter before the barrier of tile b;
      * any tile issued by the fast wave and not waited for before that barrier may land at any moment of the interval.
    -> the list of (kind, barrier tile, read tile, written tile)"""
    bad = []
    for b in range(0, n_tiles, G):
        issued = b - 1 + pf              # the last tile a wave has issued when it arrives at the barrier of tile b
        landed = issued - wait           # ... and the last one it has waited for
        group = range(b, min(b + G, n_tiles))
        for ts in group:
            reads = {ts} | ({ts + 1} if ts + 1 < n_tiles else set()) | ({ts - 1} if strict and ts >= 1 else set())
            for r in sorted(reads):
                if r > landed:
                    bad.append(("read of an unwaited tile", b, r, None))
                for x in range(r + nslot, landed + 1, nslot):
                    bad.append(("read of a slot a later tile has already landed in", b, r, x))
            for tf in group:
                if tf < ts:
                    continue
                for x in range(landed + 1, tf + pf + 1):
                    for r in sorted(reads):
                        if x != r and x % nslot == r % nslot:
                            bad.append(("overwrite of a live slot", b, r, x))
    return bad


def laziest_safe_wait(G, pf, nslot, strict=False):
    """the largest number of outstanding tiles a wave may leave in front of a barrier without a violation, or None when even waiting for everything
    (or any other count) leaves one"""
    n_tiles = 4 * nslot + G + 1
    ok = [w for w in range(0, pf + 1) if not ring_violations(G, pf, nslot, w, n_tiles, strict)]
    return max(ok) if ok else None


@pytest.mark.parametrize("nslot", [4, 8])
def test_constructor_accepts_exactly_the_rings_the_model_finds_safe(nslot):
    import attn_gen
    import isa
    accepted = []
    for G in range(1, 6):
        for pf in range(1, 9):
            w = laziest_safe_wait(G, pf, nslot)
            try:
                g = attn_gen.AttnGen("f16", tiles_per_barrier=G, pf=pf, nslot=nslot)
                built = True
            except AssertionError:
                built = False
            assert built == (w is not None), f"G={G} pf={pf} nslot={nslot}: the constructor {'accepts' if built else 'refuses'}, the model's laziest safe wait is {w}"
            # the model's closed form: read after write G + 1 <= pf, write after read pf + G <= nslot (the non-strict form the header takes) ...
            assert built == (G + 1 <= pf and pf + G <= nslot)
            # ... and the strict form (the in-flight V^T reads of the tile before the barrier counted as live) is one slot tighter
            assert (laziest_safe_wait(G, pf, nslot, strict=True) is not None) == (G + 1 <= pf and pf + G <= nslot - 1)
            if not built:
                continue
            accepted.append((G, pf))
            # every wait in front of a barrier -- the prologue's and the loop's -- is the model's laziest safe one, in pieces
            p = g.build()
            waits = [p.items[i - 1].args[0] for i, it in enumerate(p.items) if isinstance(it, isa.Ins) and it.op == "s_barrier" and isinstance(p.items[i - 1], isa.Ins)
                     and p.items[i - 1].op == "s_waitcnt" and str(p.items[i - 1].args[0]).startswith("vmcnt")]
            assert waits == [f"vmcnt({g.NP * w})"] * 2, (G, pf, waits)
    assert accepted == {4: [(1, 2), (1, 3)], 8: [(1, p) for p in range(2, 8)] + [(2, p) for p in range(3, 7)] + [(3, 4), (3, 5)]}[nslot]
    assert all(s in accepted for s in SETTINGS) or nslot == 4


def test_grouped_form_is_for_the_512_query_head_dim_64_kernel_only():
    import attn_gen
    for kw in (dict(head_dim=80), dict(head_dim=128), dict(qpw=2), dict(qk_planes=2), dict(qk_planes=2, corr="f8")):
        with pytest.raises(AssertionError):
            attn_gen.AttnGen("f16", tiles_per_barrier=2, pf=3, nslot=8, **kw)
    g = attn_gen.AttnGen("bf16", **attn_gen.GROUPED_RING)
    assert g.name == "f3r_attn_asm_bf16_grp" and g.lds_bytes == 8 * 16384 + 16 and g.lds_bytes <= 160 * 1024


def test_module_has_the_two_grouped_kernels_and_the_old_ones_unchanged():
    """the library's module: the ten kernels it had, then f3r_attn_asm_{f16,bf16}_grp built with GROUPED_RING; the plain head_dim-64 kernels are the
    text of AttnGen(dt) with default arguments (whose digest tests/test_attn_asm_emu.py pins)"""
    import attn_gen
    gens = attn_gen.product_generators()
    names = [g.name for g in gens]
    assert names[-2:] == ["f3r_attn_asm_f16_grp", "f3r_attn_asm_bf16_grp"] and len(names) == 12 and len(set(names)) == 12
    for g in gens[-2:]:
        assert (g.G, g.pf, g.nslot) == tuple(attn_gen.GROUPED_RING[k] for k in ("tiles_per_barrier", "pf", "nslot"))
        assert g.p.check_hazards() == []
    for g, dt in zip(gens[:2], ("f16", "bf16")):
        ref = attn_gen.AttnGen(dt)
        ref.build()
        assert g.text() == ref.text()
