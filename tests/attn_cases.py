"""Seeded cases of the attention family -- f3r_attn_fwd on its eleven kernel forms, f3r_attn_f32_ex and f3r_attn_f32_mfma -- at the edges of their
geometry, their float64 references, the launch rules of the hand-scheduled kernels restated as functions of the device's CU count, and the guarded
placement of their device tensors: shared by tests/test_attn_cases.py (no GPU: the references against a per-row softmax, the case lists against
the properties they are there for, the placement against itself) and tests/test_attn_geometry_gpu.py (the kernels against the references).

Guarded placement (the read / write contract of f3r_attn_args in include/f3r.h):
  q      rows [0, tq) of every sequence, columns [0, n_heads * head_dim * planes) hold values; the gap columns up to ldq, the rows between two
         sequences of a wide batch stride and the margins are NaN patterns (0xFF bytes)
  K      rows [0, seg_len), the columns of the K / V heads; rows behind seg_len, gap columns and margins are NaN patterns
  V^T    rows [0, kv_heads * head_dim), columns [0, seg_len) hold values, [seg_len, round_up(seg_len, 64)) zeros (the ABI's padding) and
         [round_up(seg_len, 64), ldvt) NaN patterns: every segment of a case has ONE ldvt (what the hand-scheduled kernels take), so a short
         segment next to a long one has such columns
  o      rows [0, tq) x [0, n_heads * head_dim) may be written; gap columns, rows between sequences and margins keep SENTINEL
  state  st_o / st_ml, fp32 between SENTINEL32 words: rows [0, batch * tq) may be written
Every margin is a whole work item of the largest form: 512 rows of the buffer's stride for q, o and the state, 64 key rows for K, 128 rows for
V^T.  A form that overruns by a whole workgroup changes sentinels or reads NaN patterns INSIDE the allocation: a miss is a failed assertion.
"""
import dataclasses
import math

import torch

from gemm_cases import BF16, CU_NOMINAL, H16, SENTINEL, SENTINEL32, Guarded, guarded_operand, guarded_rows, guards_intact  # noqa: F401  (one owner)
from fast3r_amd import _lib, ops

LOG2E = ops.LOG2E
MAX_SEG = _lib.F3R_MAX_SEG
MARGIN_ROWS = 512          # q, o, state: the rows of the largest work item (a 512-query workgroup)
K_MARGIN_ROWS = 64         # one key tile
VT_MARGIN_ROWS = 128       # the V^T planes of the widest head
GENERIC_HDS = (16, 32, 48, 80, 96, 112, 128)
ASM_MIN_KEYS = 2048        # F3R_ATTN_ASM_MIN_KEYS

# what f3r_attn_kernel_name must contain for a form
FORM_NAMES = {
    "hip": "attn_kernel (f3r_attn.hip)", "hip-batched": "attn_kernel<batched>", "hip-causal": "attn_kernel<causal>",
    "generic": "attn_generic_kernel",
    "asm512": "f3r_attn_asm_{dt} (hand-scheduled", "q256": "f3r_attn_asm_q256_{dt} (hand-scheduled", "split": "f3r_attn_asm_{dt} + f3r_attn_asm_q256_{dt} for the last round",
    "d80": "f3r_attn_asm_d80_{dt}", "d128": "f3r_attn_asm_d128_{dt}", "qk3": "f3r_attn_asm_qk3_f16", "qk3f8": "f3r_attn_asm_qk3f8_f16",
}


def _dt(dt):
    return "f16" if dt == H16 else "bf16"


@dataclasses.dataclass(frozen=True)
class AttnCase:
    tq: int
    segs: tuple                    # keys per K / V segment (0: an empty one)
    head_dim: int = 64
    dtype: torch.dtype = H16
    n_heads: int = 1
    kv_group: int = 1
    batch: int = 1
    causal: bool = False
    q_pos0: int = 0
    seg_pos0: tuple = ()           # (): consecutive segments from position 0
    q_prescaled: bool = True
    scale: float = 0.125           # (not pre-scaled only)
    ldq: int = 0                   # row strides in elements; 0: the row's width
    ldk: int = 0
    ldo: int = 0
    ldvt: int = 0                  # 0: vt_ld(the longest segment); one stride for every segment
    q_bs: int = 0                  # batch strides in elements; 0: tight (tq rows)
    o_bs: int = 0
    k_pad_rows: int = 0            # rows between two sequences of K beyond the longest segment (one batch stride for every segment)
    vt_pad_rows: int = 0           # ... of V^T beyond kv_heads * head_dim
    state: object = None           # None | ("park", cut): segments [:cut] with state_out, then [cut:] with state_in
    cross: tuple = ()              # (): both launches on the case's form; (sel, sel): park on the first kernel_sel, resume on the second
    qk_planes: int = 1             # 2 / 3: q and K rows as written by f3r_qkv_planes
    forms: tuple = ("hip",)        # the forms it is there for (forms() must list them on a device where they can occur)

    @property
    def kv_heads(self):
        return self.n_heads // self.kv_group

    @property
    def keys(self):
        return sum(self.segs)

    @property
    def qk_cols(self):
        """elements of a head in a q / K row"""
        return self.head_dim * (2 if self.qk_planes >= 2 else 1)

    @property
    def q_width(self):
        return self.n_heads * self.qk_cols

    @property
    def k_width(self):
        return self.kv_heads * self.qk_cols

    @property
    def o_width(self):
        return self.n_heads * self.head_dim

    def ld(self, name):
        width = {"ldq": self.q_width, "ldk": self.k_width, "ldo": self.o_width, "ldvt": ops.vt_ld(max(self.segs))}[name]
        return getattr(self, name) or width

    def bs(self, name):
        """batch stride of q / o / k / vt in elements"""
        if name in ("q", "o"):
            return getattr(self, name + "_bs") or self.tq * self.ld("ld" + name)
        if name == "k":
            return (max(self.segs) + self.k_pad_rows) * self.ld("ldk")
        return (self.kv_heads * self.head_dim + self.vt_pad_rows) * self.ld("ldvt")

    @property
    def positions(self):
        """global position of the first key of every segment"""
        if self.seg_pos0:
            return tuple(self.seg_pos0)
        out, run = [], 0
        for n in self.segs:
            out.append(run)
            run += n
        return tuple(out)

    @property
    def id(self):
        s = f"hd{self.head_dim}-{_dt(self.dtype)}-q{self.tq}-k{'_'.join(map(str, self.segs))}-h{self.n_heads}g{self.kv_group}b{self.batch}"
        if self.causal:
            s += f"-causal{self.q_pos0}" + ("at" + "_".join(map(str, self.seg_pos0)) if self.seg_pos0 else "")
        if not self.q_prescaled:
            s += "-scaled"
        s += "".join(f"-{n}{getattr(self, n)}" for n in ("ldq", "ldk", "ldo", "ldvt", "q_bs", "o_bs", "k_pad_rows", "vt_pad_rows") if getattr(self, n))
        if self.state:
            s += f"-park{self.state[1]}" + (f"x{self.cross[0]}{self.cross[1]}" if self.cross else "")
        if self.qk_planes > 1:
            s += f"-planes{self.qk_planes}"
        return s + "-" + "+".join(self.forms)


# ------------------------------------------------------------------------------------------------ the launch rules, restated
def pow2(x):
    return x > 0 and x & (x - 1) == 0


def wave_rows(c, q256=False):
    """query rows of a wave: 32 x the query blocks per wave of the generator (4 at head_dim 64, 2 in its 256-query form and everywhere else)"""
    return 64 if (q256 or c.head_dim != 64 or c.qk_planes >= 2) else 128


def legal(c):
    """f3r_attn_fwd's argument rules restated: None, or the first rule the case breaks"""
    if c.head_dim % 16 or not 16 <= c.head_dim <= 128:
        return "head_dim"
    if c.ld("ldq") % 8 or c.ld("ldk") % 8 or c.ld("ldo") % 4 or c.ld("ldq") < c.q_width or c.ld("ldo") < c.o_width or c.ld("ldk") < c.k_width:
        return "row strides"
    if c.bs("q") % 8 or c.bs("o") % 4 or c.bs("k") % 8 or c.bs("vt") % 8:
        return "batch strides"
    if not 1 <= len(c.segs) <= MAX_SEG or c.keys == 0:
        return "segments"
    if c.ld("ldvt") % 64 or c.ld("ldvt") < max(c.segs):
        return "ldvt"
    if c.n_heads % c.kv_group:
        return "kv_group"
    if c.causal and c.positions[[i for i, n in enumerate(c.segs) if n][0]] > c.q_pos0:   # (a parked case: its first launch is the fresh one)
        return "a fresh causal launch whose first key lies after its first query"
    if c.batch > 1 and (c.bs("q") < c.tq * c.ld("ldq") or c.bs("o") < c.tq * c.ld("ldo")):
        return "sequences overlap"
    if c.state and not 0 < c.state[1] < len(c.segs):
        return "cut"
    if c.state and (sum(c.segs[:c.state[1]]) == 0 or sum(c.segs[c.state[1]:]) == 0):
        return "a launch without keys"
    return None


def asm_eligible(c, segs=None, state=None, min_keys=0):
    """f3r_attn_asm_eligible restated (without the code object's presence): can a hand-scheduled kernel take a launch of the case over `segs`?"""
    segs = c.segs if segs is None else segs
    state = bool(c.state) if state is None else state
    if c.head_dim not in (64, 80, 128):
        return False
    if c.qk_planes >= 2 and (c.head_dim != 64 or c.dtype != H16):
        return False
    if c.causal or not c.q_prescaled or c.tq < wave_rows(c):
        return False
    if c.kv_group > 1 and not pow2(c.kv_group):
        return False
    if state and c.batch != 1 and c.qk_planes < 2:
        return False
    if any(n % 64 for n in segs) or sum(segs) == 0 or sum(segs) < min_keys:
        return False
    return True


def use_q256(c, tq, n_cu):
    """use_q256 of csrc/f3r_attn_asm.hip: a head_dim-64 launch of less than half a round of 512-query items runs on 256-query items"""
    if c.head_dim != 64 or c.qk_planes >= 2:
        return False
    hb = c.n_heads * c.batch
    n512, n256 = -(-tq // 512) * hb, -(-tq // 256) * hb
    return 0.64 * float(-(-n256 // n_cu)) < 0.97 * float(-(-n512 // n_cu))


def tail_split_rows(c, n_cu, state=None, guarded=True):
    """tail_split_rows of csrc/f3r_attn_asm.hip: the rows of the main launch when the last, partly filled round goes out as a second launch on
    256-query items; 0: one launch.  guarded=False: the rule as it was before it asked the tail for a wave's rows."""
    state = bool(c.state) if state is None else state
    if c.head_dim != 64 or c.qk_planes >= 2 or state:
        return 0
    hb = c.n_heads * c.batch
    nqb = -(-c.tq // 512)
    if nqb * hb <= n_cu:
        return 0
    g = n_cu // math.gcd(n_cu, hb)
    nqb_main = nqb // g * g
    if nqb_main in (0, nqb) or nqb_main * hb // n_cu > 8:
        return 0
    if 2 * (nqb - nqb_main) * hb > n_cu:
        return 0
    tail = c.tq - nqb_main * 512
    if guarded and tail < (64 if use_q256(c, tail, n_cu) else 128):
        return 0
    return nqb_main * 512


def work_items(c, n_cu):
    """(work items, query blocks) of a one-launch hand-scheduled form of the case"""
    wg = 4 * wave_rows(c, use_q256(c, c.tq, n_cu))
    nx = -(-c.tq // wg)
    return nx * c.n_heads * c.batch, nx


def steals(c, n_cu):
    """does a launch with a sched_counter run as persistent workgroups?  (launch_one: at least two rounds of workgroups)"""
    n, nx = work_items(c, n_cu)
    return tail_split_rows(c, n_cu) == 0 and n >= 2 * n_cu and n * nx * c.n_heads < 1 << 32


def asm_form(c, n_cu):
    if c.qk_planes >= 2:
        return "qk3" if c.qk_planes == 2 else "qk3f8"
    if c.head_dim != 64:
        return f"d{c.head_dim}"
    if tail_split_rows(c, n_cu):
        return "split"
    return "q256" if use_q256(c, c.tq, n_cu) else "asm512"


def hip_form(c):
    if c.head_dim != 64:
        return "generic"
    return "hip-causal" if c.causal else ("hip-batched" if c.batch > 1 else "hip")


def forms(c, n_cu):
    """[(form, kernel_sel)]: every kernel form that takes the case on a device of n_cu CUs.  A parked case (c.state) lists a form only when BOTH
    launches can run on it; c.cross names the two kernel_sel itself."""
    if c.cross:
        return [("cross", c.cross)]
    out = []
    if c.qk_planes < 2 and (c.head_dim == 64 or not c.causal):
        out.append((hip_form(c), 1))
    if c.state:
        cut = c.state[1]
        ok = asm_eligible(c, c.segs[:cut], True) and asm_eligible(c, c.segs[cut:], True)
    else:
        ok = asm_eligible(c)
    if ok:
        out.append((asm_form(c, n_cu), 2))
    return out


def expected_name(form, c):
    return FORM_NAMES[form].format(dt=_dt(c.dtype))


# ------------------------------------------------------------------------------------------------ 1. the HIP head_dim-64 kernel
HIP_TQ = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 257)
HIP_KEYS = (1, 7, 63, 64, 65, 127, 128, 129, 191)
HIP_HEADS = ((1, 1), (3, 1), (3, 3), (2, 2), (4, 2))     # (n_heads, kv_group): 1 or 3 heads, and the even counts kv_group 2 needs
HIP_SEGS = ((1,), (64, 1), (1, 64), (63, 0, 65), (0, 0, 5), tuple(1 + (i * 64) // (MAX_SEG - 1) for i in range(MAX_SEG)))


def _hip():
    out = []
    for i, tq in enumerate(HIP_TQ):
        for j in range(3):
            keys = HIP_KEYS[(3 * i + j + i // 3) % len(HIP_KEYS)]
            h, g = HIP_HEADS[(i + j) % len(HIP_HEADS)]
            for dt in (H16, BF16):
                out.append(AttnCase(tq, (keys,), 64, dt, h, g, q_prescaled=bool((i + j + (dt == BF16)) % 2)))
    for n, segs in enumerate(HIP_SEGS):
        for dt in (H16, BF16):
            out.append(AttnCase(97, segs, 64, dt, 2, 1 + n % 2, q_prescaled=bool(n % 2)))
    for dt in (H16, BF16):
        # three sequences, every stride wider than what it spans, ldvt one tile wider than the keys need
        out.append(AttnCase(70, (65, 0, 130), 64, dt, 3, 1, 3, ldq=3 * 64 + 8, ldk=3 * 64 + 16, ldo=3 * 64 + 4, ldvt=ops.vt_ld(130) + 64,
                            q_bs=(70 + 5) * (3 * 64 + 8), o_bs=(70 + 3) * (3 * 64 + 4), k_pad_rows=3, vt_pad_rows=2, forms=("hip-batched",)))
        out.append(AttnCase(257, (129,), 64, dt, 2, 2, 3, q_prescaled=False, ldq=2 * 64 + 8, ldk=64 + 8, ldo=2 * 64 + 4, ldvt=192 + 64,
                            q_bs=(257 + 1) * (2 * 64 + 8), o_bs=(257 + 2) * (2 * 64 + 4), k_pad_rows=1, vt_pad_rows=1, forms=("hip-batched",)))
        for cut in (1, 2):      # park and resume at every cut of a three-segment list (a batch: the HIP kernel carries state per sequence)
            out.append(AttnCase(129, (63, 64, 65), 64, dt, 2, 1, 1, state=("park", cut)))
            out.append(AttnCase(65, (1, 130, 7), 64, dt, 3, 3, 2, state=("park", cut), forms=("hip-batched",)))
    return out


HIP = _hip()


# ------------------------------------------------------------------------------------------------ 2. causal head_dim 64
CAUSAL_T = (1, 63, 64, 65, 129)
SHARD_LENS = (63, 1, 1, 64)    # shards of one 129-token sequence: edges at 63, 64 and 65


def _causal():
    out = []
    for i, T in enumerate(CAUSAL_T):
        for dt in (H16, BF16):
            out.append(AttnCase(T, (T,), 64, dt, 2, 1 + i % 2, causal=True, q_prescaled=bool(i % 2), forms=("hip-causal",)))
    for tq, keys in ((65, 129), (1, 130), (33, 64), (64, 191)):       # the last tq rows of a longer sequence
        for dt in (H16, BF16):
            out.append(AttnCase(tq, (keys,), 64, dt, 2, 1, causal=True, q_pos0=keys - tq, forms=("hip-causal",)))
    pos = [sum(SHARD_LENS[:i]) for i in range(len(SHARD_LENS))]
    for rank, n in enumerate(SHARD_LENS):   # test_attention_causal_over_shards: the rank's own shard first (parked), then every other shard
        order = [rank] + [r for r in range(len(SHARD_LENS)) if r != rank]
        for dt in (H16, BF16):
            out.append(AttnCase(n, tuple(SHARD_LENS[r] for r in order), 64, dt, 2, 1, causal=True, q_pos0=pos[rank], seg_pos0=tuple(pos[r] for r in order),
                                state=("park", 1), forms=("hip-causal",)))
    return out


CAUSAL = _causal()
# a fresh causal launch whose first key lies one position after its first query: the library must refuse it
CAUSAL_REFUSED = AttnCase(64, (64,), 64, H16, 1, causal=True, q_pos0=10, seg_pos0=(11,), forms=("hip-causal",))


# ------------------------------------------------------------------------------------------------ 3. the generic kernel
GENERIC_TQ = (1, 127, 128, 129, 255, 256, 257)   # workgroups of 256 queries up to head_dim 96, of 128 above
GENERIC_KEYS = (1, 63, 64, 65, 130)


def _generic():
    out = []
    for a, hd in enumerate(GENERIC_HDS):
        for i, tq in enumerate(GENERIC_TQ):
            keys = GENERIC_KEYS[(i + a) % len(GENERIC_KEYS)]
            h, g = ((1, 1), (2, 2), (3, 1))[(i + a) % 3]
            dt = (H16, BF16)[(i + a) % 2]
            out.append(AttnCase(tq, (keys,), hd, dt, h, g, q_prescaled=bool((i + a) % 3), forms=("generic",)))
        dt, other = ((H16, BF16), (BF16, H16))[a % 2]
        out.append(AttnCase(129, (65, 0, 64), hd, dt, 2, 2, forms=("generic",)))                                      # an empty segment, grouped heads
        out.append(AttnCase(257, (63, 130, 1), hd, other, 2, 1, state=("park", 1 + a % 2), forms=("generic",)))        # park and resume
        out.append(AttnCase(130, (65, 64), hd, dt, 2, 1, 2, ldq=2 * hd + 8, ldk=2 * hd + 16, ldo=2 * hd + 4, ldvt=128 + 64,
                            q_bs=(130 + 3) * (2 * hd + 8), o_bs=(130 + 1) * (2 * hd + 4), k_pad_rows=2, vt_pad_rows=3, forms=("generic",)))
    return out


GENERIC = _generic()


# ------------------------------------------------------------------------------------------------ 4. the hand-scheduled forms
ASM_TQ = {"asm512": (128, 129, 511, 512, 513, 640), "q256": (128, 129, 255, 256, 257, 300),
          "d80": (64, 65, 255, 256, 257, 300), "d128": (64, 65, 255, 256, 257, 300), "qk3": (64, 65, 255, 256, 257, 300), "qk3f8": (64, 65, 255, 256, 257, 300)}
ASM_TILES = (1, 2, 3, 5)
ASM_KW = {"asm512": dict(head_dim=64), "q256": dict(head_dim=64), "d80": dict(head_dim=80), "d128": dict(head_dim=128),
          "qk3": dict(head_dim=64, qk_planes=2), "qk3f8": dict(head_dim=64, qk_planes=3)}


def heads_for_512(tq, n_cu, batch=1):
    """heads (a multiple of 4) x batch for which the launch rule keeps 512-query items: one round of them, more than one round of 256-query ones"""
    hb = n_cu // 2 + 4 if tq <= 512 else n_cu // 2
    return max(4, -(-hb // batch) // 4 * 4)


def asm_cases(form, n_cu=CU_NOMINAL):
    """the cases of one hand-scheduled form.  Only "asm512" depends on n_cu: its heads x batch come from the launch rule."""
    kw = ASM_KW[form]
    planes = kw.get("qk_planes", 1)
    hd = kw["head_dim"]
    cols = hd * (2 if planes > 1 else 1)
    dts = (H16,) if planes > 1 else (H16, BF16)

    def heads(tq, want, batch=1):
        return heads_for_512(tq, n_cu, batch) if form == "asm512" else want

    out = []
    for i, tq in enumerate(ASM_TQ[form]):
        g = (1, 2, 4)[i % 3]
        h = heads(tq, 4 if g > 1 else (1, 3)[i % 2])
        out.append(AttnCase(tq, (64 * ASM_TILES[i % 4],), hd, dts[i % len(dts)], h, g, qk_planes=planes, forms=(form,)))
    t0 = ASM_TQ[form][3]     # a whole workgroup's rows
    t1 = ASM_TQ[form][5]     # ... and a partial one behind it
    for n, dt in enumerate(dts):
        H = heads(t1, 4)
        out.append(AttnCase(t1, (64, 0, 128), hd, dt, H, 2, qk_planes=planes, forms=(form,)))
        out.append(AttnCase(t0, (64,) * 8, hd, dt, heads(t0, 2), 1, qk_planes=planes, forms=(form,)))
        out.append(AttnCase(t1, (64, 192), hd, dt, H, 4, ldvt=256, qk_planes=planes, forms=(form,)))
        Hb = heads(t1, 2, batch=2)
        out.append(AttnCase(t1, (128, 64), hd, dt, Hb, 2, 2, ldq=Hb * cols + 8, ldk=Hb // 2 * cols + 16, ldo=Hb * hd + 4, ldvt=128 + 64,
                            q_bs=(t1 + 3) * (Hb * cols + 8), o_bs=(t1 + 1) * (Hb * hd + 4), k_pad_rows=2, vt_pad_rows=3, qk_planes=planes, forms=(form,)))
        out.append(AttnCase(t1, (128, 64, 64), hd, dt, H, 1, state=("park", 1 + n % 2), qk_planes=planes, forms=(form,)))
    if planes > 1:   # the three-product kernels carry state at any batch: sequence z owns rows [z tq, (z + 1) tq)
        out.append(AttnCase(300, (64, 128), hd, H16, 2, 1, 3, state=("park", 1), qk_planes=planes, forms=(form,)))
    return out


ASM_STATIC_FORMS = ("q256", "d80", "d128", "qk3", "qk3f8")
ASM_STATIC = [c for f in ASM_STATIC_FORMS for c in asm_cases(f)]


def cross_cases():
    """one state layout for every kernel: parked by the HIP / generic kernel and resumed by the hand-scheduled one, and the reverse"""
    out = []
    for hd in (64, 80, 128):
        for n, dt in enumerate((H16, BF16)):
            for cross in ((1, 2), (2, 1)):
                out.append(AttnCase(300, (128, 64, 64), hd, dt, 2, 1 + n, state=("park", 1 + n), cross=cross, forms=("cross",)))
    return out


CROSS = cross_cases()


def steal_cases(n_cu=CU_NOMINAL):
    """the smallest launches that take the work-stealing form: two rounds of workgroups (and whole rounds: no split of the last one)"""
    h = 16
    nqb = -(-2 * n_cu // h)
    return [AttnCase(512 * nqb, (64,), 64, H16, h, 2, forms=("asm512",)), AttnCase(256 * nqb - 100, (128,), 80, BF16, h, 1, forms=("d80",))]


# ------------------------------------------------------------------------------------------------ 5. the split of the last round
SPLIT_R = (1, 40, 63, 64, 65, 200, 511)
SPLIT_HEADS = ((16, 1), (8, 2), (4, 4))    # heads x batch = 16


def split_g(n_cu):
    return n_cu // math.gcd(n_cu, 16)


def split_cases(n_cu=CU_NOMINAL):
    """tq = g 512 + r: g blocks fill whole rounds at heads x batch = 16, the last block holds r rows.  r < 64 is less than a wave of the 256-query
    form takes: ONE launch (on the form use_q256 picks for all g + 1 blocks); from 64 rows on the last block goes out as a second launch"""
    out = []
    for i, r in enumerate(SPLIT_R):
        for j, keys in enumerate((64, 128)):
            h, b = SPLIT_HEADS[(i + j) % 3]
            c = AttnCase(split_g(n_cu) * 512 + r, (keys,), 64, (H16, BF16)[(i + j) % 2], h, (1, 2)[(i + j) % 2], b)
            out.append(dataclasses.replace(c, forms=(asm_form(c, n_cu),)))
    return out


def split_possible(n_cu):
    """the launch rule splits these cases only where g blocks are at most 8 rounds and the last block at most half a round"""
    g = split_g(n_cu)
    return g > 1 and g * 16 // n_cu <= 8 and 2 * 16 <= n_cu


# every case of f3r_attn_fwd that does not depend on the device
STATIC = HIP + CAUSAL + GENERIC + ASM_STATIC + CROSS


# ------------------------------------------------------------------------------------------------ 6. the exact mode
@dataclasses.dataclass(frozen=True)
class ExactCase:
    tq: int
    tk: int
    head_dim: int = 64
    n_heads: int = 2
    kv_group: int = 1
    n_seq: int = 1
    causal: bool = False
    q_pos0: int = 0
    k_pos0: int = 0
    dtype: torch.dtype = H16
    mfma: bool = False             # f3r_attn_f32_mfma (head_dim 64, no mask) instead of f3r_attn_f32_ex

    @property
    def id(self):
        return (f"exact-{'mfma' if self.mfma else 'fma'}-hd{self.head_dim}-{_dt(self.dtype)}-q{self.tq}-k{self.tk}-h{self.n_heads}g{self.kv_group}s{self.n_seq}"
                + (f"-causal{self.q_pos0}_{self.k_pos0}" if self.causal else ""))


EXACT_T = (1, 63, 64, 65, 129)


def _exact():
    out = []
    for i, tq in enumerate(EXACT_T):
        for j in range(2):
            tk = EXACT_T[(i + 2 * j + 1) % len(EXACT_T)]
            g = 1 + (i + j) % 2
            # (the MFMA form's operands ARE planes of the output dtype: the 3e-6 bar is its fp16 bar, test_exact_mfma_gpu.py; the FMA kernel's
            # fp32 output does not depend on the dtype of its hi + lo output planes)
            out.append(ExactCase(tq, tk, 64, 2, g, 1 + (i + j) % 2, dtype=(H16, BF16)[i % 2]))
            out.append(ExactCase(tq, tk, 64, 2, g, 1 + (i + j) % 2, mfma=True))
            out.append(ExactCase(tq, tk, 80, 2, g, 1 + j, dtype=(H16, BF16)[j]))
    for i, T in enumerate(EXACT_T):                                       # causal, on the FMA kernel (the only one with a mask)
        out.append(ExactCase(T, T, (64, 80)[i % 2], 2, 1 + i % 2, causal=True))
    out.append(ExactCase(65, 129, 64, 4, 2, causal=True, q_pos0=64))       # the last rows of a longer sequence
    out.append(ExactCase(64, 129, 80, 2, 1, causal=True, q_pos0=63, k_pos0=0))
    out.append(ExactCase(63, 65, 64, 2, 2, causal=True, q_pos0=70, k_pos0=64))   # gathered keys that start at another position
    return out


EXACT = _exact()


# ------------------------------------------------------------------------------------------------ operands and float64 references
def _seed(c):
    return 3000 + sum(map(ord, c.id)) % 100000


def build(c):
    """Operands of a case on the CPU -> q [batch][tq][n_heads * head_dim], k / v: per segment [batch][n][kv_heads * head_dim] (fp32 for
    qk_planes >= 2, where f3r_qkv_planes makes the planes on the device; rounded to the case's dtype otherwise)."""
    g = torch.Generator().manual_seed(_seed(c))
    hd = c.head_dim
    qs = hd ** -0.5 * LOG2E * 1.5 if c.q_prescaled else 1.0
    q = torch.randn((c.batch, c.tq, c.n_heads * hd), generator=g) * qs
    ks = [torch.randn((c.batch, n, c.kv_heads * hd), generator=g) * 1.5 for n in c.segs]
    vs = [torch.randn((c.batch, n, c.kv_heads * hd), generator=g) for n in c.segs]
    if c.qk_planes < 2:
        q, ks, vs = q.to(c.dtype), [k.to(c.dtype) for k in ks], [v.to(c.dtype) for v in vs]
    return dict(q=q, k=ks, v=vs)


def softmax64(q, k, v, n_heads, kv_group, hd, log_scale, mask=None):
    """q [tq][n_heads * hd], k / v [keys][kv_heads * hd] (any dtype) -> float64 [tq][n_heads * hd]: softmax(q k^T log_scale [masked]) v with grouped
    heads (query head h reads K / V head h // kv_group).  mask [tq][keys]: True = hidden."""
    tq, keys, kvh = q.shape[0], k.shape[0], n_heads // kv_group
    qh = q.double().reshape(tq, n_heads, hd).transpose(0, 1)
    kh = k.double().reshape(keys, kvh, hd).transpose(0, 1).repeat_interleave(kv_group, 0)
    vh = v.double().reshape(keys, kvh, hd).transpose(0, 1).repeat_interleave(kv_group, 0)
    s = (qh @ kh.transpose(1, 2)) * log_scale
    if mask is not None:
        s = s.masked_fill(mask[None], float("-inf"))
    return (s.softmax(-1) @ vh).transpose(0, 1).reshape(tq, n_heads * hd)


def causal_mask(c, rows=None):
    if not c.causal:
        return None
    kpos = torch.cat([p + torch.arange(n) for p, n in zip(c.positions, c.segs)])
    qpos = c.q_pos0 + (torch.arange(c.tq) if rows is None else rows)
    return kpos[None, :] > qpos[:, None]


def reference(c, d, rows=None):
    """float64 [batch][rows][n_heads * head_dim] on the rounded operands of build(c): base-2 softmax for pre-scaled q, grouped heads, the causal
    mask by global position.  rows: a LongTensor of query rows (default: all)."""
    ls = math.log(2.0) if c.q_prescaled else c.scale
    mask = causal_mask(c, rows)
    out = []
    for b in range(c.batch):
        q = d["q"][b] if rows is None else d["q"][b][rows]
        out.append(softmax64(q, torch.cat([k[b] for k in d["k"]]), torch.cat([v[b] for v in d["v"]]), c.n_heads, c.kv_group, c.head_dim, ls, mask))
    return torch.stack(out)


def e4m3(x64):
    return x64.float().clamp(-448, 448).to(torch.float8_e4m3fn).double()


def decode_planes(rows, heads, planes):
    """rows [n][heads * 128] fp16 as f3r_qkv_planes wrote them -> the (q-side, k-side) float64 factors [n][heads * 64] of the score products:
    planes 2: [(hi + lo)]  (the kernel drops lo x lo: below fp32's resolution of the sum);  planes 3: [hi, e4m3(hi), e4m3(lo 2^12) / 2^12]"""
    n = rows.shape[0]
    r = rows.reshape(n, heads, 2, 64)
    hi = r[:, :, 0].double().reshape(n, heads * 64)
    if planes == 2:
        return [hi + r[:, :, 1].double().reshape(n, heads * 64)]
    b = r[:, :, 1].contiguous().view(torch.uint8).view(n, heads, 128)
    hi8 = b[:, :, :64].contiguous().view(torch.float8_e4m3fn).double().reshape(n, heads * 64)
    lo8 = b[:, :, 64:].contiguous().view(torch.float8_e4m3fn).double().reshape(n, heads * 64) / 4096.0
    return [hi, hi8, lo8]


def reference_planes(c, qp, kp, v):
    """float64 [tq][n_heads * 64] of ONE sequence from the planes the device wrote (tests/test_robust_gpu.py): qp [tq][n_heads * 128], kp [keys][kv_heads * 128]
    fp16, v [keys][kv_heads * 64] fp16.  planes 2: softmax2((q_hi + q_lo)(k_hi + k_lo)) v;  planes 3: the scores the kernel forms from ITS planes,
    q_hi k_hi + q_lo8 k_hi8 + q_hi8 k_lo8."""
    qf, kf = decode_planes(qp, c.n_heads, c.qk_planes), decode_planes(kp, c.kv_heads, c.qk_planes)
    pairs = [(qf[0], kf[0])] if c.qk_planes == 2 else [(qf[0], kf[0]), (qf[2], kf[1]), (qf[1], kf[2])]
    tq, keys = qp.shape[0], kp.shape[0]
    s = 0.0
    for qq, kk in pairs:
        qh = qq.reshape(tq, c.n_heads, 64).transpose(0, 1)
        kh = kk.reshape(keys, c.kv_heads, 64).transpose(0, 1).repeat_interleave(c.kv_group, 0)
        s = s + qh @ kh.transpose(1, 2)
    vh = v.double().reshape(keys, c.kv_heads, 64).transpose(0, 1).repeat_interleave(c.kv_group, 0)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    return ((p @ vh) / p.sum(-1, keepdim=True)).transpose(0, 1).reshape(tq, c.n_heads * 64)


def build_exact(c):
    """fp32 operands of an exact-mode case and the float64 reference -> q [n_seq * tq][H hd], k, v [n_seq * tk][Hkv hd], ref [n_seq * tq][H hd]"""
    g = torch.Generator().manual_seed(_seed(c))
    hd, kvh = c.head_dim, c.n_heads // c.kv_group
    q = torch.randn((c.n_seq * c.tq, c.n_heads * hd), generator=g) * 1.5
    k = torch.randn((c.n_seq * c.tk, kvh * hd), generator=g) * 1.5
    v = torch.randn((c.n_seq * c.tk, kvh * hd), generator=g)
    mask = None
    if c.causal:
        mask = (c.k_pos0 + torch.arange(c.tk))[None, :] > (c.q_pos0 + torch.arange(c.tq))[:, None]
    scale = hd ** -0.5
    ref = torch.cat([softmax64(q[z * c.tq:(z + 1) * c.tq], k[z * c.tk:(z + 1) * c.tk], v[z * c.tk:(z + 1) * c.tk], c.n_heads, c.kv_group, hd, scale, mask)
                     for z in range(c.n_seq)])
    return dict(q=q, k=k, v=v, ref=ref, scale=scale)


# ------------------------------------------------------------------------------------------------ guarded placement
def vt_image(v, c):
    """v [batch][n][kv_heads * hd] -> the CPU image [batch][kv_heads * hd][ldvt] of a V^T segment: values, zeros up to the next multiple of 64 keys
    (the ABI's padding), NaN patterns up to ldvt"""
    ldvt, n = c.ld("ldvt"), v.shape[1]
    img = torch.full((c.batch, v.shape[2], ldvt * 2), 0xFF, dtype=torch.uint8).view(v.dtype)
    img[:, :, :ops.vt_ld(n)] = 0
    img[:, :, :n] = v.transpose(1, 2)
    return img


def place(t, ld, bs, dev, margin_rows):
    """t [batch][rows][width] as a strided view (row stride ld, batch stride bs, both in elements) inside a device buffer of NaN patterns with
    margin_rows rows of ld before and behind: the gap columns and the rows between two sequences are NaN patterns too -> (view, buffer)"""
    batch, rows, width = t.shape
    assert ld >= width and (batch == 1 or bs >= rows * ld)
    span = (batch - 1) * bs + (rows - 1) * ld + width
    full = torch.full((span * t.element_size(),), 0xFF, dtype=torch.uint8).view(t.dtype)
    full.as_strided((batch, rows, width), (bs, ld, 1)).copy_(t)
    flat, buf = guarded_operand(full, dev, margin_rows * ld * t.element_size())
    return flat.as_strided((batch, rows, width), (bs, ld, 1), flat.storage_offset()), buf


@dataclasses.dataclass
class GuardedOut(Guarded):
    batch: int = 1
    bs: int = 0


def place_out(batch, rows, width, ld, bs, dtype, dev, margin_rows=MARGIN_ROWS):
    """an output view [batch][rows][width] (row stride ld, batch stride bs) inside a buffer of sentinel words (32-bit ones for a 32-bit dtype),
    margin_rows rows of ld before and behind, 16-byte aligned"""
    assert ld >= width and (batch == 1 or bs >= rows * ld)
    wide = torch.empty((), dtype=dtype).element_size() == 4
    per16 = 4 if wide else 8
    lead = (margin_rows * ld + per16 - 1) // per16 * per16
    span = (batch - 1) * bs + rows * ld
    buf = torch.full((lead + span + lead,), SENTINEL32 if wide else SENTINEL, dtype=torch.int32 if wide else torch.int16, device=dev)
    view = buf.view(dtype).as_strided((batch, rows, width), (bs, ld, 1), lead)
    assert view.data_ptr() % 16 == 0
    return GuardedOut(view, buf, lead, rows, width, ld, batch, bs)


def out_intact(g):
    """every word of the buffer outside the [batch][rows][width] outputs -- margins, gap columns, rows between sequences -- is the sentinel"""
    s = SENTINEL32 if g.buf.dtype == torch.int32 else SENTINEL
    free = torch.ones(g.buf.numel(), dtype=torch.bool, device=g.buf.device)
    free.as_strided((g.batch, g.rows, g.width), (g.bs, g.ld, 1), g.lead).fill_(False)
    return bool((g.buf[free] == s).all())


def untouched(g):
    """the whole buffer, outputs included, is sentinel words (a launch with state_out must not write o)"""
    return bool((g.buf == (SENTINEL32 if g.buf.dtype == torch.int32 else SENTINEL)).all())
