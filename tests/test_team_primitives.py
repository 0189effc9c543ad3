"""The wavefront primitives of opensot_amd/csrc/osot_team.h, one at a time, against their host twin tests/emu/osot_team.h.

Every emulated test of this suite rests on the twin having "the same names, the same semantics" as the device header.  Here
one probe kernel (tests/probe/team_probe.h), compiled once against each header, runs every primitive on its own and each
result is compared with an independent numpy statement written in this file:

    target "twin"    emu_lib().emu_team_probe         -- no GPU needed, runs everywhere
    target "device"  team_probe_lib().osot_team_probe -- @pytest.mark.gpu; where the twin claims the device's exact order
                                                        (quad_sum, rowgroup_sum, halfsum, MFMA) the two are also compared
                                                        bit for bit

No expected number below is taken from the device's output.  Movement, masks and extrema involve no arithmetic and are
compared bit for bit (the sign of a zero result numerically); sums of integer-valued inputs are exact in any order; sums of
random inputs obey the standard bound d u sum|v| / (1 - d u) for a summation tree of depth d; fast_rcp / fast_div /
fast_sqrt_rsqrt promise "~1 ulp for normal arguments" (fast_rcp1: ~2 ulp) and are held to that against the correctly rounded
result.  The lines printed with the prefix "[team]" are the table kept in profiles/team_primitives_mi355x.txt.
"""
import ctypes as C
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

from helpers import emu_lib, team_probe_lib

ND, NI, NF = 8, 4, 2          # PROBE_ND, PROBE_NI, PROBE_NF of tests/probe/team_probe.h
OPS = ("BCAST BCAST_I BCAST_F32 BCAST_U32 UNIFORM_I UNIFORM_D UNIFORM_B UNIFORM_U32 PERMUTE_F64 ROWGROUP_GATHER4 SHIFT_DOWN "
       "SHIFT_DOWN_I FROM_HALF BALLOT_BELOW FIRST_LANE_EQUAL FIRST_LANE_EQUAL_F32 QUAD_SUM ROW16_SUM ROWGROUP_SUM COLSUM COLSUM2 "
       "HALFSUM COLMAX COLMIN COLMAX_F32 ROW16_MAX_U32 COLARGMIN MFMA_F64 FAST_RCP FAST_RCP1 FAST_DIV FAST_SQRT_RSQRT "
       "FREXP_EXPONENT SCALE_POW2").split()
OP = {name: k for k, name in enumerate(OPS)}       # the enum of team_probe.h, in its order
NPS = (32, 40, 56, 64)
LANES = np.arange(64)
U = 2.0 ** -53
NO_PAYLOAD = 0x7fffffff
I_SENTINEL = 0x5a5a5a5a


def LW(NP):
    """lanes per half: 32 -> 32; 40, 56 and 64 -> 64"""
    return 32 if NP <= 32 else 64


def half_slices(NP):
    return [slice(0, 32), slice(32, 64)] if NP <= 32 else [slice(0, 64)]


class Cases:
    """a batch of one-wave probe cases; add() returns the case index, run() the outputs [case][slot][lane]"""

    def __init__(self):
        self.op, self.np, self.s, self.d, self.i, self.f = [], [], [], [], [], []

    def add(self, op, NP=64, s=0, d=(), i=(), f=()):
        D = np.zeros((ND, 64)); I = np.zeros((NI, 64), dtype=np.int32); F = np.zeros((NF, 64), dtype=np.float32)
        for j, a in enumerate(d):
            D[j] = a
        for j, a in enumerate(i):
            I[j] = np.asarray(a).astype(np.int64).astype(np.uint32).view(np.int32) if np.asarray(a).dtype != np.int32 else a
        for j, a in enumerate(f):
            F[j] = a
        self.op.append(OP[op]); self.np.append(NP); self.s.append(s); self.d.append(D); self.i.append(I); self.f.append(F)
        return len(self.op) - 1

    def run(self, target):
        n = len(self.op)
        assert 0 < n <= 4096
        op, np_, s = (np.array(a, dtype=np.int32) for a in (self.op, self.np, self.s))
        din, iin, fin = np.ascontiguousarray(self.d), np.ascontiguousarray(self.i), np.ascontiguousarray(self.f)
        dout = np.full((n, ND, 64), np.nan); iout = np.full((n, NI, 64), I_SENTINEL, dtype=np.int32)
        fout = np.full((n, NF, 64), np.nan, dtype=np.float32)
        fn = emu_lib().emu_team_probe if target == "twin" else team_probe_lib().osot_team_probe
        fn.argtypes = [C.c_int] + [C.c_void_p] * 9
        fn.restype = C.c_int
        rc = fn(n, *[a.ctypes.data for a in (op, np_, s, din, iin, fin, dout, iout, fout)])
        assert rc == 0, f"probe ({target}) returned {rc}"
        return dout, iout, fout


@pytest.fixture(params=["twin", pytest.param("device", marks=pytest.mark.gpu)])
def target(request):
    if request.param == "device":
        request.getfixturevalue("gpu_device")
    return request.param


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def assert_same(got, want, what):
    """bit for bit; the sign of a zero is compared numerically, a NaN matches any NaN"""
    got, want = np.asarray(got, dtype=np.float64), np.broadcast_to(np.asarray(want, dtype=np.float64), np.shape(got))
    ok = (bits(got) == bits(want)) | ((got == 0) & (want == 0)) | (np.isnan(got) & np.isnan(want))
    assert ok.all(), f"{what}: lanes {np.argwhere(~ok)[:8].tolist()} got {got[~ok][:8]} want {want[~ok][:8]}"


def lane_values(case):
    """lane-distinct values, so that any lane mix-up shows"""
    return 1000.0 * case + LANES


# ---------------------------------------------------------------------------------------------------- data movement
def test_broadcasts_from_every_source_lane(target):
    cs = Cases()
    for src in range(64):
        v = lane_values(src)
        cs.add("BCAST", s=src, d=[v + 0.25])
        cs.add("BCAST_I", s=src, i=[v.astype(np.int32)])
        cs.add("BCAST_F32", s=src, f=[v + 0.5])
        cs.add("BCAST_U32", s=src, i=[(v + 0xfff00000).astype(np.int64)])
    d, i, f = cs.run(target)
    for src in range(64):
        v = lane_values(src)
        assert_same(d[4 * src, 0], v[src] + 0.25, f"bcast from {src}")
        assert (i[4 * src + 1, 0] == int(v[src])).all(), f"bcast_i from {src}"
        assert (f[4 * src + 2, 0] == np.float32(v[src] + 0.5)).all(), f"bcast_f32 from {src}"
        assert (i[4 * src + 3, 0].view(np.uint32) == int(v[src]) + 0xfff00000).all(), f"bcast_u32 from {src}"


def test_uniform_takes_the_first_lane(target):
    """v_readfirstlane: lane 0's value for everybody.  uniform_d / uniform_b DECLARE a value uniform and the twin checks the
    declaration (it aborts on a lane that disagrees), so it is handed uniform values; the device gets lane-distinct ones."""
    cs = Cases()
    v = lane_values(3)
    distinct = target == "device"
    dv = v + 0.125 if distinct else np.full(64, 3000.125)
    bv = (LANES % 2 == 0).astype(np.int32) if distinct else np.ones(64, dtype=np.int32)
    a = cs.add("UNIFORM_I", i=[v.astype(np.int32)])
    b = cs.add("UNIFORM_U32", i=[(v + 0xfff00000).astype(np.int64)])
    c = cs.add("UNIFORM_D", d=[dv])
    e = cs.add("UNIFORM_B", i=[bv])
    e0 = cs.add("UNIFORM_B", i=[np.zeros(64, dtype=np.int32) if not distinct else (LANES % 2).astype(np.int32)])
    d, i, f = cs.run(target)
    assert (i[a, 0] == 3000).all() and (i[b, 0].view(np.uint32) == 3000 + 0xfff00000).all()
    assert_same(d[c, 0], 3000.125, "uniform_d")
    assert (i[e, 0] == 1).all() and (i[e0, 0] == 0).all()


def test_permute_gather_shift_from_half(target):
    rng = np.random.default_rng(11)
    cs, checks = Cases(), []
    for name, perm in (("identity", LANES), ("reversal", LANES[::-1]), ("seeded", rng.permutation(64))):
        v = lane_values(len(cs.op))
        k = cs.add("PERMUTE_F64", d=[v], i=[(4 * perm).astype(np.int32)])
        checks.append((k, 0, v[perm], f"permute_f64 {name}"))
    v = lane_values(len(cs.op))
    k = cs.add("ROWGROUP_GATHER4", d=[v])
    for q in range(4):
        checks.append((k, q, v[(LANES & 15) + 16 * q], f"rowgroup_gather4 element {q}"))
    ichecks = []
    for NP in NPS:
        lw = LW(NP)
        src = np.where((LANES % lw) + 1 < lw, LANES + 1, LANES)          # lanes 31 (NP = 32) and 63 keep their own
        v = lane_values(len(cs.op))
        checks.append((cs.add("SHIFT_DOWN", NP, d=[v]), 0, v[src], f"shift_down<{NP}>"))
        v = lane_values(len(cs.op))
        ichecks.append((cs.add("SHIFT_DOWN_I", NP, i=[v.astype(np.int32)]), v[src].astype(np.int32), f"shift_down_i<{NP}>"))
        for hsel in (0, 1):
            v = lane_values(len(cs.op))
            checks.append((cs.add("FROM_HALF", NP, s=hsel, d=[v]), 0, v[(LANES % 32) + 32 * hsel] if NP <= 32 else v, f"from_half<{NP}>({hsel})"))
    d, i, f = cs.run(target)
    for k, slot, want, what in checks:
        assert_same(d[k, slot], want, what)
    for k, want, what in ichecks:
        assert (i[k, 0] == want).all(), what
    assert np.isnan(d[0, 1]).all() and (i[0, 1] == I_SENTINEL).all(), "a case wrote a slot that is not its own"


# ---------------------------------------------------------------------------------------------------- masks
def mask_cases():
    rng = np.random.default_rng(5)
    ms = [np.zeros(64, bool), np.ones(64, bool), LANES % 2 == 0, LANES % 2 == 1, rng.random(64) < 0.5, rng.random(64) < 0.2]
    for b in (0, 31, 32, 63):
        ms.append(LANES == b)
    return ms


def test_ballot_and_lanes_below(target):
    cs = Cases()
    ms = mask_cases()
    for m in ms:
        cs.add("BALLOT_BELOW", i=[m.astype(np.int32) * 7])
    d, i, f = cs.run(target)
    for k, m in enumerate(ms):
        mask = sum(1 << int(b) for b in np.flatnonzero(m))
        got = i[k, 0].view(np.uint32).astype(np.uint64) | (i[k, 1].view(np.uint32).astype(np.uint64) << np.uint64(32))
        assert (got == np.uint64(mask)).all(), f"wave_ballot {mask:#x}: {got[0]:#x}"
        assert (i[k, 2] == np.concatenate([[0], np.cumsum(m)[:-1]])).all(), f"lanes_below {mask:#x}"


def test_first_lane_equal(target):
    cs, want = Cases(), []
    v = lane_values(1)

    def both(vals, m, w):
        cs.add("FIRST_LANE_EQUAL", d=[vals, np.full(64, m)]); want.append(w)
        cs.add("FIRST_LANE_EQUAL_F32", f=[vals, np.full(64, m)]); want.append(w)

    both(v, np.nan, 64)                                  # a NaN extremum equals nothing
    both(np.where(LANES == 0, np.nan, v), np.nan, 64)    # ... not even a NaN
    both(v, 5.0, 64)                                     # no match
    both(np.where(np.isin(LANES, (7, 31, 32, 50)), 5.0, v), 5.0, 7)       # several matches: the lowest
    both(np.where(LANES == 63, 5.0, v), 5.0, 63)         # lane 63 only
    both(np.where(LANES >= 32, 5.0, v), 5.0, 32)         # the upper half
    both(np.where(LANES == 40, -0.0, v), 0.0, 40)        # +0 == -0
    d, i, f = cs.run(target)
    for k, w in enumerate(want):
        assert (i[k, 0] == w).all(), f"case {k}: first_lane_equal gave {i[k, 0][0]}, want {w}"


# ---------------------------------------------------------------------------------------------------- min / max / argmin
def extremum_inputs():
    """(name, values[64]) for a MINIMUM (negate for a maximum); the two halves differ unless the name says otherwise"""
    rng = np.random.default_rng(7)
    out = []
    for pos in range(64):                                # a unique extremum at each lane position
        v = rng.permutation(64) + 10.0
        v[pos] = 3.5
        out.append((f"unique at {pos}", v))
    base = rng.permutation(64) + 10.0
    out.append(("ties", np.where(np.isin(LANES, (3, 17, 30, 33, 47, 62)), 2.0, base)))
    out.append(("all equal", np.full(64, 4.25)))
    out.append(("all +inf", np.full(64, np.inf)))
    out.append(("denormals", (rng.permutation(64) + 1) * 5e-324))
    out.append(("-inf in each half", np.where(np.isin(LANES, (9, 41)), -np.inf, base)))
    out.append(("+0 against -0", np.where(LANES % 3 == 0, -0.0, 0.0)))
    out.append(("NaN in lane 0", np.where(LANES == 0, np.nan, base)))
    out.append(("NaN in lanes 13 and 45", np.where(np.isin(LANES, (13, 45)), np.nan, base)))
    out.append(("all NaN", np.full(64, np.nan)))
    return out


@pytest.mark.parametrize("NP", NPS)
def test_colmin_colmax(target, NP):
    cs = Cases()
    ins = extremum_inputs()
    for name, v in ins:
        cs.add("COLMIN", NP, d=[v])
        cs.add("COLMAX", NP, d=[-v])
    d, i, f = cs.run(target)
    for k, (name, v) in enumerate(ins):
        for h in half_slices(NP):
            with np.errstate(invalid="ignore"):
                lo, hi = np.fmin.reduce(v[h]), np.fmax.reduce(-v[h])      # fmin / fmax: a NaN operand loses
            assert_same(d[2 * k, 0, h], lo, f"colmin<{NP}> {name}")
            assert_same(d[2 * k + 1, 0, h], hi, f"colmax<{NP}> {name}")
        if name == "+0 against -0" and NP == 64:
            print(f"[team] {target}: colmin<64>(+0, -0) = {'-0' if np.signbit(d[2 * k, 0, 0]) else '+0'}, "
                  f"colmax<64>(+0, -0) = {'-0' if np.signbit(d[2 * k + 1, 0, 0]) else '+0'} (compared numerically)")


def argmin_statement(v, p, NP):
    """NP > 32: the minimum over the non-NaN values of the columns, ties take the smallest payload; every candidate NaN: (NaN,
    0x7fffffff).  NP <= 32 (the device's data flow, which the solver only uses with both halves equal): the value is each
    half's own minimum; the payload is the lower half's minimiser's for all 64 lanes when that is a single lane, and
    otherwise (ties, or no lane equal to a NaN minimum) each half's own smallest payload among its minimisers."""
    val, pay = np.empty(64), np.empty(64, dtype=np.int64)
    hs = half_slices(NP)
    for h in hs:
        fin = ~np.isnan(v[h])
        m = v[h][fin].min() if fin.any() else np.nan
        at = v[h] == m
        val[h] = m
        pay[h] = p[h][at].min() if at.any() else NO_PAYLOAD
    if NP <= 32:
        at = v[:32] == val[0]
        if at.sum() == 1:
            pay[:] = p[:32][at][0]
    return val, pay


@pytest.mark.parametrize("NP", NPS)
def test_colargmin(target, NP):
    cs = Cases()
    ins = []
    pdesc = 5000 - LANES                                   # payloads descend with the lane: the smallest is NOT at the lowest lane
    for name, v in extremum_inputs():
        ins.append((name, v, pdesc))                       # halves differ (NP = 32: the device's data flow is the statement)
        if NP <= 32:                                       # ... and as the solver calls it: both halves hold the same candidates
            ins.append((name + " (replicated)", np.tile(v[:32], 2), np.tile(pdesc[:32], 2)))
    for name, v, p in ins:
        cs.add("COLARGMIN", NP, d=[v], i=[p.astype(np.int32)])
    d, i, f = cs.run(target)
    for k, (name, v, p) in enumerate(ins):
        val, pay = argmin_statement(v, p, NP)
        assert_same(d[k, 0], val, f"colargmin<{NP}> value, {name}")
        assert (i[k, 0] == pay).all(), f"colargmin<{NP}> payload, {name}: got {i[k, 0][[0, 63]]}, want {pay[[0, 63]]}"
        if "replicated" in name or NP > 32:                # the plain statement holds for every lane
            fin = ~np.isnan(v[:LW(NP)])
            if fin.any():
                m = v[:LW(NP)][fin].min()
                assert (i[k, 0] == p[:LW(NP)][v[:LW(NP)] == m].min()).all() and (d[k, 0] == m).all(), name
            else:
                assert (i[k, 0] == NO_PAYLOAD).all() and np.isnan(d[k, 0]).all(), name


def test_colmax_f32_and_row16_max_u32(target):
    rng = np.random.default_rng(9)
    f32 = np.float32
    sets = [("random", rng.random(64).astype(f32) * 100),
            ("-0 and +0", np.where(LANES % 2 == 0, f32(-0.0), f32(0.0)).astype(f32)),
            ("-0 against a denormal", np.where(LANES == 21, f32(1e-45), f32(-0.0)).astype(f32)),
            ("denormals", ((rng.permutation(64) + 1) * 1.4e-45).astype(f32)),
            ("inf in lane 37", np.where(LANES == 37, f32(np.inf), rng.random(64).astype(f32)).astype(f32)),
            ("max in lane 63", np.where(LANES == 63, f32(7.0), f32(1.0)).astype(f32)),
            ("max in lanes 0 and 32", np.where(LANES % 32 == 0, f32(7.0) + (LANES // 32), f32(1.0)).astype(f32))]
    # outside the documented domain (negative, NaN): the sign bit is cleared and the bit patterns reduce as unsigned integers
    outside = [("negative", -(rng.random(64).astype(f32) * 100)), ("NaN in lane 5", np.where(LANES == 5, f32(np.nan), rng.random(64).astype(f32)).astype(f32))]
    cs = Cases()
    for NP in NPS:
        for name, v in sets + outside:
            cs.add("COLMAX_F32", NP, f=[v])
    usets = [rng.integers(0, 2 ** 32, 64, dtype=np.uint64), np.where(LANES % 16 == 15 - LANES // 16, 0xffffffff, LANES).astype(np.uint64),
             np.zeros(64, dtype=np.uint64), np.where(LANES == 63, 0x80000000, 0x7fffffff).astype(np.uint64)]
    u0 = len(cs.op)
    for u in usets:
        cs.add("ROW16_MAX_U32", i=[u.astype(np.int64)])
    d, i, f = cs.run(target)
    k = 0
    for NP in NPS:
        for j, (name, v) in enumerate(sets + outside):
            in_domain = j < len(sets)
            for h in half_slices(NP):
                want = np.abs(v[h]).max() if in_domain else (v[h].view(np.uint32) & 0x7fffffff).max().astype(np.uint32).view(f32)
                assert (f[k, 0, h].view(np.uint32) == np.asarray(want, dtype=f32).view(np.uint32)).all(), f"colmax_f32<{NP}> {name}"
            if name == "-0 and +0" and NP == 64:
                print(f"[team] {target}: colmax_f32<64>(-0, +0) has the bit pattern {int(f[k, 0, 0].view(np.uint32)):#010x}")
            k += 1
    for j, u in enumerate(usets):
        want = np.repeat(u.reshape(4, 16).max(axis=1), 16)
        assert (i[u0 + j, 0].view(np.uint32) == want).all(), f"row16_max_u32 set {j}"


# ---------------------------------------------------------------------------------------------------- sums
def sum_orders(v):
    """the summation orders the twin states for the device: name -> per-lane result computed in float64 in that order"""
    l = LANES
    return {"QUAD_SUM": (v[l] + v[l ^ 1]) + (v[l ^ 2] + v[l ^ 3]),
            "ROWGROUP_SUM": (v[l & 15] + v[(l & 15) + 16]) + (v[(l & 15) + 32] + v[(l & 15) + 48])}


def exact_sum(v):
    return sum((Fraction(float(x)) for x in v), Fraction(0))


def cancelling(rng):
    """64 doubles with exponents spread over +-200 and heavy cancellation: half of them nearly undo the other half"""
    a = rng.uniform(1.0, 2.0, 32) * 2.0 ** rng.integers(-200, 201, 32) * rng.choice([-1.0, 1.0], 32)
    b = -a * (1.0 + rng.integers(-4, 5, 32) * 2.0 ** -50)
    v = rng.permutation(np.concatenate([a, b]))
    assert np.abs(v).sum() < 1e300
    return v


def test_sums_of_integers_are_exact(target):
    rng = np.random.default_rng(21)
    cs, checks = Cases(), []
    for rep in range(3):
        v = rng.integers(-2 ** 20, 2 ** 20 + 1, 64).astype(np.float64)
        w = rng.integers(-2 ** 20, 2 ** 20 + 1, 64).astype(np.float64)
        checks.append((cs.add("QUAD_SUM", d=[v]), 0, np.repeat(v.reshape(16, 4).sum(axis=1), 4), "quad_sum"))
        checks.append((cs.add("ROWGROUP_SUM", d=[v]), 0, np.tile(v.reshape(4, 16).sum(axis=0), 4), "rowgroup_sum"))
        if target == "device":                             # the twin has no row16_sum
            checks.append((cs.add("ROW16_SUM", d=[v]), 0, np.repeat(v.reshape(4, 16).sum(axis=1), 16), "row16_sum"))
        for NP in NPS:
            per_half = np.concatenate([np.full(h.stop - h.start, v[h].sum()) for h in half_slices(NP)])
            checks.append((cs.add("COLSUM", NP, d=[v]), 0, per_half, f"colsum<{NP}>"))
            k = cs.add("COLSUM2", NP, d=[v, w])
            # NP = 32: ra is the sum of lanes 0..31 of va, rb the sum of lanes 32..63 of vb, both in all lanes
            checks.append((k, 0, v[:32].sum() if NP <= 32 else v.sum(), f"colsum2<{NP}> ra"))
            checks.append((k, 1, w[32:].sum() if NP <= 32 else w.sum(), f"colsum2<{NP}> rb"))
            checks.append((cs.add("HALFSUM", NP, d=[v]), 0, np.tile(v[:32] + v[32:], 2) if NP <= 32 else v, f"halfsum<{NP}>"))
    d, i, f = cs.run(target)
    for k, slot, want, what in checks:
        assert_same(d[k, slot], want, what)
    if target == "device":
        dt, _, _ = cs.run("twin")
        skip = [k for k, o in enumerate(cs.op) if o == OP["ROW16_SUM"]]
        keep = np.setdiff1d(np.arange(len(cs.op)), skip)
        assert (bits(d[keep, :2]) == bits(dt[keep, :2])).all(), "device and twin differ on integer-valued sums"


def test_sums_of_cancelling_doubles(target):
    """quad_sum, rowgroup_sum and halfsum: the twin states the device's ORDER, so the result is that order's, bit for bit
    (twin against the order written out in numpy; device against the twin).  row16_sum, colsum and colsum2 are a tree of
    depth d on the device (4 for a row of 16, 5 for 32 lanes, 6 for 64) and a sequential sum on the twin (d = 31 or 63):
    |result - exact| <= d u sum|v| / (1 - d u), the standard bound for any summation of that depth.  Nothing is measured."""
    rng = np.random.default_rng(22)
    cs, ordered, bounded = Cases(), [], []
    for rep in range(6):
        v, w = cancelling(rng), cancelling(rng)
        for name, want in sum_orders(v).items():
            ordered.append((cs.add(name, d=[v]), want, name))
        for NP in NPS:
            ordered.append((cs.add("HALFSUM", NP, d=[v]), np.tile(v[:32] + v[32:], 2) if NP <= 32 else v, f"halfsum<{NP}>"))
            depth = (5 if NP <= 32 else 6) if target == "device" else LW(NP) - 1
            k = cs.add("COLSUM", NP, d=[v])
            for h in half_slices(NP):
                bounded.append((k, 0, h, v[h], depth, f"colsum<{NP}>"))
            k = cs.add("COLSUM2", NP, d=[v, w])
            bounded.append((k, 0, slice(0, 64), v[:32] if NP <= 32 else v, depth, f"colsum2<{NP}> ra"))
            bounded.append((k, 1, slice(0, 64), w[32:] if NP <= 32 else w, depth, f"colsum2<{NP}> rb"))
        if target == "device":
            k = cs.add("ROW16_SUM", d=[v])
            for r in range(4):
                bounded.append((k, 0, slice(16 * r, 16 * r + 16), v[16 * r:16 * r + 16], 4, "row16_sum"))
    d, i, f = cs.run(target)
    for k, want, what in ordered:
        assert_same(d[k, 0], want, what)
    for k, slot, lanes, terms, depth, what in bounded:
        got = d[k, slot, lanes]
        assert (bits(got) == bits(got)[0]).all(), f"{what}: the lanes of one reduction hold different results"
        exact, mag = exact_sum(terms), exact_sum(np.abs(terms))
        bound = depth * Fraction(U) * mag / (1 - depth * Fraction(U))
        assert abs(Fraction(float(got[0])) - exact) <= bound, f"{what}: off by {float(abs(Fraction(float(got[0])) - exact)):.3e}, bound {float(bound):.3e}"
    if target == "device":
        dt, _, _ = cs.run("twin")
        for k, want, what in ordered:
            assert (bits(d[k, 0]) == bits(dt[k, 0])).all(), f"{what}: the device does not add in the order the twin states"


# ---------------------------------------------------------------------------------------------------- matrix core
MFMA_TWIN_ULPS = 0      # the twin's chain acc = fma(a_k, b_k, acc), k = 0..3, IS the matrix core's rounding (see the twin's comment)


def mfma_lanes(A, B, Cm):
    """A [16][4], B [4][16], C [16][16] -> per-lane a, b, c[4]: lane l supplies A[l & 15][l >> 4] and B[l >> 4][l & 15] and
    holds C / D [(l >> 4) + 4 r][l & 15] in element r"""
    a = A[LANES & 15, LANES >> 4]
    b = B[LANES >> 4, LANES & 15]
    c = [Cm[(LANES >> 4) + 4 * r, LANES & 15] for r in range(4)]
    return [a, b] + c


def mfma_unpack(dk):
    D = np.empty((16, 16))
    for r in range(4):
        D[(LANES >> 4) + 4 * r, LANES & 15] = dk[r]
    return D


def test_mfma_f64_16x16x4(target):
    rng = np.random.default_rng(31)
    ints = [(rng.integers(-1000, 1001, (16, 4)).astype(float), rng.integers(-1000, 1001, (4, 16)).astype(float),
             rng.integers(-10 ** 6, 10 ** 6, (16, 16)).astype(float)) for _ in range(2)]
    # distinct per (row, k) and (k, col): every entry of D names the A row and the B column that made it
    m, k4, n = np.arange(16)[:, None], np.arange(4)[None, :], np.arange(16)[None, :]
    ints.append((1.0 + m + 16 * k4, 1000.0 * (1 + np.arange(4)[:, None]) + 37.0 * n, np.zeros((16, 16))))
    rnd = []
    for _ in range(4):
        A, B = rng.normal(size=(16, 4)) * 2.0 ** rng.integers(-20, 21, (16, 4)), rng.normal(size=(4, 16)) * 2.0 ** rng.integers(-20, 21, (4, 16))
        Cm = -(A @ B) * (1.0 + rng.normal(size=(16, 16)) * 1e-8)      # the accumulator nearly cancels the product
        rnd.append((A, B, Cm))
    cs = Cases()
    for A, B, Cm in ints + rnd:
        cs.add("MFMA_F64", d=mfma_lanes(A, B, Cm))
    d, i, f = cs.run(target)
    for k, (A, B, Cm) in enumerate(ints):
        assert_same(mfma_unpack(d[k]), A @ B + Cm, f"mfma integer case {k} (A / B / D lane layout)")
    g8 = Fraction(8) * Fraction(U) / (1 - 8 * Fraction(U))
    for k, (A, B, Cm) in enumerate(rnd):
        D = mfma_unpack(d[len(ints) + k])
        for r in range(16):
            for c in range(16):
                terms = [Fraction(A[r, q]) * Fraction(B[q, c]) for q in range(4)]
                exact = Fraction(Cm[r, c]) + sum(terms)
                mag = abs(Fraction(Cm[r, c])) + sum(abs(t) for t in terms)
                assert abs(Fraction(D[r, c]) - exact) <= g8 * mag, f"mfma random case {k} D[{r}][{c}]"
    if target == "device":
        dt, _, _ = cs.run("twin")
        worst = 0
        for k in range(len(ints), len(ints) + len(rnd)):
            worst = max(worst, int(np.abs(bits(d[k, :4]) - bits(dt[k, :4])).max()))
        print(f"[team] mfma_f64_16x16x4 against the twin's k = 0..3 fma chain: " + ("bit-equal" if worst == 0 else f"largest difference {worst} ulp"))
        assert worst == MFMA_TWIN_ULPS, "the matrix core's rounding against the twin's fma chain is not what the twin's comment records"


# ---------------------------------------------------------------------------------------------------- scalar numerics
NSAMPLE = 2 ** 16
DBL_MIN, DBL_MAX, DENORM = 2.0 ** -1022, float(np.finfo(np.float64).max), 5e-324
EDGES = np.array([1.0, 1.0 + 2.0 ** -52, 2.0 - 2.0 ** -52])


def ulps(got, ref):
    """distance in units of the last place between doubles of one sign (both normal)"""
    return np.abs(bits(got) - bits(ref))


@functools.lru_cache(maxsize=None)
def rcp_sample():
    rng = np.random.default_rng(41)
    e = np.arange(-1000, 1001)
    edge = (EDGES[:, None] * 2.0 ** e[None, :]).ravel()
    n = NSAMPLE - 2 * edge.size
    x = np.concatenate([edge, -edge, rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(-1000, 1001, n) * rng.choice([-1.0, 1.0], n)])
    assert x.size == NSAMPLE
    return x


@functools.lru_cache(maxsize=None)
def div_sample():
    """(a, b, n_exact): the first n_exact pairs are exact quotients a = q b"""
    rng = np.random.default_rng(42)
    nq = 4096
    q = rng.integers(1, 2 ** 26, nq).astype(float) * 2.0 ** rng.integers(-400, 401, nq)
    bq = rng.integers(1, 2 ** 26, nq).astype(float) * 2.0 ** rng.integers(-400, 401, nq) * rng.choice([-1.0, 1.0], nq)
    aq = q * bq                                           # exact: 52 bits at the most
    e = np.arange(-500, 501)
    eb = (EDGES[:, None] * 2.0 ** e[None, :]).ravel()
    ea = np.roll(eb, 7)[::-1].copy()
    n = NSAMPLE - nq - eb.size
    b = rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(-1000, 1001, n) * rng.choice([-1.0, 1.0], n)
    qe = rng.integers(-999, 1000, n)                      # the quotient's exponent stays within +-1000
    ae = np.clip(qe + np.floor(np.log2(np.abs(b))).astype(int), -1000, 1000)
    a = rng.uniform(1.0, 2.0, n) * 2.0 ** ae * rng.choice([-1.0, 1.0], n)
    A, Bv = np.concatenate([aq, ea, a]), np.concatenate([bq, eb, b])
    ex = np.floor(np.log2(np.abs(A / Bv)))
    assert A.size == NSAMPLE and (np.abs(ex) <= 1001).all()
    return A, Bv, nq


@functools.lru_cache(maxsize=None)
def sqrt_sample():
    """(x, n_squares, n_pow4, correctly rounded 1 / sqrt(x)): the first n_squares are k^2, the next n_pow4 are 4^e"""
    import mpmath
    rng = np.random.default_rng(43)
    sq = np.arange(1, 4097, dtype=float) ** 2
    p4 = 4.0 ** np.arange(-500, 501)
    e = np.arange(-1000, 1000, 2)
    edge = (np.concatenate([EDGES, [4.0 - 2.0 ** -51, 2.0, 2.0 + 2.0 ** -51]])[:, None] * 2.0 ** e[None, :]).ravel()
    n = NSAMPLE - sq.size - p4.size - edge.size
    x = np.concatenate([sq, p4, edge, rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(-1000, 1000, n)])
    assert x.size == NSAMPLE and (x >= 2.0 ** -1000).all() and (x <= 2.0 ** 1000).all()
    mpmath.mp.prec = 100
    rs = np.array([float(1 / mpmath.sqrt(mpmath.mpf(float(v)))) for v in x])      # 100 bits, rounded once to 53
    return x, sq.size, p4.size, rs


def run_scalar(target, op, slots):
    """slots: list of arrays of NSAMPLE-like length -> the outputs [ND][n], each lane of each case one argument"""
    n = slots[0].size
    per = 64 * (ND // len(slots))
    nblk = -(-n // per)
    pad = [np.concatenate([s, np.ones(nblk * per - n)]).reshape(nblk, ND // len(slots), 64) for s in slots]
    cs = Cases()
    for k in range(nblk):
        cs.add(op, d=np.concatenate([p[k] for p in pad]))
    d, i, f = cs.run(target)
    g = ND // len(slots)
    return [d[:, j * g:(j + 1) * g].reshape(-1)[:n] for j in range(len(slots))] if len(slots) > 1 else \
        [d.reshape(-1)[:n]]


def test_fast_rcp_within_one_ulp(target):
    x = rcp_sample()
    r = run_scalar(target, "FAST_RCP", [x])[0]
    worst = int(ulps(r, 1.0 / x).max())
    print(f"[team] {target}: fast_rcp, {x.size} normal arguments: largest error {worst} ulp from the correctly rounded 1 / x")
    assert worst <= 1


def test_fast_rcp1_within_two_ulp(target):
    x = rcp_sample()
    r = run_scalar(target, "FAST_RCP1", [x])[0]
    worst = int(ulps(r, 1.0 / x).max())
    print(f"[team] {target}: fast_rcp1, {x.size} normal arguments: largest error {worst} ulp from the correctly rounded 1 / x")
    assert worst <= 2


def test_fast_div_within_one_ulp(target):
    a, b, nq = div_sample()
    # FAST_DIV: slots 0..3 are a, slots 4..7 the matching b; outputs in slots 0..3
    q = run_scalar(target, "FAST_DIV", [a, b])[0]
    worst = int(ulps(q, a / b).max())
    inexact = int((q[:nq] != (a / b)[:nq]).sum())
    print(f"[team] {target}: fast_div, {a.size} normal pairs: largest error {worst} ulp from the correctly rounded a / b; "
          f"{inexact} of {nq} exact quotients a = q b do not come back as q (not asserted)")
    assert worst <= 1


def test_fast_sqrt_rsqrt_within_one_ulp_and_exact_on_exact_roots(target):
    x, nsq, np4, rs_ref = sqrt_sample()
    s, rs = run_scalar(target, "FAST_SQRT_RSQRT", [x, x])      # (the second half of the slots is output only)
    ws, wr = int(ulps(s, np.sqrt(x)).max()), int(ulps(rs, rs_ref).max())
    print(f"[team] {target}: fast_sqrt_rsqrt, {x.size} normal arguments: s at most {ws} ulp from the correctly rounded root, "
          f"rs at most {wr} ulp from the correctly rounded 1 / sqrt(x)")
    # "exact inputs stay exact": the root of every perfect square, and both results for 4^e
    assert (s[:nsq] == np.arange(1, nsq + 1)).all(), "the root of a perfect square is not exact"
    assert (s[nsq:nsq + np4] == 2.0 ** np.arange(-500, 501)).all() and (rs[nsq:nsq + np4] == 2.0 ** -np.arange(-500.0, 501.0)).all(), "4^e"
    assert ws <= 1 and wr <= 1


# the sequence of the device's routines, stated in numpy on an IEEE seed (rcp(0) = inf, rcp(inf) = 0, rsq(0) = inf, rsq(inf) = 0,
# rsq(x < 0) = NaN) with an exactly rounded fused multiply-add
def fma(a, b, c):
    a, b, c = float(a), float(b), float(c)
    if math.isnan(a) or math.isnan(b) or math.isnan(c):
        return math.nan
    if math.isinf(a) or math.isinf(b):
        if a == 0 or b == 0:
            return math.nan
        p = math.copysign(math.inf, a) * math.copysign(1.0, b)
        return math.nan if math.isinf(c) and c != p else p
    if math.isinf(c):
        return c
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    if exact == 0:
        psign = math.copysign(1.0, a) * math.copysign(1.0, b)
        if Fraction(a) * Fraction(b) == 0 and c == 0:
            return -0.0 if psign < 0 and math.copysign(1.0, c) < 0 else 0.0
        return 0.0
    try:
        return float(exact)            # correctly rounded (ties to even), denormals included
    except OverflowError:
        return math.copysign(math.inf, exact)


def ieee_rcp(x):
    with np.errstate(all="ignore"):
        return float(np.float64(1.0) / np.float64(x))


def ieee_rsq(x):
    with np.errstate(all="ignore"):
        return float(np.float64(1.0) / np.sqrt(np.float64(x)))


def seq_rcp(x):
    r = ieee_rcp(x)
    for _ in range(2):
        e = fma(-x, r, 1.0)
        r = fma(r, e, r)
    return r


def seq_rcp1(x):
    r = ieee_rcp(x)
    e = fma(-x, r, 1.0)
    return fma(r, fma(e, e, e), r)


def seq_div(a, b):
    r = seq_rcp(b)
    with np.errstate(all="ignore"):
        q = float(np.float64(a) * np.float64(r))
    return fma(fma(-b, q, a), r, q)


def seq_sqrt(x):
    with np.errstate(all="ignore"):
        y = ieee_rsq(x)
        g, h = float(np.float64(x) * np.float64(y)), 0.5 * y
        r = fma(-h, g, 0.5)
        g, h = fma(g, r, g), fma(h, r, h)
        r = fma(-h, g, 0.5)
        g, h = fma(g, r, g), fma(h, r, h)
        g = fma(fma(-g, g, x), h, g)
        q = float(np.float64(h) + np.float64(h))
    return g, fma(q, fma(-g, q, 1.0), q)


def klass(v):
    v = float(v)
    if math.isnan(v):
        return "NaN"
    s = "-" if math.copysign(1.0, v) < 0 else "+"
    return s + ("inf" if math.isinf(v) else "0" if v == 0 else "finite")


SPECIALS = [0.0, -0.0, DENORM, DBL_MIN, DBL_MAX, math.inf, -1.0, math.nan]
DIV_SPECIALS = [(1.0, 0.0), (1.0, -0.0), (0.0, 1.0), (-0.0, 1.0), (0.0, 0.0), (1.0, math.inf), (math.inf, 1.0), (math.inf, math.inf),
                (DBL_MAX, DBL_MIN), (DBL_MIN, DBL_MAX), (1.0, math.nan), (math.nan, 1.0), (1.0, DENORM), (DENORM, 1.0), (-1.0, DBL_MAX),
                (0.0, -3.0)]


def test_special_arguments_have_the_class_of_the_device_sequence(target):
    """zero, infinite, NaN, negative and denormal arguments: what comes back has the class (NaN, +-inf, +-0, finite with its
    sign) of the device's own steps run on the IEEE seed.  fast_rcp(0), fast_rcp(inf), fast_sqrt_rsqrt(0) are NaN."""
    cs = Cases()
    sp = np.array(SPECIALS + [1.0] * (64 - len(SPECIALS)))
    da = np.array([a for a, b in DIV_SPECIALS] + [1.0] * (64 - len(DIV_SPECIALS)))
    db = np.array([b for a, b in DIV_SPECIALS] + [1.0] * (64 - len(DIV_SPECIALS)))
    one = np.ones(64)
    k_rcp = cs.add("FAST_RCP", d=[sp] + [one] * 7)
    k_rcp1 = cs.add("FAST_RCP1", d=[sp] + [one] * 7)
    k_div = cs.add("FAST_DIV", d=[da, one, one, one, db, one, one, one])
    k_sqrt = cs.add("FAST_SQRT_RSQRT", d=[sp, one, one, one])
    d, i, f = cs.run(target)
    bad = []
    for j, x in enumerate(SPECIALS):
        s, rs = seq_sqrt(x)
        for name, got, want in (("fast_rcp", d[k_rcp, 0, j], seq_rcp(x)), ("fast_rcp1", d[k_rcp1, 0, j], seq_rcp1(x)),
                                ("fast_sqrt_rsqrt s", d[k_sqrt, 0, j], s), ("fast_sqrt_rsqrt rs", d[k_sqrt, 4, j], rs)):
            print(f"[team] {target}: {name}({x!r}) = {float(got)!r}  [sequence on the IEEE seed: {want!r}]")
            if klass(got) != klass(want):
                bad.append((name, x, float(got), want))
    for j, (a, b) in enumerate(DIV_SPECIALS):
        got, want = d[k_div, 0, j], seq_div(a, b)
        print(f"[team] {target}: fast_div({a!r}, {b!r}) = {float(got)!r}  [sequence on the IEEE seed: {want!r}]")
        if klass(got) != klass(want):
            bad.append(("fast_div", (a, b), float(got), want))
    assert klass(seq_rcp(0.0)) == "NaN" and klass(seq_rcp(math.inf)) == "NaN" and klass(seq_sqrt(0.0)[0]) == "NaN"
    assert not bad, bad


def test_frexp_exponent_and_scale_pow2(target):
    xs = np.array([0.0, -0.0, DENORM, 3 * DENORM, 2.0 ** -1040, DBL_MIN, 1.0, -1.0, 0.75, 3.0, DBL_MAX, math.inf, -math.inf, 1e-300, 6.5e200, -2.0 ** 52])
    x4 = np.concatenate([xs] * 4)
    shift = np.repeat(np.array([0, 1100, -1100, 60], dtype=np.int32), xs.size)
    shift2 = np.repeat(np.array([-1074, 1023, -52, 2100], dtype=np.int32), xs.size)
    cs = Cases()
    a = cs.add("FREXP_EXPONENT", d=[x4] * 4)
    b = cs.add("SCALE_POW2", d=[x4] * 4, i=[shift, shift2, shift, shift2])
    d, i, f = cs.run(target)
    want_e = np.array([math.frexp(v)[1] for v in x4])          # frexp's exponent: 0 for zero and for inf
    assert (i[a, 0] == want_e).all(), f"frexp_exponent: {i[a, 0][:xs.size]} want {want_e[:xs.size]}"
    with np.errstate(all="ignore"):
        assert_same(d[b, 0], np.ldexp(x4, shift), "scale_pow2 (overflow, underflow into and out of the denormals)")
        assert_same(d[b, 1], np.ldexp(x4, shift2), "scale_pow2")
