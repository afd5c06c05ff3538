"""EccChip's ec_add_unequal (non-strict) and ec_double filled on the device (h2hip_ec_fill_dev: every own cell of a curve operation, the 9 k
range checks left as gaps for h2hip_range_fill_checks_dev), shared by tests/test_ec_fill.py (the CPU-emulated build) and
tests/test_ec_fill_gpu.py: every check takes a ctx.  Every comparison is bit-exact.

The definition is a Python-integer restatement of the two reference functions (halo2-ecc/src/ecc/mod.rs:153-179, :302-327) over
virtual_region.Context, GateChip and RangeChip, built from restatements of sub_no_carry::crt, scalar_mul_no_carry::crt, mul_no_carry::crt,
FpChip::load_private, check_carry_mod_to_zero::crt and carry_mod::crt (with divide_unsafe, fields/mod.rs:217-238), the range checks included,
so one thread holds the full run and the lookup queue.

  A  the fill against the definition over sentinel-filled columns: the bare call (own cells, gaps untouched, results), ec_fill_with_ranges
     (the whole run and the lookup columns), ec_layout and ec_range_tables alike;
  B  chaining: a call reads R = P + Q from the results of the call before it, a third doubles it;
  C  column breaks: the same thread laid down by virtual_region.assign_witnesses and by the fill;
  D  every reachable refusal; E  the structs in the header, the Rust sys crate and ctypes;
  F  a BaseConfig proof of R = P + Q, D = 2 R, S = D + P whose trace three fill calls write.
"""
import math

import numpy as np

from halo2_lib_amd import plonk as PL
from halo2_lib_amd import virtual_region as VR
from tests import fp_mul_checks as F
from tests import fused_fill_harness as FH
from tests.fp_mul_checks import BN254_Q, MODULI, SECP_N, SECP_P, Spec
from tests.fused_fill_harness import SENTINEL, EcOp, compare, lookup_positions, own_mask, place, signed, tdiv
from tests.util import R, fr

ADD, DOUBLE = PL.EC_ADD_UNEQUAL, PL.EC_DOUBLE
OPS = {"add_unequal": ADD, "double": DOUBLE}
SOLVE_BLOCK, PLACE_BLOCK = 64, 256   # ec_fill.hip: lanes per workgroup of the per-unit and of the per-(unit, segment) kernel
PARAMS = [(88, 3, 8), (88, 3, 18), (90, 3, 15), (64, 4, 8)]   # (limb_bits, num_limbs, lookup_bits)
CURVES = {"secp256k1_p": (SECP_P, 7, (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798,
                                       0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)),
          "bn254_q": (BN254_Q, 3, (1, 2))}


def segments(k, op):
    """lanes per unit of the placing kernel: 7 subs, 3 (k + 1) product limbs, the load, 3 k + 2 of the zero check, 2 (3 k + 3) of the two
    carry_mods (DOUBLE: 3 scalar products, 4 products, 4 subs)"""
    return (7 + 3 * (k + 1) if op == ADD else 3 + 4 * (k + 1) + 4) + 1 + 3 * k + 2 + 2 * (3 * k + 3)


# ------------------------------------------------------------------------------------------------ curve arithmetic in integers
def aff_add(p, a, b):
    lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, p) % p
    x = (lam * lam - a[0] - b[0]) % p
    return x, (lam * (a[0] - x) - a[1]) % p


def aff_double(p, a):
    lam = 3 * a[0] * a[0] * pow(2 * a[1], -1, p) % p
    x = (lam * lam - 2 * a[0]) % p
    return x, (lam * (a[0] - x) - a[1]) % p


def multiples(curve, count):
    """G, 2 G, ..., count G of a curve of CURVES, each checked to lie on it"""
    p, b, g = CURVES[curve]
    out = [g]
    for i in range(1, count):
        out.append(aff_double(p, g) if i == 1 else aff_add(p, out[-1], g))
    assert all((y * y - x * x * x - b) % p == 0 for x, y in out)
    return out


# ------------------------------------------------------------------------------------------------ the definition
class Crt:
    """CRTInteger: the limb cells, the native cell, the integer the reference tracks beside them, max_limb_bits"""

    def __init__(self, limbs, native, value, mlb):
        self.limbs, self.native, self.value, self.mlb = limbs, native, value, mlb

    def cells(self):
        return self.limbs + [self.native]


def operand(sp, cells):
    """a CRT operand from k + 1 cells; its integer is the library's definition for every input: sum (cell_i mod 2^n) 2^(n i)"""
    mask = (1 << sp.n) - 1
    return Crt(list(cells[:sp.k]), cells[sp.k], sum((c.value & mask) << (sp.n * i) for i, c in enumerate(cells[:sp.k])), sp.n)


def sub_no_carry(ctx, a, b):
    """sub_no_carry::crt (bigint/sub_no_carry.rs:24-34)"""
    limbs = [VR.GateChip.sub(ctx, x, y) for x, y in zip(a.limbs, b.limbs)]
    return Crt(limbs, VR.GateChip.sub(ctx, a.native, b.native), a.value - b.value, max(a.mlb, b.mlb) + 1)


def scalar_mul_no_carry(ctx, a, c):
    """scalar_mul_no_carry::crt (bigint/scalar_mul_no_carry.rs:20-39), c > 0"""
    limbs = [VR.GateChip.mul(ctx, x, VR.Constant(c)) for x in a.limbs]
    return Crt(limbs, VR.GateChip.mul(ctx, a.native, VR.Constant(c)), a.value * c, a.mlb + (c - 1).bit_length())


def mul_no_carry(ctx, sp, a, b):
    """mul_no_carry::crt (bigint/mul_no_carry.rs:37-49)"""
    log2_ceil = (sp.k - 1).bit_length()
    assert log2_ceil + a.mlb + b.mlb <= 252
    limbs = [VR.GateChip.inner_product(ctx, a.limbs[:i + 1], list(reversed(b.limbs[:i + 1]))) for i in range(sp.k)]
    return Crt(limbs, VR.GateChip.mul(ctx, a.native, b.native), a.value * b.value, log2_ceil + a.mlb + b.mlb)


def _ranged(u, ctx, chip, cell, bits, res):
    at = len(ctx.advice)
    chip.range_check(ctx, cell, bits)
    u.gaps.append((at - u.start, len(ctx.advice) - at, bits, res))
    u.results[res] = cell.value


def load_private(ctx, chip, sp, value, u, res):
    """FpChip::load_private (fields/fp.rs:187-197): the limbs, evaluate_native, range_check at Fp::NUM_BITS = bits(p)"""
    n, k = sp.n, sp.k
    limbs = [ctx.load_witness((value >> (n * i)) & ((1 << n) - 1)) for i in range(k)]
    native = VR.RangeChip._inner_product_from_one(ctx, limbs, [VR.Constant(c) for c in sp.limb_bases])
    remaining = sp.p.bit_length()
    for i, cell in enumerate(limbs):                                          # fp.rs:334-338
        bits = min(n, remaining)
        remaining -= bits
        _ranged(u, ctx, chip, cell, bits, res + i)
    u.results[res + k] = native.value
    return Crt(limbs, native, value, n)


def _decompose(v, k, n):
    """decompose_bigint (halo2-base/src/utils/mod.rs:290-296): the low k limbs of |v|, negated in Fr for a negative v"""
    limbs = [(abs(v) >> (n * i)) & ((1 << n) - 1) for i in range(k)]
    return [-x % R for x in limbs] if v < 0 else limbs


def _quot_shifts(u, ctx, chip, sp, quot_assigned, res):
    for i, cell in enumerate(quot_assigned):
        bits = sp.quot_last if i == sp.k - 1 else sp.n
        _ranged(u, ctx, chip, VR.GateChip.add(ctx, cell, VR.Constant(pow(2, bits, R))), bits + 1, res + i)


def _carry_to_zero(u, ctx, chip, sp, check_assigned, mlb, res):
    """check_carry_to_zero::truncate (bigint/check_carry_to_zero.rs:27-86) -> rb"""
    n, lb = sp.n, sp.lb
    rb = (mlb - n + 1 + lb) // lb * lb - 1
    carries, previous = [], None
    for cell in check_assigned:
        carries.append(tdiv(signed(cell.value) + (carries[-1] if carries else 0), 1 << n))
    for i, (cell, carry) in enumerate(zip(check_assigned, carries)):
        ctx.assign_region([VR.Existing(cell), VR.Witness(-carry % R), VR.Constant(sp.limb_bases[1]),
                           VR.Existing(previous) if previous is not None else VR.Constant(0)], [0])
        neg_carry = ctx.get(-3)
        _ranged(u, ctx, chip, VR.GateChip.add(ctx, neg_carry, VR.Constant(pow(2, rb, R))), rb + 1, res + i)
        previous = neg_carry
    return rb


def check_carry_mod_to_zero(ctx, chip, sp, a, u, res):
    """check_carry_mod_to_zero::crt (bigint/check_carry_mod_to_zero.rs:16-125); the debug assertions assert nothing here"""
    n, k = sp.n, sp.k
    quot, rem = divmod(a.value, sp.p)                                         # :44 div_mod_floor
    u.quots.append((quot, rem))
    quot_vec = _decompose(quot, k, n)
    quot_assigned, check_assigned = [], []
    u.zero_gate_offsets = []
    for i in range(k):                                                        # :71-87
        row_offset = len(ctx.advice)
        prod = VR.GateChip.inner_product(ctx, quot_assigned + [VR.Witness(quot_vec[i])], [VR.Constant(m) for m in reversed(sp.mod_vec[:i + 1])])
        new_quot = ctx.get(row_offset + 1 + 3 * i)
        ctx.assign_region([VR.Constant(R - 1), VR.Existing(a.limbs[i]), VR.Witness((prod.value - a.limbs[i].value) % R)], [-1])
        u.zero_gate_offsets.append(len(ctx.advice) - 4 - u.start)
        check_assigned.append(ctx.last())
        quot_assigned.append(new_quot)
    _quot_shifts(u, ctx, chip, sp, quot_assigned, res)                        # :92-100
    u.rb.append(_carry_to_zero(u, ctx, chip, sp, check_assigned, max(a.mlb, 2 * n + k.bit_length()), res + k))   # :102-113
    quot_native = VR.RangeChip._inner_product_from_one(ctx, quot_assigned, [VR.Constant(c) for c in sp.limb_bases])
    ctx.assign_region([VR.Constant(0), VR.Constant(sp.mod_native), VR.Existing(quot_native), VR.Existing(a.native)], [0])   # :121-124


def carry_mod(ctx, chip, sp, a, u, res_out, res):
    """carry_mod::crt (bigint/carry_mod.rs:29-191) of the CRT value a; the debug assertions assert nothing here"""
    n, k = sp.n, sp.k
    quot, out = divmod(a.value, sp.p)                                         # :68 div_mod_floor
    u.quots.append((quot, out))
    out_vec, quot_vec = _decompose(out, k, n), _decompose(quot, k, n)
    quot_assigned, out_assigned, check_assigned = [], [], []
    for i in range(k):                                                        # :100-134
        row_offset = len(ctx.advice)
        prod = VR.GateChip.inner_product(ctx, quot_assigned + [VR.Witness(quot_vec[i])], [VR.Constant(m) for m in reversed(sp.mod_vec[:i + 1])])
        new_quot = ctx.get(row_offset + 1 + 3 * i)
        temp1 = (prod.value - a.limbs[i].value) % R
        ctx.assign_region([VR.Constant(R - 1), VR.Existing(a.limbs[i]), VR.Witness(temp1), VR.Constant(1), VR.Witness(out_vec[i]),
                           VR.Witness((temp1 + out_vec[i]) % R)], [-1, 2])
        check_assigned.append(ctx.last())
        out_assigned.append(ctx.get(-2))
        quot_assigned.append(new_quot)
        u.out_offsets.append(len(ctx.advice) - 2 - u.start)
    for i, cell in enumerate(out_assigned):                                   # :139-142
        _ranged(u, ctx, chip, cell, sp.out_last if i == k - 1 else n, res_out + i)
    _quot_shifts(u, ctx, chip, sp, quot_assigned, res)                        # :145-153
    u.rb.append(_carry_to_zero(u, ctx, chip, sp, check_assigned, max(max(n, a.mlb) + 1, 2 * n + k.bit_length()), res + k))   # :155-168
    bases = [VR.Constant(c) for c in sp.limb_bases]
    quot_native = VR.RangeChip._inner_product_from_one(ctx, quot_assigned, bases)
    out_native = VR.RangeChip._inner_product_from_one(ctx, out_assigned, bases)
    ctx.assign_region([VR.Constant(sp.mod_native), VR.Existing(quot_native), VR.Existing(a.native)], [-1])   # :181-184
    u.results[res_out + k] = out_native.value
    u.out_offsets.append(len(ctx.advice) - 4 - u.start)
    return Crt(out_assigned, out_native, out, n)


def divide_unsafe(ctx, chip, sp, a, b, u):
    """FieldChip::divide_unsafe (fields/mod.rs:217-238); b_val.invert().unwrap_or_default(): 0 for a denominator with no inverse"""
    k = sp.k
    a_val, b_val = a.value % sp.p, b.value % sp.p
    quot_val = a_val * pow(b_val, -1, sp.p) % sp.p if math.gcd(b_val, sp.p) == 1 else 0
    lam_offsets = [len(ctx.advice) - u.start + i for i in range(k)]
    quot = load_private(ctx, chip, sp, quot_val, u, 2 * (k + 1))
    u.lam_offsets = lam_offsets + [u.gaps[0][0] - 1]
    quot_b = mul_no_carry(ctx, sp, quot, b)
    check_carry_mod_to_zero(ctx, chip, sp, sub_no_carry(ctx, quot_b, a), u, 3 * k + 3)
    return quot


class Unit:
    pass


def ec_op(ctx, chip, sp, op, pt, qt=None):
    """ec_add_unequal(P, Q, is_strict = false) or ec_double(P) of points given as 2 (k + 1) cells (x's limbs and native, then y's) -> a
    Unit: where its run starts, the gaps (start, cells, width, results index) in context order, the offsets of the cells of x3, y3 and lambda,
    the results entries, the out cells, the three (quotient, remainder) pairs"""
    k = sp.k
    u = Unit()
    u.start, u.queue = len(ctx.advice), len(chip.lookup_manager.cells_to_lookup.get(ctx.tag(), []))
    u.gaps, u.results, u.quots, u.rb, u.out_offsets = [], [None] * (9 * k + 3), [], [], []
    px, py = operand(sp, pt[:k + 1]), operand(sp, pt[k + 1:])
    if op == ADD:                                                             # ecc/mod.rs:162-178
        qx, qy = operand(sp, qt[:k + 1]), operand(sp, qt[k + 1:])
        dx = sub_no_carry(ctx, qx, px)
        dy = sub_no_carry(ctx, qy, py)
        lam = divide_unsafe(ctx, chip, sp, dy, dx, u)
        lam_sq = mul_no_carry(ctx, sp, lam, lam)
        x3nc = sub_no_carry(ctx, sub_no_carry(ctx, lam_sq, px), qx)
    else:                                                                     # :309-318
        two_y = scalar_mul_no_carry(ctx, py, 2)
        three_x = scalar_mul_no_carry(ctx, px, 3)
        three_x_sq = mul_no_carry(ctx, sp, three_x, px)
        lam = divide_unsafe(ctx, chip, sp, three_x_sq, two_y, u)
        lam_sq = mul_no_carry(ctx, sp, lam, lam)
        x3nc = sub_no_carry(ctx, lam_sq, scalar_mul_no_carry(ctx, px, 2))
    x3 = carry_mod(ctx, chip, sp, x3nc, u, 0, 5 * k + 3)
    dx13 = sub_no_carry(ctx, px, x3)
    y3nc = sub_no_carry(ctx, mul_no_carry(ctx, sp, lam, dx13), py)
    y3 = carry_mod(ctx, chip, sp, y3nc, u, k + 1, 7 * k + 3)
    u.lam, u.x3, u.y3 = lam.value, x3.value, y3.value
    u.out_offsets += u.lam_offsets
    u.out_cells = x3.cells() + y3.cells()
    u.end = len(ctx.advice)
    u.lookups = len(chip.lookup_manager.cells_to_lookup.get(ctx.tag(), [])) - u.queue
    return u


def unit_def(sp, op, p_vals, q_vals=None):
    """one unit on a thread of its own -> (the Unit, its cells, the lookup values in queue order, the thread)"""
    ctx, chip, _ = FH.thread(sp.lb)
    u = ec_op(ctx, chip, sp, op, FH.operand(p_vals, 0), FH.operand(q_vals, 1) if op == ADD else None)
    return u, list(ctx.advice), [c.value for c in chip.lookup_manager.cells_to_lookup.get(ctx.tag(), [])], ctx


def point(sp, x, y):
    return sp.crt(x) + sp.crt(y)


def operand_pool(sp, modulus, seed=0xEC):
    """[(P's 2 (k + 1) values, Q's)]: curve points (where the modulus has a curve), arbitrary reduced pairs, Q = P + (1, 1) (lambda = 1 and
    lambda^2 - x1 - x2 < 0), P.x = Q.x with equal and with different y (the denominator is 0: lambda = 0), y = 0 (DOUBLE's denominator is 0),
    coordinates from {0, 1, p - 1}, a coordinate equal to p and one equal to 2^(n k) - 1 (improper values, truncated quotients), one improper
    limb x_1 = 2^n"""
    p, n, k = sp.p, sp.n, sp.k
    g = np.random.default_rng([seed, n, k, p % (1 << 32)])
    rnd = [int.from_bytes(g.bytes(40), "little") % p for _ in range(8)]
    top = (1 << (n * k)) - 1
    pairs = []
    if modulus in CURVES:
        m = multiples(modulus, 6)
        pairs += [(m[0], m[1]), (m[4], m[2]), (m[5], m[3]), (m[1], m[5])]
    pairs += [((rnd[0], rnd[1]), (rnd[2], rnd[3])), ((rnd[4], rnd[5]), (rnd[6], rnd[7]))]
    pairs += [((rnd[0], rnd[1]), (rnd[0] + 1, rnd[1] + 1)), ((5, 9), (6, 10))]                      # lambda = 1 (the first unless a coordinate is p - 1)
    pairs += [((rnd[2], rnd[3]), (rnd[2], rnd[3])), ((rnd[2], rnd[3]), (rnd[2], rnd[5]))]           # P.x = Q.x
    pairs += [((rnd[4], 0), (rnd[5], 0)), ((0, 1), (1, p - 1)), ((p - 1, p - 1), (0, 0)), ((1, 0), (p - 1, 1))]
    pairs += [((p, rnd[1]), (rnd[2], top)), ((top, rnd[3]), (rnd[0], p)), ((top, top), (rnd[6], rnd[7]))]
    pool = [(point(sp, *a), point(sp, *b)) for a, b in pairs]
    a = point(sp, rnd[0], rnd[1])
    a[1] = 1 << n                                                             # the improper limb x_1 = 2^n
    pool.append((a, point(sp, rnd[2], rnd[3])))
    return pool


def check_definition():
    """the restatement itself: for points of secp256k1 and of BN254 G1 (x3, y3) is the affine sum / double computed independently; every flex
    gate of the thread holds; the cell counts are the issue's at k = 3 and the layout's everywhere; the carry_mod part fed a product of proper
    operands gives fp_mul_checks.fp_mul's cells; at (88, 3) the three carry widths come from max_limb_bits 180, 181, 181 (ADD_UNEQUAL)"""
    for n, k, lb in PARAMS:
        for curve, (p, _b, _g) in CURVES.items():
            sp = Spec(n, k, lb, p)
            m = multiples(curve, 7)
            for a, b in ((m[0], m[1]), (m[2], m[6]), (m[5], m[3])):
                for op, want in ((ADD, aff_add(p, a, b)), (DOUBLE, aff_double(p, a))):
                    u, cells, lookups, ctx = unit_def(sp, op, point(sp, *a), point(sp, *b))
                    assert (u.x3, u.y3) == want, (curve, n, op)
                    got = [sum(cells[off] << (n * i) for i, off in enumerate(u.out_offsets[j * (k + 1):j * (k + 1) + k])) for j in range(3)]
                    assert got == [want[0], want[1], u.lam] and all(rem == 0 for _q, rem in u.quots[:1]), (curve, n, op)
                    assert [cells[u.out_offsets[j * (k + 1) + k]] for j in range(3)] == [v % R for v in got]
                    # at n k = 256 DOUBLE's 3 x^2 passes the reference's bound |a| <= 2^(n k - 1 + 252): the zero check's quotient has more than
                    # k limbs, decompose_bigint drops them and the native identity over the truncated quot_native cannot hold
                    truncated = any(abs(q) >> (n * k) for q, _rem in u.quots)
                    assert not truncated or ((n, k) == (64, 4) and op == DOUBLE), (curve, n, k, op)
                    bad = [s for s, q in enumerate(ctx.selector) if q and (cells[s] + cells[s + 1] * cells[s + 2] - cells[s + 3]) % R]
                    assert (len(bad) == 1 and cells[bad[0] + 1] == p % R) if truncated else not bad, (curve, n, k, lb, op, bad)
                    lay = PL.ec_layout(sp.params(), op)
                    own = int(own_mask(u).sum())
                    assert (lay.num_cells, lay.num_own_cells, lay.num_lookup_cells) == (len(cells), own, len(lookups)) and len(u.gaps) == 9 * k
                    if k == 3:
                        assert own == (458 if op == ADD else 483), own
    sp = Spec(88, 3, 18, SECP_P)
    m = multiples("secp256k1_p", 3)
    u, _c, _l, _t = unit_def(sp, ADD, point(sp, *m[0]), point(sp, *m[2]))
    rb = lambda mlb: (mlb - 88 + 1 + 18) // 18 * 18 - 1
    assert u.rb == [rb(180), rb(181), rb(181)], u.rb
    u, _c, _l, _t = unit_def(sp, DOUBLE, point(sp, *m[0]))
    assert u.rb == [rb(181), rb(180), rb(181)], u.rb
    # carry_mod over mul_no_carry of proper operands: FpChip::mul's cells, as tests/fp_mul_checks.py states them
    for n, k, lb in PARAMS:
        sp = Spec(n, k, lb, SECP_N)
        for a_vals, b_vals in F.operand_pairs(sp, 7)[:12]:
            want = F.unit_def(sp, a_vals, b_vals)
            ctx, chip, _ = FH.thread(lb)
            u = Unit()
            u.start, u.gaps, u.results, u.quots, u.rb, u.out_offsets = 0, [], [None] * (3 * k + 1), [], [], []
            a, b = operand(sp, FH.operand(a_vals, 0)), operand(sp, FH.operand(b_vals, 1))
            carry_mod(ctx, chip, sp, mul_no_carry(ctx, sp, a, b), u, 0, k + 1)
            assert list(ctx.advice) == want[1] and [c.value for c in chip.lookup_manager.cells_to_lookup[ctx.tag()]] == want[2], (n, k, lb)
            assert u.gaps == want[0].gaps and u.results == want[0].results


CARRY_WIDTHS = (88, 3, 47)   # lookup_bits 47 divides 94: max_limb_bits 180 and 181 round to different carry widths (rb 93 and 140)


def check_three_carry_widths(ctx):
    """a parameter set at which a unit's reductions do not share one carry width: the layout's widths and the fill (both ops, bare and with
    ranges) against the definition"""
    n, k, lb = CARRY_WIDTHS
    sp = Spec(n, k, lb, SECP_P)
    m = multiples("secp256k1_p", 3)
    assert unit_def(sp, ADD, point(sp, *m[0]), point(sp, *m[2]))[0].rb == [93, 140, 140]
    assert unit_def(sp, DOUBLE, point(sp, *m[0]))[0].rb == [140, 93, 140]
    pool = operand_pool(sp, "secp256k1_p")
    for op in (ADD, DOUBLE):
        check_op_fill(ctx, n, k, lb, "secp256k1_p", op, 5, pool=pool[:10])


def check_pool_signs():
    """the pools contain a negative and a positive quotient in each of the three reductions and an exact multiple of p in at least one"""
    for op in (ADD, DOUBLE):
        for n, k, lb in PARAMS[:1] + PARAMS[-1:]:
            for modulus, p in MODULI.items():
                sp = Spec(n, k, lb, p)
                quots = [unit_def(sp, op, a, b)[0].quots for a, b in operand_pool(sp, modulus)]
                for r in range(3):
                    assert any(q[r][0] < 0 for q in quots) and any(q[r][0] > 0 for q in quots), (op, modulus, r)
                assert any(q[r][1] == 0 for q in quots for r in range(3)), (op, modulus)
                assert any(q[0][1] != 0 for q in quots), "no unit whose zero check has a remainder (denominator 0, numerator != 0)"


# ------------------------------------------------------------------------------------------------ A: the fill against its definition
def width_groups(gaps):
    """{width: [gap index]} in the order of first appearance"""
    groups = {}
    for j, g in enumerate(gaps):
        groups.setdefault(g[2], []).append(j)
    return groups


def check_layout_and_ranges():
    """ec_layout equals the definition's counts, gaps and offsets for every parameter set, modulus and op; ec_range_tables gives, per width in
    the order of first appearance, the definition's positions and lookup queue order unit by unit, rows and slots ascending inside a width"""
    for n, k, lb in PARAMS + [CARRY_WIDTHS]:
        for modulus, p in MODULI.items():
            sp = Spec(n, k, lb, p)
            for op in (ADD, DOUBLE):
                u, cells, lookups, _ = unit_def(sp, op, point(sp, 3, 5), point(sp, p - 2, 11))
                lay = PL.ec_layout(sp.params(), op)
                assert (lay.num_cells, lay.num_own_cells, lay.num_lookup_cells) == (len(cells), int(own_mask(u).sum()), len(lookups)), (n, k, lb)
                assert lay.ranges == u.gaps and lay.out_cell_offsets == u.out_offsets, (n, k, lb, op, lay, u.gaps, u.out_offsets)
                assert len(width_groups(u.gaps)) <= 7
    sp = Spec(88, 3, 8, SECP_P)
    for op in (ADD, DOUBLE):
        thread, chip, _ = FH.thread(sp.lb)
        bps, ncols, units, slots_, defs = [700, 650], 3, [], [], []
        pos = (0, 5)
        thread.advice += [0] * 5
        for j in range(4):
            u = ec_op(thread, chip, sp, op, FH.operand(point(sp, 3 + j, 5), 2 * j), FH.operand(point(sp, 9, 11 + j), 2 * j + 1))
            units.append(pos + (0, 0))
            slots_.append(u.queue + 3)
            defs.append(u)
            pos = place(pos[0], pos[1], u.end - u.start, bps, ncols)[1]
        tables = PL.ec_range_tables(bps, ncols, sp.params(), op, units, slots_)
        groups = width_groups(defs[0].gaps)
        assert [w for w, _t in tables] == list(groups)
        queue_before = lambda u, j: sum(-(-g[2] // sp.lb) + (1 if g[2] % sp.lb > 1 else 0) for g in u.gaps[:j])
        for (width, table), idx in zip(tables, groups.values()):
            want = []
            for ui, u in enumerate(defs):
                first = {}
                for i, c, r in place(units[ui][0], units[ui][1], u.end - u.start, bps, ncols)[0]:
                    first.setdefault(i, (c, r))
                want += [first[u.gaps[j][0]] + (ui * (9 * sp.k + 3) + u.gaps[j][3], slots_[ui] + queue_before(u, j)) for j in idx]
            got = [(t.column, t.row, t.a_offset, t.lookup_slot) for t in table]
            assert got == want, (op, width)
            assert all(a[3] < b[3] and (a[0], a[1]) < (b[0], b[1]) for a, b in zip(got, got[1:])), "slots and rows ascend inside a width"


def check_op_fill(ctx, n, k, lb, modulus, op, count, nl=1, pool=None):
    """the harness's check_fill over the operand pool: the bare call and ec_fill_with_ranges over nl lookup columns"""
    sp = Spec(n, k, lb, MODULI[modulus])
    FH.check_fill(ctx, EcOp(sp, op), operand_pool(sp, modulus) if pool is None else pool, count, nl)


# ------------------------------------------------------------------------------------------------ B: chaining
def check_chained(ctx, n, k, lb, count=3):
    """R = P + Q by a first call; a second call adds P to R read from the first call's results (values_dev = the first call's results_dev,
    where unit j's point lies at j (9 k + 3), and, both points of a unit indexing one buffer, Q = R of another unit); a third doubles the second's
    results.  Columns, lookup columns and the three results buffers equal the definition's over sentinels; with curve points the final point is
    2 ((P + Q) + (P' + Q')) computed in integers."""
    p = SECP_P
    sp = Spec(n, k, lb, p)
    nres, pt = 9 * k + 3, 2 * (k + 1)
    m = multiples("secp256k1_p", 2 * count + 2)
    firsts = [(point(sp, *m[2 * j]), point(sp, *m[2 * j + 3])) for j in range(count)]
    vals = [v for a, b in firsts for v in a + b]
    defs1 = [unit_def(sp, ADD, a, b) for a, b in firsts]
    ncells = len(defs1[0][1])
    units1 = [(0, 2 + j * (ncells + 1), 2 * pt * j, 2 * pt * j + pt) for j in range(count)]
    ops2 = [(defs1[j][0].results[:pt], defs1[(j + 1) % count][0].results[:pt]) for j in range(count)]
    defs2 = [unit_def(sp, ADD, a, b) for a, b in ops2]
    units2 = [(1, 1 + j * (ncells + 2), nres * j, nres * ((j + 1) % count)) for j in range(count)]
    defs3 = [unit_def(sp, DOUBLE, defs2[j][0].results[:pt]) for j in range(count)]
    ncells3 = len(defs3[0][1])
    units3 = [(2, 4 + j * (ncells3 + 1), nres * j, 0) for j in range(count)]
    for j in range(count):
        s1, s2 = aff_add(p, m[2 * j], m[2 * j + 3]), aff_add(p, m[2 * ((j + 1) % count)], m[2 * ((j + 1) % count) + 3])
        assert (defs3[j][0].x3, defs3[j][0].y3) == aff_double(p, aff_add(p, s1, s2))
    slots_, slot = [[], []], 3
    for which, defs in enumerate((defs2, defs3)):
        for u, _c, lookups, _t in defs:
            slots_[which].append(slot)
            slot += len(lookups) + 1
    rows_n = max(4 + count * (ncells3 + 2), slot) + 9
    where = lookup_positions(slot, 1)
    sent, sent_res = np.tile(SENTINEL, (rows_n, 1)), np.tile(SENTINEL, (count * nres + 2, 1))
    d_cols = [ctx.to_device(sent) for _ in range(3)]
    d_lk = ctx.to_device(sent)
    d_vals = ctx.to_device(fr(vals))
    d_res = [ctx.to_device(sent_res) for _ in range(3)]
    try:
        PL.ec_fill(ctx, d_cols, rows_n - 2, None, sp.params(), ADD, d_vals, len(vals), d_res[0], count * nres, units1)
        PL.ec_fill_with_ranges(ctx, d_cols, rows_n - 2, None, [d_lk], sp.params(), ADD, d_res[0], count * nres, d_res[1], count * nres, units2, slots_[0])
        PL.ec_fill_with_ranges(ctx, d_cols, rows_n - 2, None, [d_lk], sp.params(), DOUBLE, d_res[1], count * nres, d_res[2], count * nres, units3, slots_[1])
        ctx.sync()
        want = [sent.copy() for _ in range(3)]
        want_lk, want_res = sent.copy(), [sent_res.copy() for _ in range(3)]
        for which, (units, defs) in enumerate(((units1, defs1), (units2, defs2), (units3, defs3))):
            for j, ((col, row, _a, _b), (u, cells, lookups, _t)) in enumerate(zip(units, defs)):
                keep = own_mask(u) if which == 0 else np.ones(len(cells), dtype=bool)
                want[col][row:row + len(cells)][keep] = fr(cells)[keep]
                want_res[which][j * nres:(j + 1) * nres] = fr(u.results)
                if which:
                    for i, v in enumerate(fr(lookups)):
                        want_lk[where[slots_[which - 1][j] + i][1]] = v
        compare(ctx, d_cols + [d_lk] + d_res, want + [want_lk] + want_res, "chained calls, (n, k, lb) = (%d, %d, %d)" % (n, k, lb))
    finally:
        for ptr in d_cols + [d_lk, d_vals] + d_res:
            ctx.free(ptr)


# ------------------------------------------------------------------------------------------------ C: column breaks
def _break_cells(sp):
    """the cell of an ADD_UNEQUAL unit each case's break falls on, from the definition's own offsets"""
    u, cells, _, _ = unit_def(sp, ADD, point(sp, 3, 5), point(sp, 7, 11))
    k = sp.k
    return {
        "a_subtraction": 4 * (k + 1) + 5,                         # dy = sub(Q.y, P.y), its second gate: out [b] 1 a
        "load_witness_cells": u.lam_offsets[1],
        "zero_check_overlapped_gate": u.zero_gate_offsets[1],     # prod_1, the cell the three-cell region's gate starts on
        "a_gap": u.gaps[k + 1][0] + 1,                            # inside the range check of zero's q_1 + B (the range fill writes the copy)
        "out_native": u.out_offsets[k],                           # x3's, overlapped by the native identity's gate
        "unit_last": len(cells) - 1,                              # the next unit right behind
    }


BREAK_CASES = ["a_subtraction", "load_witness_cells", "zero_check_overlapped_gate", "a_gap", "out_native", "unit_last"]


def check_op_breaks(ctx, case, ncols, op=ADD):
    """the harness's check_breaks over (88, 3, 8) units through ec_fill_with_ranges: the first break inside the third unit, every later one
    3 units further down the thread, each on the cell the case names"""
    sp = Spec(88, 3, 8, SECP_P)
    kind = EcOp(sp, op)
    ncells, filler = kind.layout(ctx.lib).num_cells, 50
    targets = [(2 + 3 * b, _break_cells(sp)[case]) for b in range(ncols - 1)]
    usable = max(FH.break_points(filler, ncells, targets)) + 100
    pool = operand_pool(sp, "secp256k1_p", 0xB7)
    FH.check_breaks(ctx, kind, [pool[(5 * j) % len(pool)] for j in range(targets[-1][0] + 2)], targets, filler, usable, ncols)


# ------------------------------------------------------------------------------------------------ D: the refusals
def check_rejections(ctx):
    """one case per reachable refusal: H2HIP_ERR_INVALID, the reason in h2hip_last_error, the sentinel everywhere (columns and results); then
    count == 0 and a good call from the same context.  Not reachable: a product with ceil(log2 k) + a + b > 252 (n k <= 318 and k >= 3 give
    n <= 106, and the largest product, DOUBLE's 3 x * x, has 2 + (n + 2) + n <= 216 bits) and a width whose limbs take more than 253 bits."""
    sp = Spec(88, 3, 8, SECP_P)
    nres, pt = 30, 8
    kind = EcOp(sp, ADD)
    lay = kind.layout(ctx.lib)
    ncells = lay.num_cells
    m = multiples("secp256k1_p", 4)
    vals = [v for a in m for v in point(sp, *a)]
    with FH.RefusalBench(ctx, kind, vals, (0, pt), (pt, 2 * pt), ncells, segments(3, ADD), 4 * nres) as b:
        usable, nv, fill, refused = b.usable, b.nv, b.fill, b.refused
        b.refuse_nulls()
        refused("an unknown op", "unknown op", fill([b.ok], op=2))
        b.refuse_params(behind={"a limb of p equal to 1": [("bits(p) > 256", "more than 256 bits", dict(p=(1 << 260) + 12345)),
                                                           ("p even", "even", dict(p=(1 << 255) + 12346)),
                                                           ("n k > 318", "> 318", dict(n=80, k_=4, p=SECP_P))]})
        b.refuse_placement()
        refused("P past values_len", "outside values_len", fill([b.ok, (1, 0, nv - pt + 1, 0)]))
        refused("Q past values_len", "outside values_len", fill([(1, 0, 0, (1 << 64) - 2)]))
        b.refuse_results_len()
        b.refuse_count()
        b.refuse_overlaps(lay.ranges[0][0])
        b.refuse_aliasing((5, 300))
        for what, prm, op in (("layout: flags", FH.par(flags=2), ADD), ("layout: p", FH.par(p=0), DOUBLE), ("layout: op", kind.params, 7)):
            FH.layout_refused(what, lambda: PL.ec_layout(prm, op, ctx.lib))
        # count == 0 needs nothing
        ctx._chk(ctx.lib.h2hip_ec_fill_dev(ctx.handle, None, 0, 0, None, None, 9, None, 0, None, 0, None, 0))
        # the largest run that still fits (its last cell on row usable - 1), a point that ends with values_len, a DOUBLE whose q_offset is
        # past everything (ignored), a unit that ends on its break point
        units = [(0, usable - ncells, nv - pt, 0), (1, 30, pt, 2 * pt)]
        bps = [usable - 1, 30 + ncells - 1]
        fill(units, bps=bps, rlen=2 * nres)()
        lay2 = PL.ec_layout(sp.params(), DOUBLE, ctx.lib)
        dbl = [(2, 3, 2 * pt, (1 << 64) - 1)]
        fill(dbl, op=DOUBLE, rdev=b.d_res + 32 * 2 * nres, rlen=nres)()
        ctx.sync()
        want = [np.tile(SENTINEL, (b.n_rows, 1)) for _ in range(3)]
        want_res = np.tile(SENTINEL, (4 * nres, 1))
        for j, (op, (col, row, a, b_)) in enumerate([(ADD, units[0]), (ADD, units[1]), (DOUBLE, dbl[0])]):
            u, cells, _, _ = unit_def(sp, op, vals[a:a + pt], vals[b_:b_ + pt] if op == ADD else None)
            own = own_mask(u)
            for i, c, r in place(col, row, len(cells), bps if op == ADD else None, 3)[0]:
                if own[i]:
                    want[c][r] = fr([cells[i]])[0]
            want_res[j * nres:(j + 1) * nres] = fr(u.results)
        assert lay2.num_cells + 3 < b.n_rows
        compare(ctx, b.d_cols + [b.d_res], want + [want_res], "after the refusals")


# ------------------------------------------------------------------------------------------------ E: the structs in every layer
def check_struct_layout():
    """h2hip_ec_op: the same fields in the header, the Rust sys crate and ctypes, 24 bytes; the two op constants alike; every function named
    in the C++ mirror and the safe Rust wrapper"""
    FH.check_names(constants=[("H2HIP_EC_ADD_UNEQUAL", ADD), ("H2HIP_EC_DOUBLE", DOUBLE)], structs=[("h2hip_ec_op", PL.EcOpStruct, 24)],
                   mirrored=("h2hip_ec_fill_dev", "h2hip_ec_layout", "h2hip_ec_range_checks"))
    assert [nm for nm, _ty in PL.EcOpStruct._fields_] == ["column", "row", "p_offset", "q_offset"]
    assert PL.EcOpStruct.p_offset.offset == 8 and PL.EcOpStruct.q_offset.offset == 16


# ------------------------------------------------------------------------------------------------ F: inside a proof
def _ec_program(builder, sp, p_vals, q_vals):
    """loads P and Q as witnesses (2 (k + 1) cells each), then R = P + Q, D = 2 R, S = D + P.  The first limb of P.x is the instance.
    -> [(thread offset of the unit's first cell, queue position, the Unit)] of the three units"""
    ctx = builder.main()
    chip = VR.RangeChip(sp.lb, builder.lookup_manager)
    pt, qt = [ctx.load_witness(v) for v in p_vals], [ctx.load_witness(v) for v in q_vals]
    r = ec_op(ctx, chip, sp, ADD, pt, qt)
    d = ec_op(ctx, chip, sp, DOUBLE, r.out_cells)
    s = ec_op(ctx, chip, sp, ADD, d.out_cells, pt)
    builder.assigned_instances = [[pt[0]]]
    return [(u.start, u.queue, u) for u in (r, d, s)]


def check_proof(ctx, kk, seed, nl, mode="proof"):
    """F: a BaseConfig circuit built through the Context mirror (R = P + Q, D = 2 R, S = D + P on secp256k1 at (88, 3)); keygen from the
    mirror's selectors and copies; the device advice starts with the loaded witnesses only; three ec_fill_with_ranges calls (each reads the
    results of the one before) write every other gate cell and the whole lookup columns.  mode "proof": the columns equal the Python-computed
    advice, the proof has the bytes of the proof from it, both verifiers accept it, check_witness finds nothing; with the lambda_1 witness
    cell of the first unit changed by one on the device check_witness reports copy constraints only (load_private's witness cells lie on no
    gate); with the copy of lambda_1 inside the product lambda * dx changed instead, the gate row of that product's inner product, which
    feeds the zero check.  mode "equal_x": Q = (P.x, another
    y): the denominator is 0, lambda = 0, the fill still equals the definition and check_witness names the zero check's native identity."""
    lb = kk - 1
    sp = Spec(88, 3, lb, SECP_P)
    k, nres, pt = sp.k, 9 * sp.k + 3, 2 * (sp.k + 1)
    m = multiples("secp256k1_p", 5)
    p_vals = point(sp, *m[1])
    q_vals = point(sp, *m[4]) if mode == "proof" else point(sp, m[1][0], m[4][1])
    with FH.ProofBench(ctx, kk, nl, lb, seed, lambda builder: _ec_program(builder, sp, p_vals, q_vals)) as pb:
        calls, first = pb.calls, pb.first
        # one device buffer: [gate columns][results of R][of D][of S]: a unit finds one point in the results of the call before it, P among the witnesses
        res_at = pb.buffers(3 * nres, [range(2 * pt)])
        res_at = [res_at + j * nres for j in range(3)]
        tables = [first[calls[0][0]] + (0, pt), first[calls[1][0]] + (res_at[0], 0), first[calls[2][0]] + (res_at[1], 0)]
        for j, op in enumerate((ADD, DOUBLE, ADD)):
            PL.ec_fill_with_ranges(ctx, pb.d_cols, pb.sh.usable_rows, pb.bps, pb.d_lks, sp.params(), op, pb.d_gate, len(pb.host), pb.d_gate + 32 * res_at[j], nres,
                                   [tables[j]], [calls[j][1]])
        ctx.sync()
        pb.check_columns()
        s0, _q, u0 = calls[0]
        if mode == "equal_x":
            assert u0.lam == 0 and u0.quots[0][1] != 0
            total_f, fails = pb.check_witness(max_failures=4096)
            # the zero check's native identity 0 + m_nat * quot_native = qc_nat is the gate four cells before x3's first reduction segment
            native_gate = first[s0 + u0.gaps[3 * k - 1][0] + u0.gaps[3 * k - 1][1] + 3 * k - 2]
            assert total_f >= 1 and any(f.kind == "gate" and (f.column, f.row) == native_gate for f in fails), (native_gate, fails[:8])
            return
        pb.check_proof()
        # ---- the lambda_1 witness cell itself changed by one: its copies no longer equal it, no gate sees it
        total_f, fails = pb.changed(s0 + u0.lam_offsets[1])
        assert total_f >= 1 and fails and all(f.kind == "copy" for f in fails), fails
        # ---- lambda_1 changed by one on the device, where the zero check reads it: its copy inside ip(lambda_0, lambda_1; dx_1, dx_0), the
        # second limb of lambda * dx (0 l_0 dx_1 s_0 [l_1] dx_0 s_1).  The gate on s_0 no longer holds: a row of divide_unsafe's constraint
        off = u0.gaps[k - 1][0] + u0.gaps[k - 1][1] + 4 + 4             # behind lambda's last gap: ip_0 (4 cells), then 0 l_0 dx_1 s_0 [l_1]
        assert pb.cell(s0 + off) == pb.cell(s0 + u0.lam_offsets[1])
        gate_row = first[s0 + off - 1]
        assert first[s0 + off + 2] == (gate_row[0], gate_row[1] + 3), "a break cuts the gate"
        total_f, fails = pb.changed(s0 + off)
        assert total_f >= 1 and any(f.kind == "gate" and (f.column, f.row) == gate_row for f in fails), fails
