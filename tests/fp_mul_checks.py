"""FpChip::mul filled on the device (h2hip_fp_mul_fill_dev: the cells of mul_no_carry::crt and carry_mod::crt, the nine range checks left as
gaps for h2hip_range_fill_checks_dev), shared by tests/test_fp_mul.py (the CPU-emulated build) and tests/test_fp_mul_gpu.py: every check
takes a ctx.  Every comparison is bit-exact.

The definition is a Python-integer restatement of the four reference functions over virtual_region.Context, GateChip and RangeChip
(halo2-ecc/src/bigint/mul_no_carry.rs:9-49, carry_mod.rs:29-191, check_carry_to_zero.rs:27-86, bigint/mod.rs:66-74 evaluate_native), the nine
range_check calls included, so one thread holds the full run and the lookup queue.

  A  the fill against the definition over sentinel-filled columns (a stray write fails): the bare call (own cells, gaps untouched, results),
     fp_mul_fill_with_ranges (the whole run and the lookup columns), fp_mul_layout and trace_seek alike;
  B  column breaks: the same thread laid down by virtual_region.assign_witnesses and by the fill;
  C  every refusal: H2HIP_ERR_INVALID, its reason in h2hip_last_error, all columns and results untouched (but "a width whose limbs take more
     than 253 bits": with n <= 125 and lookup_bits <= 63 every width is at most 191 bits and its limbs at most 252, so no parameters reach it);
  D  the structs in the header, the Rust sys crate and ctypes;
  E  a BaseConfig proof whose field multiplications two fill calls write, the second reading the first's results.
"""
import itertools

import numpy as np

import halo2_lib_amd as H
from halo2_lib_amd import plonk as PL
from halo2_lib_amd import virtual_region as VR
from tests import fused_fill_harness as FH
from tests.fused_fill_harness import ERR_INVALID, SENTINEL, FpMul, compare, lookup_positions, operand, own_mask, place, signed, tdiv, thread
from tests.util import R, fr

SOLVE_BLOCK, PLACE_BLOCK = 64, 256   # fp_mul.hip: lanes per workgroup of the per-unit and of the per-(unit, slot) kernel
SECP_P = (1 << 256) - (1 << 32) - 977
SECP_N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
BN254_Q = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
MODULI = {"secp256k1_p": SECP_P, "secp256k1_n": SECP_N, "bn254_q": BN254_Q}
PARAMS = [(88, 3, 8), (88, 3, 18), (90, 3, 15), (91, 3, 13), (64, 4, 8)]   # (limb_bits, num_limbs, lookup_bits)


def slots(k):
    """lanes per unit of the placing kernel"""
    return 4 * k + 3


# ------------------------------------------------------------------------------------------------ the definition
class Spec:
    """what FpChip::new derives (fields/fp.rs:57-95) and the widths carry_mod / check_carry_to_zero compute"""

    def __init__(self, n, k, lb, p):
        self.n, self.k, self.lb, self.p = n, k, lb, p
        mask = (1 << n) - 1
        self.mod_vec = [(p >> (n * i)) & mask for i in range(k)]
        self.mod_native = p % R
        self.limb_bases = [pow(2, n * i, R) for i in range(k)]
        self.quot_max_bits = n * k - 1 + 254 - 1 - p.bit_length()             # carry_mod.rs:53
        self.quot_last = self.quot_max_bits - n * (k - 1)                      # :58
        self.out_last = p.bit_length() - n * (k - 1)                           # :62
        log2_ceil, k_bits = (k - 1).bit_length(), k.bit_length()
        self.max_limb_bits = max(max(n, log2_ceil + 2 * n) + 1, 2 * n + k_bits)   # :155-158, a.truncation.max_limb_bits from mul_no_carry.rs:34
        self.rb = (self.max_limb_bits - n + 1 + lb) // lb * lb - 1             # check_carry_to_zero.rs:52-55
        self.widths = [n, self.out_last, n + 1, self.quot_last + 1, self.rb + 1]

    def params(self):
        return PL.fp_params(self.n, self.k, self.lb, self.p)

    def crt(self, x):
        """the k limbs and the native residue of the integer x < 2^(n k)"""
        return [(x >> (self.n * i)) & ((1 << self.n) - 1) for i in range(self.k)] + [x % R]


class Unit:
    pass


def fp_mul(ctx, chip, sp, a, b):
    """FieldChip::mul (fields/mod.rs:188-196) of the CRT integers a, b (k limb cells, then the native cell) -> a Unit: where its run starts,
    the gaps (start, cells, width, results index) in context order, the offsets of o_i / out_native, the results entries, the out cells"""
    n, k, p = sp.n, sp.k, sp.p
    mask = (1 << n) - 1
    u = Unit()
    u.start, u.queue = len(ctx.advice), len(chip.lookup_manager.cells_to_lookup.get(ctx.tag(), []))
    # the integers the reference tracks beside the cells (for proper operands; the library's definition for every input)
    A = sum((a[i].value & mask) << (n * i) for i in range(k))
    B = sum((b[i].value & mask) << (n * i) for i in range(k))
    # mul_no_carry::crt (mul_no_carry.rs:24-32, :45)
    prods = [VR.GateChip.inner_product(ctx, a[:i + 1], list(reversed(b[:i + 1]))) for i in range(k)]
    native = VR.GateChip.mul(ctx, a[k], b[k])
    # carry_mod::crt
    quot, out = divmod(A * B, p)                                              # carry_mod.rs:68 div_mod_floor
    out_vec = [(out >> (n * i)) & mask for i in range(k)]                     # :74-75 decompose_bigint drops the limbs past k
    quot_vec = [(quot >> (n * i)) & mask for i in range(k)]
    u.A, u.B, u.quot, u.out = A, B, quot, out
    assert 1 not in sp.mod_vec, "inner_product_simple would write its Constant(1) form"
    quot_assigned, out_assigned, check_assigned, out_offsets, quot_offsets = [], [], [], [], []
    for i in range(k):                                                        # :100-134
        row_offset = len(ctx.advice)
        prod = VR.GateChip.inner_product(ctx, quot_assigned + [VR.Witness(quot_vec[i])], [VR.Constant(m) for m in reversed(sp.mod_vec[:i + 1])])
        new_quot = ctx.get(row_offset + 1 + 3 * i)
        temp1 = (prod.value - prods[i].value) % R
        ctx.assign_region([VR.Constant(R - 1), VR.Existing(prods[i]), VR.Witness(temp1), VR.Constant(1), VR.Witness(out_vec[i]),
                           VR.Witness((temp1 + out_vec[i]) % R)], [-1, 2])
        check_assigned.append(ctx.last())
        out_assigned.append(ctx.get(-2))
        quot_assigned.append(new_quot)
        out_offsets.append(len(ctx.advice) - 2 - u.start)
        quot_offsets.append(row_offset + 1 + 3 * i - u.start)
    u.gaps, u.results = [], [c.value for c in out_assigned] + [None] + [None] * (2 * k)

    def ranged(cell, bits, res):
        at = len(ctx.advice)
        chip.range_check(ctx, cell, bits)
        u.gaps.append((at - u.start, len(ctx.advice) - at, bits, res))
        u.results[res] = cell.value

    for i, cell in enumerate(out_assigned):                                   # :139-142
        ranged(cell, sp.out_last if i == k - 1 else n, i)
    for i, cell in enumerate(quot_assigned):                                  # :145-153
        bits = sp.quot_last if i == k - 1 else n
        ranged(VR.GateChip.add(ctx, cell, VR.Constant(pow(2, bits, R))), bits + 1, k + 1 + i)
    carries, previous = [], None                                              # check_carry_to_zero.rs:38-49
    for cell in check_assigned:
        carries.append(tdiv(signed(cell.value) + (carries[-1] if carries else 0), 1 << n))
    u.carries, u.checks = carries, [c.value for c in check_assigned]
    for i, (cell, carry) in enumerate(zip(check_assigned, carries)):          # :64-85
        ctx.assign_region([VR.Existing(cell), VR.Witness(-carry % R), VR.Constant(sp.limb_bases[1]),
                           VR.Existing(previous) if previous is not None else VR.Constant(0)], [0])
        neg_carry = ctx.get(-3)
        ranged(VR.GateChip.add(ctx, neg_carry, VR.Constant(pow(2, sp.rb, R))), sp.rb + 1, 2 * k + 1 + i)
        previous = neg_carry
    bases = [VR.Constant(c) for c in sp.limb_bases]
    quot_native = VR.RangeChip._inner_product_from_one(ctx, quot_assigned, bases)     # carry_mod.rs:171-176, bigint/mod.rs:66-74
    out_native = VR.RangeChip._inner_product_from_one(ctx, out_assigned, bases)
    ctx.assign_region([VR.Constant(sp.mod_native), VR.Existing(quot_native), VR.Existing(native)], [-1])   # :181-184
    u.results[k] = out_native.value
    u.end = len(ctx.advice)
    u.out_cells = out_assigned + [out_native]
    u.out_offsets = out_offsets + [u.end - 4 - u.start]
    u.quot_cell_offset = quot_offsets[1]
    u.lookups = len(chip.lookup_manager.cells_to_lookup.get(ctx.tag(), [])) - u.queue
    return u


def unit_def(sp, a_vals, b_vals):
    """one unit on a thread of its own -> (the Unit, its cells, the lookup values in queue order, the thread)"""
    ctx, chip, _ = thread(sp.lb)
    u = fp_mul(ctx, chip, sp, operand(a_vals, 0), operand(b_vals, 1))
    return u, list(ctx.advice), [c.value for c in chip.lookup_manager.cells_to_lookup.get(ctx.tag(), [])], ctx


def integer_pool(sp, seed):
    """0, 1, p - 1, p, p + 1, 2^(n k) - 1; uniform below p and below 2^(n k)"""
    g = np.random.default_rng([seed, sp.n, sp.k])
    top = 1 << (sp.n * sp.k)
    edge = [0, 1, sp.p - 1, sp.p, (sp.p + 1) % top, top - 1]
    rnd = [int.from_bytes(g.bytes(48), "little") for _ in range(4)]
    return edge, [rnd[0] % sp.p, rnd[1] % sp.p, rnd[2] % top, rnd[3] % top]


def operand_pairs(sp, seed):
    """every pair of the six edge integers, the uniform values against each other and against the edges, and the two improper units:
    a_1 = 2^n, and a_0 = r - 1 (they exercise the "mod 2^n" and the toward-zero definitions) -> [(a's k + 1 values, b's)]"""
    edge, rnd = integer_pool(sp, seed)
    ints = [(x, y) for x in edge for y in edge] + [(rnd[0], rnd[1]), (rnd[2], rnd[3]), (rnd[0], edge[5]), (rnd[3], rnd[1])]
    pairs = [(sp.crt(x), sp.crt(y)) for x, y in ints]
    a = sp.crt(rnd[0])
    a[1] = 1 << sp.n
    pairs.append((a, sp.crt(rnd[1])))
    a = sp.crt(rnd[1])
    a[0] = R - 1
    pairs.append((a, sp.crt(rnd[0])))
    return pairs


def check_definition():
    """the restatement itself: o recomposes to (A B) mod p computed independently; every flex gate of the thread holds; the cell counts match
    the formula; for the pools at (88, 3) the carry sums divide exactly and |c_i| < 2^90 (2^95 is allowed), also where Q is truncated"""
    for n, k, lb in PARAMS:
        for name, p in MODULI.items():
            sp = Spec(n, k, lb, p)
            assert all(-(-w // lb) * lb <= 253 for w in sp.widths), (n, k, lb, name)
            assert sp.quot_max_bits < n * k and 1 not in sp.mod_vec
            for a_vals, b_vals in operand_pairs(sp, 7):
                u, cells, lookups, ctx = unit_def(sp, a_vals, b_vals)
                proper = all(v < (1 << n) for v in a_vals[:k] + b_vals[:k])
                o = sum(cells[off] << (n * i) for i, off in enumerate(u.out_offsets[:k]))
                if proper:
                    A, B = (sum(v << (n * i) for i, v in enumerate(x[:k])) for x in (a_vals, b_vals))
                    assert o == (A % p) * (B % p) % p and o == u.out, (name, n)
                    assert cells[u.out_offsets[k]] == o % R
                # every gate holds for proper operands; where Q has more than k limbs (operands >= p) the native identity of S9, the gate on
                # out_native, cannot hold over the truncated quot_native; improper limbs break check_carry_to_zero's exact division
                truncated = u.quot >> (n * k) != 0
                for s in (i for i, q in enumerate(ctx.selector) if q and proper):
                    holds = (cells[s] + cells[s + 1] * cells[s + 2] - cells[s + 3]) % R == 0
                    assert holds != (truncated and s == u.out_offsets[k]), (name, n, k, lb, s)
                own = own_mask(u)
                assert int(own.sum()) == 3 * k * k + 29 * k + 3 and len(u.gaps) == 3 * k
                if (n, k) == (88, 3) and proper:
                    acc = 0
                    for chk, c in zip(u.checks, u.carries):
                        acc += signed(chk)
                        assert acc % (1 << n) == 0 and acc >> n == c and abs(c) < 1 << 90, (name, c.bit_length())
                        acc = c
    sp = Spec(88, 3, 18, SECP_P)
    u, cells, lookups, _ = unit_def(sp, sp.crt(5), sp.crt(7))
    assert sp.widths == [88, 80, 89, 85, 108] and (len(cells), len(lookups)) == (267, 54) and int(own_mask(u).sum()) == 117
    lay = PL.fp_mul_layout(sp.params())                 # the library computes the same widths and counts from the same formulas
    assert (lay.num_cells, lay.num_own_cells, lay.num_lookup_cells) == (267, 117, 54) and [r[2] for r in lay.ranges] == [88, 88, 80, 89, 89, 85, 108, 108, 108]


# ------------------------------------------------------------------------------------------------ A: the fill against its definition
def check_layout_and_seek():
    """fp_mul_layout equals the definition's counts, gaps and offsets for every parameter set and modulus; trace_seek equals assign_witnesses'
    placement for offsets before, on and after every break"""
    for n, k, lb in PARAMS:
        for p in MODULI.values():
            sp = Spec(n, k, lb, p)
            u, cells, lookups, _ = unit_def(sp, sp.crt(3), sp.crt(p - 2))
            lay = PL.fp_mul_layout(sp.params())
            assert (lay.num_cells, lay.num_own_cells, lay.num_lookup_cells) == (len(cells), int(own_mask(u).sum()), len(lookups)), (n, k, lb)
            assert lay.ranges == u.gaps and lay.out_cell_offsets == u.out_offsets, (n, k, lb, lay, u.gaps, u.out_offsets)
    bps = [40, 17, 23]
    cells_at, _ = place(1, 5, 90, bps, 4)              # a run from (column 1, row 5) of a four-column layout: bps[1], bps[2] lie ahead
    first = {}
    for i, c, r in cells_at:
        first.setdefault(i, (c, r))
    for off in (0, 11, 12, 13, 14, 35, 36, 37, 89):    # 12: on the first break (row 17), 13 behind it; 35: on the second (row 23 of column 2)
        assert PL.trace_seek(bps, 4, 1, 5, off) == first[off], (off, first[off])
    assert first[12] == (1, 17) and first[13] == (2, 1) and first[35] == (2, 23) and first[36] == (3, 1)
    assert PL.trace_seek(None, 4, 1, 5, 60) == (1, 65) and PL.trace_seek(bps, 4, 0, 41, 7) == (0, 48)   # no breaks; past the column's break
    for args in ((bps, 4, 4, 0, 0), (None, 1, 0, 0xFFFFFFFF, 1)):
        try:
            PL.trace_seek(*args)
        except H.H2HipError as e:
            assert e.code == ERR_INVALID
        else:
            raise AssertionError("trace_seek accepted %r" % (args,))


def check_seek_grid():
    """trace_seek equals the first position place() gives, exhaustively over a small grid: 1 to 3 columns of 6 usable rows, every break-point
    vector (none included), every start (column, row), every offset that still fits.  The walk is the one the kernels' seek and the range-check
    builders share.  The grid holds a run that starts on a break cell, breaks in consecutive columns with one cell between them (a break at
    row 1: the copy lies at row 0), a break on the run's last cell, and the last column, which never breaks."""
    rows, seen = 6, set()
    for ncols in (1, 2, 3):
        for bps in [None] + [list(b) for b in itertools.product(range(rows), repeat=ncols - 1)]:
            for col in range(ncols):
                for row in range(rows):
                    first, (c, r), prev_copied = {}, (col, row), False
                    for n in range(ncols * rows):            # grow the run cell by cell while it fits
                        cells_at, (c, r) = place(c, r, 1, bps, ncols)
                        if any(rr >= rows for _, _, rr in cells_at):
                            break
                        first[n] = cells_at[0][1:]
                        last_copied = len(cells_at) == 2
                        assert PL.trace_seek(bps, ncols, col, row, n) == first[n], (ncols, bps, col, row, n, first[n])
                        if bps is not None:
                            if n == 0 and last_copied:
                                seen.add("starts on a break cell")
                            if last_copied and prev_copied and first[n] == (c - 1, 1):
                                seen.add("one cell between two breaks")
                            if last_copied:
                                seen.add("break on the last cell")
                            if c == ncols - 1 and ncols > 1 and r > 1:
                                seen.add("in the last column")
                        prev_copied = last_copied
    assert seen == {"starts on a break cell", "one cell between two breaks", "break on the last cell", "in the last column"}, seen


def check_mul_fill(ctx, n, k, lb, modulus, count, nl=1, pairs=None, seed=0xF9):
    """the harness's check_fill over every operand pair: the bare call and fp_mul_fill_with_ranges over nl lookup columns"""
    sp = Spec(n, k, lb, MODULI[modulus])
    FH.check_fill(ctx, FpMul(sp), operand_pairs(sp, seed) if pairs is None else pairs, count, nl)


def check_chained(ctx, n, k, lb, modulus, count=5, seed=0xC4):
    """operands read from results_dev of a previous call, over sentinel-filled columns: the first call multiplies `count` pairs, the second
    call's units take their left operand from the first call's results (values_dev = the first call's results_dev: o_0 .. o_{k-1},
    out_native) and, since both operands of a unit index one buffer, their right operand from results of another unit of the first call.
    The second call's columns, lookup columns and results equal the definition's; the first call's results, written before, are unchanged;
    every other cell keeps its sentinel."""
    sp = Spec(n, k, lb, MODULI[modulus])
    nres = 3 * k + 1
    _, rnd = integer_pool(sp, seed)
    edge, _ = integer_pool(sp, seed)
    firsts = [(sp.crt(x), sp.crt(y)) for x, y in [(rnd[0], rnd[1]), (edge[2], edge[2]), (rnd[2], edge[3]), (edge[5], rnd[3]), (rnd[1], edge[4])][:count]]
    vals = [v for a, b in firsts for v in a + b]
    defs1 = [unit_def(sp, a, b) for a, b in firsts]
    ncells = len(defs1[0][1])
    units1 = [(0, 2 + j * (ncells + 1), 2 * (k + 1) * j, 2 * (k + 1) * j + k + 1) for j in range(count)]
    # the second call: unit j = (result j) x (result (j + 2) mod count) of the first
    ops2 = [(defs1[j][0].results[:k + 1], defs1[(j + 2) % count][0].results[:k + 1]) for j in range(count)]
    defs2 = [unit_def(sp, a, b) for a, b in ops2]
    units2 = [(1 + j % 2, 1 + (j // 2) * (ncells + 2), nres * j, nres * ((j + 2) % count)) for j in range(count)]
    slots2, slot = [], 3
    for u, _c, lookups, _t in defs2:
        slots2.append(slot)
        slot += len(lookups) + 1
    rows_n = max(2 + count * (ncells + 1), slot) + 9
    where = lookup_positions(slot, 1)
    sent = np.tile(SENTINEL, (rows_n, 1))
    d_cols = [ctx.to_device(sent) for _ in range(3)]
    d_lk = ctx.to_device(sent)
    d_vals = ctx.to_device(fr(vals))
    d_res1 = ctx.to_device(np.tile(SENTINEL, (count * nres + 2, 1)))
    d_res2 = ctx.to_device(np.tile(SENTINEL, (count * nres + 2, 1)))
    try:
        PL.fp_mul_fill(ctx, d_cols, rows_n - 2, None, sp.params(), d_vals, len(vals), d_res1, count * nres, units1)
        PL.fp_mul_fill_with_ranges(ctx, d_cols, rows_n - 2, None, [d_lk], sp.params(), d_res1, count * nres, d_res2, count * nres, units2, slots2)
        ctx.sync()
        want = [sent.copy() for _ in range(3)]
        want_lk, want_res = sent.copy(), [np.tile(SENTINEL, (count * nres + 2, 1)) for _ in range(2)]
        for j, ((col, row, _a, _b), (u, cells, _l, _t)) in enumerate(zip(units1, defs1)):
            own = own_mask(u)
            want[col][row:row + ncells][own] = fr(cells)[own]
            want_res[0][j * nres:(j + 1) * nres] = fr(u.results)
        for j, ((col, row, _a, _b), (u, cells, lookups, _t), s) in enumerate(zip(units2, defs2, slots2)):
            want[col][row:row + ncells] = fr(cells)
            want_res[1][j * nres:(j + 1) * nres] = fr(u.results)
            for i, v in enumerate(fr(lookups)):
                want_lk[where[s + i][1]] = v
        what = "chained calls, (n, k, lb) = (%d, %d, %d), %s" % (n, k, lb, modulus)
        compare(ctx, d_cols + [d_lk, d_res1, d_res2], want + [want_lk] + want_res, what)
    finally:
        for ptr in d_cols + [d_lk, d_vals, d_res1, d_res2]:
            ctx.free(ptr)


def check_results_null(ctx):
    """results_dev = NULL: the same own cells"""
    sp = Spec(88, 3, 8, SECP_P)
    FH.check_no_results(ctx, FpMul(sp), [(sp.crt(SECP_P - 3), sp.crt(12345))], 9, 1)


# ------------------------------------------------------------------------------------------------ B: column breaks
def _break_cells(sp):
    """the cell of a unit each case's break falls on, from the definition's own offsets"""
    u, cells, _, _ = unit_def(sp, sp.crt(3), sp.crt(5))
    k = sp.k
    first_gap = u.gaps[0][0]
    return {
        "s1_running_sum": 4 + 3,                      # S1_1: 0 a0 b1 [s_0] a1 b0 s_1
        "s3_prod": u.out_offsets[1] - 5,              # prod_1: the cell the six-cell region overlaps at offset -1
        "last_own_before_a_gap": first_gap - 1,       # check_{k-1}, the range check of o_0 right behind
        "last_cell_of_a_gap": u.gaps[k][0] - 4 - 1,   # the last cell of o_{k-1}'s range check (the range fill writes the copy)
        "out_native": u.out_offsets[k],               # overlapped by S9's gate
        "unit_last": len(cells) - 1,                  # the next unit right behind
    }


BREAK_CASES = ["s1_running_sum", "s3_prod", "last_own_before_a_gap", "last_cell_of_a_gap", "out_native", "unit_last"]


def check_mul_breaks(ctx, case, ncols):
    """the harness's check_breaks over (88, 3, 8) units in ncols columns of about 1,500 usable rows, through fp_mul_fill_with_ranges: the
    first break at row 1450, every later one 3 units further down the thread, each on the cell the case names"""
    sp = Spec(88, 3, 8, SECP_P)
    usable = 1500
    cell = _break_cells(sp)[case]
    ncells = PL.fp_mul_layout(sp.params(), ctx.lib).num_cells
    filler = 1450 - 2 * ncells - cell
    assert filler >= 5
    targets = [(2 + 3 * b, cell) for b in range(ncols - 1)]
    bps = FH.break_points(filler, ncells, targets)
    assert all(1200 < b < usable for b in bps), bps
    pairs = operand_pairs(sp, 0xB7)
    FH.check_breaks(ctx, FpMul(sp), [pairs[(5 * j) % len(pairs)] for j in range(targets[-1][0] + 2)], targets, filler, usable, ncols)


# ------------------------------------------------------------------------------------------------ C: the refusals
def check_rejections(ctx):
    """one case per refusal of include/h2hip.h's list: H2HIP_ERR_INVALID, the reason in h2hip_last_error, the sentinel everywhere (columns and
    results); then count == 0 and a good call from the same context"""
    sp = Spec(88, 3, 8, SECP_P)
    k, nres = sp.k, 10
    kind = FpMul(sp)
    lay = kind.layout(ctx.lib)
    ncells = lay.num_cells
    ops = [sp.crt(SECP_P - 5), sp.crt(77), sp.crt(SECP_N), sp.crt(1 << 200), sp.crt(3), sp.crt(9)]
    vals = [v for x in ops for v in x]
    assert len(vals) == 24
    with FH.RefusalBench(ctx, kind, vals, (0, 4), (8, 12), ncells, slots(3), 4 * nres) as b:
        usable, nv, fill, refused = b.usable, b.nv, b.fill, b.refused
        b.refuse_nulls()
        b.refuse_params(behind={"n k > 320": [("log2 k + 2 n > 252", "> 252", dict(n=126, k_=2, p=(1 << 252) - 1))]})
        b.refuse_placement()
        refused("an operand past values_len", "outside values_len", fill([b.ok, (1, 0, nv - k, 0)]))
        refused("the right operand past values_len", "outside values_len", fill([(1, 0, 0, (1 << 64) - 2)]))
        b.refuse_results_len()
        b.refuse_count()
        b.refuse_overlaps(lay.ranges[0][0])
        b.refuse_aliasing((5, 300))
        for what, prm in (("layout: flags", FH.par(flags=2)), ("layout: p", FH.par(p=0)), ("layout: lookup_bits", FH.par(lb=64))):
            FH.layout_refused(what, lambda: PL.fp_mul_layout(prm, ctx.lib))
        # count == 0 needs nothing
        ctx._chk(ctx.lib.h2hip_fp_mul_fill_dev(ctx.handle, None, 0, 0, None, None, None, 0, None, 0, None, 0))
        # the largest run that still fits (its last cell on row usable - 1), an operand that ends with values_len, a unit that ends on its
        # break point
        units = [(0, usable - ncells, nv - k - 1, 0), (1, 30, 8, 12)]
        bps = [usable - 1, 30 + ncells - 1]
        fill(units, bps=bps, rlen=2 * nres)()
        ctx.sync()
        want = [np.tile(SENTINEL, (b.n_rows, 1)) for _ in range(3)]
        want_res = np.tile(SENTINEL, (4 * nres, 1))
        for j, (col, row, a, b_) in enumerate(units):
            u, cells, _, _ = unit_def(sp, vals[a:a + k + 1], vals[b_:b_ + k + 1])
            own = own_mask(u)
            for i, c, r in place(col, row, ncells, bps, 3)[0]:
                if own[i]:
                    want[c][r] = fr([cells[i]])[0]
            want_res[j * nres:(j + 1) * nres] = fr(u.results)
        compare(ctx, b.d_cols + [b.d_res], want + [want_res], "after the refusals")


# ------------------------------------------------------------------------------------------------ D: the structs in every layer
def check_struct_layout():
    """h2hip_fp_params, h2hip_fp_mul and h2hip_fp_mul_range: the same fields in the header, the Rust sys crate and ctypes; 64, 24 and 16
    bytes; every function named in the C++ mirror and the safe Rust wrapper"""
    FH.check_names(structs=[("h2hip_fp_params", PL.FpParamsStruct, 64), ("h2hip_fp_mul", PL.FpMulStruct, 24), ("h2hip_fp_mul_range", PL.FpMulRangeStruct, 16)],
                   mirrored=("h2hip_fp_mul_fill_dev", "h2hip_fp_mul_layout", "h2hip_trace_seek"))


# ------------------------------------------------------------------------------------------------ E: inside a proof
PROOF_LB = 8


def _fp_program(builder, sp, xs, reps):
    """loads three field elements as CRT witnesses (k limbs, then the native residue), then per repetition multiplies the first two and the
    product by the third.  The first limb of the first operand is the instance.  -> [[(thread offset of the unit's first cell, queue position,
    the Unit)] of the first multiplications, the same of the second]"""
    ctx = builder.main()
    chip = VR.RangeChip(sp.lb, builder.lookup_manager)
    loaded = [[ctx.load_witness(v) for v in (sp.crt(x) if isinstance(x, int) else x)] for x in xs]   # (a list: the k + 1 values themselves)
    calls = [[], []]
    for _ in range(reps):
        u1 = fp_mul(ctx, chip, sp, loaded[0], loaded[1])
        calls[0].append((u1.start, u1.queue, u1))
        u2 = fp_mul(ctx, chip, sp, u1.out_cells, loaded[2])
        calls[1].append((u2.start, u2.queue, u2))
    builder.assigned_instances = [[loaded[0][0]]]
    return calls


def check_proof(ctx, kk, seed, nl=1, xs=None, truncated=False):
    """E: a BaseConfig circuit built through the Context mirror; keygen from the mirror's selectors and copies; the device advice starts with
    the loaded witnesses only; two fp_mul_fill_with_ranges calls (the second reads the first's results) write every other gate cell and the
    whole lookup columns.  The columns equal the Python-computed advice, the proof has the bytes of the proof from it, both verifiers accept
    it, check_witness finds nothing; with a q_1 cell changed after the fill it names that gate row.  truncated: the operands are 2^(n k) - 1
    (Q is truncated): the fill still equals the definition and check_witness names the gate on out_native; with xs = (2^(n k) - 1,
    3 2^254 + 12345, 2^(n k) - 1) also a range-check lookup (the comment below says why the all-ones operands alone do not reach one); with a list as xs[0]
    (an operand with an improper limb, whose carries do not divide exactly) only that the fill equals the definition and the check fails."""
    sp = Spec(88, 3, PROOF_LB, SECP_P)
    k, lb, nres = sp.k, sp.lb, 3 * sp.k + 1
    g = np.random.default_rng([seed, 0xE])
    top = (1 << (sp.n * k)) - 1
    xs = xs or ([top, top, top] if truncated else [int.from_bytes(g.bytes(40), "little") % SECP_P for _ in range(3)])
    lay = PL.fp_mul_layout(sp.params(), ctx.lib)
    n = 1 << kk
    reps = -(-13 * n // (10 * 2 * lay.num_cells))      # 1.3 columns of cells and more
    with FH.ProofBench(ctx, kk, nl, lb, seed, lambda builder: _fp_program(builder, sp, xs, reps), num_advice=2) as pb:
        calls, first = pb.calls, pb.first
        assert any(first[s][0] != first[s + lay.num_cells - 1][0] for call in calls for s, _q, _u in call), "no break falls inside a unit"
        # one device buffer: [gate columns][results of the first call][results of the second], so that a unit of the second call finds one
        # operand in the first call's results and the other among the loaded witnesses
        res_at = pb.buffers(2 * reps * nres, [range(3 * (k + 1))])
        res_at = [res_at, res_at + reps * nres]
        tables = [[first[s] + (0, k + 1) for s, _q, _u in calls[0]],
                  [first[s] + (res_at[0] + j * nres, 2 * (k + 1)) for j, (s, _q, _u) in enumerate(calls[1])]]
        for c in range(2):
            PL.fp_mul_fill_with_ranges(ctx, pb.d_cols, pb.sh.usable_rows, pb.bps, pb.d_lks, sp.params(), pb.d_gate, len(pb.host), pb.d_gate + 32 * res_at[c],
                                       reps * nres, tables[c], [q for _s, q, _u in calls[c]])
        ctx.sync()
        pb.check_columns()
        if truncated:
            # 2^(n k) - 1 squared: Q = 2^272 + 2^48 + ... has more than k limbs and its low k limbs are small, so every range check holds and
            # what fails is S9's native identity, the gate on out_native, over the truncated quot_native.  With 3 2^254 + 12345 as the second
            # operand Q is about 3/4 of 2^264 (past quot_max_bits, not truncated), q_2 + 2^84 does not fit 85 bits and the tail product of its range check is not in the table
            s, _q, u1 = calls[0][0]
            improper = not isinstance(xs[0], int)
            assert improper or (u1.quot.bit_length() > sp.quot_max_bits and (xs[1] != top or u1.quot >> (sp.n * k))), "Q is within its bound"
            total_f, fails = pb.check_witness(max_failures=4096)
            s9_fails = [f for f in fails if f.kind == "gate" and (f.column, f.row) == first[s + u1.out_offsets[k]]]
            assert total_f >= 1 and (improper or bool(s9_fails) == (xs[1] == top)), fails[:8]
            lk_rows = set(lookup_positions(sum(u.lookups for call in calls for _s, _q, u in call), nl))
            lookup_fails = [f for f in fails if f.kind == "lookup" and (f.column, f.row) in lk_rows]
            assert improper or bool(lookup_fails) == (xs[1] != top), fails[:8]
            return
        pb.check_proof()
        # ---- the q_1 cell of S3_1 (ip(q_0, q_1; m_1, m_0): 0 q_0 m_1 s_0 [q_1] m_0 prod_1) changed on the device: the gate on s_0, one row up
        s, u = next((s, u) for s, _q, u in calls[1]
                    if first[s + u.quot_cell_offset + 2] == (first[s + u.quot_cell_offset - 1][0], first[s + u.quot_cell_offset - 1][1] + 3))   # (no break cuts the gate)
        c0, r0 = first[s + u.quot_cell_offset - 1]
        total_f, fails = pb.changed(s + u.quot_cell_offset)
        assert total_f >= 1 and any(f.kind == "gate" and f.column == c0 and f.row == r0 for f in fails), fails
