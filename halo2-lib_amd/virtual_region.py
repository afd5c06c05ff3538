"""
Host-side mirror of halo2-base's virtual-region layout: how a `BaseCircuitBuilder`'s virtual `Context` cell streams become the physical
columns, selector rows and copy constraints that `keygen_*` / `create_proof` (plonk.py -> libh2hip) take.  This is the code behind
INTEGRATION.md's statement that circuits written against halo2-base lay out unchanged: the prover's input is exactly what the reference's
`synthesize` writes into its region.

Restated from (file:line in /root/reference/halo2-base/src):

  lib.rs:91-104, 225-262            ContextCell (ordered by (type_id, context_id, offset)), Context::assign_cell
  lib.rs:306-334, 430-452           Context::assign_region, load_witness / load_constant
  gates/flex_gate/threads/single_phase.rs:193-263   assign_with_constraints  (keygen: break points, selectors, the break cell's copy)
  gates/flex_gate/threads/single_phase.rs:273-312   assign_witnesses         (proving: the same layout from the recorded break points)
  virtual_region/lookups.rs:129-156 LookupAnyManager::assign_raw   (cells to look up: left to right, then top to bottom)
  virtual_region/copy_constraints.rs:120-173        CopyConstraintManager::assign_raw (constants sorted, then advice / constant equalities)
  gates/circuit/builder.rs:260-288, 291-309, 327-375  calculate_params, assign_instances, assign_lookups_in_phase
  gates/circuit/mod.rs:159-203      BaseCircuitBuilder::synthesize (order: gate threads, lookups, copy manager, instances)
  gates/range/mod.rs:154-170        load_lookup_table
  gates/range/mod.rs:476-635        RangeChip: limb_bases, _range_check, check_less_than (the definition of h2hip_range_fill_checks_dev's cells)
  gates/flex_gate/mod.rs:158-168, 246-277, 346-353, 1149-1190 (inner_product_simple)   the gate layouts used by the tests' tiny GateChip

First phase only (h2hip_base_circuit_params is single-phase: include/h2hip.h).  Values are canonical integers mod r here; `synthesize`
returns Montgomery-limb columns.  [UPSTREAM-RECALL]: `F: Ord` compares canonical representations numerically; `constrain_instance(cell, col, row)`
records the copy as (advice cell, instance cell).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

R_MOD = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
FIRST_PHASE_TYPE_ID = "halo2-base:SinglePhaseCoreManager:FirstPhase"     # single_phase.rs:114-121
EXTERNAL_CELL_TYPE_ID = "halo2-base:External Raw Halo2 Cell"              # copy_constraints.rs:19
ROTATIONS = 4                                                             # the vertical gate q * (a + b * c - d) spans four rows


@dataclass(frozen=True, order=True)
class ContextCell:
    type_id: str
    context_id: int
    offset: int


@dataclass
class AssignedValue:
    value: int
    cell: Optional[ContextCell] = None


# QuantumCell variants (lib.rs:43-89)
@dataclass
class Existing:
    cell: AssignedValue

    @property
    def value(self):
        return self.cell.value


@dataclass
class Witness:
    value: int


@dataclass
class Constant:
    value: int


RawCell = Tuple[Tuple[str, int], int]      # ((kind, column index), row) — the copy-constraint endpoints plonk.keygen takes


@dataclass
class CopyConstraintManager:
    advice_equalities: List[Tuple[ContextCell, ContextCell]] = field(default_factory=list)
    constant_equalities: List[Tuple[int, ContextCell]] = field(default_factory=list)
    assigned_advices: Dict[ContextCell, RawCell] = field(default_factory=dict)
    assigned_constants: Dict[int, RawCell] = field(default_factory=dict)


class Context:
    """lib.rs:157-262: one virtual column of advice cells with its selector bits"""

    def __init__(self, witness_gen_only: bool, type_id: str, context_id: int, copy_manager: CopyConstraintManager, phase: int = 0):
        self.witness_gen_only, self.type_id, self.context_id, self.copy_manager, self.phase = witness_gen_only, type_id, context_id, copy_manager, phase
        self.advice: List[int] = []
        self.selector: List[bool] = []
        self.zero_cell: Optional[AssignedValue] = None

    def tag(self):
        return (self.type_id, self.context_id)

    def _latest_cell(self) -> ContextCell:
        return ContextCell(self.type_id, self.context_id, len(self.advice) - 1)

    def assign_cell(self, inp):
        if isinstance(inp, AssignedValue):
            inp = Existing(inp)
        if isinstance(inp, Existing):
            self.advice.append(inp.cell.value % R_MOD)
            if not self.witness_gen_only:
                self.copy_manager.advice_equalities.append((self._latest_cell(), inp.cell.cell))
        elif isinstance(inp, Witness):
            self.advice.append(inp.value % R_MOD)
        elif isinstance(inp, Constant):
            self.advice.append(inp.value % R_MOD)
            if not self.witness_gen_only:
                self.copy_manager.constant_equalities.append((inp.value % R_MOD, self._latest_cell()))
        else:
            raise TypeError(inp)

    def last(self) -> AssignedValue:
        return AssignedValue(self.advice[-1], None if self.witness_gen_only else self._latest_cell())

    def get(self, offset: int) -> AssignedValue:
        if offset < 0:
            offset += len(self.advice)
        assert 0 <= offset < len(self.advice)
        return AssignedValue(self.advice[offset], None if self.witness_gen_only else ContextCell(self.type_id, self.context_id, offset))

    def constrain_equal(self, a: AssignedValue, b: AssignedValue):
        if not self.witness_gen_only:
            self.copy_manager.advice_equalities.append((a.cell, b.cell))

    def assign_region(self, inputs, gate_offsets=()):
        row_offset = len(self.advice)
        for inp in inputs:
            self.assign_cell(inp)
        if not self.witness_gen_only:
            self.selector.extend([False] * (len(self.advice) - len(self.selector)))
            for off in gate_offsets:
                idx = row_offset + off
                assert 0 <= idx < len(self.selector), "Invalid selector offset"
                self.selector[idx] = True

    def assign_region_last(self, inputs, gate_offsets=()) -> AssignedValue:
        self.assign_region(inputs, gate_offsets)
        return self.last()

    def load_witness(self, v: int) -> AssignedValue:
        self.assign_region([Witness(v)])
        return self.last()

    def load_constant(self, c: int) -> AssignedValue:
        self.assign_region([Constant(c)])
        return self.last()

    def load_zero(self) -> AssignedValue:
        if self.zero_cell is None:
            self.zero_cell = self.load_constant(0)
        return self.zero_cell


# ---------------------------------------------------------------------------------------------------------------- physical layout
class Region:
    """the physical columns a `synthesize` writes: advice values, enabled selector rows, copy constraints in call order"""

    def __init__(self, n: int, num_advice: int):
        self.n = n
        self.advice: List[Dict[int, int]] = [dict() for _ in range(num_advice)]
        self.selectors: Dict[str, Dict[int, set]] = {}
        self.fixed: Dict[int, Dict[int, int]] = {}
        self.copies: List[Tuple[RawCell, RawCell]] = []

    def assign_advice(self, column: int, row: int, value: int) -> RawCell:
        assert 0 <= row < self.n, "row outside the circuit"
        self.advice[column][row] = value % R_MOD
        return (("advice", column), row)

    def assign_fixed(self, column: int, row: int, value: int) -> RawCell:
        assert 0 <= row < self.n
        self.fixed.setdefault(column, {})[row] = value % R_MOD
        return (("fixed", column), row)

    def enable(self, kind: str, column: int, row: int):
        self.selectors.setdefault(kind, {}).setdefault(column, set()).add(row)

    def constrain_equal(self, a: RawCell, b: RawCell):
        self.copies.append((a, b))


def assign_with_constraints(threads: Sequence[Context], gate_columns: Sequence[int], region: Region, copy_manager: CopyConstraintManager,
                            max_rows: int, rotations: int = ROTATIONS) -> List[int]:
    """single_phase.rs:193-263.  Keygen-side layout: walks the threads' cells down gate column 0, 1, ...; a column is left at the first row
    where the next gate would not fit (or at max_rows - 1), the cell at the break is assigned AGAIN at row 0 of the next column and the two
    are constrained equal (two gates may overlap in it).  Returns the break points (the row offsets at which columns were left)."""
    break_points: List[int] = []
    gate_index, row_offset = 0, 0
    for ctx in threads:
        if not ctx.advice:
            continue
        if gate_index >= len(gate_columns):
            raise RuntimeError("NOT ENOUGH ADVICE COLUMNS. Perhaps blinding factors were not taken into account. The max non-poisoned rows is %d" % max_rows)
        assert len(ctx.selector) == len(ctx.advice)
        for i, (advice, q) in enumerate(zip(ctx.advice, ctx.selector)):
            cell = region.assign_advice(gate_columns[gate_index], row_offset, advice)
            key = ContextCell(ctx.type_id, ctx.context_id, i)
            old = copy_manager.assigned_advices.get(key)
            copy_manager.assigned_advices[key] = cell
            assert old is None or old == cell, "Trying to overwrite virtual cell with a different raw cell"
            if (q and row_offset + rotations > max_rows) or row_offset >= max_rows - 1:
                break_points.append(row_offset)
                row_offset = 0
                gate_index += 1
                if rotations > 1 and i + 2 >= rotations:
                    for delta in range(1, rotations - 1):
                        assert not ctx.selector[i - delta], "We do not support overlaps with delta = %d" % delta
                if gate_index >= len(gate_columns):
                    raise RuntimeError("NOT ENOUGH ADVICE COLUMNS. Perhaps blinding factors were not taken into account. The max non-poisoned rows is %d" % max_rows)
                ncell = region.assign_advice(gate_columns[gate_index], row_offset, advice)
                region.constrain_equal(ncell, cell)
            if q:
                region.enable("q_enable", gate_index, row_offset)
            row_offset += 1
    return break_points


def assign_witnesses(threads: Sequence[Context], gate_columns: Sequence[int], region: Region, break_points: Sequence[int]):
    """single_phase.rs:273-312.  Proving-side layout: no constraints, the columns are left exactly at the recorded break points."""
    if not gate_columns:
        assert sum(len(c.advice) for c in threads) == 0, "Trying to assign threads in a phase with no columns"
        return
    bps = iter(break_points)
    break_point = next(bps, None)
    gate_index, row_offset = 0, 0
    for ctx in threads:
        for advice in ctx.advice:
            region.assign_advice(gate_columns[gate_index], row_offset, advice)
            if break_point == row_offset:
                break_point = next(bps, None)
                row_offset = 0
                gate_index += 1
                region.assign_advice(gate_columns[gate_index], row_offset, advice)
            row_offset += 1


class LookupAnyManager:
    """virtual_region/lookups.rs (ADVICE_COLS = 1: the range lookup): cells queued per context tag, iterated in the BTreeMap's tag order"""

    def __init__(self, witness_gen_only: bool, copy_manager: CopyConstraintManager):
        self.witness_gen_only, self.copy_manager = witness_gen_only, copy_manager
        self.cells_to_lookup: Dict[Tuple[str, int], List[AssignedValue]] = {}

    def add_lookup(self, tag, cell: AssignedValue):
        self.cells_to_lookup.setdefault(tag, []).append(cell)

    def _flat(self):
        return [c for tag in sorted(self.cells_to_lookup) for c in self.cells_to_lookup[tag]]

    def total_rows(self) -> int:
        return len(self._flat())

    def assign_raw(self, lookup_columns: Sequence[int], region: Region):
        lookup_offset, lookup_col = 0, 0
        for advice in self._flat():
            if lookup_col >= len(lookup_columns):
                lookup_col = 0
                lookup_offset += 1
            bcell = region.assign_advice(lookup_columns[lookup_col], lookup_offset, advice.value)
            if not self.witness_gen_only:
                constrain_virtual_equals_external(region, advice, bcell, self.copy_manager)
            lookup_col += 1


def constrain_virtual_equals_external(region: Region, virtual_cell: AssignedValue, external_cell: RawCell, copy_manager: CopyConstraintManager):
    """utils/halo2.rs:56-75"""
    acell = copy_manager.assigned_advices.get(virtual_cell.cell)
    if acell is not None:
        region.constrain_equal(acell, external_cell)
    else:
        assert virtual_cell.cell.type_id == EXTERNAL_CELL_TYPE_ID
        copy_manager.assigned_advices[virtual_cell.cell] = external_cell


def copy_manager_assign_raw(copy_manager: CopyConstraintManager, constant_columns: Sequence[int], region: Region):
    """copy_constraints.rs:120-173: constants sorted by (value, cell) and assigned left to right, then top to bottom; advice equalities
    sorted; every equality imposed on the raw cells"""
    copy_manager.constant_equalities.sort(key=lambda t: (t[0], t[1]))
    fixed_col, fixed_offset = 0, 0
    for c, _ in copy_manager.constant_equalities:
        if c not in copy_manager.assigned_constants:
            assert constant_columns, "constants used but the circuit has no constants column"
            copy_manager.assigned_constants[c] = region.assign_fixed(constant_columns[fixed_col], fixed_offset, c)
            fixed_col += 1
            if fixed_col >= len(constant_columns):
                fixed_col = 0
                fixed_offset += 1
    copy_manager.advice_equalities.sort()
    for left, right in copy_manager.advice_equalities:
        region.constrain_equal(copy_manager.assigned_advices[left], copy_manager.assigned_advices[right])
    for c, right in copy_manager.constant_equalities:
        region.constrain_equal(copy_manager.assigned_constants[c], copy_manager.assigned_advices[right])
    copy_manager.assigned_constants.clear()   # keygen_vk and keygen_pk both call this


# ---------------------------------------------------------------------------------------------------------------- the builder
class BaseCircuitBuilder:
    """gates/circuit/builder.rs: first-phase threads + the range lookup manager + assigned instances, and `synthesize` (gates/circuit/mod.rs:159-203)
    over this repository's column numbering (a `shape`: the attributes halo2_lib_amd.testing.build_circuit reads — gate_advice, lookup_advice,
    table_col, constant_cols, q_lookup_col, q_enable_cols, num_fixed_total, num_instance, usable_rows, n, lookup_bits)."""

    def __init__(self, witness_gen_only: bool = False):
        self.witness_gen_only = witness_gen_only
        self.copy_manager = CopyConstraintManager()
        self.threads: List[Context] = []
        self.lookup_manager = LookupAnyManager(witness_gen_only, self.copy_manager)
        self.assigned_instances: List[List[AssignedValue]] = []
        self.break_points: Optional[List[int]] = None

    def new_thread(self) -> Context:
        ctx = Context(self.witness_gen_only, FIRST_PHASE_TYPE_ID, len(self.threads), self.copy_manager)
        self.threads.append(ctx)
        return ctx

    def main(self) -> Context:
        return self.threads[-1] if self.threads else self.new_thread()

    def statistics(self):
        """(total advice cells, distinct constants, cells to look up) — builder.rs:245-258"""
        return (sum(len(c.advice) for c in self.threads), len({c for c, _ in self.copy_manager.constant_equalities}), self.lookup_manager.total_rows())

    def calculate_params(self, k: int, minimum_rows: int, lookup_bits: Optional[int], num_instance_columns: int = 0):
        """builder.rs:260-288 / multi_phase.rs:131-153 -> (k, num_advice, num_lookup_advice, num_fixed, num_instance, lookup_bits)"""
        max_rows = (1 << k) - minimum_rows
        total_advice, total_fixed, total_lookup = self.statistics()
        num_advice = -(-total_advice // max_rows)
        num_fixed = (total_fixed + (1 << k) - 1) >> k
        num_lookup_advice = -(-total_lookup // max_rows)
        return (k, num_advice, num_lookup_advice, num_fixed, num_instance_columns, lookup_bits)

    def synthesize(self, shape):
        """-> (advice, fixed, copies, instances, break_points) with Montgomery-limb columns, as plonk.keygen / plonk.create_proof take them.
        Keygen stage (witness_gen_only False): assign_with_constraints, selectors, constants, copies.  Prover stage: assign_witnesses from
        `self.break_points`; fixed / copies come out empty (the proving key has them)."""
        # gate.max_rows = 2^k - meta.minimum_rows() (flex_gate/mod.rs:142, range/mod.rs:117): minimum_rows = blinding_factors + 3, i.e. two rows
        # fewer than the prover's own usable rows (n - blinding_factors - 1)
        n, max_rows = shape.n, shape.n - (shape.blinding_factors + 3)
        region = Region(n, len(shape.gate_advice) + len(shape.lookup_advice))
        gate_cols, lookup_cols = list(shape.gate_advice), list(shape.lookup_advice)
        if self.witness_gen_only:
            assert self.break_points is not None, "break points not set"
            assign_witnesses(self.threads, gate_cols, region, self.break_points)
        else:
            self.break_points = assign_with_constraints(self.threads, gate_cols, region, self.copy_manager, max_rows)
        # builder.rs:327-375
        if self.lookup_manager.total_rows():
            assert shape.table_col is not None, "range lookups were queued but the circuit was configured without a RangeConfig"
            if shape.q_lookup_col is not None:
                assert len(gate_cols) == 1
                if not self.witness_gen_only:
                    for advice in self.lookup_manager._flat():
                        (kind, col), row = self.copy_manager.assigned_advices[advice.cell]
                        assert row < max_rows, "range lookup assigned to an unusable row"
                        assert (kind, col) == ("advice", gate_cols[0]), "lookup column does not match"
                        region.enable("q_lookup", 0, row)
            else:
                assert lookup_cols, "range lookups require lookup advice columns"
                assert -(-self.lookup_manager.total_rows() // len(lookup_cols)) <= max_rows, "range lookups would be assigned to unusable rows"
                self.lookup_manager.assign_raw(lookup_cols, region)
        if not self.witness_gen_only:
            copy_manager_assign_raw(self.copy_manager, list(shape.constant_cols), region)
            # builder.rs:291-309
            assert len(self.assigned_instances) == shape.num_instance
            for col, instances in enumerate(self.assigned_instances):
                for i, inst in enumerate(instances):
                    region.constrain_equal(self.copy_manager.assigned_advices[inst.cell], (("instance", col), i))
        return self._export(shape, region)

    def _export(self, shape, region: Region):
        n = shape.n
        advice = [_column(n, col) for col in region.advice]
        fixed, copies = [], []
        if not self.witness_gen_only:
            fcols: List[Dict[int, int]] = [dict() for _ in range(shape.num_fixed_total)]
            if shape.table_col is not None:      # range/mod.rs:154-170
                for v in range(1 << shape.lookup_bits):
                    fcols[shape.table_col][v] = v
            for c, rows in region.fixed.items():
                fcols[c].update(rows)
            for gi, rows in region.selectors.get("q_enable", {}).items():
                for r in rows:
                    fcols[shape.q_enable_cols[gi]][r] = 1
            for rows in region.selectors.get("q_lookup", {}).values():
                for r in rows:
                    fcols[shape.q_lookup_col][r] = 1
            fixed = [_column(n, c) for c in fcols]
            copies = list(region.copies)
        instances = [_limbs([v.value for v in col]) for col in self.assigned_instances]
        return advice, fixed, copies, instances, list(self.break_points or [])


def _limbs(vals) -> np.ndarray:
    out = np.zeros((len(vals), 4), dtype=np.uint64)
    for i, v in enumerate(vals):
        m = (int(v) << 256) % R_MOD
        out[i] = [(m >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)]
    return out


def _column(n: int, cells: Dict[int, int]) -> np.ndarray:
    out = np.zeros((n, 4), dtype=np.uint64)
    if cells:
        rows = sorted(cells)
        out[rows] = _limbs([cells[r] for r in rows])
    return out


# ---------------------------------------------------------------------------------------------------------------- a tiny GateChip / RangeChip
class GateChip:
    """the few GateInstructions the layout tests need, with the reference's cell order (flex_gate/mod.rs:158-168, 246-277, 1149-1190)"""

    @staticmethod
    def add(ctx: Context, a, b) -> AssignedValue:
        a, b = _q(a), _q(b)
        return ctx.assign_region_last([a, b, Constant(1), Witness((a.value + b.value) % R_MOD)], [0])

    @staticmethod
    def sub(ctx: Context, a, b) -> AssignedValue:
        """| a - b | b | 1 | a | (flex_gate/mod.rs:184-196) -> the first cell"""
        a, b = _q(a), _q(b)
        ctx.assign_region([Witness((a.value - b.value) % R_MOD), b, Constant(1), a], [0])
        return ctx.get(-4)

    @staticmethod
    def mul(ctx: Context, a, b) -> AssignedValue:
        a, b = _q(a), _q(b)
        return ctx.assign_region_last([Constant(0), a, b, Witness(a.value * b.value % R_MOD)], [0])

    @staticmethod
    def mul_add(ctx: Context, a, b, c) -> AssignedValue:
        a, b, c = _q(a), _q(b), _q(c)
        return ctx.assign_region_last([c, a, b, Witness((a.value * b.value + c.value) % R_MOD)], [0])

    @staticmethod
    def and_(ctx: Context, a, b) -> AssignedValue:
        """gate.and = mul (flex_gate/mod.rs:555-562)"""
        return GateChip.mul(ctx, a, b)

    @staticmethod
    def is_zero(ctx: Context, a: AssignedValue) -> AssignedValue:
        """| out | a | inv | 1 | 0 | a | out | 0 | with gates on cells 0 and 4 and cell 0 constrained equal to cell 6 (flex_gate/mod.rs:789-809):
        out = [a == 0], inv = a^-1, 1 for a = 0 -> the second out cell"""
        x = a.value % R_MOD
        out, inv = (1, 1) if x == 0 else (0, pow(x, -1, R_MOD))
        row_offset = len(ctx.advice)
        ctx.assign_region([Witness(out), Existing(a), Witness(inv), Constant(1), Constant(0), Existing(a), Witness(out), Constant(0)], [0, 4])
        ctx.constrain_equal(ctx.get(row_offset), ctx.get(row_offset + 6))
        return ctx.get(-2)

    @staticmethod
    def is_equal(ctx: Context, a, b) -> AssignedValue:
        """is_zero(sub(a, b)) (flex_gate/mod.rs:815-823)"""
        return GateChip.is_zero(ctx, GateChip.sub(ctx, a, b))

    @staticmethod
    def inner_product(ctx: Context, a: Sequence, b: Sequence) -> AssignedValue:
        """inner_product_simple: | 0 | a0 | b0 | s1 | a1 | b1 | s2 | ... with a gate every three rows — consecutive gates OVERLAP in the
        running-sum cell, the case the break-point copy exists for"""
        a, b = [_q(v) for v in a], [_q(v) for v in b]
        assert len(a) == len(b) and a
        cells, s = [Constant(0)], 0
        for x, y in zip(a, b):
            s = (s + x.value * y.value) % R_MOD
            cells += [x, y, Witness(s)]
        ctx.assign_region(cells, [3 * i for i in range(len(a))])
        return ctx.last()

    @staticmethod
    def select(ctx: Context, a, b, sel) -> AssignedValue:
        """sel ? a : b as | a - b | 1 | b | a | b | sel | a - b | out | with gates on cells 0 and 4, cell 0 constrained equal to cell 6 and cell 2
        to cell 4 (flex_gate/mod.rs:1144-1170): out = (a - b) sel + b -> the last cell"""
        a, b, sel = _q(a), _q(b), _q(sel)
        diff = (a.value - b.value) % R_MOD
        row_offset = len(ctx.advice)
        ctx.assign_region([Witness(diff), Constant(1), b, a, b, sel, Witness(diff), Witness((diff * sel.value + b.value) % R_MOD)], [0, 4])
        ctx.constrain_equal(ctx.get(row_offset), ctx.get(row_offset + 6))
        ctx.constrain_equal(ctx.get(row_offset + 2), ctx.get(row_offset + 4))
        return ctx.last()

    @staticmethod
    def assert_bit(ctx: Context, x: AssignedValue):
        """| 0 | x | x | x | (flex_gate/mod.rs:303-305)"""
        ctx.assign_region([Constant(0), Existing(x), Existing(x), Existing(x)], [0])

    @staticmethod
    def bits_to_indicator(ctx: Context, bits: Sequence[AssignedValue]) -> List[AssignedValue]:
        """the indicator of the number the little-endian `bits` spell (flex_gate/mod.rs:609-656): | 1 - b | b | 1 | 1 | for the last bit, then
        bit by bit downwards, per entry ind of the level before, | (1 - bit) ind | ind | bit | ind | and mul(ind, bit) -> the 2^len(bits)
        entries of the last level.  The products are defined for bits that are none."""
        k = len(bits)
        assert k > 0, "bits_to_indicator: bits must be non-empty"
        ctx.assign_region([Witness((1 - bits[k - 1].value) % R_MOD), Existing(bits[k - 1]), Constant(1), Constant(1)], [0])
        indicator = [ctx.get(-4), ctx.get(-3)]
        offset = 0
        for idx in range(1, k):
            bit = bits[k - 1 - idx]
            for old_idx in range(1 << idx):
                ind = indicator[offset + old_idx]
                ctx.assign_region([Witness((1 - bit.value) * ind.value % R_MOD), Existing(ind), Existing(bit), Existing(ind)], [0])
                indicator.append(ctx.get(-4))
                indicator.append(GateChip.mul(ctx, Existing(ind), Existing(bit)))
            offset += 1 << idx
        return indicator[(1 << k) - 2:]

    @staticmethod
    def select_by_indicator(ctx: Context, a: Sequence, indicator: Sequence[AssignedValue]) -> AssignedValue:
        """| 0 | a_0 | ind_0 | s_0 | a_1 | ind_1 | s_1 | ... with a gate every three rows (flex_gate/mod.rs:709-730), the sums in the arithmetic
        form s_i = s_{i-1} + a_i ind_i: the reference's "a where ind != 0" for a one-hot indicator, and a satisfied gate for any other"""
        a = [_q(v) for v in a]
        assert len(a) == len(indicator) and a
        cells, s = [Constant(0)], 0
        for x, ind in zip(a, indicator):
            s = (s + x.value * ind.value) % R_MOD
            cells += [x, Existing(ind), Witness(s)]
        ctx.assign_region(cells, [3 * i for i in range(len(a))])
        return ctx.last()

    @staticmethod
    def num_to_bits(ctx: Context, a: AssignedValue, range_bits: int) -> List[AssignedValue]:
        """the little-endian bits of a (flex_gate/mod.rs:1215-1241): the inner product of the bits against the powers of two in the "b starts
        with Constant(1)" form, constrained equal to a, then assert_bit per bit.  to_u64_limbs truncates: a value that does not fit gets the
        bits of its low range_bits bits, and the copy constraint between a and the sum then fails."""
        assert range_bits > 0
        bits = [Witness((a.value >> i) & 1) for i in range(range_bits)]
        row_offset = len(ctx.advice)
        if range_bits == 1:
            ctx.assign_region(bits)
            acc = ctx.last()
        else:
            acc = RangeChip._inner_product_from_one(ctx, bits, [Constant(1 << i) for i in range(range_bits)])
        ctx.constrain_equal(a, acc)
        bit_cells = [ctx.get(row_offset)] + [ctx.get(row_offset + 1 + 3 * (i - 1)) for i in range(1, range_bits)]
        for cell in bit_cells:
            GateChip.assert_bit(ctx, cell)
        return bit_cells


FR_CAPACITY = 253                                                        # F::CAPACITY of bn256's Fr: 2^253 < r


class RangeChip:
    """RangeChip (range/mod.rs:476-687) with the reference's cell order and lookup queue order: add_cell_to_lookup for a cell that is already
    < 2^lookup_bits, range_check / _range_check (limb decomposition, the tail gate on the last limb) and check_less_than"""

    def __init__(self, lookup_bits: int, lookup_manager: LookupAnyManager):
        self.lookup_bits, self.lookup_manager = lookup_bits, lookup_manager
        # range/mod.rs:477-485: Constant(1), Constant(2^lb), Constant(2^(2 lb)), ...
        self.limb_bases = [Constant(pow(2, i * lookup_bits, R_MOD)) for i in range(max(FR_CAPACITY // lookup_bits, 1) + 1)]

    def add_cell_to_lookup(self, ctx: Context, a: AssignedValue):
        assert a.value < (1 << self.lookup_bits)
        self.lookup_manager.add_lookup(ctx.tag(), a)

    def _queue(self, ctx: Context, a: AssignedValue):
        """range/mod.rs:491-495: the reference queues whatever it is given (the lookup argument, not the chip, refuses a value outside the table)"""
        self.lookup_manager.add_lookup(ctx.tag(), a)

    @staticmethod
    def _inner_product_from_one(ctx: Context, a: Sequence, b: Sequence[Constant]) -> AssignedValue:
        """inner_product_simple when b starts with Constant(1) (flex_gate/mod.rs:953-962): | a0 | a1 | b1 | s1 | a2 | b2 | s2 | ..., a gate on a0
        and on every running sum but the last"""
        a = [_q(v) for v in a]
        assert len(a) == len(b) and len(a) >= 2 and b[0].value == 1
        s = a[0].value % R_MOD
        cells = [a[0]]
        for x, y in zip(a[1:], b[1:]):
            s = (s + x.value * y.value) % R_MOD
            cells += [x, y, Witness(s)]
        ctx.assign_region(cells, [3 * i for i in range(len(a) - 1)])
        return ctx.last()

    def _range_check(self, ctx: Context, a: AssignedValue, range_bits: int) -> AssignedValue:
        """range/mod.rs:512-564 -> the last (highest) limb.  decompose_fe_to_u64_limbs truncates: a value that does not fit gets the limbs of
        its low num_limbs * lookup_bits bits, and the copy constraint between a and the sum then fails."""
        assert range_bits > 0, "range_bits == 0 is assert_is_const, not a range check"
        lb = self.lookup_bits
        num_limbs, rem_bits = -(-range_bits // lb), range_bits % lb
        assert num_limbs * lb <= FR_CAPACITY and len(self.limb_bases) >= num_limbs
        if num_limbs == 1:
            self._queue(ctx, a)
            last_limb = a
        else:
            limbs = [Witness((a.value >> (i * lb)) & ((1 << lb) - 1)) for i in range(num_limbs)]
            row_offset = len(ctx.advice)
            acc = self._inner_product_from_one(ctx, limbs, self.limb_bases[:num_limbs])
            ctx.constrain_equal(a, acc)
            self._queue(ctx, ctx.get(row_offset))
            for i in range(num_limbs - 1):
                self._queue(ctx, ctx.get(row_offset + 1 + 3 * i))
            last_limb = ctx.get(row_offset + 1 + 3 * (num_limbs - 2))
        if rem_bits == 1:      # assert_bit: | 0 | x | x | x |
            ctx.assign_region([Constant(0), Existing(last_limb), Existing(last_limb), Existing(last_limb)], [0])
        elif rem_bits > 1:
            check = GateChip.mul(ctx, last_limb, Constant(1 << (lb - rem_bits)))
            self._queue(ctx, check)
        return last_limb

    def range_check(self, ctx: Context, a: AssignedValue, range_bits: int):
        self._range_check(ctx, a, range_bits)

    def _shifted_difference(self, ctx: Context, a, b, shift_bits: int) -> AssignedValue:
        """the seven cells in front of check_less_than's / is_less_than's range check (range/mod.rs:617-632, 662-680):
        | a + 2^shift - b | b | 1 | a + 2^shift | -2^shift | 1 | a | -> the first of them"""
        a, b = _q(a), _q(b)
        pow_of_two = 1 << shift_bits
        shift_a = (pow_of_two + a.value) % R_MOD
        ctx.assign_region([Witness((shift_a - b.value) % R_MOD), b, Constant(1), Witness(shift_a), Constant(-pow_of_two % R_MOD), Constant(1), a], [0, 3])
        return ctx.get(-7)

    def check_less_than(self, ctx: Context, a, b, num_bits: int):
        """range/mod.rs:604-635"""
        assert num_bits < FR_CAPACITY, "num_bits must leave one native-field bit of headroom for check_less_than"
        self.range_check(ctx, self._shifted_difference(ctx, a, b, num_bits), num_bits)

    def is_less_than(self, ctx: Context, a, b, num_bits: int) -> AssignedValue:
        """range/mod.rs:646-687: the seven cells over padded_bits = ceil(num_bits / lookup_bits) lookup_bits, the range check of the first of
        them at padded_bits + lookup_bits, is_zero of that check's last limb -> 1 when a < b, else 0"""
        padded_bits = -(-num_bits // self.lookup_bits) * self.lookup_bits
        assert padded_bits + self.lookup_bits <= FR_CAPACITY, "num_bits is too large for this is_less_than implementation"
        last_limb = self._range_check(ctx, self._shifted_difference(ctx, a, b, padded_bits), padded_bits + self.lookup_bits)
        return GateChip.is_zero(ctx, last_limb)


def _q(v):
    if isinstance(v, AssignedValue):
        return Existing(v)
    if isinstance(v, int):
        return Witness(v)
    return v


# ---------------------------------------------------------------------------------------------------------------- the dynamic lookup table
class BasicDynLookupConfig:
    """virtual_region/lookups/basic.rs:38-199 over this repository's column numbering (include/h2hip.h, h2hip_dyn_circuit_params): advice
    columns [table t_0..t_{m-1}] [set 0: k_0..k_{m-1}] ... then the gate columns; fixed columns [table_is_enabled] [key_is_enabled per set] ..."""

    def __init__(self, key_cols: int, lu_sets: int):
        self.key_cols, self.lu_sets = key_cols, lu_sets
        self.table = list(range(key_cols))
        self.table_is_enabled = 0
        self.to_lookup = [(list(range(key_cols * (1 + s), key_cols * (2 + s))), 1 + s) for s in range(lu_sets)]

    def assign_virtual_to_lookup_to_raw(self, region: Region, keys: Sequence[Sequence[AssignedValue]], copy_manager: Optional[CopyConstraintManager],
                                        offset: int = 0):
        """basic.rs:115-143: left to right over the sets, then top to bottom; key_is_enabled = 1 on every row used"""
        lookup_col = 0
        for key in keys:
            if lookup_col >= len(self.to_lookup):
                lookup_col = 0
                offset += 1
            key_cols, key_is_enabled = self.to_lookup[lookup_col]
            region.assign_fixed(key_is_enabled, offset, 1)
            for cell, column in zip(key, key_cols):
                bcell = region.assign_advice(column, offset, cell.value)
                if copy_manager is not None:
                    constrain_virtual_equals_external(region, cell, bcell, copy_manager)
            lookup_col += 1

    def assign_virtual_table_to_raw(self, region: Region, rows: Sequence[Sequence[AssignedValue]], copy_manager: Optional[CopyConstraintManager],
                                    offset: int = 0):
        """basic.rs:170-198: one enabled row per table row, then ONE disabled all-zero row (a disabled, all-zero key always finds a match)"""
        for row in rows:
            region.assign_fixed(self.table_is_enabled, offset, 1)
            for cell, column in zip(row, self.table):
                bcell = region.assign_advice(column, offset, cell.value)
                if copy_manager is not None:
                    constrain_virtual_equals_external(region, cell, bcell, copy_manager)
            offset += 1
        region.assign_fixed(self.table_is_enabled, offset, 0)
        for column in self.table:
            region.assign_advice(column, offset, 0)


class RAMCircuit:
    """The RAMCircuit of virtual_region/tests/lookups/memory.rs:30-158: a memory table of (index, value) rows, every access (ptr, memory[ptr])
    looked up in it, the values summed up on the flex gate.  key_cols = 2 as there; key_cols 1 looks up the index only, key_cols 3 adds
    (index + value) as a third key column.  `prank` appends memory.rs:174-181's false access (0, 0).

    The cells are laid out as one chain of overlapping gates, | s | v | 1 | s+v | p | 0 | s+v | ..., a gate every third cell, instead of
    memory.rs's load_witness + add: every gate column then starts with an enabled gate at row 0 (a column break always falls on a gate), so no
    two q_enable columns are disjoint — the backend keeps one fixed column per gate selector and refuses keys whose selectors halo2's
    compress_selectors would merge (h2hip_plonk_keygen, include/h2hip.h LIMITS (2))."""

    def __init__(self, memory: Sequence[int], ptrs: Sequence[int], key_cols: int = 2, prank: bool = False):
        self.memory, self.ptrs, self.key_cols = [m % R_MOD for m in memory], list(ptrs), key_cols
        self.copy_manager = CopyConstraintManager()
        self.ctx = Context(False, FIRST_PHASE_TYPE_ID, 0, self.copy_manager)
        self.mem_access: List[List[AssignedValue]] = []
        self.sum = self.ctx.load_constant(0)
        for ptr in self.ptrs:
            self._access(ptr, self.memory[ptr])
        if prank:
            self._access(0, 0)

    def _access(self, ptr: int, value: int):
        ctx = self.ctx
        ctx.assign_region([Witness(value), Constant(1), Witness((self.sum.value + value) % R_MOD)], [-1])   # s + v * 1 = s'
        v, self.sum = ctx.get(-3), ctx.last()
        extra = {}
        for name, e in (("p", ptr), ("pv", (ptr + value) % R_MOD))[: 1 if self.key_cols < 3 else 2]:
            ctx.assign_region([Witness(e), Constant(0), Existing(self.sum)], [-1])                       # s + e * 0 = s
            extra[name], self.sum = ctx.get(-3), ctx.last()
        self.mem_access.append([extra["p"], v, extra.get("pv")][: self.key_cols])

    def table_rows(self) -> List[List[AssignedValue]]:
        rows = []
        for i, m in enumerate(self.memory):
            cols = [i, m, (i + m) % R_MOD][: self.key_cols]
            rows.append([AssignedValue(c, ContextCell(EXTERNAL_CELL_TYPE_ID, j, i)) for j, c in enumerate(cols)])
        return rows

    def num_advice_needed(self, k: int, blinding_factors: int = 6) -> int:
        """gate columns the layout fills (a dry run of assign_with_constraints): an empty gate column would have a disjoint selector"""
        max_rows = (1 << k) - (blinding_factors + 3)
        cols = len(self.ctx.advice) // max(max_rows - ROTATIONS, 1) + 2
        return len(assign_with_constraints([self.ctx], list(range(cols)), Region(1 << k, cols), CopyConstraintManager(), max_rows)) + 1

    def synthesize(self, params):
        """-> (advice, fixed, copies) for plonk.keygen / plonk.create_proof with a DynLookupCircuitParams: memory.rs:115-157 (the gate thread,
        the table, the accesses, then the copy manager)"""
        n, m, L = 1 << params.k, params.key_cols, params.lu_sets
        assert m == self.key_cols
        ndyn = m * (1 + L)
        max_rows = n - (6 + 3)   # gate.max_rows = 2^k - minimum_rows, blinding factors 6
        region = Region(n, ndyn + params.num_advice)
        gate_cols = list(range(ndyn, ndyn + params.num_advice))
        self.copy_manager.assigned_advices.clear()
        self.copy_manager.assigned_constants.clear()
        assign_with_constraints([self.ctx], gate_cols, region, self.copy_manager, max_rows)
        cfg = BasicDynLookupConfig(m, L)
        assert len(self.memory) + 1 <= max_rows and -(-len(self.mem_access) // L) <= max_rows, "the table or the accesses do not fit the rows"
        cfg.assign_virtual_table_to_raw(region, self.table_rows(), self.copy_manager)
        cfg.assign_virtual_to_lookup_to_raw(region, self.mem_access, self.copy_manager)
        constant_cols = list(range(1 + L, 1 + L + params.num_fixed))
        copy_manager_assign_raw(self.copy_manager, constant_cols, region)
        fcols: List[Dict[int, int]] = [dict() for _ in range(1 + L + params.num_fixed + params.num_advice)]
        for c, rows in region.fixed.items():
            fcols[c].update(rows)
        for gi, rows in region.selectors.get("q_enable", {}).items():
            for r in rows:
                fcols[1 + L + params.num_fixed + gi][r] = 1
        advice = [_column(n, col) for col in region.advice]
        fixed = [_column(n, c) for c in fcols]
        return advice, fixed, list(region.copies)
