"""Test-side checker of h2hip_plonk_check_witness's contract (include/h2hip.h): MockProver's verdict for the one gate form and the lookup forms
of BaseConfig, the dynamic lookup table and multi-phase BaseConfig, in plain Python integers.

Shapes: oracle.plonk.Shape (BaseConfig), tests.shape_oracle.Shape.dyn and Shape.phased.  All three carry `gates`
[(q_enable fixed column, advice column)], `perm_columns` [(kind, index)] and `usable_rows`; their lookups are (q, advice, table) triples
(BaseConfig) or (input expressions, table expressions) with every expression a product of (kind, index) factors.

The failures come out as (kind, column, row, peer_column, peer_row) tuples in canonical order, kind 1 = gate, 2 = lookup, 3 = copy, as the
library reports them."""
from oracle import bn254 as O
from oracle import plonk as P
from tests.util import R

GATE, LOOKUP, COPY = 1, 2, 3


def _ints(col):
    return O.limbs_to_ints(col, R)


def _lookup_exprs(sh, lookup):
    """(input expressions, table expressions) of one lookup, every expression a list of (kind, index) factors"""
    if len(lookup) == 3:   # BaseConfig: (q_lookup fixed column | None, advice column, table fixed column)
        q, a, t = lookup
        return [([("fixed", q)] if q is not None else []) + [("advice", a)]], [[("fixed", t)]]
    return lookup


def check(sh, fixed, advice, instances, copies):
    """-> (total, failures): fixed / advice as (n, 4) Montgomery arrays in the key's layout (advice: every phase), instances as lists of ints or
    (m, 4) arrays, copies as (((kind, column), row), ((kind, column), row)) pairs"""
    u = sh.usable_rows
    cols = {"fixed": [_ints(c) for c in fixed], "advice": [_ints(c) for c in advice], "instance": []}
    for inst in instances:
        vals = list(inst) if isinstance(inst, list) else _ints(inst)
        assert len(vals) <= u, "InstanceTooLarge"
        cols["instance"].append([v % R for v in vals] + [0] * (sh.n - len(vals)))
    out = []
    for q_col, a_col in sh.gates:
        q, a = cols["fixed"][q_col], cols["advice"][a_col]
        for r in range(u):
            if q[r] == 0:
                continue
            if r + 3 >= u or q[r] * (a[r] + a[r + 1] * a[r + 2] - a[r + 3]) % R:
                out.append((GATE, a_col, r, 0, 0))
    for li, lk in enumerate(sh.lookups):
        ins, tab = _lookup_exprs(sh, lk)

        def value(exprs, r):
            t = []
            for e in exprs:
                v = 1
                for kind, idx in e:
                    v = v * cols[kind][idx][r] % R
                t.append(v)
            return tuple(t)

        table = {value(tab, r) for r in range(u)}
        out += [(LOOKUP, li, r, 0, 0) for r in range(u) if value(ins, r) not in table]
    asm = P.PermutationAssembly(sh)
    for left, right in copies:
        asm.copy(left, right)
    for p, (kind, idx) in enumerate(sh.perm_columns):
        for r in range(u):
            pc, pr = asm.mapping[p][r]
            k2, i2 = sh.perm_columns[pc]
            if cols[kind][idx][r] != cols[k2][i2][pr]:
                out.append((COPY, p, r, pc, pr))
    return len(out), out
