//! Safe layer: what the `halo2-axiom-hip` fork calls instead of its CPU kernels.
//! NOT COMPILED in this repository's environment (no Rust toolchain) — see ffi/rust/README.md.
use super::*;
use halo2curves::bn256::{Fr, G1Affine, G1};
use std::ffi::CStr;
use std::ptr;

#[derive(Debug)]
pub struct HipError {
    pub code: i32,
    pub message: String,
}
fn check(rc: c_int) -> Result<(), HipError> {
    if rc == H2HIP_OK {
        Ok(())
    } else {
        let message = unsafe { CStr::from_ptr(h2hip_last_error()) }.to_string_lossy().into_owned();
        Err(HipError { code: rc, message })
    }
}

/// One per GPU and process; work is serialised on its HIP stream (create_proof is driven from one thread,
/// reference halo2-base/src/utils/testing.rs:32-50).
pub struct Backend {
    ctx: *mut h2hip_ctx,
}
unsafe impl Send for Backend {}
impl Backend {
    pub fn new(device: i32) -> Result<Self, HipError> {
        let mut ctx = ptr::null_mut();
        check(unsafe { h2hip_init(device, ptr::null_mut(), &mut ctx) })?;
        Ok(Self { ctx })
    }
}
impl Drop for Backend {
    fn drop(&mut self) {
        unsafe { h2hip_destroy(self.ctx) }
    }
}

/// Resident SRS column (`ParamsKZG::g` or `::g_lagrange`), uploaded once with precomputed window tables.
pub struct ResidentBases<'b> {
    be: &'b Backend,
    h: *mut h2hip_bases,
}
impl<'b> ResidentBases<'b> {
    pub fn upload(be: &'b Backend, points: &[G1Affine]) -> Result<Self, HipError> {
        let mut h = ptr::null_mut();
        check(unsafe { h2hip_bases_upload(be.ctx, points.as_ptr().cast(), points.len(), H2HIP_BASES_PRECOMPUTE, &mut h) })?;
        Ok(Self { be, h })
    }
    pub fn len(&self) -> usize {
        unsafe { h2hip_bases_len(self.h) }
    }
    /// `best_multiexp(coeffs, &bases[..coeffs.len()])` — the body of `ParamsKZG::commit` / `commit_lagrange`
    /// (KZG ignores the blind).  Returns the projective point like upstream.
    pub fn multiexp(&self, coeffs: &[Fr]) -> Result<G1, HipError> {
        let mut out = G1::default();
        check(unsafe {
            h2hip_msm_g1(self.be.ctx, self.h, coeffs.as_ptr().cast(), coeffs.len(), H2HIP_POINT_JACOBIAN, (&mut out as *mut G1).cast())
        })?;
        Ok(out)
    }
}
impl Drop for ResidentBases<'_> {
    fn drop(&mut self) {
        unsafe { h2hip_bases_free(self.be.ctx, self.h) }
    }
}

/// Replacement body of `arithmetic::best_fft(a, omega, log_n)`.
pub fn best_fft(be: &Backend, a: &mut [Fr], omega: Fr, log_n: u32) -> Result<(), HipError> {
    assert_eq!(a.len(), 1 << log_n);
    check(unsafe { h2hip_best_fft(be.ctx, a.as_mut_ptr().cast(), (&omega as *const Fr).cast(), log_n) })
}
/// Replacement body of `EvaluationDomain::ifft` (omega_inv and the 2^-k divisor come from the domain).
pub fn ifft(be: &Backend, a: &mut [Fr], omega_inv: Fr, log_n: u32, divisor: Fr) -> Result<(), HipError> {
    assert_eq!(a.len(), 1 << log_n);
    check(unsafe { h2hip_ifft(be.ctx, a.as_mut_ptr().cast(), (&omega_inv as *const Fr).cast(), log_n, (&divisor as *const Fr).cast()) })
}
/// Replacement body of `EvaluationDomain::coeff_to_extended`.
pub fn coeff_to_extended(be: &Backend, coeffs: &[Fr], k: u32, extended_k: u32, extended_omega: Fr, zeta: Fr) -> Result<Vec<Fr>, HipError> {
    assert_eq!(coeffs.len(), 1 << k);
    let mut out = vec![Fr::zero(); 1 << extended_k];
    check(unsafe {
        h2hip_coeff_to_extended(be.ctx, coeffs.as_ptr().cast(), k, out.as_mut_ptr().cast(), extended_k,
                                (&extended_omega as *const Fr).cast(), (&zeta as *const Fr).cast())
    })?;
    Ok(out)
}
/// Replacement body of `EvaluationDomain::extended_to_coeff` (including upstream's final truncate).
pub fn extended_to_coeff(be: &Backend, mut a: Vec<Fr>, extended_k: u32, extended_omega_inv: Fr, extended_ifft_divisor: Fr, zeta_inv: Fr,
                         n: usize, quotient_poly_degree: usize) -> Result<Vec<Fr>, HipError> {
    assert_eq!(a.len(), 1 << extended_k);
    check(unsafe {
        h2hip_extended_to_coeff(be.ctx, a.as_mut_ptr().cast(), extended_k, (&extended_omega_inv as *const Fr).cast(),
                                (&extended_ifft_divisor as *const Fr).cast(), (&zeta_inv as *const Fr).cast())
    })?;
    a.truncate(n * quotient_poly_degree);
    Ok(a)
}

// ------------------------------------------------------------------------------------------------------------------
// The rest of INTEGRATION.md §2's call-site table.  Polynomials that stay on the device between calls are `DeviceVec`s.

/// A column / polynomial resident in HBM.
pub struct DeviceVec<'b> {
    be: &'b Backend,
    ptr: *mut c_void,
    len: usize,
}
impl<'b> DeviceVec<'b> {
    pub fn zeroed(be: &'b Backend, len: usize) -> Result<Self, HipError> {
        let mut ptr = ptr::null_mut();
        check(unsafe { h2hip_malloc(be.ctx, 32 * len.max(1), &mut ptr) })?;
        let v = Self { be, ptr, len };
        v.upload(&vec![Fr::zero(); len])?;
        Ok(v)
    }
    pub fn from_slice(be: &'b Backend, values: &[Fr]) -> Result<Self, HipError> {
        let mut ptr = ptr::null_mut();
        check(unsafe { h2hip_malloc(be.ctx, 32 * values.len().max(1), &mut ptr) })?;
        let v = Self { be, ptr, len: values.len() };
        v.upload(values)?;
        Ok(v)
    }
    pub fn upload(&self, values: &[Fr]) -> Result<(), HipError> {
        assert_eq!(values.len(), self.len);
        check(unsafe { h2hip_upload(self.be.ctx, self.ptr, values.as_ptr().cast(), 32 * self.len) })
    }
    pub fn to_vec(&self) -> Result<Vec<Fr>, HipError> {
        let mut out = vec![Fr::zero(); self.len];
        check(unsafe { h2hip_download(self.be.ctx, out.as_mut_ptr().cast(), self.ptr, 32 * self.len) })?;
        Ok(out)
    }
    pub fn len(&self) -> usize {
        self.len
    }
}
impl Drop for DeviceVec<'_> {
    fn drop(&mut self) {
        unsafe { h2hip_free(self.be.ctx, self.ptr) };
    }
}
fn fr_ptr(v: &Fr) -> *const c_void {
    (v as *const Fr).cast()
}

impl<'b> ResidentBases<'b> {
    /// all commitments of one prover round (`advice.iter().map(|p| params.commit_lagrange(p))` upstream) as ONE pipelined batch
    pub fn multiexp_many(&self, columns: &[&DeviceVec<'b>]) -> Result<Vec<G1>, HipError> {
        let n = columns.first().map_or(0, |c| c.len);
        assert!(columns.iter().all(|c| c.len == n));
        let ptrs: Vec<*const c_void> = columns.iter().map(|c| c.ptr as *const c_void).collect();
        let mut out = vec![G1::default(); columns.len()];
        check(unsafe { h2hip_msm_g1_batch_dev(self.be.ctx, self.h, ptrs.as_ptr(), n, columns.len(), H2HIP_POINT_JACOBIAN, out.as_mut_ptr().cast()) })?;
        Ok(out)
    }
}

/// `batch_invert_assigned`: Assigned::Rational(num, den) columns -> values, 0^-1 := 0 (halo2-base/src/gates/flex_gate/mod.rs:677-681)
pub fn assigned_resolve<'b>(be: &'b Backend, num: &DeviceVec<'b>, den: &DeviceVec<'b>) -> Result<DeviceVec<'b>, HipError> {
    assert_eq!(num.len, den.len);
    let out = DeviceVec::zeroed(be, num.len)?;
    check(unsafe { h2hip_assigned_resolve_dev(be.ctx, out.ptr, num.ptr, den.ptr, num.len) })?;
    Ok(out)
}
/// `GateChip::inner_product*` / `sum` / `select_by_indicator` / `select_from_idx` as cells (halo2-base/src/gates/flex_gate/mod.rs:412, 709-753,
/// 940-1110): s_0, a_1, b_1, s_1, ... with s_i = s_{i-1} + a_i * b_i for every piece of `chains`, written into `columns` from the operands
/// `a` and `b`, which may be other columns of the proof (include/h2hip.h states the piece forms and the refusals).
/// Safety: every pointer of `columns` is a device column of at least `usable_rows` elements on `be`'s device (the phase-witness callback's).
pub unsafe fn gate_fill_chains(be: &Backend, columns: &[*mut c_void], usable_rows: usize, a: &DeviceVec, b: &DeviceVec, chains: &[h2hip_gate_chain])
                               -> Result<(), HipError> {
    check(h2hip_gate_fill_chains_dev(be.ctx, columns.as_ptr(), columns.len(), usable_rows, a.ptr, a.len, b.ptr, b.len, chains.as_ptr(), chains.len()))
}
/// `RangeChip::_range_check` as cells (halo2-base/src/gates/range/mod.rs:512-564; behind check_less_than's / is_less_than's seven cells with
/// `H2HIP_RANGE_LESS_THAN`): the limb decomposition and the tail gate of every unit of `checks` at one width, written down `columns` across
/// `break_points`, and the limbs' copies into `lookup_columns` at each unit's queue position; the checked values are elements of `values`,
/// which may be a column of the proof (include/h2hip.h states the cell form and the refusals).
/// Safety: every pointer of `columns` and `lookup_columns` is a device column of at least `usable_rows` elements on `be`'s device.
pub unsafe fn range_fill_checks(be: &Backend, columns: &[*mut c_void], usable_rows: usize, break_points: Option<&[u32]>,
                                lookup_columns: &[*mut c_void], values: &DeviceVec, range_bits: u32, lookup_bits: u32, shift_bits: u32, flags: u32,
                                checks: &[h2hip_range_check]) -> Result<(), HipError> {
    assert!(break_points.map_or(true, |b| b.len() + 1 == columns.len()));
    check(h2hip_range_fill_checks_dev(be.ctx, columns.as_ptr(), columns.len(), usable_rows, break_points.map_or(ptr::null(), |b| b.as_ptr()),
                                      lookup_columns.as_ptr(), lookup_columns.len(), values.ptr, values.len, range_bits, lookup_bits, shift_bits, flags,
                                      checks.as_ptr(), checks.len()))
}
/// (gate cells of one unit, its lookup cells, the offset of the last-limb cell among the gate cells or None when the unit has none of its own)
pub fn range_check_layout(range_bits: u32, lookup_bits: u32, flags: u32) -> Result<(usize, usize, Option<u32>), HipError> {
    let (mut cells, mut lookups, mut last) = (0usize, 0usize, 0u32);
    check(unsafe { h2hip_range_check_layout(range_bits, lookup_bits, flags, &mut cells, &mut lookups, &mut last) })?;
    Ok((cells, lookups, if last == u32::MAX { None } else { Some(last) }))
}
/// `FpChip::mul` as cells (halo2-ecc/src/fields/mod.rs:188-196: mul_no_carry::crt, then carry_mod::crt) for every unit of `units`: the own cells
/// written down `columns` across `break_points`, the cells of the nine range checks left as gaps for `range_fill_checks` over `results`
/// (3 k + 1 elements per unit: o_i, out_native, q_i + B, -c_i + 2^rb); operands are k + 1 consecutive elements of `values` (include/h2hip.h
/// states the cell form and the refusals).
/// Safety: every pointer of `columns` is a device column of at least `usable_rows` elements on `be`'s device.
pub unsafe fn fp_mul_fill(be: &Backend, columns: &[*mut c_void], usable_rows: usize, break_points: Option<&[u32]>, params: &h2hip_fp_params,
                          values: &DeviceVec, results: Option<&mut DeviceVec>, units: &[h2hip_fp_mul]) -> Result<(), HipError> {
    assert!(break_points.map_or(true, |b| b.len() + 1 == columns.len()));
    let (rptr, rlen) = results.map_or((ptr::null_mut(), 0), |r| (r.ptr, r.len));
    check(h2hip_fp_mul_fill_dev(be.ctx, columns.as_ptr(), columns.len(), usable_rows, break_points.map_or(ptr::null(), |b| b.as_ptr()), params,
                                values.ptr, values.len, rptr, rlen, units.as_ptr(), units.len()))
}
/// (cells of one unit, its own cells, the lookup cells of its range checks, the 3 k gaps in context order, the offsets of o_i and out_native)
pub fn fp_mul_layout(params: &h2hip_fp_params) -> Result<(usize, usize, usize, Vec<h2hip_fp_mul_range>, Vec<u32>), HipError> {
    let (mut cells, mut own, mut lookups) = (0usize, 0usize, 0usize);
    let (mut ranges, mut outs) = ([h2hip_fp_mul_range::default(); 12], [0u32; 5]);
    check(unsafe { h2hip_fp_mul_layout(params, &mut cells, &mut own, &mut lookups, ranges.as_mut_ptr(), outs.as_mut_ptr()) })?;
    let k = params.num_limbs as usize;
    Ok((cells, own, lookups, ranges[..3 * k].to_vec(), outs[..k + 1].to_vec()))
}
/// the 3 k range units of every unit of `units`, gap-major (`[j * units.len() + u]`): what `range_fill_checks` takes, five calls over the results
pub fn fp_mul_range_checks(break_points: Option<&[u32]>, num_columns: usize, params: &h2hip_fp_params, units: &[h2hip_fp_mul], lookup_slots: &[u64])
                           -> Result<Vec<h2hip_range_check>, HipError> {
    assert!(break_points.map_or(true, |b| b.len() + 1 == num_columns) && lookup_slots.len() == units.len());
    let mut out = vec![h2hip_range_check::default(); 3 * params.num_limbs as usize * units.len()];
    check(unsafe { h2hip_fp_mul_range_checks(break_points.map_or(ptr::null(), |b| b.as_ptr()), num_columns, params, units.as_ptr(), lookup_slots.as_ptr(),
                                             units.len(), out.as_mut_ptr()) })?;
    Ok(out)
}
/// `ec_add_unequal` (non-strict, op = H2HIP_EC_ADD_UNEQUAL) or `ec_double` (H2HIP_EC_DOUBLE) of halo2-ecc as cells for every unit of `units`:
/// the own cells written down `columns` across `break_points`, the cells of the 9 k range checks left as gaps for `range_fill_checks` over
/// `results` (9 k + 3 elements per unit: x3, y3, lambda, then per reduction q_i + B and -c_i + 2^rb); a point is 2 (k + 1) consecutive
/// elements of `values` (include/h2hip.h states the cell form and the refusals).
/// Safety: every pointer of `columns` is a device column of at least `usable_rows` elements on `be`'s device.
pub unsafe fn ec_fill(be: &Backend, columns: &[*mut c_void], usable_rows: usize, break_points: Option<&[u32]>, params: &h2hip_fp_params, op: u32,
                      values: &DeviceVec, results: Option<&mut DeviceVec>, units: &[h2hip_ec_op]) -> Result<(), HipError> {
    assert!(break_points.map_or(true, |b| b.len() + 1 == columns.len()));
    let (rptr, rlen) = results.map_or((ptr::null_mut(), 0), |r| (r.ptr, r.len));
    check(h2hip_ec_fill_dev(be.ctx, columns.as_ptr(), columns.len(), usable_rows, break_points.map_or(ptr::null(), |b| b.as_ptr()), params, op,
                            values.ptr, values.len, rptr, rlen, units.as_ptr(), units.len()))
}
/// (cells of one unit, its own cells, the lookup cells of its range checks, the 9 k gaps in context order, the offsets of the cells of x3, y3, lambda)
pub fn ec_layout(params: &h2hip_fp_params, op: u32) -> Result<(usize, usize, usize, Vec<h2hip_fp_mul_range>, Vec<u32>), HipError> {
    let (mut cells, mut own, mut lookups) = (0usize, 0usize, 0usize);
    let (mut ranges, mut outs) = ([h2hip_fp_mul_range::default(); 36], [0u32; 15]);
    check(unsafe { h2hip_ec_layout(params, op, &mut cells, &mut own, &mut lookups, ranges.as_mut_ptr(), outs.as_mut_ptr()) })?;
    let k = params.num_limbs as usize;
    Ok((cells, own, lookups, ranges[..9 * k].to_vec(), outs[..3 * (k + 1)].to_vec()))
}
/// the 9 k range units of every unit of `units`, grouped by width (the distinct widths of `ec_layout`'s gaps in the order of first appearance),
/// unit by unit inside a width: what `range_fill_checks` takes, one call per width over the results
pub fn ec_range_checks(break_points: Option<&[u32]>, num_columns: usize, params: &h2hip_fp_params, op: u32, units: &[h2hip_ec_op], lookup_slots: &[u64])
                       -> Result<Vec<h2hip_range_check>, HipError> {
    assert!(break_points.map_or(true, |b| b.len() + 1 == num_columns) && lookup_slots.len() == units.len());
    let mut out = vec![h2hip_range_check::default(); 9 * params.num_limbs as usize * units.len()];
    check(unsafe { h2hip_ec_range_checks(break_points.map_or(ptr::null(), |b| b.as_ptr()), num_columns, params, op, units.as_ptr(), lookup_slots.as_ptr(),
                                         units.len(), out.as_mut_ptr()) })?;
    Ok(out)
}
/// where cell `offset` of a run laid down from (column, row) lies under assign_witnesses' break rule
pub fn trace_seek(break_points: Option<&[u32]>, num_columns: usize, column: u32, row: u32, offset: u64) -> Result<(u32, u32), HipError> {
    assert!(break_points.map_or(true, |b| b.len() + 1 == num_columns));
    let (mut c, mut r) = (0u32, 0u32);
    check(unsafe { h2hip_trace_seek(break_points.map_or(ptr::null(), |b| b.as_ptr()), num_columns, column, row, offset, &mut c, &mut r) })?;
    Ok((c, r))
}
/// `ff::BatchInvert` on a resident column, in place
pub fn batch_invert(be: &Backend, a: &mut DeviceVec) -> Result<(), HipError> {
    check(unsafe { h2hip_fr_batch_invert_dev(be.ctx, a.ptr, a.len) })
}
/// permutation argument: z over the usable rows of one column set, starting at `first` (the previous set's last value)
pub fn permutation_product<'b>(be: &'b Backend, columns: &[&DeviceVec<'b>], sigmas: &[&DeviceVec<'b>], first_col_index: u32, usable_rows: usize,
                               beta: Fr, gamma: Fr, delta: Fr, omega: Fr, first: Fr) -> Result<DeviceVec<'b>, HipError> {
    assert_eq!(columns.len(), sigmas.len());
    let (num, den) = (DeviceVec::zeroed(be, usable_rows)?, DeviceVec::zeroed(be, usable_rows)?);
    let c: Vec<*const c_void> = columns.iter().map(|v| v.ptr as *const c_void).collect();
    let s: Vec<*const c_void> = sigmas.iter().map(|v| v.ptr as *const c_void).collect();
    check(unsafe {
        h2hip_permutation_product_terms_dev(be.ctx, num.ptr, den.ptr, c.as_ptr(), s.as_ptr(), c.len() as u32, first_col_index, usable_rows,
                                            fr_ptr(&beta), fr_ptr(&gamma), fr_ptr(&delta), fr_ptr(&omega))
    })?;
    let z = DeviceVec::zeroed(be, usable_rows + 1)?;
    check(unsafe { h2hip_fr_grand_product_dev(be.ctx, z.ptr, num.ptr, den.ptr, usable_rows) })?;
    check(unsafe { h2hip_fr_scale_dev(be.ctx, z.ptr, fr_ptr(&first), usable_rows + 1) })?;
    Ok(z)
}
/// lookup argument: `permute_expression_pair` over the usable rows (Err = upstream's ConstraintSystemFailure)
pub fn permute_expression_pair<'b>(be: &'b Backend, input: &DeviceVec<'b>, table: &DeviceVec<'b>, usable_rows: usize)
                                   -> Result<(DeviceVec<'b>, DeviceVec<'b>), HipError> {
    let (a, s) = (DeviceVec::zeroed(be, input.len)?, DeviceVec::zeroed(be, input.len)?);
    check(unsafe { h2hip_lookup_permute_dev(be.ctx, input.ptr, table.ptr, usable_rows, a.ptr, s.ptr) })?;
    Ok((a, s))
}
/// lookup argument: the grand product z over the usable rows
pub fn lookup_product<'b>(be: &'b Backend, input: &DeviceVec<'b>, table: &DeviceVec<'b>, permuted_input: &DeviceVec<'b>,
                          permuted_table: &DeviceVec<'b>, usable_rows: usize, beta: Fr, gamma: Fr) -> Result<DeviceVec<'b>, HipError> {
    let (num, den) = (DeviceVec::zeroed(be, usable_rows)?, DeviceVec::zeroed(be, usable_rows)?);
    check(unsafe {
        h2hip_lookup_product_terms_dev(be.ctx, num.ptr, den.ptr, input.ptr, table.ptr, permuted_input.ptr, permuted_table.ptr, usable_rows,
                                       fr_ptr(&beta), fr_ptr(&gamma))
    })?;
    let z = DeviceVec::zeroed(be, usable_rows + 1)?;
    check(unsafe { h2hip_fr_grand_product_dev(be.ctx, z.ptr, num.ptr, den.ptr, usable_rows) })?;
    Ok(z)
}
/// evaluate_h, gate term: acc = acc*y + q*(a + a(wX)*a(w^2 X) - a(w^3 X)) on the extended domain
pub fn quotient_flex_gate(be: &Backend, acc: &mut DeviceVec, q: &DeviceVec, a: &DeviceVec, extended_k: u32, k: u32, y: Fr) -> Result<(), HipError> {
    check(unsafe { h2hip_quotient_flex_gate_dev(be.ctx, acc.ptr, q.ptr, a.ptr, extended_k, k, fr_ptr(&y)) })
}
/// evaluate_h, the lookup argument's five identities
#[allow(clippy::too_many_arguments)]
pub fn quotient_lookup(be: &Backend, acc: &mut DeviceVec, z: &DeviceVec, input: &DeviceVec, table: &DeviceVec, permuted_input: &DeviceVec,
                       permuted_table: &DeviceVec, l0: &DeviceVec, l_last: &DeviceVec, l_blind: &DeviceVec, extended_k: u32, k: u32, beta: Fr,
                       gamma: Fr, y: Fr) -> Result<(), HipError> {
    check(unsafe {
        h2hip_quotient_lookup_dev(be.ctx, acc.ptr, z.ptr, input.ptr, table.ptr, permuted_input.ptr, permuted_table.ptr, l0.ptr, l_last.ptr,
                                  l_blind.ptr, extended_k, k, fr_ptr(&beta), fr_ptr(&gamma), fr_ptr(&y))
    })
}
/// evaluate_h, one permutation set's terms (`terms`: mask of H2HIP_PERM_*)
#[allow(clippy::too_many_arguments)]
pub fn quotient_permutation_set(be: &Backend, acc: &mut DeviceVec, z: &DeviceVec, z_prev: Option<&DeviceVec>, columns: &[&DeviceVec],
                                sigmas: &[&DeviceVec], first_col_index: u32, l0: &DeviceVec, l_last: &DeviceVec, l_blind: &DeviceVec,
                                extended_k: u32, k: u32, terms: u32, last_rotation: i32, beta: Fr, gamma: Fr, delta: Fr, zeta: Fr,
                                extended_omega: Fr, y: Fr) -> Result<(), HipError> {
    let c: Vec<*const c_void> = columns.iter().map(|v| v.ptr as *const c_void).collect();
    let s: Vec<*const c_void> = sigmas.iter().map(|v| v.ptr as *const c_void).collect();
    check(unsafe {
        h2hip_quotient_permutation_set_dev(be.ctx, acc.ptr, z.ptr, z_prev.map_or(ptr::null(), |v| v.ptr as *const c_void), c.as_ptr(), s.as_ptr(),
                                           c.len() as u32, first_col_index, l0.ptr, l_last.ptr, l_blind.ptr, extended_k, k, terms, last_rotation,
                                           fr_ptr(&beta), fr_ptr(&gamma), fr_ptr(&delta), fr_ptr(&zeta), fr_ptr(&extended_omega), fr_ptr(&y))
    })
}
/// `EvaluationDomain::divide_by_vanishing_poly`
pub fn divide_by_vanishing_poly(be: &Backend, a: &mut DeviceVec, extended_k: u32, k: u32, extended_omega: Fr, zeta: Fr) -> Result<(), HipError> {
    check(unsafe { h2hip_divide_by_vanishing_poly_dev(be.ctx, a.ptr, extended_k, k, fr_ptr(&extended_omega), fr_ptr(&zeta)) })
}
/// `arithmetic::eval_polynomial` for a whole evaluation round: out[j] = polys[j](points[j])
pub fn eval_polynomials(be: &Backend, polys: &[&DeviceVec], points: &[Fr]) -> Result<Vec<Fr>, HipError> {
    assert_eq!(polys.len(), points.len());
    let p: Vec<*const c_void> = polys.iter().map(|v| v.ptr as *const c_void).collect();
    let l: Vec<usize> = polys.iter().map(|v| v.len).collect();
    let mut out = vec![Fr::zero(); polys.len()];
    check(unsafe { h2hip_fr_eval_polynomial_batch_dev(be.ctx, p.as_ptr(), l.as_ptr(), points.as_ptr().cast(), polys.len(), out.as_mut_ptr().cast()) })?;
    Ok(out)
}
/// `arithmetic::kate_division`: (f(X) - f(b)) / (X - b)
pub fn kate_division<'b>(be: &'b Backend, f: &DeviceVec<'b>, b: Fr) -> Result<DeviceVec<'b>, HipError> {
    let q = DeviceVec::zeroed(be, f.len.saturating_sub(1))?;
    check(unsafe { h2hip_fr_kate_division_dev(be.ctx, q.ptr, f.ptr, f.len, fr_ptr(&b)) })?;
    Ok(q)
}
/// halo2-base's `PoseidonHasher`, batched over messages; the constants come from the library (`h2hip_poseidon_spec_generate`)
pub struct PoseidonHasher<'b> {
    be: &'b Backend,
    t: u32,
    r_f: u32,
    r_p: u32,
    round_constants: Vec<Fr>,
    mds: Vec<Fr>,
}
impl<'b> PoseidonHasher<'b> {
    pub fn new(be: &'b Backend, t: u32, r_f: u32, r_p: u32) -> Result<Self, HipError> {
        let mut round_constants = vec![Fr::zero(); ((r_f + r_p) * t) as usize];
        let mut mds = vec![Fr::zero(); (t * t) as usize];
        check(unsafe { h2hip_poseidon_spec_generate(t, r_f, r_p, round_constants.as_mut_ptr().cast(), mds.as_mut_ptr().cast()) })?;
        Ok(Self { be, t, r_f, r_p, round_constants, mds })
    }
    fn select(&self) -> Result<(), HipError> {
        check(unsafe { h2hip_poseidon_set_spec(self.be.ctx, self.t, self.r_f, self.r_p, self.round_constants.as_ptr().cast(), self.mds.as_ptr().cast()) })
    }
    /// `hash_fix_len_array` of `inputs.len() / len` messages of `len` elements each (row-major)
    pub fn hash_fix_len_array(&self, inputs: &DeviceVec<'b>, len: usize) -> Result<DeviceVec<'b>, HipError> {
        let n = if len == 0 { inputs.len } else { inputs.len / len };
        assert!(len == 0 || inputs.len % len == 0);
        self.select()?;
        let out = DeviceVec::zeroed(self.be, n)?;
        check(unsafe { h2hip_poseidon_hash_batch_dev(self.be.ctx, out.ptr, inputs.ptr, len, ptr::null(), n) })?;
        Ok(out)
    }
    /// `hash_var_len_array`: message i = the first `lens_dev[i]` elements of row i of `inputs` (`n` rows of `max_len`); `lens_dev`: n u32 on the device
    pub fn hash_var_len_array(&self, inputs: &DeviceVec<'b>, max_len: usize, lens_dev: *const u32, n: usize) -> Result<DeviceVec<'b>, HipError> {
        assert!(inputs.len >= max_len * n);
        self.select()?;
        let out = DeviceVec::zeroed(self.be, n)?;
        check(unsafe { h2hip_poseidon_hash_batch_dev(self.be.ctx, out.ptr, inputs.ptr, max_len, lens_dev, n) })?;
        Ok(out)
    }
    /// the heap-layout Merkle tree over 2^log_leaves leaves: node j = H([node 2j, node 2j+1]), node 1 the root
    pub fn merkle_tree(&self, leaves: &DeviceVec<'b>, log_leaves: u32) -> Result<DeviceVec<'b>, HipError> {
        assert_eq!(leaves.len, 1usize << log_leaves);
        self.select()?;
        let nodes = DeviceVec::zeroed(self.be, 2usize << log_leaves)?;
        check(unsafe { h2hip_poseidon_merkle_tree_dev(self.be.ctx, nodes.ptr, leaves.ptr, log_leaves) })?;
        Ok(nodes)
    }
    /// makes this hasher's `OptimizedPoseidonSpec` (derived by `h2hip_poseidon_spec_optimize`) the context's, for `fill_hashes`; a caller
    /// that holds a spec object of its own passes that object's arrays to `h2hip_poseidon_set_optimized_spec` instead
    pub fn select_optimized(&self) -> Result<(), HipError> {
        let (t, half, r_p) = (self.t as usize, (self.r_f / 2) as usize, self.r_p as usize);
        let mut start = vec![Fr::zero(); (half + 1) * t];
        let mut partial = vec![Fr::zero(); r_p + 1];
        let mut end = vec![Fr::zero(); half * t];
        let mut pre = vec![Fr::zero(); t * t];
        let mut sparse = vec![Fr::zero(); r_p * (2 * t - 1) + 1];
        check(unsafe {
            h2hip_poseidon_spec_optimize(self.t, self.r_f, self.r_p, self.round_constants.as_ptr().cast(), self.mds.as_ptr().cast(),
                                         start.as_mut_ptr().cast(), partial.as_mut_ptr().cast(), end.as_mut_ptr().cast(), pre.as_mut_ptr().cast(),
                                         sparse.as_mut_ptr().cast())
        })?;
        check(unsafe {
            h2hip_poseidon_set_optimized_spec(self.be.ctx, self.t, self.r_f, self.r_p, start.as_ptr().cast(), partial.as_ptr().cast(), end.as_ptr().cast(),
                                              self.mds.as_ptr().cast(), pre.as_ptr().cast(), sparse.as_ptr().cast())
        })
    }
    /// (the cells one unit of `len` inputs writes, the offsets of its t final-state cells; [1] is the digest)
    pub fn trace_layout(&self, len: u32, flags: u32) -> Result<(usize, Vec<u32>), HipError> {
        let mut cells = 0usize;
        let mut offsets = vec![0u32; self.t as usize];
        check(unsafe { h2hip_poseidon_trace_layout(self.t, self.r_f, self.r_p, len, flags, &mut cells, offsets.as_mut_ptr()) })?;
        Ok((cells, offsets))
    }
    /// every gate cell of `hash_fix_len_array` over `len` inputs for each unit of `hashes`, written into `columns` across `break_points`
    /// (`columns.len() - 1` entries, or None); inputs and states may lie inside the columns (include/h2hip.h states the cells and the refusals).
    /// Safety: every pointer of `columns` is a device column of at least `usable_rows` elements on the backend's device; `states_in` /
    /// `states_out` are null or point to `hashes.len() * t` elements there.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn fill_hashes(&self, columns: &[*mut c_void], usable_rows: usize, break_points: Option<&[u32]>, inputs: *const c_void, inputs_len: usize,
                              len: u32, hashes: &[h2hip_poseidon_hash], states_in: *const c_void, states_out: *mut c_void) -> Result<(), HipError> {
        assert!(break_points.map_or(true, |b| b.len() + 1 == columns.len()));
        check(h2hip_poseidon_fill_hashes_dev(self.be.ctx, columns.as_ptr(), columns.len(), usable_rows, break_points.map_or(ptr::null(), |b| b.as_ptr()),
                                             inputs, inputs_len, len, states_in, states_out, hashes.as_ptr(), hashes.len()))
    }
}
/// `poly * scalar` / `poly += other * scalar` of the multiopen argument
pub fn axpy(be: &Backend, y: &mut DeviceVec, a: Fr, x: &DeviceVec) -> Result<(), HipError> {
    check(unsafe { h2hip_fr_axpy_dev(be.ctx, y.ptr, fr_ptr(&a), x.ptr, x.len.min(y.len)) })
}
/// `EvaluationDomain::lagrange_to_coeff` over many columns at once (32 per kernel launch)
pub fn lagrange_to_coeff_many(be: &Backend, columns: &mut [&mut DeviceVec], omega_inv: Fr, k: u32, ifft_divisor: Fr) -> Result<(), HipError> {
    let p: Vec<*mut c_void> = columns.iter().map(|v| v.ptr).collect();
    check(unsafe { h2hip_ifft_batch_dev(be.ctx, p.as_ptr(), p.len(), fr_ptr(&omega_inv), k, fr_ptr(&ifft_divisor)) })
}
/// `EvaluationDomain::coeff_to_extended` over many columns at once
pub fn coeff_to_extended_many<'b>(be: &'b Backend, coeffs: &[&DeviceVec<'b>], k: u32, extended_k: u32, extended_omega: Fr, zeta: Fr)
                                  -> Result<Vec<DeviceVec<'b>>, HipError> {
    let outs = coeffs.iter().map(|_| DeviceVec::zeroed(be, 1usize << extended_k)).collect::<Result<Vec<_>, _>>()?;
    let pi: Vec<*const c_void> = coeffs.iter().map(|v| v.ptr as *const c_void).collect();
    let po: Vec<*mut c_void> = outs.iter().map(|v| v.ptr).collect();
    check(unsafe { h2hip_coeff_to_extended_batch_dev(be.ctx, pi.as_ptr(), k, po.as_ptr(), extended_k, pi.len(), fr_ptr(&extended_omega), fr_ptr(&zeta)) })?;
    Ok(outs)
}
/// all grand products of one argument: `num` / `den` hold the factors of `segments` products back to back; chained = the permutation
/// argument's sets (z_i(0) = z_{i-1}(last usable row)), unchained = the lookup arguments
pub fn grand_products<'b>(be: &'b Backend, num: &DeviceVec<'b>, den: &DeviceVec<'b>, segments: usize, chained: bool) -> Result<Vec<DeviceVec<'b>>, HipError> {
    assert!(segments > 0 && num.len == den.len && num.len % segments == 0);
    let seg = num.len / segments;
    let zs = (0..segments).map(|_| DeviceVec::zeroed(be, seg + 1)).collect::<Result<Vec<_>, _>>()?;
    let pz: Vec<*mut c_void> = zs.iter().map(|v| v.ptr).collect();
    check(unsafe { h2hip_fr_grand_products_dev(be.ctx, pz.as_ptr(), num.ptr, den.ptr, segments, seg, chained as c_int) })?;
    Ok(zs)
}
/// sum_j coeffs[j] * polys[j]: a rotation set's sum_j y^j P_j(X) of the multiopen argument in one pass
pub fn linear_combination<'b>(be: &'b Backend, polys: &[&DeviceVec<'b>], coeffs: &[Fr]) -> Result<DeviceVec<'b>, HipError> {
    assert_eq!(polys.len(), coeffs.len());
    let n = polys.iter().map(|v| v.len).min().unwrap_or(0);
    let p: Vec<*const c_void> = polys.iter().map(|v| v.ptr as *const c_void).collect();
    let out = DeviceVec::zeroed(be, n)?;
    check(unsafe { h2hip_fr_linear_combination_dev(be.ctx, out.ptr, p.as_ptr(), coeffs.as_ptr().cast(), polys.len(), n) })?;
    Ok(out)
}

// ------------------------------------------------------------------------------------------------------------------
// plonk::{keygen_pk, create_proof}: the whole prover on the device.  This is what `halo2_proofs::plonk::create_proof` becomes in the fork
// for `ConcreteCircuit = BaseCircuitBuilder<Fr>` (the reference's only circuit type, halo2-base/src/utils/testing.rs:32-50): synthesis, the
// RNG and the transcript's verifying-key hash stay in Rust, everything else is one FFI call.

/// The C key stores the raw `h2hip_bases*` of `g` and `g_lagrange` and reads them on every commitment (include/h2hip.h: "the bases must
/// outlive the key"): the key therefore BORROWS both base sets for its whole life (`'g`), so that safe code cannot drop a `ResidentBases`
/// (whose `Drop` frees the tables) while a key that points into it is alive.
pub struct ProvingKeyHip<'b, 'g> {
    be: &'b Backend,
    pk: *mut h2hip_plonk_pk,
    pub params: h2hip_base_circuit_params,
    /// Some for a circuit with more than one phase or with challenges (h2hip_plonk_keygen_phased)
    pub phased: Option<h2hip_phased_circuit_params>,
    /// Some for a circuit with RLC columns (h2hip_plonk_keygen_rlc); `phased` is then its base
    pub rlc: Option<h2hip_rlc_circuit_params>,
    pub shape: h2hip_plonk_shape,
    _g: &'g ResidentBases<'b>,
    _g_lagrange: &'g ResidentBases<'b>,
}
fn invalid(message: String) -> HipError {
    HipError { code: H2HIP_ERR_INVALID, message }
}
/// `BaseCircuitParams::num_advice_per_phase` / `num_lookup_advice_per_phase` and the number of `challenge_usable_after(phase)` challenges of
/// each phase (halo2-base/src/gates/circuit/mod.rs:25-45; MAX_PHASE = 3)
#[derive(Clone, Debug, Default)]
pub struct PhaseCounts {
    pub num_advice_per_phase: Vec<u32>,
    pub num_lookup_advice_per_phase: Vec<u32>,
    pub num_challenges_per_phase: Vec<u32>,
    /// RLC columns configured next to BaseConfig (downstream's RlcConfig): non-zero routes to the h2hip_*_rlc entries
    pub num_rlc_advice: u32,
}
impl PhaseCounts {
    fn is_first_phase_only(&self) -> bool {
        self.num_rlc_advice == 0 && self.num_advice_per_phase.len() <= 1 && self.num_lookup_advice_per_phase.len() <= 1
            && self.num_challenges_per_phase.iter().all(|&c| c == 0)
    }
    fn to_c_rlc(&self, params: &h2hip_base_circuit_params) -> Result<Option<h2hip_rlc_circuit_params>, HipError> {
        if self.num_rlc_advice == 0 {
            return Ok(None);
        }
        Ok(Some(h2hip_rlc_circuit_params::new(&self.to_c(params)?, self.num_rlc_advice)))
    }
    fn to_c(&self, params: &h2hip_base_circuit_params) -> Result<h2hip_phased_circuit_params, HipError> {
        let arr = |v: &[u32], what: &str| -> Result<[u32; 3], HipError> {
            if v.len() > 3 {
                return Err(invalid(format!("{what}: {} phases, MAX_PHASE is 3", v.len())));
            }
            let mut a = [0u32; 3];
            a[..v.len()].copy_from_slice(v);
            Ok(a)
        };
        Ok(h2hip_phased_circuit_params {
            k: params.k,
            num_advice_per_phase: arr(&self.num_advice_per_phase, "num_advice_per_phase")?,
            num_lookup_advice_per_phase: arr(&self.num_lookup_advice_per_phase, "num_lookup_advice_per_phase")?,
            num_fixed: params.num_fixed,
            num_instance: params.num_instance,
            lookup_bits: params.lookup_bits,
            num_challenges_per_phase: arr(&self.num_challenges_per_phase, "num_challenges_per_phase")?,
        })
    }
}
/// the advice columns of each phase of a multi-phase layout, in index order (include/h2hip.h states the layout)
fn phase_columns(p: &h2hip_phased_circuit_params) -> Vec<usize> {
    let (g, la) = (p.num_advice_per_phase, p.num_lookup_advice_per_phase);
    let range = p.lookup_bits >= 0 && la.iter().sum::<u32>() != 0;
    let q_lookup = range && g[0] == 1 && la[0] != 0;
    (0..3).map(|ph| (g[ph] + if !range || (ph == 0 && q_lookup) { 0 } else { la[ph] }) as usize).collect()
}
impl<'b, 'g> ProvingKeyHip<'b, 'g> {
    /// `keygen_vk` + `keygen_pk`: `fixed` = the fixed columns after synthesis (table, constants, selector columns), `copies` = the copy
    /// constraints as (permutation column, row, permutation column, row) in emission order.
    /// `params` carries phase 0's counts; `phases` all of them: a circuit with more than one phase or with challenges goes through
    /// `h2hip_plonk_keygen_phased`, one with RLC columns (`phases.num_rlc_advice != 0`) through `h2hip_plonk_keygen_rlc` (include/h2hip.h states
    /// the layouts and the limits).
    pub fn keygen(be: &'b Backend, params: h2hip_base_circuit_params, phases: &PhaseCounts, g: &'g ResidentBases<'b>, g_lagrange: &'g ResidentBases<'b>,
                  fixed: &[Vec<Fr>], copies: &[[u32; 4]], transcript_repr: impl FnOnce(&[G1Affine], &[G1Affine]) -> Fr) -> Result<Self, HipError> {
        let phased = if phases.is_first_phase_only() { None } else { Some(phases.to_c(&params)?) };
        let rlc = phases.to_c_rlc(&params)?;
        let mut shape = h2hip_plonk_shape::default();
        match (&rlc, &phased) {
            (Some(rp), _) => check(unsafe { h2hip_plonk_shape_of_rlc(rp, &mut shape) })?,
            (None, Some(pp)) => check(unsafe { h2hip_plonk_shape_of_phased(pp, &mut shape) })?,
            (None, None) => check(unsafe { h2hip_plonk_shape_of(&params, &mut shape) })?,
        }
        // the C side reads num_fixed_total pointers and 2^k elements behind each: check the shapes here, in safe code
        let n = 1usize << params.k;
        if fixed.len() != shape.num_fixed_total as usize {
            return Err(invalid(format!("keygen: {} fixed columns, the shape has {}", fixed.len(), shape.num_fixed_total)));
        }
        if let Some(c) = fixed.iter().position(|c| c.len() != n) {
            return Err(invalid(format!("keygen: fixed column {c} has {} rows, expected 2^k = {n}", fixed[c].len())));
        }
        if g.len() < n || g_lagrange.len() < n {
            return Err(invalid(format!("keygen: the SRS holds fewer than 2^k = {n} bases")));
        }
        let cols: Vec<*const c_void> = fixed.iter().map(|c| c.as_ptr().cast()).collect();
        let mut pk = ptr::null_mut();
        check(unsafe {
            match (&rlc, &phased) {
                (Some(rp), _) => h2hip_plonk_keygen_rlc(be.ctx, rp, g.h, g_lagrange.h, cols.as_ptr(), copies.as_ptr().cast(), copies.len(), &mut pk),
                (None, Some(pp)) => h2hip_plonk_keygen_phased(be.ctx, pp, g.h, g_lagrange.h, cols.as_ptr(), copies.as_ptr().cast(), copies.len(), &mut pk),
                (None, None) => h2hip_plonk_keygen(be.ctx, &params, g.h, g_lagrange.h, cols.as_ptr(), copies.as_ptr().cast(), copies.len(), &mut pk),
            }
        })?;
        // from here on `key`'s Drop frees the handle on every early return and on a panic inside the caller's `transcript_repr`
        let key = Self { be, pk, params, phased, rlc, shape, _g: g, _g_lagrange: g_lagrange };
        let mut fc = vec![G1Affine::default(); shape.num_fixed_total as usize];
        let mut pc = vec![G1Affine::default(); (shape.num_perm_columns as usize).max(1)];
        check(unsafe { h2hip_plonk_pk_commitments(key.pk, fc.as_mut_ptr().cast(), pc.as_mut_ptr().cast()) })?;
        pc.truncate(shape.num_perm_columns as usize);
        let repr = transcript_repr(&fc, &pc);   // VerifyingKey::transcript_repr, computed by the Rust side from the pinned key
        check(unsafe { h2hip_plonk_pk_set_transcript_repr(key.pk, fr_ptr(&repr)) })?;
        Ok(key)
    }
    /// `MockProver::run(k, &circuit, instances).verify()` on the GPU with this key (h2hip_plonk_check_witness): `advice` holds EVERY advice
    /// column of the key's layout (all phases, index order), at least usable_rows rows each.  Returns the exact number of failures and the
    /// first `max_failures` of them in canonical order (gate, lookup, copy; by column, then row).
    pub fn check_witness(&self, advice: &[Vec<Fr>], instances: &[&[Fr]], max_failures: usize)
                         -> Result<(usize, Vec<h2hip_witness_failure>), HipError> {
        self.check_witness_challenges(advice, instances, &[], max_failures)
    }
    /// the same with the phases' challenges (squeeze order): a key with RLC columns needs challenge 0, with which its RLC gates are checked
    /// (h2hip_plonk_check_witness_challenges); without challenges this is h2hip_plonk_check_witness.
    pub fn check_witness_challenges(&self, advice: &[Vec<Fr>], instances: &[&[Fr]], challenges: &[Fr], max_failures: usize)
                                    -> Result<(usize, Vec<h2hip_witness_failure>), HipError> {
        if advice.len() != self.shape.num_advice_total as usize {
            return Err(invalid(format!("check_witness: {} advice columns, the key has {}", advice.len(), self.shape.num_advice_total)));
        }
        if let Some(c) = advice.iter().position(|c| c.len() < self.shape.usable_rows as usize) {
            return Err(invalid(format!("check_witness: advice column {c} has fewer than the {} usable rows", self.shape.usable_rows)));
        }
        if instances.len() != self.params.num_instance as usize {
            return Err(invalid(format!("check_witness: {} instance columns, the circuit has {}", instances.len(), self.params.num_instance)));
        }
        let adv: Vec<*const c_void> = advice.iter().map(|c| c.as_ptr().cast()).collect();
        let ins: Vec<*const c_void> = instances.iter().map(|c| c.as_ptr().cast()).collect();
        let lens: Vec<usize> = instances.iter().map(|c| c.len()).collect();
        let mut out = vec![h2hip_witness_failure::default(); max_failures];
        let mut total = 0usize;
        let out_ptr = if max_failures == 0 { ptr::null_mut() } else { out.as_mut_ptr() };
        check(unsafe {
            if challenges.is_empty() {
                h2hip_plonk_check_witness(self.be.ctx, self.pk, adv.as_ptr(), 0, ins.as_ptr(), lens.as_ptr(), out_ptr, max_failures, &mut total)
            } else {
                h2hip_plonk_check_witness_challenges(self.be.ctx, self.pk, adv.as_ptr(), 0, ins.as_ptr(), lens.as_ptr(), challenges.as_ptr().cast(),
                                                     challenges.len(), out_ptr, max_failures, &mut total)
            }
        })?;
        out.truncate(total.min(max_failures));
        Ok((total, out))
    }
    /// `MockProver::assert_satisfied`: panics with one line per failure (at most 16) when the witness does not satisfy the circuit
    pub fn assert_satisfied(&self, advice: &[Vec<Fr>], instances: &[&[Fr]]) {
        let (total, fails) = self.check_witness(advice, instances, 16).expect("check_witness");
        if total > 0 {
            let lines: Vec<String> = fails.iter().map(|f| match f.kind {
                H2HIP_WITNESS_GATE => format!("gate column {} not satisfied at row {}", f.column, f.row),
                H2HIP_WITNESS_LOOKUP => format!("lookup {}: input at row {} is not in the table", f.column, f.row),
                _ => format!("copy: permutation column {} row {} != column {} row {}", f.column, f.row, f.peer_column, f.peer_row),
            }).collect();
            panic!("witness not satisfied: {total} failures\n{}", lines.join("\n"));
        }
    }
    /// `create_proof(params, pk, &[circuit], &[instances], rng, &mut transcript)` after synthesis: returns what
    /// `transcript.finalize()` would.  `rng_fill` is called for every batch of `Fr::random(rng)` draws, in upstream's order.
    /// `advice` holds phase 0's columns; `later_phases(phase, challenges)` synthesises every later phase's columns (gate columns, then
    /// lookup-advice columns, index order; a key with RLC columns: phase 1's list ends with them) from the challenges squeezed so far — where
    /// halo2-axiom's create_proof runs the next phase's synthesis.
    pub fn create_proof<R: FnMut(&mut [Fr]), W: FnMut(u32, &[Fr]) -> Result<Vec<Vec<Fr>>, E>, E: std::fmt::Display>(
        &self, advice: &[Vec<Fr>], instances: &[&[Fr]], rng_fill: R, later_phases: W) -> Result<Vec<u8>, HipError> {
        self.prove(advice, instances, rng_fill, later_phases, None).map(|p| p.unwrap_or_default())
    }
    /// `create_proof(params, pk, &[circuit], &[instances], rng, &mut transcript)` for ANY transcript (h2hip_plonk_create_proof_transcript):
    /// every transcript operation of the proof goes to `transcript`, in upstream's order, and the proof's bytes are the transcript's — the
    /// caller takes them with its own `finalize()`.  The other arguments are `create_proof`'s.  An `Err` from the transcript aborts the proof:
    /// its message comes back with H2HIP_ERR_INVALID, and the key and the context serve the next proof.
    pub fn create_proof_with_transcript<T: TranscriptWrite, R: FnMut(&mut [Fr]), W: FnMut(u32, &[Fr]) -> Result<Vec<Vec<Fr>>, E>, E: std::fmt::Display>(
        &self, advice: &[Vec<Fr>], instances: &[&[Fr]], rng_fill: R, later_phases: W, transcript: &mut T) -> Result<(), HipError> {
        let mut bridge = WriteBridge { t: transcript, err: None };
        let cb = h2hip_transcript {
            user: (&mut bridge as *mut WriteBridge<T>).cast(),
            common_point: None,
            write_point: Some(write_point_trampoline::<T>),
            common_scalar: Some(common_scalar_trampoline::<T>),
            write_scalar: Some(write_scalar_trampoline::<T>),
            read_point: None,
            read_scalar: None,
            squeeze_challenge: Some(squeeze_trampoline::<T>),
        };
        let res = self.prove(advice, instances, rng_fill, later_phases, Some(&cb));
        match (res, bridge.err.take()) {
            (Err(e), Some(message)) => Err(HipError { code: e.code, message: format!("{message} ({})", e.message) }),
            (Err(e), None) => Err(e),
            (Ok(_), _) => Ok(()),
        }
    }
    /// one proof: into the built-in Blake2b transcript (`transcript` = None, returns its bytes) or over the caller's callbacks (returns None)
    fn prove<R: FnMut(&mut [Fr]), W: FnMut(u32, &[Fr]) -> Result<Vec<Vec<Fr>>, E>, E: std::fmt::Display>(
        &self, advice: &[Vec<Fr>], instances: &[&[Fr]], mut rng_fill: R, later_phases: W, transcript: Option<&h2hip_transcript>)
        -> Result<Option<Vec<u8>>, HipError> {
        unsafe extern "C" fn trampoline<R: FnMut(&mut [Fr])>(user: *mut c_void, out: *mut c_void, n: usize) {
            let f = &mut *(user as *mut R);
            f(std::slice::from_raw_parts_mut(out as *mut Fr, n));
        }
        struct Later<'a, W, E> {
            f: W,
            ctx: *mut h2hip_ctx,
            usable: usize,
            n: usize,
            err: &'a mut Option<String>,
            _e: std::marker::PhantomData<E>,
        }
        unsafe extern "C" fn witness<W: FnMut(u32, &[Fr]) -> Result<Vec<Vec<Fr>>, E>, E: std::fmt::Display>(
            user: *mut c_void, phase: u32, challenges: *const c_void, nch: usize, cols: *const *mut c_void, ncols: usize) -> c_int {
            let l = &mut *(user as *mut Later<W, E>);
            let ch = if nch == 0 { &[][..] } else { std::slice::from_raw_parts(challenges as *const Fr, nch) };
            let got = match (l.f)(phase, ch) {
                Ok(v) => v,
                Err(e) => {
                    *l.err = Some(format!("phase {phase}: {e}"));
                    return 1;
                }
            };
            if got.len() != ncols || got.iter().any(|c| c.len() < l.usable || c.len() > l.n) {
                *l.err = Some(format!("phase {phase}: {} columns of usable_rows..2^k rows expected, got {}", ncols, got.len()));
                return 1;
            }
            for (j, c) in got.iter().enumerate() {
                if h2hip_upload(l.ctx, *cols.add(j), c.as_ptr().cast(), 32 * c.len()) != H2HIP_OK {
                    *l.err = Some(format!("phase {phase}: upload failed"));
                    return 1;
                }
            }
            0
        }
        // the C side reads the (phase-0) column pointers with usable_rows elements each and num_instance instance arrays
        let want = match &self.phased {
            Some(pp) => phase_columns(pp)[0],
            None => self.shape.num_advice_total as usize,
        };
        if advice.len() != want {
            return Err(invalid(format!("create_proof: {} advice columns, phase 0 has {}", advice.len(), want)));
        }
        if let Some(c) = advice.iter().position(|c| c.len() < self.shape.usable_rows as usize) {
            return Err(invalid(format!("create_proof: advice column {c} has {} rows, fewer than the {} usable rows", advice[c].len(), self.shape.usable_rows)));
        }
        if instances.len() != self.params.num_instance as usize {
            return Err(invalid(format!("create_proof: {} instance columns, the circuit has {}", instances.len(), self.params.num_instance)));
        }
        if let Some(c) = instances.iter().position(|c| c.len() > self.shape.usable_rows as usize) {
            return Err(invalid(format!("create_proof: instance column {c} is longer than the usable rows")));
        }
        let adv: Vec<*const c_void> = advice.iter().map(|c| c.as_ptr().cast()).collect();
        let ins: Vec<*const c_void> = instances.iter().map(|c| c.as_ptr().cast()).collect();
        let lens: Vec<usize> = instances.iter().map(|c| c.len()).collect();
        let mut proof = vec![0u8; 32 * (self.shape.num_commitments + self.shape.num_evals) as usize];
        let mut len = 0usize;
        let mut err = None;
        let rc = match (&self.phased, transcript) {
            (None, Some(t)) => unsafe {
                h2hip_plonk_create_proof_transcript(self.be.ctx, self.pk, adv.as_ptr(), 0, ins.as_ptr(), lens.as_ptr(), Some(trampoline::<R>),
                                                    (&mut rng_fill as *mut R).cast(), ptr::null(), t, ptr::null_mut())
            },
            (None, None) => unsafe {
                h2hip_plonk_create_proof(self.be.ctx, self.pk, adv.as_ptr(), 0, ins.as_ptr(), lens.as_ptr(), Some(trampoline::<R>),
                                         (&mut rng_fill as *mut R).cast(), proof.as_mut_ptr(), proof.len(), &mut len, ptr::null_mut())
            },
            (Some(_), _) => {
                let mut later = Later::<W, E> { f: later_phases, ctx: self.be.ctx, usable: self.shape.usable_rows as usize, n: 1usize << self.params.k,
                                                err: &mut err, _e: std::marker::PhantomData };
                let w = h2hip_phase_witness { fill: Some(witness::<W, E>), user: (&mut later as *mut Later<W, E>).cast() };
                unsafe {
                    match transcript {
                        Some(t) => h2hip_plonk_create_proof_transcript(self.be.ctx, self.pk, adv.as_ptr(), 0, ins.as_ptr(), lens.as_ptr(),
                                                                       Some(trampoline::<R>), (&mut rng_fill as *mut R).cast(), &w, t, ptr::null_mut()),
                        None => h2hip_plonk_create_proof_phased(self.be.ctx, self.pk, adv.as_ptr(), 0, ins.as_ptr(), lens.as_ptr(), Some(trampoline::<R>),
                                                                (&mut rng_fill as *mut R).cast(), &w, proof.as_mut_ptr(), proof.len(), &mut len,
                                                                ptr::null_mut()),
                    }
                }
            }
        };
        if let Some(message) = err {
            return Err(HipError { code: rc, message });
        }
        check(rc)?;
        if transcript.is_some() {
            return Ok(None);
        }
        proof.truncate(len);
        Ok(Some(proof))
    }
}

/// The writing half of a transcript as `create_proof_with_transcript` drives it: upstream's `TranscriptWrite<G1Affine, _>` with its
/// `Transcript` supertrait, over the curve this library serves.  The fork implements it for every `T: halo2_proofs::transcript::TranscriptWrite`
/// by forwarding (`squeeze_challenge` = `*squeeze_challenge_scalar::<()>()`); the proof's byte encoding belongs to the implementation.
/// The methods run while the proof is in flight and must not use the proof's `Backend`.
pub trait TranscriptWrite {
    fn common_scalar(&mut self, scalar: Fr) -> std::io::Result<()>;
    fn write_point(&mut self, point: G1Affine) -> std::io::Result<()>;
    fn write_scalar(&mut self, scalar: Fr) -> std::io::Result<()>;
    fn squeeze_challenge(&mut self) -> Fr;
}
/// The reading half (`TranscriptRead<G1Affine, _>`): `read_*` parse the next value (decompressing, if the encoding compresses) and absorb it.
pub trait TranscriptRead {
    fn common_scalar(&mut self, scalar: Fr) -> std::io::Result<()>;
    fn read_point(&mut self) -> std::io::Result<G1Affine>;
    fn read_scalar(&mut self) -> std::io::Result<Fr>;
    fn squeeze_challenge(&mut self) -> Fr;
}
struct WriteBridge<'a, T> {
    t: &'a mut T,
    err: Option<String>,
}
struct ReadBridge<'a, T> {
    t: &'a mut T,
    err: Option<String>,
}
/// keeps the first error and turns it into the callback's non-zero return: nothing unwinds through the C frames
fn io_status(err: &mut Option<String>, what: &str, r: std::io::Result<()>) -> c_int {
    match r {
        Ok(()) => 0,
        Err(e) => {
            err.get_or_insert_with(|| format!("transcript {what}: {e}"));
            1
        }
    }
}
unsafe extern "C" fn common_scalar_trampoline<T: TranscriptWrite>(user: *mut c_void, fr: *const c_void) -> c_int {
    let b = &mut *(user as *mut WriteBridge<T>);
    let r = b.t.common_scalar(ptr::read_unaligned(fr as *const Fr));
    io_status(&mut b.err, "common_scalar", r)
}
unsafe extern "C" fn write_scalar_trampoline<T: TranscriptWrite>(user: *mut c_void, fr: *const c_void) -> c_int {
    let b = &mut *(user as *mut WriteBridge<T>);
    let r = b.t.write_scalar(ptr::read_unaligned(fr as *const Fr));
    io_status(&mut b.err, "write_scalar", r)
}
unsafe extern "C" fn write_point_trampoline<T: TranscriptWrite>(user: *mut c_void, g1_affine: *const c_void) -> c_int {
    let b = &mut *(user as *mut WriteBridge<T>);
    let r = b.t.write_point(ptr::read_unaligned(g1_affine as *const G1Affine));
    io_status(&mut b.err, "write_point", r)
}
unsafe extern "C" fn squeeze_trampoline<T: TranscriptWrite>(user: *mut c_void, out: *mut c_void) -> c_int {
    let b = &mut *(user as *mut WriteBridge<T>);
    ptr::write_unaligned(out as *mut Fr, b.t.squeeze_challenge());
    0
}
unsafe extern "C" fn read_common_scalar_trampoline<T: TranscriptRead>(user: *mut c_void, fr: *const c_void) -> c_int {
    let b = &mut *(user as *mut ReadBridge<T>);
    let r = b.t.common_scalar(ptr::read_unaligned(fr as *const Fr));
    io_status(&mut b.err, "common_scalar", r)
}
unsafe extern "C" fn read_point_trampoline<T: TranscriptRead>(user: *mut c_void, out: *mut c_void) -> c_int {
    let b = &mut *(user as *mut ReadBridge<T>);
    match b.t.read_point() {
        Ok(p) => {
            ptr::write_unaligned(out as *mut G1Affine, p);
            0
        }
        Err(_) => 1,   // a value that cannot be read is a rejection, not an error
    }
}
unsafe extern "C" fn read_scalar_trampoline<T: TranscriptRead>(user: *mut c_void, out: *mut c_void) -> c_int {
    let b = &mut *(user as *mut ReadBridge<T>);
    match b.t.read_scalar() {
        Ok(s) => {
            ptr::write_unaligned(out as *mut Fr, s);
            0
        }
        Err(_) => 1,
    }
}
unsafe extern "C" fn read_squeeze_trampoline<T: TranscriptRead>(user: *mut c_void, out: *mut c_void) -> c_int {
    let b = &mut *(user as *mut ReadBridge<T>);
    ptr::write_unaligned(out as *mut Fr, b.t.squeeze_challenge());
    0
}

/// `verify_proof(params, vk, SingleStrategy::new(params), &[instances], &mut transcript)` for ANY reading transcript
/// (h2hip_plonk_verify_proof_transcript); arguments as for `verify_proof`.  A read that fails, or hands over a bad value, rejects the proof
/// (`Ok(false)`); trailing input is the reader's business.  -> (accepted, the proof's KZG accumulator (W', outer): accepted <=> well-formed and
/// e(W', s_g2) * e(-outer, g2) = 1, what an aggregator defers instead of pairing; the identity twice for a malformed proof).
pub fn verify_proof_with_transcript<T: TranscriptRead>(params: h2hip_base_circuit_params, phases: &PhaseCounts, fixed_commitments: &[G1Affine],
                                                       permutation_commitments: &[G1Affine], transcript_repr: Fr, g1: G1Affine, g2: &[u8; 128],
                                                       s_g2: &[u8; 128], instances: &[&[Fr]], transcript: &mut T)
                                                       -> Result<(bool, [G1Affine; 2]), HipError> {
    let phased = if phases.is_first_phase_only() { None } else { Some(phases.to_c(&params)?) };
    let rlc = phases.to_c_rlc(&params)?;
    let mut shape = h2hip_plonk_shape::default();
    match (&rlc, &phased) {
        (Some(rp), _) => check(unsafe { h2hip_plonk_shape_of_rlc(rp, &mut shape) })?,
        (None, Some(pp)) => check(unsafe { h2hip_plonk_shape_of_phased(pp, &mut shape) })?,
        (None, None) => check(unsafe { h2hip_plonk_shape_of(&params, &mut shape) })?,
    }
    if fixed_commitments.len() != shape.num_fixed_total as usize || permutation_commitments.len() != shape.num_perm_columns as usize {
        return Err(invalid(format!("verify_proof: {} fixed / {} permutation commitments, the shape has {} / {}", fixed_commitments.len(),
                                   permutation_commitments.len(), shape.num_fixed_total, shape.num_perm_columns)));
    }
    if instances.len() != params.num_instance as usize {
        return Err(invalid(format!("verify_proof: {} instance columns, the circuit has {}", instances.len(), params.num_instance)));
    }
    let ins: Vec<*const c_void> = instances.iter().map(|c| c.as_ptr().cast()).collect();
    let lens: Vec<usize> = instances.iter().map(|c| c.len()).collect();
    let (kind, params_ptr): (c_int, *const c_void) = match (&rlc, &phased) {
        (Some(rp), _) => (H2HIP_CIRCUIT_RLC, (rp as *const h2hip_rlc_circuit_params).cast()),
        (None, Some(pp)) => (H2HIP_CIRCUIT_PHASED, (pp as *const h2hip_phased_circuit_params).cast()),
        (None, None) => (H2HIP_CIRCUIT_BASE, (&params as *const h2hip_base_circuit_params).cast()),
    };
    let mut bridge = ReadBridge { t: transcript, err: None };
    let cb = h2hip_transcript {
        user: (&mut bridge as *mut ReadBridge<T>).cast(),
        common_point: None,
        write_point: None,
        common_scalar: Some(read_common_scalar_trampoline::<T>),
        write_scalar: None,
        read_point: Some(read_point_trampoline::<T>),
        read_scalar: Some(read_scalar_trampoline::<T>),
        squeeze_challenge: Some(read_squeeze_trampoline::<T>),
    };
    let mut ok: c_int = 0;
    let mut acc = [G1Affine::default(); 2];
    let rc = unsafe {
        h2hip_plonk_verify_proof_transcript(kind, params_ptr, fixed_commitments.as_ptr().cast(), permutation_commitments.as_ptr().cast(),
                                            fr_ptr(&transcript_repr), (&g1 as *const G1Affine).cast(), g2.as_ptr().cast(), s_g2.as_ptr().cast(),
                                            ins.as_ptr(), lens.as_ptr(), &cb, &mut ok, acc.as_mut_ptr().cast())
    };
    if let (true, Some(message)) = (rc != H2HIP_OK, bridge.err.take()) {
        return Err(HipError { code: rc, message });
    }
    check(rc)?;
    Ok((ok != 0, acc))
}
/// `verify_proof(params, vk, SingleStrategy::new(params), &[instances], &mut Blake2bRead::init(proof))` (check_proof,
/// halo2-base/src/utils/testing.rs:64-88): `g1` = params.get_g()[0], `g2` / `s_g2` = the verifier half of the SRS in RawBytes form.
/// `phases`: as for `ProvingKeyHip::keygen` (a circuit with more than one phase or with challenges goes through h2hip_plonk_verify_proof_phased,
/// one with RLC columns through h2hip_plonk_verify_proof_rlc).
pub fn verify_proof(params: h2hip_base_circuit_params, phases: &PhaseCounts, fixed_commitments: &[G1Affine], permutation_commitments: &[G1Affine],
                    transcript_repr: Fr, g1: G1Affine, g2: &[u8; 128], s_g2: &[u8; 128], instances: &[&[Fr]], proof: &[u8]) -> Result<bool, HipError> {
    let phased = if phases.is_first_phase_only() { None } else { Some(phases.to_c(&params)?) };
    let rlc = phases.to_c_rlc(&params)?;
    // the C side reads num_fixed_total / num_perm_columns commitments and num_instance instance arrays: check the slices first
    let mut shape = h2hip_plonk_shape::default();
    match (&rlc, &phased) {
        (Some(rp), _) => check(unsafe { h2hip_plonk_shape_of_rlc(rp, &mut shape) })?,
        (None, Some(pp)) => check(unsafe { h2hip_plonk_shape_of_phased(pp, &mut shape) })?,
        (None, None) => check(unsafe { h2hip_plonk_shape_of(&params, &mut shape) })?,
    }
    if fixed_commitments.len() != shape.num_fixed_total as usize || permutation_commitments.len() != shape.num_perm_columns as usize {
        return Err(invalid(format!("verify_proof: {} fixed / {} permutation commitments, the shape has {} / {}", fixed_commitments.len(),
                                   permutation_commitments.len(), shape.num_fixed_total, shape.num_perm_columns)));
    }
    if instances.len() != params.num_instance as usize {
        return Err(invalid(format!("verify_proof: {} instance columns, the circuit has {}", instances.len(), params.num_instance)));
    }
    let ins: Vec<*const c_void> = instances.iter().map(|c| c.as_ptr().cast()).collect();
    let lens: Vec<usize> = instances.iter().map(|c| c.len()).collect();
    let mut ok: c_int = 0;
    check(unsafe {
        match (&rlc, &phased) {
            (Some(rp), _) => h2hip_plonk_verify_proof_rlc(rp, fixed_commitments.as_ptr().cast(), permutation_commitments.as_ptr().cast(),
                                                          fr_ptr(&transcript_repr), (&g1 as *const G1Affine).cast(), g2.as_ptr().cast(), s_g2.as_ptr().cast(),
                                                          ins.as_ptr(), lens.as_ptr(), proof.as_ptr(), proof.len(), &mut ok),
            (None, Some(pp)) => h2hip_plonk_verify_proof_phased(pp, fixed_commitments.as_ptr().cast(), permutation_commitments.as_ptr().cast(),
                                                        fr_ptr(&transcript_repr), (&g1 as *const G1Affine).cast(), g2.as_ptr().cast(), s_g2.as_ptr().cast(),
                                                        ins.as_ptr(), lens.as_ptr(), proof.as_ptr(), proof.len(), &mut ok),
            (None, None) => h2hip_plonk_verify_proof(&params, fixed_commitments.as_ptr().cast(), permutation_commitments.as_ptr().cast(), fr_ptr(&transcript_repr),
                                             (&g1 as *const G1Affine).cast(), g2.as_ptr().cast(), s_g2.as_ptr().cast(), ins.as_ptr(), lens.as_ptr(),
                                             proof.as_ptr(), proof.len(), &mut ok),
        }
    })?;
    Ok(ok != 0)
}

/// `BatchVerifier::finalize`: every proof of `proofs` under one (first-phase-only BaseConfig) verifying key with ONE pairing; the proofs' points are
/// decompressed and all scalar multiplications run on the GPU (h2hip_plonk_verify_batch).  `instances[i]`: the instance columns of proof i.
/// `rng_fill` draws one combiner per proof, in one call.  -> (accepted, per-proof rejections).
pub fn verify_proofs<R: FnMut(&mut [Fr])>(be: &Backend, params: h2hip_base_circuit_params, fixed_commitments: &[G1Affine],
                                         permutation_commitments: &[G1Affine], transcript_repr: Fr, g1: G1Affine, g2: &[u8; 128], s_g2: &[u8; 128],
                                         instances: &[&[&[Fr]]], proofs: &[&[u8]], mut rng_fill: R) -> Result<(bool, Vec<bool>), HipError> {
    unsafe extern "C" fn trampoline<R: FnMut(&mut [Fr])>(user: *mut c_void, out: *mut c_void, n: usize) {
        let f = &mut *(user as *mut R);
        f(std::slice::from_raw_parts_mut(out as *mut Fr, n));
    }
    let mut shape = h2hip_plonk_shape::default();
    check(unsafe { h2hip_plonk_shape_of(&params, &mut shape) })?;
    if fixed_commitments.len() != shape.num_fixed_total as usize || permutation_commitments.len() != shape.num_perm_columns as usize {
        return Err(invalid(format!("verify_proofs: {} fixed / {} permutation commitments, the shape has {} / {}", fixed_commitments.len(),
                                   permutation_commitments.len(), shape.num_fixed_total, shape.num_perm_columns)));
    }
    if instances.len() != proofs.len() || instances.iter().any(|cols| cols.len() != params.num_instance as usize) {
        return Err(invalid(format!("verify_proofs: {} instance columns per proof, one list per proof", params.num_instance)));
    }
    let ins: Vec<*const c_void> = instances.iter().flat_map(|cols| cols.iter().map(|c| c.as_ptr().cast())).collect();
    let lens: Vec<usize> = instances.iter().flat_map(|cols| cols.iter().map(|c| c.len())).collect();
    let ptrs: Vec<*const u8> = proofs.iter().map(|p| p.as_ptr()).collect();
    let plens: Vec<usize> = proofs.iter().map(|p| p.len()).collect();
    let mut rejected = vec![0u8; proofs.len().max(1)];
    let mut ok: c_int = 0;
    check(unsafe {
        h2hip_plonk_verify_batch(be.ctx, H2HIP_CIRCUIT_BASE, (&params as *const h2hip_base_circuit_params).cast(), fixed_commitments.as_ptr().cast(),
                                 permutation_commitments.as_ptr().cast(), fr_ptr(&transcript_repr), (&g1 as *const G1Affine).cast(), g2.as_ptr().cast(),
                                 s_g2.as_ptr().cast(), proofs.len(), ins.as_ptr(), lens.as_ptr(), ptrs.as_ptr(), plens.as_ptr(), Some(trampoline::<R>),
                                 (&mut rng_fill as *mut R).cast(), &mut ok, rejected.as_mut_ptr(), ptr::null_mut())
    })?;
    rejected.truncate(proofs.len());
    Ok((ok != 0, rejected.iter().map(|&b| b != 0).collect()))
}

impl Drop for ProvingKeyHip<'_, '_> {
    fn drop(&mut self) {
        unsafe { h2hip_plonk_pk_free(self.be.ctx, self.pk) }
    }
}
