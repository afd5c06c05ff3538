"""The state a context carries from one call to the next, on the GPU: the sequences of tests/context_state_checks.py, every result against an
independent reference.  Here the zero-fills behind a reduction, the lanes and the job uploads run on real streams (the emulated build of
tests/test_context_state.py executes them at once and in order)."""
import contextlib

import pytest

import halo2_lib_amd as H
from tests import context_state_checks as K

pytestmark = pytest.mark.gpu

NT = 16   # oracle threads


@contextlib.contextmanager
def fresh_context():
    c = H.Context()
    try:
        yield c
    finally:
        c.close()


def test_lone_msm_bucket_array():
    assert K.check_lone_bucket_array(fresh_context, NT) == 17


def test_batch_shared_bucket_array():
    K.check_batch_shared_bucket_array(fresh_context, NT)


def test_twiddle_sets_and_direct_table_slots():
    assert K.check_twiddle_sets(fresh_context, NT) > K.TWIDDLE_SETS + 20


def test_job_ring_wraps():
    assert K.check_job_ring(fresh_context, NT) >= 2


def test_poseidon_specs():
    K.check_poseidon_specs(fresh_context)


@pytest.mark.parametrize("order", K.ORDERS)
def test_any_order(order):
    assert K.check_any_order(fresh_context, order) == 14
