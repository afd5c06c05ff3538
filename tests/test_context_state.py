"""The state a context carries from one call to the next, on the CPU-emulated build: the sequences of tests/context_state_checks.py, every result
against an independent reference.  The emulated runtime runs every stream operation at once and in order, so what fails here is bookkeeping — a
slot trusted that was not zeroed, a table looked up under the wrong key, a spec overwritten; an ordering between streams can only go wrong on the
device, where the same sequences run from tests/test_context_state_gpu.py."""
import contextlib

import pytest

from tests import context_state_checks as K

NT = 4   # oracle threads


@contextlib.contextmanager
def fresh_context():
    from tests.emu_util import emu_context

    c = emu_context()
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
