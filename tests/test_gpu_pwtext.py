"""wtz_pwtext_batch on the GPU: the cases of tests/pwtextref.py (every shape the kernel can go wrong at: tile and wave boundaries in columns and operations,
every output alignment, every view) against the restatement of kswx.h:1150-1194 + pairaln.c:115-125, which tests/test_pwtext_cpu.py pins to the reference's
own pictures.  Here the scans, the 65-way search and the ballots run with 64 lanes."""
import pytest

import pwtextref as pw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return pw.Cases()


@pytest.fixture(scope="module")
def ctx(cases):
    c = pw.context(cases)
    yield c
    c.close()


def test_device_equals_the_restatement_on_every_case(ctx, cases):
    pw.check_whole_batch(ctx, cases)


def test_reversed_batch_and_single_alignments_give_the_same_bytes(ctx, cases):
    pw.check_batching_does_not_matter(ctx, cases)


def test_argument_errors_leave_the_context_usable(ctx, cases):
    pw.check_argument_errors(ctx, cases)


def test_a_small_pool_cuts_the_call_into_launch_groups(cases):
    pw.check_small_pool(cases, None)


def test_one_alignment_larger_than_the_pool_is_a_pool_error(cases):
    pw.check_pool_error(cases, None)
