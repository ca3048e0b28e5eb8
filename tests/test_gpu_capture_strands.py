"""GPU: captured cpi_preintegrate_batch calls on strands (include/cpi_amd.h: cpi_ctx_set_capture_strands) must write bit for bit
what the eager, serial sequence writes.  Twelve calls captured into one HIP graph and replayed five times; sha256 of every output
tensor after every replay against the eager run.  Models 1 and 2, mean-only and with (analytic) Jacobians, at W = 640, N = 9
(several lanes per window) and W = 130, N = 50; the context's default and 2, 3 and 4 strands.  Programs: a ring of 4 output sets
from 4 batches (the sets sort themselves onto strands), one set (a chain), 12 sets (a round-robin), the caller's copy_ into `lin`
between calls 5 and 6 (a join by the caller), and capture, eager, second capture.  tests/test_gpu_capture_strands_cpp.py reads
the graph's edges."""
import pytest

from tests.test_gpu_capture_overlap import CALLS, SHAPES, VARIANTS, Case

pytestmark = pytest.mark.gpu

STRANDS = (None, 2, 3, 4)   # the context's default, and every strand count that overlaps


def _case(variant, W, N, nsets, strands):
    c = Case(variant, W, N, nsets, None)
    if strands is not None:
        c.engs[0].set_capture_strands(strands)
    return c


def _cases(fn):
    fn = pytest.mark.parametrize("strands", STRANDS, ids=lambda s: "default" if s is None else "strands%d" % s)(fn)
    return pytest.mark.parametrize("variant", sorted(VARIANTS))(fn)


@_cases
def test_four_batches_into_a_ring_of_four_output_sets(variant, strands):
    for W, N in SHAPES:
        c = _case(variant, W, N, 4, strands)

        def program():
            for i in range(CALLS):
                c.call((i + i // 4) % 4, i % 4)   # set s is written by calls s, s + 4, s + 8 from three different batches
        want = c.eager(program)
        c.check_replays(c.capture(program), want, "W=%d N=%d" % (W, N))


@_cases
def test_all_calls_into_one_output_set(variant, strands):
    """The last writer wins, every replay: every call conflicts with the one strand in use and follows it."""
    for W, N in SHAPES:
        c = _case(variant, W, N, 1, strands)

        def program():
            for i in range(CALLS):
                c.call((i + i // 4) % 4, 0)
        want = c.eager(program)
        c.check_replays(c.capture(program), want, "W=%d N=%d" % (W, N))


@_cases
def test_twelve_calls_into_twelve_output_sets(variant, strands):
    for W, N in SHAPES:
        c = _case(variant, W, N, CALLS, strands)

        def program():
            for i in range(CALLS):
                c.call((i + i // 4) % 4, i)
        want = c.eager(program)
        c.check_replays(c.capture(program), want, "W=%d N=%d" % (W, N))


@_cases
def test_copy_into_the_next_calls_lin_between_two_calls(variant, strands):
    """The caller's own copy_ into `lin`, captured between calls 5 and 6: calls 0-5 read what was there before (and must not
    see the copy), calls 6-11 read what it wrote.  The program restores lin first, so every replay can tell."""
    for W, N in SHAPES:
        c = _case(variant, W, N, CALLS, strands)
        lin = c.batches[0][1].clone()
        before, after = c.batches[1][1].clone(), c.batches[2][1].clone()

        def program():
            lin.copy_(before)
            for i in range(6):
                c.call(i % 4, i, lin=lin)
            lin.copy_(after)
            for i in range(6, CALLS):
                c.call(i % 4, i, lin=lin)
        want = c.eager(program)
        c.check_replays(c.capture(program), want, "W=%d N=%d" % (W, N))


@_cases
def test_capture_then_eager_then_second_capture(variant, strands):
    for W, N in SHAPES:
        c = _case(variant, W, N, 4, strands)

        def program():
            for i in range(CALLS):
                c.call((i + i // 4) % 4, i % 4)

        def program2():
            for i in range(CALLS):
                c.call((2 * i + 1 + i // 4) % 4, (i + 1) % 4)
        want, want2 = c.eager(program), c.eager(program2)
        g1 = c.capture(program)
        c.check_replays(g1, want, "first capture W=%d N=%d" % (W, N))
        assert c.eager(program2) == want2, "eager use after a capture"
        g2 = c.capture(program2)
        c.check_replays(g2, want2, "second capture W=%d N=%d" % (W, N))
        c.check_replays(g1, want, "first graph again W=%d N=%d" % (W, N))
