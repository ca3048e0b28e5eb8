"""GPU: captured cpi_preintegrate_batch calls may overlap in the graph (include/cpi_amd.h: cpi_ctx_set_capture_overlap) and must
still write bit for bit what the eager, serial sequence writes.  Twelve calls captured into one HIP graph and replayed five
times; sha256 of every output tensor after every replay against the eager run.  Models 1 and 2, mean-only and with (analytic)
Jacobians -- the single-kernel routes the overlap applies to -- at W = 640, N = 9 (several lanes per window) and W = 130, N = 50,
at the default depth and at the largest.  tests/test_gpu_capture_overlap_cpp.py reads the graph's edges."""
import hashlib

import pytest
import torch

import cpi_amd
from cpi_amd import synth

pytestmark = pytest.mark.gpu

SHAPES = ((640, 9), (130, 50))
CALLS, REPLAYS = 12, 5
VARIANTS = {"m1-mean": (1, ("mean",)), "m1-jac": (1, ("mean", "jac")), "m2-mean": (2, ("mean",)), "m2-jac": (2, ("mean", "jac"))}


def _digest(outs):
    h = hashlib.sha256()
    for out in outs:
        for k in sorted(out):
            h.update(out[k].cpu().numpy().tobytes())
    return h.hexdigest()


class Case:
    """Four input batches and `nsets` output sets of one shape and variant on one device."""

    def __init__(self, variant, W, N, nsets, depth, nengines=1):
        assert torch.cuda.is_available(), "GPU tests need a GPU"
        self.model, self.want = VARIANTS[variant]
        self.dev = torch.device("cuda", 0)
        self.streams = [torch.cuda.Stream(self.dev) for _ in range(nengines)] if nengines > 1 else [None]
        self.engs = [cpi_amd.Engine(device=0, stream=s) for s in self.streams]
        for e in self.engs:
            if depth is not None:
                e.set_capture_overlap(depth)
        # model 2 with Jacobians: the analytic ones (one mean kernel), not those read out of the covariance recursion
        self.prm = self.engs[0].make_params(self.model, state_transition_jacobians=False)
        self.batches = [synth.make_windows(W, N, seed=900 + 7 * b + N, device=self.dev) for b in range(4)]
        self.outs = [self.engs[0].alloc_outputs(W, self.want, self.model) for _ in range(nsets)]
        self.poison()
        torch.cuda.synchronize()

    def poison(self):
        for out in self.outs:
            for t in out.values():
                t.fill_(float("nan"))

    def call(self, b, s, eng=0, lin=None):
        kn, l, q = self.batches[b]
        self.engs[eng].preintegrate(kn, l if lin is None else lin, q if self.model == 2 else None, self.prm, want=self.want, out=self.outs[s])

    def eager(self, program):
        s = torch.cuda.Stream(self.dev)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            program()
        torch.cuda.synchronize()
        d = _digest(self.outs)
        self.poison()
        torch.cuda.synchronize()
        return d

    def capture(self, program):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            program()
        return g

    def check_replays(self, g, want, label):
        for r in range(REPLAYS):
            g.replay()
            torch.cuda.synchronize()
            assert _digest(self.outs) == want, "%s: replay %d differs from the eager sequence" % (label, r)
            self.poison()
            torch.cuda.synchronize()


DEPTHS = (None, 4)   # the context's default, and the deepest window


def _cases(fn):
    fn = pytest.mark.parametrize("depth", DEPTHS, ids=lambda d: "default" if d is None else "depth%d" % d)(fn)
    return pytest.mark.parametrize("variant", sorted(VARIANTS))(fn)


@_cases
def test_four_batches_into_four_output_sets(variant, depth):
    for W, N in SHAPES:
        c = Case(variant, W, N, 4, depth)

        def program():
            for i in range(CALLS):
                c.call((i + i // 4) % 4, i % 4)   # set s is written by calls s, s + 4, s + 8 from three different batches
        want = c.eager(program)
        c.check_replays(c.capture(program), want, "W=%d N=%d" % (W, N))


@_cases
def test_all_calls_into_one_output_set(variant, depth):
    """The last writer wins, every replay: the calls conflict pairwise and stay a chain."""
    for W, N in SHAPES:
        c = Case(variant, W, N, 1, depth)

        def program():
            for i in range(CALLS):
                c.call((i + i // 4) % 4, 0)
        want = c.eager(program)
        c.check_replays(c.capture(program), want, "W=%d N=%d" % (W, N))


@_cases
def test_copy_into_the_next_calls_lin_between_two_calls(variant, depth):
    """The caller's own copy_ into `lin`, captured between calls 5 and 6: calls 0-5 read what was there before (and must not
    see the copy), calls 6-11 read what it wrote.  The program restores lin first, so every replay can tell."""
    for W, N in SHAPES:
        c = Case(variant, W, N, CALLS, depth)
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
def test_two_contexts_on_two_forked_streams_in_one_capture(variant, depth):
    for W, N in SHAPES:
        c = Case(variant, W, N, CALLS, depth, nengines=2)

        def program():
            cur = torch.cuda.current_stream()
            for e, s in enumerate(c.streams):
                s.wait_stream(cur)
                with torch.cuda.stream(s):
                    for i in range(CALLS // 2):
                        c.call((i + e) % 4, 2 * i + e, eng=e)
            for s in c.streams:
                cur.wait_stream(s)
        want = c.eager(program)
        c.check_replays(c.capture(program), want, "W=%d N=%d" % (W, N))


@_cases
def test_capture_then_eager_then_second_capture(variant, depth):
    for W, N in SHAPES:
        c = Case(variant, W, N, 4, depth)

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


@_cases
def test_exception_inside_a_capture_block_leaves_the_context_usable(variant, depth):
    W, N = SHAPES[0]
    c = Case(variant, W, N, 4, depth)

    def program():
        for i in range(CALLS):
            c.call((i + i // 4) % 4, i % 4)
    want = c.eager(program)

    class Boom(Exception):
        pass
    g = torch.cuda.CUDAGraph()
    with pytest.raises(Boom):
        with torch.cuda.graph(g):
            for i in range(5):
                c.call(i % 4, i % 4)
            raise Boom()
    del g
    torch.cuda.synchronize()
    c.poison()
    assert c.eager(program) == want, "eager use after the failed block"
    c.check_replays(c.capture(program), want, "capture after the failed block")
