"""The shared test modules themselves: no test file imports from another, the capture protocol is written once, and the two
capture harnesses of capture.py fail when they should.

GPU (-m gpu): each harness is handed a case that must not pass -- a replay checked against the wrong version, a "refused" call
that is in fact accepted -- and has to raise.  Nothing faults: both are failing assertions.
"""
import glob
import os
import re

import numpy as np
import pytest

import capture
from support import SENTINEL, Guarded, packbits

HERE = os.path.dirname(os.path.abspath(__file__))
AND = 0
N = 4096 + 5  # one full 4096-row span and a ragged tail

# files that construct a graph of their own, with what makes their sequence differ from capture.capture_replay
OWN_CAPTURE = {
    "test_gpu_parity.py": "test_scan_can_be_captured_in_a_hip_graph: an engine on the default stream, outputs allocated by the captured call",
    "test_graph_capture.py": "the engine pipeline allocates its outputs inside the capture; the Infinity Cache test reads divisors inside it and scans "
                             "eagerly between capture and replays",
}

gpu = pytest.mark.gpu


def sources():
    return sorted(glob.glob(os.path.join(HERE, "*.py")))


def test_no_test_module_imports_another():
    assert len(sources()) > 30
    for path in sources():
        found = re.findall(r"^\s*(?:from|import)\s+test_\w*", open(path).read(), flags=re.M)
        assert not found, f"{os.path.basename(path)}: {found}: what two test files share belongs in support.py, capture.py or kernel_cases.py"


def test_capture_protocol_lives_once():
    users = {os.path.basename(p) for p in sources() if p != os.path.abspath(__file__) and "torch.cuda.CUDAGraph(" in open(p).read()}
    assert "capture.py" in users
    assert users - {"capture.py"} == set(OWN_CAPTURE), sorted(users)


def bitmaps(seed):
    rng = np.random.default_rng(seed)
    return rng.random(N) < 0.4, rng.random(N) < 0.6


def combine_and(eng, a, b, out):
    from shared_simd_scan_amd import lib

    return lib().mi355_bitmap_combine_dev(eng._ctx, AND, a.data_ptr(), b.data_ptr(), out.ptr, N, None)


@gpu
def test_harness_catches_a_stale_replay():
    """mi355_bitmap_combine_dev (AND) over two versions of its inputs; check(1) is given version 0's expectation, as a replay that
    did not follow its inputs would need it: capture_replay must fail, and say at which replay"""
    import torch

    versions = [bitmaps(1), bitmaps(2)]
    wants = [packbits(a & b) for a, b in versions]
    assert not np.array_equal(wants[0], wants[1])

    def steps(eng):
        stage = [[torch.from_numpy(packbits(x)).cuda() for x in v] for v in versions]
        a, b = torch.empty_like(stage[0][0]), torch.empty_like(stage[0][1])
        out = Guarded((N + 7) // 8)

        def load(r):
            a.copy_(stage[r][0])
            b.copy_(stage[r][1])
            out.t.fill_(SENTINEL)

        def run():
            assert combine_and(eng, a, b, out) == 0

        def check(r, what):
            assert np.array_equal(out.fetch(), wants[0]), what  # version 0's, whatever r is

        def untouched():
            assert (out.fetch() == SENTINEL).all()

        return capture.Steps(load, run, check, untouched)

    with pytest.raises(AssertionError, match="replay of version 1"):
        capture.capture_replay(steps, (0, 1))


@gpu
def test_refusal_harness_catches_a_call_that_is_not_refused():
    """the "big" call is the size of the small one: nothing has to grow, the library accepts it under capture, and
    refused_under_capture must fail on its status"""
    import torch

    x, y = bitmaps(3)

    def setup(eng):
        a, b = torch.from_numpy(packbits(x)).cuda(), torch.from_numpy(packbits(y)).cuda()
        out, refused = Guarded((N + 7) // 8), Guarded((N + 7) // 8)

        def small():
            assert combine_and(eng, a, b, out) == 0

        def check_small():
            assert np.array_equal(out.fetch(), packbits(x & y))

        return small, lambda: combine_and(eng, a, b, refused), lambda: out.t.fill_(SENTINEL), check_small, refused

    with pytest.raises(AssertionError, match="not refused for the capture's sake: status 0"):
        capture.refused_under_capture(setup)
