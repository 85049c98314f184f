"""Graph capture of the library's calls, once for every test file: the capture-and-replay protocol (capture_replay) and the
"refused while capturing" harness (refused_under_capture).  torch.cuda.CUDAGraph is constructed here and in the few tests that
tests/test_support_harness.py lists with the reason they differ.

A plain module like support.py: a test file keeps its data, its closures and its launch-record assertion, and hands them over."""
from dataclasses import dataclass
from typing import Callable, Optional

from support import E_INVALID, SENTINEL, parse_record


@dataclass
class Steps:
    """what a captured call brings to capture_replay"""
    load: Callable                              # load(r): inputs of version r in place, every output refilled
    run: Callable                               # run(): the call, or the chain of calls, that is captured
    check: Callable                             # check(r, what): every output holds version r's expectation, guards intact
    untouched: Callable                         # untouched(): every output still holds what load(0) left there
    warmed: Optional[Callable] = None           # warmed(record): the parsed launch record of the eager run's last call
    before_capture: Optional[Callable] = None   # before_capture(): directly in front of the capture
    between: Optional[Callable] = None          # between(r): eager work on the same stream and context in front of replay r


def last_record(eng):
    from shared_simd_scan_amd import lib

    return parse_record((lib().mi355_ctx_last_launch(eng._ctx) or b"").decode())


def capture_replay(setup, replays, opts=()):
    """The protocol.  The context lives on the side stream that is captured (a fresh ScanEngine(0, stream=side) with the context
    options `opts`); setup(eng) -> Steps runs on that stream, so every buffer exists before the capture.  The call runs once eagerly
    (kernel code loaded, occupancy queried, workspace grown), warmed() sees its launch record and check(0, "eager warm-up") its
    result; the inputs are loaded again and the call is captured on that one stream (a linear chain of nodes: no second stream, no
    fork / join) with torch's default capture_error_mode "global", so an illegal call anywhere ends the capture with an error;
    after the capture and before the first replay untouched() finds every output as load(0) left it -- the call was recorded, not
    executed; then one replay per r of `replays`, each over inputs overwritten in place and outputs refilled by load(r), each
    held to check(r, "replay of version r").  Whatever happens, the stream is drained, the graph dropped and the engine closed."""
    import torch

    from shared_simd_scan_amd import ScanEngine

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        eng = ScanEngine(0, stream=side)
        g = None
        try:
            for name, value in opts:
                eng.set_option(name, value)
            s = setup(eng)
            s.load(0)
            s.run()
            side.synchronize()
            if s.warmed:
                s.warmed(last_record(eng))
            s.check(0, "eager warm-up")
            s.load(0)
            side.synchronize()
            if s.before_capture:
                s.before_capture()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                s.run()
            side.synchronize()
            try:
                s.untouched()
            except AssertionError as e:
                raise AssertionError(f"ran instead of being recorded: {e}") from e
            for r in replays:
                if s.between:
                    s.between(r)
                s.load(r)
                g.replay()
                side.synchronize()
                s.check(r, f"replay of version {r}")
        finally:
            side.synchronize()
            del g
            eng.close()


def refused_under_capture(setup):
    """A fresh context that has seen the small call only: under capture the big one is refused (MI355_E_INVALID, the message names
    graph capture), nothing is enqueued for it and the capture stays intact -- the small call around it replays.
    setup(eng) -> (small, big, reset, check_small, refused): small() is the call that is recorded; big() the call that must be
    refused, it returns its status; reset() puts the outputs back after the warm-up; check_small() runs after the replay;
    refused is the Guarded output of the refused call."""
    import torch

    from shared_simd_scan_amd import ScanEngine, lib

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        eng = ScanEngine(0, stream=side)
        g = None
        try:
            small, big, reset, check_small, refused = setup(eng)
            small()
            side.synchronize()
            reset()
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                small()
                rc = big()
                msg = (lib().mi355_last_error() or b"").decode()
                record = (lib().mi355_ctx_last_launch(eng._ctx) or b"").decode()
            side.synchronize()
            assert rc == E_INVALID and "graph" in msg and "captur" in msg, f"not refused for the capture's sake: status {rc}, message {msg!r}"
            assert record == "", f"the refused call left a launch record: {record!r}"
            g.replay()
            side.synchronize()
            check_small()
            assert (refused.fetch() == SENTINEL).all(), "the refused call wrote to its output"
        finally:
            side.synchronize()
            del g
            eng.close()
