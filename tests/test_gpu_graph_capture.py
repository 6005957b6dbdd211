"""`ladcast_amd.graphs.capture`: the one hipGraph capture-and-replay routine, without a model.  The captured callable is two dependent
launches over 1024 floats (`scale_f32` into a scratch tensor, `axpby_f32` from it): launch-only, with inputs, an output and a
dependency between the launches."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_gpu_ops import hip, rnd  # noqa: E402,F401  (`hip`: the module fixture of the op tests)

N = 1024


def _callable(hip, log=None):
    def fn(x, y):
        if log is not None:
            log.append(("fn", torch.cuda.current_stream(), torch.cuda.is_current_stream_capturing()))
        mid, out = torch.empty_like(x), torch.empty_like(x)
        hip.scale_f32(x, 3.0, mid)
        hip.axpby_f32(mid, 0.5, y, -2.0, out)
        return out

    return fn


def _inputs(seed):
    return rnd(N, seed=seed).cuda(), rnd(N, seed=100 + seed).cuda()


def test_callable_runs_twice_on_the_capture_stream_and_replays_match_eager(hip):
    from ladcast_amd import graphs

    log, side = [], torch.cuda.Stream()
    x, y = _inputs(0)
    ent = graphs.capture(_callable(hip, log), [x, y], x.device, side)
    assert [(s, c) for _, s, c in log] == [(side, False), (side, True)]  # warm-up, then capture, both on the stream passed in
    eager = _callable(hip)
    for seed in (1, 2, 3):
        a, b = _inputs(seed)
        got = ent.replay(a, b)
        assert torch.equal(got, eager(a, b))
        got.fill_(float("nan"))  # a fresh tensor: writing into it must not reach the graph's own output
        assert torch.equal(ent.replay(a, b), eager(a, b))
    assert len(log) == 2  # replays never call it


def test_reset_runs_once_between_a_completed_warm_up_and_the_capture(hip):
    from ladcast_amd import graphs

    side, order, done = torch.cuda.Stream(), [], torch.cuda.Event()
    big = torch.empty(1 << 28, device="cuda")
    with torch.cuda.stream(side):  # a few ms of work in front of the warm-up: its launches complete only if somebody waits for them
        for _ in range(8):
            big.zero_()
    inner = _callable(hip)

    def fn(x, y):
        capturing = torch.cuda.is_current_stream_capturing()
        order.append("capture" if capturing else "warm-up")
        out = inner(x, y)
        if not capturing:
            done.record()
        return out

    def reset():
        with torch.cuda.stream(side):
            capturing = torch.cuda.is_current_stream_capturing()
        order.append(("reset", done.query(), capturing))

    x, y = _inputs(4)
    ent = graphs.capture(fn, [x, y], x.device, side, reset=reset)
    ent.replay(x, y)
    assert order == ["warm-up", ("reset", True, False), "capture"]


def test_capture_zeroes_a_dirty_attention_workspace_of_the_capture_stream(hip):
    """a faulted / aborted balanced fp32-attention launch may leave ticket counters non-zero: every capture re-arms them first"""
    from ladcast_amd import graphs

    side = torch.cuda.Stream()
    x, y = _inputs(5)
    with torch.cuda.stream(side):
        ws = hip._attn_f32_workspace(x.device)
    torch.cuda.synchronize()  # (the stream handle may be one a model captured on earlier: nothing of it is in flight now)
    try:
        ws.fill_(1.0)  # no attention kernel is launched while it is dirty
        ent = graphs.capture(_callable(hip), [x, y], x.device, side)
        torch.cuda.synchronize()
        assert int(torch.count_nonzero(ws)) == 0
        assert torch.equal(ent.replay(x, y), _callable(hip)(x, y))
    finally:
        ws.zero_()
        torch.cuda.synchronize()


def test_entry_keeps_the_bag_and_the_stream_alive(hip):
    from ladcast_amd import graphs

    side, bag = torch.cuda.Stream(), {"table": torch.arange(4, device="cuda")}
    x, y = _inputs(6)
    ent = graphs.capture(_callable(hip), [x, y], x.device, side, keep=bag)
    assert ent.keep is bag and ent.stream is side
    assert isinstance(ent, tuple)  # what the models' graph stores are counted by
    assert [t.data_ptr() for t in ent.inputs] != [x.data_ptr(), y.data_ptr()]  # static copies, not the caller's tensors
