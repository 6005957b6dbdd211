"""The per-stream workspace store of `ladcast_amd/hip.py` (`_workspace`): one block per (name, device, stream), created at the first call
outside a graph capture, never replaced unless it is the growing scoring scratch.  Each test runs on an empty store of its own (the
session's store comes back afterwards), so a stream handle that torch's stream pool hands out a second time cannot carry entries."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_gpu_ops import hip  # noqa: E402,F401  (`hip`: the module fixture of the op tests)

DEV = torch.device("cuda:0")
FIXED = {
    "gemm_grouped": lambda hip: hip._grouped_workspace(DEV),
    "attn_fwd": lambda hip: hip._attn_f32_workspace(DEV),
    "attn_fwd_split": lambda hip: hip._attn_workspace(DEV, 1),
}


@pytest.fixture
def store(hip, monkeypatch):
    monkeypatch.setattr(hip, "_workspaces", {})
    monkeypatch.setattr(hip, "_outgrown", [])
    yield hip._workspaces
    torch.cuda.synchronize()  # nothing of a test's workspaces is in flight when they are freed


def _entries(store, stream):
    return [k for k in store if k[2] == stream.cuda_stream]


@pytest.mark.parametrize("kind", sorted(FIXED))
def test_first_use_inside_a_capture_is_refused_and_allocates_nothing(hip, store, monkeypatch, kind):
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with monkeypatch.context() as m:
            m.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
            with pytest.raises(RuntimeError, match="outside a graph capture"):
                FIXED[kind](hip)
        assert _entries(store, s) == []
        ws = FIXED[kind](hip)  # the warm-up call
        assert _entries(store, s) == [(kind, str(DEV), s.cuda_stream)]
        with monkeypatch.context() as m:
            m.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
            assert FIXED[kind](hip).data_ptr() == ws.data_ptr()  # inside a capture the warmed-up stream gets its own block


def test_two_streams_get_two_workspaces_of_each_kind(hip, store):
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    assert s1.cuda_stream != s2.cuda_stream
    got = {}
    for s in (s1, s2):
        with torch.cuda.stream(s):
            got[s] = {kind: get(hip) for kind, get in FIXED.items()}
            assert all(got[s][kind].data_ptr() == get(hip).data_ptr() for kind, get in FIXED.items())  # never replaced
    ptrs = [ws.data_ptr() for d in got.values() for ws in d.values()]
    assert len(set(ptrs)) == 6 and len(store) == 6


def test_grouped_workspace_has_its_counter_block_zeroed(hip, store):
    nbytes = hip.lib.ldc_gemm_grouped_workspace_bytes()
    counters = 1 << 20  # LDC_GEMM_COUNTER_BYTES (csrc/common.h)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        junk = torch.full((nbytes // 4,), 1.0, device=DEV)  # the allocator hands this block to the workspace: not zero by luck
        ptr = junk.data_ptr()
        del junk
        ws = hip._grouped_workspace(DEV)
        assert ws.numel() * 4 == nbytes and nbytes > counters
        assert int(torch.count_nonzero(ws[: counters // 4].view(torch.int32))) == 0
    if ws.data_ptr() == ptr:  # the slabs behind the counters are not initialised
        assert float(ws[counters // 4]) == 1.0


def test_scoring_scratch_grows_and_keeps_the_smaller_block(hip, store):
    from ladcast_amd.evaluate.utils import ensemble_scores

    def run(C, H, W):
        g = torch.Generator().manual_seed(C)
        dec, ref, clim = torch.randn(4, C, H, W, generator=g), torch.randn(C, H, W, generator=g), torch.randn(C, H, W, generator=g)
        ensemble_scores(dec.cuda(), ref.cuda(), clim.cuda(), torch.ones(H).cuda(), 0)
        (ws,) = [v for k, v in store.items() if k[0] == "ensemble_scores"]
        return ws

    small_shape, large_shape = (2, 6, 8), (8, 24, 32)
    need = hip.lib.ldc_ensemble_scores_workspace_bytes
    assert 0 < need(*small_shape) < need(*large_shape)
    small = run(*small_shape)
    assert small.numel() * 4 >= need(*small_shape) and hip._outgrown == []
    large = run(*large_shape)
    assert large.numel() * 4 >= need(*large_shape) and large.data_ptr() != small.data_ptr()
    assert [t.data_ptr() for t in hip._outgrown] == [small.data_ptr()]  # a captured graph may still point at it
    assert run(*small_shape).data_ptr() == large.data_ptr() and len(hip._outgrown) == 1  # never shrinks
