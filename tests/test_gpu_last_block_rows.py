"""`skip_unread_rows`: the last single-stream block computes proj_mlp, the attention's queries and proj_out for the Nx pred rows only (the
output head reads nothing else); its QKV projection still covers all S rows.  Model level, on the smallest model the code accepts: head
dim 128, 2 heads, one dual block, TWO single blocks (so that one block keeps all rows and one drops them), R = 2 frames of the 15 x 30
grid: Nx = 900 pred rows (7 query tiles + 4 rows), Nc = 450, S = 1350.

Bounds of "switch on agrees with switch off": the per-forward figures the suite already states per mode - the fp32 ceiling of the tiny
forward (tests/precision_bands.py) and the stated per-forward tolerances of the two split modes (ladcast_amd/precision.py).  Both
settings see the same operands on the pred rows; only tile and unit counts of three launches differ."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from ladcast_amd.precision import tolerance  # noqa: E402
from tests.precision_bands import ceiling  # noqa: E402
from tests.synth import make_ar, rel_l2, synth_known, tiny_ar_config  # noqa: E402
from tests.test_gpu_model import to_hip  # noqa: E402

BAND = {"fp32": ceiling("tiny_forward"), "bf16x3": tolerance("bf16x3", "forward"), "bf16": tolerance("bf16", "forward")}


@pytest.fixture(scope="module")
def model():
    cfg = tiny_ar_config(heads=2, layers=1, single=2, refiner=1)
    return to_hip(make_ar(cfg), cfg)


@pytest.fixture(scope="module")
def args():
    x = torch.randn(2, 84, 2, 15, 30, generator=torch.Generator().manual_seed(3)).cuda()
    return x, torch.tensor([0.3]).cuda(), synth_known(2).cuda(), torch.tensor([2018010100]).cuda()


def _fwd(g, args, x=None):
    x0, t, known, stamp = args
    return g(x0 if x is None else x, t, known, time_elapsed=stamp).sample.clone()


def _restore(g):
    g.enable_hip_graph(False)
    g.skip_unread_rows = True
    g.set_gemm_precision("fp32")


@pytest.mark.parametrize("mode", ["fp32", "bf16x3", "bf16"])
def test_switch_on_agrees_with_switch_off_and_graph_equals_eager(model, args, mode):
    g = model
    assert type(g).skip_unread_rows is True  # ships on
    try:
        g.set_gemm_precision(mode)
        g.skip_unread_rows = False
        off = _fwd(g, args)
        g.skip_unread_rows = True
        on = _fwd(g, args)
        err = rel_l2(on, off)
        print(f"\nlast single block on the pred rows only, {mode}: rel-L2 against all rows {err:.3e} (band {BAND[mode]:.2e}), "
              f"bitwise equal: {torch.equal(on, off)}")
        assert torch.isfinite(on).all()
        assert err < BAND[mode]
        assert torch.equal(_fwd(g, args), on)  # deterministic: the rows the block leaves alone hold nothing a later forward reads
        g.enable_hip_graph(True)
        x2 = torch.randn(2, 84, 2, 15, 30, generator=torch.Generator().manual_seed(4)).cuda()
        graphed = [_fwd(g, args), _fwd(g, args, x2)]  # capture + replay, replay with another sample
        g.enable_hip_graph(False)
        assert torch.equal(graphed[0], on) and torch.equal(graphed[1], _fwd(g, args, x2))
    finally:
        _restore(g)


def test_flipping_the_switch_never_replays_a_stale_graph(model, args):
    g = model
    try:
        eager = {}
        for flag in (True, False):
            g.skip_unread_rows = flag
            eager[flag] = _fwd(g, args)
        g.enable_hip_graph(True)
        n0 = len(g._graphs)
        for i, flag in enumerate((True, False, True, False)):
            g.skip_unread_rows = flag
            assert torch.equal(_fwd(g, args), eager[flag]), (i, flag)
        assert len(g._graphs) == n0 + 2  # one graph per setting, each captured once
    finally:
        _restore(g)


def test_chunk_graphs_are_keyed_by_the_switch(model, args):
    """the whole-chunk graphs of both sampler loops bake the choice in as well"""
    from ladcast_amd.pipelines import AutoRegressive2DPipeline, ensemble_AR_sampler
    from ladcast_amd.schedulers import EDMDPMSolverMultistepScheduler

    g = model
    known, stamp = args[2][:1], args[3]
    pipe = AutoRegressive2DPipeline(g, EDMDPMSolverMultistepScheduler())
    try:
        for sampler in ("edm", "pipeline"):
            run = lambda: ensemble_AR_sampler(pipe, 2, 2, 3, known_latents=known, timestamps=stamp, sampler_type=sampler, device="cuda").clone()  # noqa: E731
            eager = {}
            for flag in (True, False):
                g.skip_unread_rows = flag
                eager[flag] = run()
            g.enable_hip_graph(True)
            for flag in (True, False, True):
                g.skip_unread_rows = flag
                assert torch.equal(run(), eager[flag]), (sampler, flag)
            g.enable_hip_graph(False)
    finally:
        _restore(g)


def test_foreign_processor_on_the_last_block_keeps_every_row(model, args):
    """a user-supplied attention processor on the last single block: that block computes all rows whatever the switch says"""
    from ladcast_amd.models import LaDCastAttnProcessor2_0
    from oracle.ar_model import LaDCastAttnProcessor as OracleProcessor

    g = model
    names = list(g.attn_processors)
    last = "single_transformer_blocks.1.attn.processor"
    assert last in names
    try:
        g.skip_unread_rows = True
        fused = _fwd(g, args)
        g.set_attn_processor({k: (OracleProcessor() if k == last else LaDCastAttnProcessor2_0()) for k in names})
        on = _fwd(g, args)
        g.skip_unread_rows = False
        off = _fwd(g, args)
        assert torch.equal(on, off)
        assert rel_l2(on, fused) < tolerance("fp32", "forward")  # the processor restates the fused attention (torch fp32 arithmetic)
    finally:
        g.set_attn_processor(LaDCastAttnProcessor2_0())
        _restore(g)
