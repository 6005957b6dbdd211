"""The one hipGraph capture-and-replay routine of the package: every captured graph (a model forward, a sampler chunk, the pipeline
loop, a DC-AE encode / decode) is made by `capture` and replayed through the entry it returns."""
from __future__ import annotations

from typing import Any, Callable, List, NamedTuple, Optional

import torch

from . import hip


class CapturedGraph(NamedTuple):
    graph: torch.cuda.CUDAGraph
    inputs: List[torch.Tensor]  # the static copies the graph reads
    out: torch.Tensor  # the static tensor the graph writes
    stream: torch.cuda.Stream  # the capture stream: its workspaces are the ones the graph points into
    keep: Any  # whatever else the graph reads (device tables made for it), alive as long as the entry

    def replay(self, *inputs):
        """copy `inputs` into the static ones, replay, return a fresh tensor"""
        for a, b in zip(self.inputs, inputs):
            a.copy_(b)
        self.graph.replay()
        return self.out.clone()


def capture(fn: Callable[..., torch.Tensor], inputs, device, stream, reset: Optional[Callable[[], None]] = None, keep=None) -> CapturedGraph:
    """Capture `fn(*static copies of inputs) -> tensor` (kernel launches only, on the current stream) on `stream`.

    The warm-up runs on the capture stream, so the per-stream workspaces (hip.py) are created and initialised there and no allocation
    or memset ends up inside the graph.  After it, with nothing in flight: `reset()` (host state the warm-up advanced and the capture
    must see as new, e.g. a scheduler's step index), then the ticket counters of the balanced fp32 attention are zeroed, which is what
    makes a re-capture safe after an aborted launch.  `capture_error_mode="thread_local"`: other threads (the RCCL watchdog) may touch
    the runtime meanwhile."""
    static = [torch.empty_like(t) for t in inputs]
    for a, b in zip(static, inputs):
        a.copy_(b)
    stream.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(stream):
        fn(*static)
    torch.cuda.synchronize()
    if reset is not None:
        reset()
    hip.rearm_attention_workspaces(device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
        out = fn(*static)
    return CapturedGraph(graph, static, out, stream, keep)
