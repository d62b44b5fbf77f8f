"""Side streams of the attention backward and the fused module: cached per device, switched
without ``torch.cuda.stream``'s lookups."""
from __future__ import annotations

import torch

__all__ = ["_side_stream", "_prep_event", "_on_stream"]

_SIDE = {}


def _side_stream(dev: torch.device, priority: int = -1) -> "torch.cuda.Stream":
    """Per-device compute stream of the backward (created once per priority; -1 = high)."""
    i = dev.index if dev.index is not None else torch.cuda.current_device()
    if (i, priority) not in _SIDE:
        _SIDE[(i, priority)] = torch.cuda.Stream(device=i, priority=priority)
    return _SIDE[(i, priority)]


_EV = {}


def _prep_event(dev) -> "torch.cuda.Event":
    """One reusable event per device for "δ is ready" (a stream wait captures the event's state at
    the call, so re-recording it next step is safe): no event creation per backward."""
    i = dev.index if dev.index is not None else torch.cuda.current_device()
    if i not in _EV:
        _EV[i] = torch.cuda.Event()
    return _EV[i]


class _on_stream:
    """``with _on_stream(s, cur):`` makes ``s`` current and restores ``cur`` (the caller's
    current stream, already looked up).  Same effect as ``torch.cuda.stream(s)`` on one device
    without its device-index and current-stream lookups: 0.9 vs 5.8 µs of host per switch on
    MI355X (``benchmarks/micro/stream_ctx.py``)."""
    __slots__ = ("s", "cur")

    def __init__(self, s, cur):
        self.s, self.cur = s, cur

    def __enter__(self):
        if self.s is not self.cur:
            torch.cuda.set_stream(self.s)
        return self.s

    def __exit__(self, *exc):
        if self.s is not self.cur:
            torch.cuda.set_stream(self.cur)
        return False
