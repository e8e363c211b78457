"""The one call path from torch tensors into the engine library: device pointers, the stream, and ``call``, which every
launching entry point of include/mgn_hip.h goes through (``_capi`` itself stays importable without torch)."""
from __future__ import annotations

from typing import Optional

import torch

from . import _capi


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream(dev: torch.device) -> int:
    """the hipStream_t of torch's current stream on ``dev`` (what every launch of the engine is queued on).  The raw query is one C call;
    building a ``torch.cuda.Stream`` object for it costs ~5 us, 60-90 times per training step"""
    if _raw_stream is not None:
        idx = dev.index
        return _raw_stream(torch.cuda.current_device() if idx is None else idx)
    return torch.cuda.current_stream(dev).cuda_stream


def stream_object(dev: torch.device) -> torch.cuda.Stream:
    """torch's current stream on ``dev`` as an object: for events and ``wait_stream``, never for a launch (see :func:`stream`)"""
    return torch.cuda.current_stream(dev)


def call(name: str, dev: torch.device, *args, accept=()) -> int:
    """``lib().<name>(*args, stream of dev)`` with ``dev`` current (the stream is the last argument of every launching entry point).  A return code other than 0 and those in ``accept`` (codes the
    caller maps to an exception of its own) raises with the message of the translation unit that defines ``name``."""
    with torch.cuda.device(dev):
        rc = getattr(_capi.lib(), name)(*args, stream(dev))
    if rc != 0 and rc not in accept:
        _capi.check(rc, name)
    return rc


def workspace(nbytes: int, dev: torch.device) -> torch.Tensor:
    """device scratch of at least ``nbytes`` bytes (never an empty tensor: its data pointer would be null)"""
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
