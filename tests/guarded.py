"""Output buffers with guard zones for the GPU tests of the engine's entry points: every output lies between
two zones of GUARD sentinel words, and after the call the zones must be intact and the output fully written."""

import numpy as np

SENTINEL = -7.25e300
GUARD = 512


def run(call, sizes):
    """``call(*outputs)`` with one flat float64 output of ``sizes[k]`` words each -> the outputs' bits (uint64)."""
    import torch
    buffers = [torch.full((GUARD + size + GUARD,), SENTINEL, dtype=torch.float64, device="cuda") for size in sizes]
    call(*[buf[GUARD:GUARD + size] for buf, size in zip(buffers, sizes)])
    torch.cuda.synchronize()
    outs = []
    for buf, size in zip(buffers, sizes):
        host = buf.cpu().numpy()
        assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + size:] == SENTINEL).all(), "guard zone written"
        assert not (host[GUARD:GUARD + size] == SENTINEL).any(), "output left unwritten"
        outs.append(host[GUARD:GUARD + size].view(np.uint64).copy())
    return outs
