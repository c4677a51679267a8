"""TEST INFRASTRUCTURE: what the GPU tests of the three coefficient-rate entry points share -- the upload of a host
array and output tensors between guard bytes.  Nothing here is imported by the product."""
import numpy as np

GUARD, GUARD_BYTES = 0xA5, 256


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(shape, dtype):
    """a device tensor of `shape` inside a buffer with 256 guard bytes before and behind it"""
    import torch
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    raw = torch.full((n + 2 * GUARD_BYTES,), GUARD, dtype=torch.uint8, device="cuda")
    return raw, raw[GUARD_BYTES:GUARD_BYTES + n].view(dtype).view(*shape)


def _guards_intact(raw):
    g = raw.cpu().numpy()
    return bool((g[:GUARD_BYTES] == GUARD).all() and (g[-GUARD_BYTES:] == GUARD).all())
