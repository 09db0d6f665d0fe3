"""Host-side helpers of the descriptor tables the kernels read: 64-bit offsets and addresses as two int32 words (the
kernels join them again: bbd_join64 of csrc/bbd_ragged_math.h), and the upload of a table that never blocks the caller."""
import numpy as np
import torch


def split64(v):
    """0 <= v < 2^63 -> (low word, high word), both in int32 range: the low word carries bit 31 as its sign."""
    lo = v & 0xFFFFFFFF
    return (lo - (1 << 32) if lo >= (1 << 31) else lo), v >> 32


def join64(lo, hi):
    return (lo & 0xFFFFFFFF) | (hi << 32)


def upload(table, device):
    """Host array or tensor -> device tensor without blocking the calling thread on the stream (pinned staging +
    asynchronous copy; the caching host allocator keeps the staging block until the copy has run).  The loader's producer
    thread plans and launches batches ahead of the training step: a pageable copy would make it wait for its stream -
    which shares the GPU with a replaying step graph - three times per batch."""
    t = table if torch.is_tensor(table) else torch.from_numpy(np.ascontiguousarray(table))
    if torch.device(device).type != "cuda":
        return t.to(device)
    return t.pin_memory().to(device, non_blocking=True)
