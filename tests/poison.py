"""Poisoned allocations: every torch.empty of a test is filled with a known byte pattern before the caller sees it.

The library's workspace, the buffers its setters pack into and every output tensor come from torch.empty
(solver.py).  The caching allocator usually hands a fresh handle the block the previous one freed -- the same layout, the
right stale values -- so a read of memory the library never wrote passes every "same call on a fresh handle" comparison.
Under poisoned(pattern) such a read sees the pattern instead, and a result that depends on it differs between patterns.

A plain module (pytest does not collect it).  Nothing in the product changes: solver.py calls torch.empty through the
module attribute, which the context manager replaces and restores."""
import contextlib

import torch

# The three patterns, and no others.  What a word read before it is written sees:
#   ZERO   every byte 0x00: int32 0, double +0.0
#   MINUS  every byte 0xFF: int32 -1, double a NaN
#   ONE    every int32 1:   double 0x0000000100000001, a denormal that is neither zero nor not finite
# An int the code uses as an index stays at -1, 0 or 1, inside the handle's own arrays for B >= 2, Bp >= 4: a byte pattern
# such as 0x7F or 0xA5, or the stale bytes of another solve, would turn it into a wild address.
ZERO, MINUS, ONE = "ZERO", "MINUS", "ONE"
PATTERNS = (ZERO, MINUS, ONE)
_WORD = {ZERO: (0x00, 0x00, 0x00, 0x00), MINUS: (0xFF, 0xFF, 0xFF, 0xFF), ONE: (0x01, 0x00, 0x00, 0x00)}  # little endian


def fill(t, pattern):
    """Fill tensor t (contiguous, as torch.empty returns it) with `pattern` through its raw bytes, in place.  The pattern
    repeats every four bytes from the tensor's first byte; a tail shorter than a word takes the word's first bytes."""
    word = _WORD[pattern]
    if t.numel() == 0:
        return t
    raw = t.view(torch.uint8).reshape(-1) if t.dim() else t.reshape(1).view(torch.uint8)
    if word[0] == word[1] == word[2] == word[3]:
        raw.fill_(word[0])
    else:
        raw.zero_()
        raw[0::4] = word[0]
    return t


@contextlib.contextmanager
def poisoned(pattern, fill_cpu=False):
    """For the duration, torch.empty returns tensors filled with `pattern` (fill): those on a CUDA device always, those on
    the CPU only with fill_cpu=True (which exists so that the helper can be tested without a GPU).  torch.empty is the
    original object again on exit, after an exception too."""
    if pattern not in _WORD:
        raise ValueError("pattern must be one of %s" % (PATTERNS,))
    original = torch.empty

    def empty(*args, **kwargs):
        t = original(*args, **kwargs)
        if t.is_cuda or fill_cpu:
            fill(t, pattern)
        return t

    torch.empty = empty
    try:
        yield
    finally:
        torch.empty = original
