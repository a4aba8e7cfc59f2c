"""Poisoned memory for the scratch contract ("Scratch contract"): the documented outputs of an entry point, and
of every host object built on it, are the same bits whatever the caller's scratch, workspace and not-yet-written output
memory held before the call.  The tests mostly hand the kernels fresh allocations, which are usually all zero; the helpers
here hand them something else.

FILLS           byte patterns, each with the reason it is in the list.
fill            byte-fills a tensor or array of any dtype, on the device or the host, strided or not.
guarded         a byte buffer of exactly n bytes between sentinel fences, with assert_tail_intact().
fenced          an output array of a shape and dtype between sentinel fences, pre-filled with a pattern.
poisoned_alloc  a context that makes every primitive the package uses to get uninitialised memory return pattern-filled
                memory instead, and counts what it served per dtype and per calling module.

The primitives (grep of qpgesture_amd/ for empty / empty_like / empty_strided / new_empty / resize_ / pin_memory):
    torch.empty                   device buffers, and host buffers (db_cache.py)
    torch.empty_like              device buffers
    torch.empty(...).pin_memory() every pinned buffer that is not born from torch.zeros: pin_memory() COPIES the pageable
                                  tensor, so a poisoned torch.empty gives a poisoned pinned buffer; torch.empty(...,
                                  pin_memory=True) passes through the same patch
    np.empty                      host arrays (code_knn.rank_rows' host path, data_processing, db_cache, synth)
No empty_strided, new_empty or resize_ in the package.  np.empty_like is patched as well, for whoever adds one.  Arrays of
dtype object (synth.py) hold pointers and are left alone, and not counted."""
import contextlib
import sys

import numpy as np

FILLS = {
    "zeros_00": 0x00,       # the baseline: what a fresh allocation usually holds
    "ones_ff": 0xFF,        # NaN as f16/f32/f64, -1 as ints, and the library's own "none" markers 0xFFFF / ~0ull: can hide as "absent"
    "nophase_ee": 0xEE,     # what test_gpu_nophase.py already uses; NaN-free as f32 (-3.69e28)
    "plausible_3c": 0x3C,   # f32 0x3C3C3C3C ~ 0.0115, a plausible finite value; i32 a large positive; i16 15420 > any K: gets silently used
}
SENTINEL = 0xA5             # the fences' byte: none of the FILLS
_INT_OF_SIZE = {1: "uint8", 2: "int16", 4: "int32", 8: "int64"}


def _replicated(pattern, size):
    """The signed integer of `size` bytes whose every byte is `pattern`."""
    return int.from_bytes(bytes([pattern]) * size, "little", signed=size > 1)


def fill(t, pattern):
    """Set every byte of the tensor / array t to `pattern`, in place; t is returned.  Works through a same-width integer
    view, so any stride and any float payload (NaNs included) come out exact."""
    assert 0 <= pattern <= 0xFF
    if isinstance(t, np.ndarray):
        if t.dtype == object:
            raise TypeError("an object array holds pointers")
        if t.dtype.itemsize in _INT_OF_SIZE:
            t.view(_INT_OF_SIZE[t.dtype.itemsize])[...] = _replicated(pattern, t.dtype.itemsize)
        else:                                                   # complex128, structured: contiguous arrays only
            t.reshape(-1).view(np.uint8)[...] = pattern
        return t
    import torch
    size = t.element_size()
    if size in _INT_OF_SIZE:
        t.view(getattr(torch, _INT_OF_SIZE[size])).fill_(_replicated(pattern, size))
    else:
        t.view(torch.uint8).fill_(pattern)
    return t


class Guarded:
    """`buf`: n_bytes bytes (u8 tensor) filled with `pattern`, between a `head`-byte and a `tail`-byte fence of SENTINEL.
    The fences are multiples of 256 bytes, so buf keeps the allocation's alignment."""

    def __init__(self, n_bytes, pattern, tail=4096, head=0, device="cpu"):
        import torch
        assert head % 256 == 0 and tail > 0 and n_bytes >= 0
        self.n_bytes, self.head, self.tail = int(n_bytes), head, tail
        self.whole = torch.empty((head + self.n_bytes + tail,), dtype=torch.uint8, device=device)
        self.whole.fill_(SENTINEL)
        self.buf = self.whole[head:head + self.n_bytes]
        fill(self.buf, pattern)

    def view(self, dtype, shape=None):
        v = self.buf.view(dtype)
        return v if shape is None else v.view(shape)

    def tail_intact(self):
        h, n = self.head, self.n_bytes
        return bool((self.whole[:h] == SENTINEL).all()) and bool((self.whole[h + n:] == SENTINEL).all())

    def assert_tail_intact(self, what=""):
        w = self.whole.cpu().numpy()
        bad = np.flatnonzero(np.r_[w[:self.head], w[self.head + self.n_bytes:]] != SENTINEL)
        assert bad.size == 0, "%s: %d fence byte(s) overwritten, the first at offset %d of head+tail (buffer of %d bytes)" % (
            what, bad.size, int(bad[0]), self.n_bytes)


def guarded(n_bytes, pattern, tail=4096, head=0, device="cpu"):
    return Guarded(n_bytes, pattern, tail=tail, head=head, device=device)


def fenced(shape, dtype, pattern, device="cpu", fence=256):
    """(array view of `shape` / `dtype` filled with `pattern`, its Guarded): an output with sentinels on both sides."""
    import torch
    shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    g = Guarded(n, pattern, tail=fence, head=fence, device=device)
    return g.view(dtype, shape), g


class Served:
    """What a poisoned_alloc context handed out: by_dtype[str(dtype)] and by_module[caller's __name__] count calls."""

    def __init__(self):
        self.by_dtype, self.by_module = {}, {}

    def note(self, dtype, module):
        self.by_dtype[str(dtype)] = self.by_dtype.get(str(dtype), 0) + 1
        self.by_module[module] = self.by_module.get(module, 0) + 1

    @property
    def total(self):
        return sum(self.by_dtype.values())

    def from_modules(self, *prefixes):
        return sum(n for m, n in self.by_module.items() if m.startswith(prefixes))


@contextlib.contextmanager
def poisoned_alloc(monkeypatch, pattern):
    """Inside the context torch.empty, torch.empty_like, np.empty and np.empty_like return memory whose every byte is
    `pattern` (device, host and - through pin_memory()'s copy - pinned).  Yields the Served counter.  The patch goes through
    pytest's monkeypatch and is undone on exit."""
    import torch
    served = Served()
    real = {"te": torch.empty, "tl": torch.empty_like, "ne": np.empty, "nl": np.empty_like}

    def _wrap(make):
        def alloc(*args, **kwargs):
            t = make(*args, **kwargs)
            if isinstance(t, np.ndarray) and t.dtype == object:
                return t
            fill(t, pattern)
            served.note(t.dtype, sys._getframe(1).f_globals.get("__name__", "?"))
            return t
        return alloc

    with monkeypatch.context() as m:
        m.setattr(torch, "empty", _wrap(real["te"]))
        m.setattr(torch, "empty_like", _wrap(real["tl"]))
        m.setattr(np, "empty", _wrap(real["ne"]))
        m.setattr(np, "empty_like", _wrap(real["nl"]))
        yield served
