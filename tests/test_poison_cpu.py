"""tests/poison.py on the host: the patterns read back as the table in its FILLS claims, the fences notice a byte, the
allocation patch fills, counts and is undone, and a control shows that the method can tell a read-before-write from a
write-before-read."""
import numpy as np
import pytest
import torch

from tests import poison as P

DTYPES = [torch.uint8, torch.int16, torch.int32, torch.int64, torch.float16, torch.float32, torch.float64]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("name", list(P.FILLS))
def test_every_pattern_reads_back_as_claimed(name, dtype):
    pat = P.FILLS[name]
    t = P.fill(torch.zeros((3, 5), dtype=dtype) + 1, pat)
    a = t.numpy()
    assert (a.view(np.uint8) == pat).all()
    strided = torch.ones((4, 6), dtype=dtype)
    P.fill(strided[:, ::2], pat)                                  # a strided view: only its own elements change
    s = strided.numpy()
    assert (s[:, ::2].copy().view(np.uint8) == pat).all() and (s[:, 1::2] == 1).all()
    n = P.fill(np.ones((2, 7), a.dtype), pat)
    assert (n.view(np.uint8) == pat).all()
    is_float = dtype.is_floating_point
    if name == "zeros_00":
        assert (a == 0).all()
    elif name == "ones_ff":
        if is_float:
            assert np.isnan(a).all()                              # NaN in every float format
        elif dtype == torch.uint8:
            assert (a == 0xFF).all()
        else:
            assert (a == -1).all()                                # -1: the int tables' "none"; as u16 / u64 0xFFFF / ~0ull
            assert (a.view("u%d" % a.dtype.itemsize) == np.iinfo("u%d" % a.dtype.itemsize).max).all()
    elif name == "nophase_ee":
        if is_float:
            assert np.isfinite(a).all() and (a < 0).all()         # NaN-free
        if dtype == torch.float32:
            assert a.view(np.uint32)[0, 0] == 0xEEEEEEEE
    else:
        if dtype == torch.float32:
            assert a.view(np.uint32)[0, 0] == 0x3C3C3C3C and abs(float(a[0, 0]) - 0.0115) < 1e-4     # a plausible finite value
        if is_float:
            assert np.isfinite(a).all() and (a > 0).all() and (a < 2).all()
        if dtype == torch.int16:
            assert (a == 15420).all()                             # > any K
        if dtype == torch.int32:
            assert (a == 0x3C3C3C3C).all() and a[0, 0] > 1 << 29  # a large positive
        if dtype == torch.int64:
            assert (a > 1 << 61).all()


def test_fences_notice_one_byte_on_either_side():
    g = P.guarded(1000, 0x3C)
    assert g.buf.numel() == 1000 and g.tail == 4096 and bool((g.buf == 0x3C).all())
    g.buf.fill_(7)                                                # the whole stated size may be written
    g.assert_tail_intact()
    assert g.tail_intact()
    g.whole[1000] = 0
    assert not g.tail_intact()
    with pytest.raises(AssertionError, match="1 fence byte"):
        g.assert_tail_intact("ws")
    out, og = P.fenced((3, 5), torch.float32, 0xFF)
    assert out.shape == (3, 5) and out.dtype == torch.float32 and bool(torch.isnan(out).all())
    out.zero_()
    og.assert_tail_intact()
    og.whole[og.head - 1] = 0                                     # one byte in front of the output
    with pytest.raises(AssertionError):
        og.assert_tail_intact()
    assert P.guarded(0, 0x00).buf.numel() == 0
    assert P.guarded(16, 0xEE).view(torch.float64).shape == (2,)
    assert P.SENTINEL not in P.FILLS.values()


def test_patch_fills_counts_and_is_undone(monkeypatch):
    before = (torch.empty, torch.empty_like, np.empty, np.empty_like)
    with P.poisoned_alloc(monkeypatch, 0x3C) as served:
        assert torch.empty is not before[0] and np.empty is not before[2]
        a = torch.empty((4, 3), dtype=torch.float32)
        b = torch.empty_like(a, dtype=torch.int16)
        c = torch.empty(5, dtype=torch.int32)
        d = np.empty((2, 2), np.float64)
        e = np.empty_like(d)
        o = np.empty((2,), dtype=object)                          # pointers: left alone, not counted
        assert (a.view(torch.int32) == 0x3C3C3C3C).all() and (b == 15420).all() and (c == 0x3C3C3C3C).all()
        assert (d.view(np.uint8) == 0x3C).all() and (e.view(np.uint8) == 0x3C).all() and o[0] is None
        assert served.by_dtype == {"torch.float32": 1, "torch.int16": 1, "torch.int32": 1, "float64": 2}
        assert served.total == 5 and served.by_module == {__name__: 5} and served.from_modules("tests.") == 5
        assert served.from_modules("qpgesture_amd") == 0
    assert (torch.empty, torch.empty_like, np.empty, np.empty_like) == before
    with P.poisoned_alloc(monkeypatch, 0xFF) as again:            # a second context starts from zero
        assert bool(torch.isnan(torch.empty(3)).all())
        assert again.total == 1
    assert torch.empty is before[0]


def test_patch_is_undone_when_the_body_raises(monkeypatch):
    before = torch.empty
    with pytest.raises(ZeroDivisionError):
        with P.poisoned_alloc(monkeypatch, 0xEE):
            1 / 0
    assert torch.empty is before


def test_control_a_read_before_write_shows_and_a_write_before_read_does_not(monkeypatch):
    """The method's own check: an "op" that sums scratch it never wrote differs between two patterns; one that writes its
    scratch first gives the same bits under every pattern."""
    x = torch.arange(16, dtype=torch.float32)

    def leaky(x):
        acc = torch.empty(4)                                      # never written: the bug this PR's tests look for
        return acc + x.view(4, 4).sum(1)

    def sound(x):
        acc = torch.empty(4)
        acc[:] = 0
        return acc + x.view(4, 4).sum(1)

    def np_leaky(a):
        return np.empty(3, np.float64) + a

    got = {}
    for name, pat in P.FILLS.items():
        with P.poisoned_alloc(monkeypatch, pat) as served:
            got[name] = (leaky(x).numpy().view(np.uint32).copy(), sound(x).numpy().view(np.uint32).copy(),
                         np_leaky(np.zeros(3)).view(np.uint64).copy())
            assert served.total == 3
    base = got["zeros_00"]
    for name in ("ones_ff", "nophase_ee", "plausible_3c"):
        assert not np.array_equal(got[name][0], base[0]), name
        assert not np.array_equal(got[name][2], base[2]), name
        assert np.array_equal(got[name][1], base[1]), name
    assert not np.array_equal(got["ones_ff"][0], got["plausible_3c"][0])
