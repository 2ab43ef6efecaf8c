"""GPU: the blocks64 snapshot kernels (csrc/k_maskhist.hip) in their device forms against the numpy restatement
(tests/_history_ref.py): header, pool and restored bytes with np.array_equal, at the sizes where the kernels can go wrong --
one block +- 1, one wave's 64 blocks +- 1, an odd tail, and a popcount scan past one 4096-word workgroup."""
import ctypes

import numpy as np
import pytest

import _history_ref as R

pytestmark = pytest.mark.gpu

GUARD = 0xAB
BIG = 64 * 64 * 4096 + 65
SMALL_NS = (1, 63, 64, 65, 4095, 4096, 4097, 274625)


def contents(n, seed):
    """name -> stream of n bytes"""
    rng = np.random.default_rng(seed)
    B = R.cdiv(n, 64)
    out = {"zeros": np.zeros(n, np.uint8), "ones255": np.full(n, 255, np.uint8), "sevens": np.full(n, 7, np.uint8)}
    out["all_literal"] = (np.arange(n) % 251).astype(np.uint8)
    alt = np.repeat((np.arange(B) % 5 + 1).astype(np.uint8), 64)[:n].copy()
    alt[(np.arange(n) // 64) % 2 == 1] = (np.arange(n) % 13).astype(np.uint8)[(np.arange(n) // 64) % 2 == 1]
    out["alternating"] = alt
    edge = np.full(n, 3, np.uint8)
    for blk, at in ((0, 63), (B // 2, 1), (B - 1, 63), (max(B - 2, 0), 1)):
        if 64 * blk + at < n:
            edge[64 * blk + at] = 9  # a block that differs only in its last byte / only in its second byte
    out["edges"] = edge
    if n % 64 >= 2:
        t = np.full(n, 5, np.uint8)
        t[-1] = 6
        out["literal_tail"] = t
    if n % 64 and n > 64:
        t = np.full(n, 5, np.uint8)
        t[(n // 64) * 64:] = 200
        out["uniform_tail"] = t
    vals = np.array([0, 1, 2, 253, 254, 255], np.uint8)
    lens = rng.integers(1, 700, n // 100 + 2)
    out["runs"] = np.repeat(vals[rng.integers(0, 6, lens.size)], lens)[:n].copy()
    if out["runs"].size < n:
        out["runs"] = np.resize(out["runs"], n)
    return out


class Dev:
    """a guarded range in device memory: `pre` guard bytes, n bytes, 80 guard bytes"""

    def __init__(self, L, x, pre):
        from invesalius3_amd.device import DeviceBuffer
        self.L, self.n, self.pre = L, x.size, pre
        self.buf = DeviceBuffer(pre + x.size + 80)
        self.buf.upload(np.concatenate([np.full(pre, GUARD, np.uint8), x, np.full(80, GUARD, np.uint8)]))

    @property
    def ptr(self):
        return self.buf.at(self.pre)

    def read(self):
        """(the n bytes, guards intact?)"""
        a = self.buf.download((self.pre + self.n + 80,), np.uint8)
        return a[self.pre:self.pre + self.n].copy(), bool((a[:self.pre] == GUARD).all() and (a[self.pre + self.n:] == GUARD).all())

    def close(self):
        self.buf.close()


def dev_encode(L, src_ptr, n):
    """-> (header buffer, pool buffer, literal blocks, header bytes, pool bytes) through the device forms"""
    from invesalius3_amd import history
    from invesalius3_amd.device import DeviceBuffer
    hb = history.header_bytes(n)
    header = DeviceBuffer(hb)
    nlit = L.c_i64(-1)
    L.check(L.lib().ivx_dev_mask_snapshot_scan(src_ptr, n, header.ptr, ctypes.byref(nlit), None), "scan")
    pool = DeviceBuffer(max(64 * nlit.value, 16) + 64)
    pool.upload(np.full(pool.nbytes, GUARD, np.uint8))
    L.check(L.lib().ivx_dev_mask_snapshot_pack(src_ptr, n, header.ptr, pool.ptr, nlit.value, None), "pack")
    L.synchronize()
    p = pool.download((pool.nbytes,), np.uint8)
    assert (p[64 * nlit.value:] == GUARD).all(), "the pack wrote past its %d blocks" % nlit.value
    return header, pool, nlit.value, header.download((hb,), np.uint8), p[:64 * nlit.value].copy()


def dev_restore(L, dst_ptr, n, header, pool, nlit, plane_bytes=None):
    from invesalius3_amd.device import DeviceBuffer
    flags = None
    if plane_bytes:
        np_ = R.cdiv(n, plane_bytes)
        flags = DeviceBuffer(np_ + 16)
        flags.upload(np.concatenate([np.zeros(np_, np.uint8), np.full(16, GUARD, np.uint8)]))
    L.check(L.lib().ivx_dev_mask_snapshot_restore(dst_ptr, n, header.ptr, pool.ptr, nlit, plane_bytes or 1, flags.ptr if flags else None, None),
            "restore")
    L.synchronize()
    if flags is None:
        return None
    f = flags.download((np_ + 16,), np.uint8)
    flags.close()
    assert (f[np_:] == GUARD).all(), "a flag was written past the last plane"
    return f[:np_].copy()


def check_stream(L, name, x, pre, old=None, plane_bytes=110):
    n = x.size
    want_h, want_p, want_l = R.encode(x)
    src = Dev(L, x, pre)
    header, pool, nlit, got_h, got_p = dev_encode(L, src.ptr, n)
    try:
        assert nlit == want_l, "%s n=%d pre=%d: %d literal blocks, the restatement has %d" % (name, n, pre, nlit, want_l)
        assert np.array_equal(got_h, want_h), "%s n=%d pre=%d: header" % (name, n, pre)
        assert np.array_equal(got_p, want_p), "%s n=%d pre=%d: pool" % (name, n, pre)
        kept, guards = src.read()
        assert guards and np.array_equal(kept, x)  # (the source is only read)
        old = np.full(n, 77, np.uint8) if old is None else old
        dst = Dev(L, old, pre)
        flags = dev_restore(L, dst.ptr, n, header, pool, nlit, plane_bytes)
        got, guards = dst.read()
        assert guards, "%s n=%d pre=%d: the restore wrote outside its range" % (name, n, pre)
        assert np.array_equal(got, x), "%s n=%d pre=%d: decode(encode(x)) != x" % (name, n, pre)
        assert np.array_equal(flags, R.changed_planes(old, x, plane_bytes)), "%s n=%d pre=%d: plane flags" % (name, n, pre)
        dst.close()
    finally:
        src.close()
        header.close()
        pool.close()


@pytest.mark.parametrize("n", SMALL_NS)
def test_encode_pack_restore_equal_the_restatement(ivxlib, n):
    for name, x in contents(n, n).items():
        for pre in (64, 3):  # an aligned sub-range of a larger buffer, and one that is not
            check_stream(ivxlib, name, x, pre)
        if name in ("zeros", "ones255", "sevens"):
            assert R.encode(x)[2] == 0
    lit = R.encode(contents(n, n)["all_literal"])[2]
    assert lit == (R.cdiv(n, 64) if n % 64 != 1 else n // 64)  # (a tail block of one byte equals its first byte)


def test_scan_past_one_workgroup_of_popcount_words(ivxlib):
    """64 * 64 * 4096 + 65 bytes: 4097 bitmap words, so the exclusive scan of the popcounts needs its second workgroup"""
    c = contents(BIG, 1)
    assert R.layout(BIG)[1] == 4097
    check_stream(ivxlib, "runs", c["runs"], 64, old=c["alternating"], plane_bytes=4096)
    check_stream(ivxlib, "all_literal", c["all_literal"], 3, old=c["runs"], plane_bytes=4096)
    check_stream(ivxlib, "sevens", c["sevens"], 64, old=c["sevens"], plane_bytes=4096)


@pytest.mark.parametrize("plane_bytes,n", ((110, 440), (110, 4097), (4096, 3 * 4096 + 5)))
def test_restore_flags_exactly_the_planes_that_differ(ivxlib, plane_bytes, n):
    L = ivxlib
    rng = np.random.default_rng(plane_bytes + n)
    old = np.repeat(rng.integers(0, 4, R.cdiv(n, 64)).astype(np.uint8), 64)[:n].copy()
    old[rng.integers(0, n, 20)] = 99
    b = plane_bytes  # the first plane boundary: a block (and, at 110, a 16-byte chunk) straddles it
    for pre in (64, 3):
        for where in ([b - 1], [b], [b - 1, b], [b - 2], [b + 1], [0], [n - 1], [b - 1, n - 1], []):
            new = old.copy()
            for at in where:
                new[at] ^= 0x55
            src = Dev(L, new, 0)
            header, pool, nlit, _, _ = dev_encode(L, src.ptr, n)
            dst = Dev(L, old, pre)
            flags = dev_restore(L, dst.ptr, n, header, pool, nlit, plane_bytes)
            got, guards = dst.read()
            assert guards and np.array_equal(got, new)
            assert np.nonzero(flags)[0].tolist() == sorted({at // plane_bytes for at in where}), (where, pre)
            # restoring onto identical bytes flags nothing, and without flags the restore still restores
            assert not dev_restore(L, dst.ptr, n, header, pool, nlit, plane_bytes).any()
            dst2 = Dev(L, old, pre)
            assert dev_restore(L, dst2.ptr, n, header, pool, nlit, None) is None
            got2, guards2 = dst2.read()
            assert guards2 and np.array_equal(got2, new)
            for o in (src, dst, dst2, header, pool):
                o.close()


def test_header_size_is_a_pure_function_of_n(ivxlib):
    from invesalius3_amd import history
    for n in SMALL_NS + (BIG,):
        assert history.header_bytes(n) == R.layout(n)[4]
