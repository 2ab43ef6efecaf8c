"""CPU: the host-only half of the resident-array registry, csrc/resident_ranges.h built for the host
(tests/resident_host_emu.cpp) -- extents of strided views against numpy's own byte bounds, containment, overlap refusal, the
pending-touch interval list, the lifecycle of a handle and partial-overlap writes -- and `resident.bind` without a device."""
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """run(commands) -> the answers, one per command, from a fresh registry"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    tmp = tmp_path_factory.mktemp("resident_emu")
    exe = str(tmp / "emu")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "resident_host_emu.cpp")], check=True)

    def run(commands):
        src = str(tmp / "commands.txt")
        with open(src, "w") as fh:
            fh.write("\n".join(commands) + "\n")
        out = subprocess.run([exe, src], check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(out) == len(commands)
        return out
    return run


def _bounds(a):
    """numpy's byte_bounds rule: every element's first byte lies in [lo, hi - itemsize]"""
    lo = hi = a.__array_interface__["data"][0]
    for n, s in zip(a.shape, a.strides):
        if s < 0:
            lo += (n - 1) * s
        else:
            hi += (n - 1) * s
    return lo, hi + a.itemsize


def _views(p):
    return {"whole": p, "interior": p[1:, 1:, 1:], "slab": p[2:4], "coronal": p[:, 3:4, :], "sagittal": p[:, :, 5:6],
            "reversed": p[::-1], "stepped": p[:, ::2], "transposed": p.transpose(2, 0, 1),
            "reversed_rows": p[:, ::-1, ::-1], "one_voxel": p[3:4, 4:5, 6:7]}


def _extent_cmd(a):
    return "extent %d %d %d %s %s" % (a.__array_interface__["data"][0], a.itemsize, a.ndim, " ".join(map(str, a.shape)),
                                      " ".join(map(str, a.strides)))


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.float64])
def test_extents_of_views_equal_numpys_byte_bounds(emu, dtype):
    parent = np.zeros((6, 9, 21), dtype)
    views = _views(parent)
    got = emu([_extent_cmd(v) for v in views.values()])
    plo, phi = _bounds(parent)
    for (name, v), line in zip(views.items(), got):
        lo, hi = _bounds(v)
        assert line == "ok %d %d" % (lo, hi), name
        assert plo <= lo < hi <= phi, name
        # the bounds are tight: the first and the last byte belong to elements of the view
        idx = np.indices(v.shape).reshape(v.ndim, -1)
        first = v.__array_interface__["data"][0] + (idx * np.array(v.strides)[:, None]).sum(0)
        assert first.min() == lo and first.max() + v.itemsize == hi, name


def test_empty_and_broadcast_views_have_no_extent(emu):
    parent = np.zeros((6, 9, 21), np.int16)
    empty = parent[3:3]
    broadcast = np.broadcast_to(parent[:1], parent.shape)
    assert broadcast.strides[0] == 0
    one_long = np.lib.stride_tricks.as_strided(parent[2, 4], (1, 1, 21), (0, 0, 2))  # zero strides on axes of length 1 repeat nothing
    got = emu([_extent_cmd(empty), _extent_cmd(broadcast), _extent_cmd(one_long),
               "extent 4096 2 3 1 9 21 0 42 2"])  # what download_strided2 hands on: a 2-D view behind an axis of length 1
    assert got[:2] == ["none", "none"]
    assert got[2] == "ok %d %d" % _bounds(parent[2, 4])
    assert got[3] == "ok 4096 %d" % (4096 + 8 * 42 + 21 * 2)


def test_containment_one_byte_short_and_one_byte_past_at_both_ends(emu):
    lo, hi = 1 << 20, (1 << 20) + 4096
    got = emu(["reg %d %d 0" % (lo, hi - lo),
               "find %d %d 0" % (lo, hi),          # the whole range
               "find %d %d 0" % (lo + 1, hi),      # one byte short at the front
               "find %d %d 0" % (lo, hi - 1),      # one byte short at the back
               "find %d %d 0" % (lo - 1, hi),      # one byte past the front
               "find %d %d 0" % (lo, hi + 1),      # one byte past the back
               "find %d %d 0" % (lo - 1, lo),      # the byte in front
               "find %d %d 0" % (hi, hi + 1),      # the byte behind
               "find %d %d 0" % (lo + 7, lo + 7),  # nothing
               "find %d %d 1" % (lo, hi),          # another device: not registered there
               "contains %d %d %d %d" % (lo, hi, lo, hi), "contains %d %d %d %d" % (lo, hi, lo - 1, hi),
               "contains %d %d %d %d" % (lo, hi, lo, hi + 1), "contains %d %d %d %d" % (lo, hi, hi - 1, hi)])
    assert got == ["ok 1", "1", "1", "1", "0", "0", "0", "0", "0", "0", "1", "0", "0", "1"]


def test_overlapping_registrations_are_refused(emu):
    got = emu(["reg 1000 100 0",
               "reg 1000 100 0",   # the same range
               "reg 1099 10 0",    # its last byte
               "reg 990 11 0",     # its first byte
               "reg 900 400 0",    # around it
               "reg 1040 10 1",    # inside it, for another device: one host range has one mirror
               "reg 1100 10 0",    # adjacent behind
               "reg 990 10 0",     # adjacent in front
               "reg 0 10 0", "reg 2000 0 0",  # null, empty
               "reg %d 32 0" % (2 ** 64 - 16),  # wraps around
               "count", "find 1000 1100 0", "find 1100 1110 0", "find 1095 1105 0"])
    assert got == ["ok 1", "einval", "einval", "einval", "einval", "einval", "ok 2", "ok 3", "einval", "einval", "einval",
                   "3", "1", "2", "0"]


def test_touch_intervals_merge_and_a_refresh_empties_the_list(emu):
    got = emu(["reg 4096 1000 0", "state 1", "pending 1",
               "touch 1 100 50", "state 1", "pending 1",
               "touch 1 300 10", "pending 1",
               "touch 1 150 20", "pending 1",     # adjacent behind the first: one interval
               "touch 1 90 10", "pending 1",      # adjacent in front of it
               "touch 1 160 145", "pending 1",    # overlaps the first and the second: they fuse
               "touch 1 120 5", "pending 1",      # inside: nothing changes
               "touch 1 0 0", "pending 1",        # nothing written
               "touch 1 999 1", "pending 1",      # the last byte
               "touch 1 999 2", "touch 1 1000 1", "touch 1 1001 0", "touch 1 5 18446744073709551615",  # leave the range
               "touch 1 1000 0",                  # the empty range at the end is inside
               "pending 1", "refresh 1", "pending 1", "state 1", "refresh 1",
               "touch 1 0 1000", "touch 1 10 10", "pending 1", "refresh 1"])
    assert got == ["ok 1", "valid", "-",
                   "ok", "stale", "100:150",
                   "ok", "100:150 300:310",
                   "ok", "100:170 300:310",
                   "ok", "90:170 300:310",
                   "ok", "90:310",
                   "ok", "90:310",
                   "ok", "90:310",
                   "ok", "90:310 999:1000",
                   "einval", "einval", "einval", "einval",
                   "ok",
                   "90:310 999:1000", "221", "-", "valid", "0",
                   "ok", "ok", "0:1000", "1000"]


def test_a_released_handle_is_dead_and_the_address_gets_a_new_generation(emu):
    got = emu(["reg 8192 64 0", "touch 1 0 8", "release 1", "count",
               "state 1", "touch 1 0 8", "pending 1", "stats 1", "release 1", "find 8192 8256 0",
               "reg 8192 64 0", "state 2", "pending 2", "find 8192 8256 0", "stats 2",
               "touch 1 0 8", "state 1", "release 7", "count"])
    assert got == ["ok 1", "ok", "ok", "0",
                   "released", "einval", "einval", "einval", "einval", "0",
                   "ok 2", "valid", "-", "2", "0 0 0 0 0 0 0 2",
                   "einval", "released", "einval", "1"]


def test_a_partly_overlapping_write_marks_exactly_the_overlap_stale(emu):
    got = emu(["reg 1000 100 0", "reg 1200 100 0", "reg 1400 100 1",
               "write 900 1000", "write 1100 1200",       # adjacent on either side: nothing overlaps
               "state 1", "state 2",
               "write 950 1010", "pending 1", "state 1", "state 2",   # the first ten bytes
               "write 1090 1210", "pending 1", "pending 2",            # the tail of one and the head of the next
               "write 1250 1260", "pending 2",                          # inside (a write from another device, say)
               "write 1350 1600", "pending 3",                          # around a registration of another device
               "stats 1", "stats 2", "stats 3",
               "refresh 1", "refresh 2", "state 1", "state 2", "state 3"])
    assert got == ["ok 1", "ok 2", "ok 3",
                   "0", "0", "valid", "valid",
                   "1", "0:10", "stale", "valid",
                   "2", "0:10 90:100", "0:10",
                   "1", "0:10 50:60",
                   "1", "0:100",
                   "0 0 0 0 0 0 2 1", "0 0 0 0 0 0 2 2", "0 0 0 0 0 0 1 3",
                   "20", "20", "valid", "valid", "stale"]


def test_bind_without_a_device_is_the_loud_runtime_error():
    from invesalius3_amd import _lib, resident
    _lib.lib()
    if _lib.device_count() > 0:  # (on a GPU box the same call simply works; tests/test_gpu_resident.py takes it from there)
        with resident.bind(np.zeros((4, 5, 6), np.int16)) as r:
            assert r.stats()["generation"] >= 1
        return
    with pytest.raises(RuntimeError, match="no HIP device visible and there is no CPU fallback"):
        resident.bind(np.zeros((4, 5, 6), np.int16))
    from invesalius3_amd import mask, slice_
    for fn in (slice_.bind_image, mask.bind_matrix):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(np.zeros((4, 5, 6), np.uint8))
    with pytest.raises(TypeError):
        resident.bind([1, 2, 3])


def test_python_byte_bounds_and_root_resolution():
    """resident._byte_bounds is the rule above; resident._root ends at the array that owns the allocation"""
    from invesalius3_amd import resident
    parent = np.zeros((6, 9, 21), np.int16)
    for name, v in _views(parent).items():
        assert resident._byte_bounds(v) == _bounds(v), name
        assert resident._root(v) is parent, name
    assert resident._byte_bounds(parent[3:3])[0] == resident._byte_bounds(parent[3:3])[1]
    assert resident._root(parent[1:][:, 2:][..., ::2]) is parent
    assert resident._root(parent) is parent
