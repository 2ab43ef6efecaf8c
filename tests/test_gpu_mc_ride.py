"""GPU parity: marching cubes' count in the launch of the flood's mask write (k_mc_count_write in csrc/k_mc.hip, queued by
ivx_dev_flood_grow_select_count, taken by DeviceVolume.region_grow when the surface call before it has armed the ride:
invesalius3_amd/mc_ride.py).  Every case runs on two DeviceVolumes of the same input, ride on and ride off.  Both are held bit
for bit against numpy / scipy.ndimage.label for the mask and the number of reached voxels, and the ride-on volume against the
ride-off one for the triangle soup and the triangle count.  The ride-on volume's book says whether a region growing counted
(`rides`) and whether the surface call behind it used that count (`taken`); both are asserted, so a case cannot pass by
quietly taking the old path.

Which launch of the write goes ahead (IVX_FLOOD_TRACE=1 on these inputs; every early try is the fused kernel too, and one that
finds work left returns without counting): on one tile the first early try, queued behind round 2; on (40, 24, 192) and on
the long rows a first try behind round 2 returns at once and the second, behind round 10 / 21, goes ahead; with the lower
threshold of the first test's second step both tries return (rounds 2 and 11 of 13) and the launch after the host has seen
the end counts, as on the corridor (one try, behind round 2 of 24, returns); a seed outside the range has no round and no try."""
import functools
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
from scipy.ndimage import generate_binary_structure, label

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI = 750, 3071  # (8 % of the noise is in range: many small components, a ragged surface)
# one tile; partial tiles in y and z; 60 chunks of 16 voxels: a tail shorter than one 1024-chunk stretch, workgroups without one
SHAPES = [(16, 16, 64), (40, 24, 192), (3, 5, 64)]
# without the padding the count's grid (23 * 39 * 16 cell words = 57 workgroups) is shorter than the write's 60 stretches: a second trip
LONG = (24, 40, 1024)


@functools.lru_cache(maxsize=None)
def _image(shape):
    """noise with many small in-range components, a line along y and one along x that cross, and a solid block"""
    dz, dy, dx = shape
    img = np.random.default_rng(dz * dx + dy).integers(-900, 900, shape).astype(np.int16)
    img[dz // 2, :, 45] = 1000
    img[dz // 2, dy // 2, 2:dx - 2] = 1000
    img[1:5, 1:7, 8:40] = 1000
    img[0, 0, 0] = -1000
    img.setflags(write=False)
    return img


def _seed(shape):
    return [(shape[0] // 2, shape[1] // 2, 45)]


def _corridor(ntiles):
    """a voxel-wide line along y through `ntiles` tiles in an empty volume: one round per tile, the list never halves"""
    img = np.full((16, 16 * ntiles, 64), -1000, np.int16)
    img[8, 2:16 * ntiles - 2, 32] = 1000
    return img, [(8, 2, 32)]


def _expect(img, lo, hi, seeds, t0, t1, conn, select):
    """threshold(lo, hi), then the seeds' components of t0 <= img <= t1 set to `select` -> (mask, voxels reached)"""
    mask = np.where((img >= lo) & (img <= hi), 255, 0).astype(np.uint8)
    inr = (img >= t0) & (img <= t1)
    lab, _ = label(inr, generate_binary_structure(3, conn))
    ids = {int(lab[s]) for s in seeds if inr[s]} - {0}
    reached = np.isin(lab, sorted(ids)) if ids else np.zeros(img.shape, bool)
    mask[reached] = select
    return mask, int(reached.sum())


class _Pair:
    def __init__(self, img):
        from invesalius3_amd.device import DeviceVolume
        from invesalius3_amd.mc_ride import RideBook
        self.img = np.asarray(img)
        self.on, self.off = DeviceVolume(img), DeviceVolume(img)
        assert self.on._ride.enabled
        self.off._ride = RideBook(False)
        for v in (self.on, self.off):
            v.timer.only = set()  # (a timer that brackets the count or the write keeps the separate kernels: its own case below)

    def each(self, f):
        return f(self.on), f(self.off)

    def grow(self, seeds, kind="planes", conn=3, select=254, lo=LO, hi=HI, t0=None, t1=None, rides=True):
        """zero out_mask, threshold, region growing on both; -> rounds.  kind: "planes" = the mask's bytes are still pending
        (MASK_FROM_PLANES), "levels" = written first (APPLY_LEVELS)"""
        t0, t1 = lo if t0 is None else t0, hi if t1 is None else t1
        self.each(lambda v: v.zero_out_mask())
        self.each(lambda v: v.threshold(lo, hi))
        if kind == "levels":
            self.each(lambda v: v._materialize_mask())
        assert self.on._mask_pending == (kind == "planes") and self.off._mask_pending == (kind == "planes")
        before = self.on._ride.rides
        xyz = [tuple(int(c) for c in s[::-1]) for s in seeds]
        strct = generate_binary_structure(3, conn).astype(np.uint8)
        r_on, r_off = self.each(lambda v: v.region_grow(xyz, t0, t1, strct, fill=1, select_value=select))
        assert r_on == r_off
        assert self.on._ride.rides - before == int(rides) and self.off._ride.rides == 0
        self.mask, self.count = _expect(self.img, lo, hi, seeds, t0, t1, conn, select)
        return r_on

    def surface(self, taken=True, **kw):
        """the surface call on both -> the soup; the ride-on volume's is the ride-off volume's, bit for bit"""
        before = self.on._ride.taken
        s_on, s_off = self.each(lambda v: v.marching_cubes(from_binary=True, download=True, **kw))
        assert self.on._ride.taken - before == int(taken) and self.off._ride.taken == 0
        assert s_on.shape == s_off.shape and s_on.dtype == np.float32 and np.array_equal(s_on, s_off)
        return s_on

    def check_mask(self):
        for v in (self.on, self.off):
            assert v.reached_count() == self.count
            assert np.array_equal(v.download_mask(), self.mask)

    def arm(self, **kw):
        """a first step: its surface call arms the ride for the next region growing"""
        self.grow(_seed(self.img.shape), rides=False)
        self.surface(taken=False, **kw)

    def close(self):
        self.each(lambda v: v.close())


@pytest.fixture
def pair():
    made = []

    def make(img):
        made.append(_Pair(img))
        return made[-1]
    yield make
    for p in made:
        p.close()


# ---- the ride itself: shapes, both kinds of write, both launches that can go ahead ------------------------------------------
@pytest.mark.parametrize("kind", ["planes", "levels"])
@pytest.mark.parametrize("shape", SHAPES)
def test_ride_gives_the_separate_kernels_results(ivxlib, pair, shape, kind):
    p = pair(_image(shape))
    p.arm()
    p.grow(_seed(shape), kind)
    soup = p.surface()
    p.check_mask()
    assert p.count > 0 and len(soup) > 0 and (p.mask == 254).any() and (p.mask == 255).any()
    # and once more: the surface call has armed again
    p.grow(_seed(shape), kind, lo=LO - 50)
    assert len(p.surface()) > 0
    p.check_mask()


@pytest.mark.parametrize("kind", ["planes", "levels"])
def test_write_longer_than_the_counts_grid(ivxlib, pair, kind):
    p = pair(_image(LONG))
    p.arm(fill_border_holes=False)
    p.grow(_seed(LONG), kind)
    assert len(p.surface(fill_border_holes=False)) > 0
    p.check_mask()


@pytest.mark.parametrize("kind", ["planes", "levels"])
def test_corridor_the_launch_after_the_end(ivxlib, pair, kind):
    img, seeds = _corridor(24)
    p = pair(img)
    p.grow(seeds, rides=False)
    p.surface(taken=False)
    rounds = p.grow(seeds, kind)
    print("corridor rounds", rounds)
    assert 16 < rounds < 48
    assert len(p.surface()) > 0
    p.check_mask()
    assert p.count == 16 * 24 - 4


def test_corridor_past_the_escape_does_not_count(ivxlib, pair):
    """64 tiles: the union-find engine finishes the flood; the write is queued as before and the surface call counts"""
    img, seeds = _corridor(64)
    p = pair(img)
    p.grow(seeds, rides=False)
    p.surface(taken=False)
    assert p.grow(seeds, rides=False) >= 48
    assert len(p.surface(taken=False)) > 0
    p.check_mask()


@pytest.mark.parametrize("kind", ["planes", "levels"])
def test_empty_region(ivxlib, pair, kind):
    """a seed outside the range: no round, the write goes ahead and the count is the threshold's surface"""
    shape = SHAPES[1]
    p = pair(_image(shape))
    p.arm()
    assert p.grow([(0, 0, 0)], kind) == 0
    assert len(p.surface()) > 0
    p.check_mask()
    assert p.count == 0 and not (p.mask == 254).any()


def test_three_steps_without_a_sync(ivxlib, pair):
    shape = SHAPES[1]
    p = pair(_image(shape))
    p.arm()
    counts = []
    for lo in (LO, LO - 50, LO + 40):
        p.grow(_seed(shape), lo=lo)
        before = p.on._ride.taken
        counts.append(p.each(lambda v: v.marching_cubes(from_binary=True)))
        assert p.on._ride.taken == before + 1
    assert all(a == b and a > 0 for a, b in counts) and len({a for a, _ in counts}) == 3
    p.each(lambda v: v.sync())
    n = counts[-1][0]
    s_on, s_off = p.each(lambda v: v._tris.download((n, 3, 3), np.float32))
    assert np.array_equal(s_on, s_off)
    p.check_mask()
    assert p.on._ride.rides == 3


# ---- every way the note dies, and every way the ride is refused: the ride-off result each time -------------------------------
def _ridden(pair, shape=SHAPES[1]):
    p = pair(_image(shape))
    p.arm()
    p.grow(_seed(shape))
    return p


def test_note_dies_with_another_threshold(ivxlib, pair):
    p = _ridden(pair)
    p.each(lambda v: v.threshold(LO + 100, HI))
    soup = p.surface(taken=False)
    assert len(soup) > 0
    for v in (p.on, p.off):
        assert np.array_equal(v.download_mask(), np.where((p.img >= LO + 100) & (p.img <= HI), 255, 0))


def test_note_dies_with_other_surface_parameters(ivxlib, pair):
    p = _ridden(pair)
    a = p.surface(taken=False, fill_border_holes=False)
    p.check_mask()
    # ... and that call armed its own piece
    p.grow(_seed(SHAPES[1]))
    b = p.surface(fill_border_holes=False)
    assert np.array_equal(a, b)
    p.check_mask()


def test_note_dies_with_the_indexed_surface(ivxlib, pair):
    p = _ridden(pair)
    (v_on, f_on), (v_off, f_off) = p.each(lambda v: v.marching_cubes_indexed(from_binary=True, download=True))
    assert np.array_equal(v_on, v_off) and np.array_equal(f_on, f_off) and len(f_on) > 0
    assert p.on._ride.note is None
    assert len(p.surface(taken=False)) > 0
    p.check_mask()


def test_note_dies_with_a_prefetch(ivxlib, pair):
    p = _ridden(pair)
    assert p.each(lambda v: v.surface_prefetch(from_binary=True)) == (True, True)
    assert p.on._ride.note is None
    assert len(p.surface(taken=False)) > 0
    p.check_mask()


def test_note_dies_with_a_mask_edit(ivxlib, pair):
    p = _ridden(pair)
    edited = p.mask.copy()
    edited[2:12, 3:15, 20:90] = 255
    edited[20:30, :, 100:140] = 0
    p.each(lambda v: v.mask.upload(edited))
    assert len(p.surface(taken=False)) > 0
    for v in (p.on, p.off):
        assert np.array_equal(v.download_mask(), edited)


def test_note_dies_with_a_recorded_count(ivxlib, pair):
    p = _ridden(pair)
    p.on.timer.only = {"mc_count"}
    assert len(p.surface(taken=False)) > 0
    assert len(p.on.timer.collect()["mc_count"]) == 1
    p.check_mask()
    # while the timer brackets the count (or the write), the region growing does not carry it either
    p.grow(_seed(SHAPES[1]), rides=False)
    p.surface(taken=False)
    p.on.timer.only = {"mask_bytes"}
    p.grow(_seed(SHAPES[1]), rides=False)
    p.surface(taken=False)
    p.check_mask()


def test_select_below_the_iso_value_does_not_ride(ivxlib, pair):
    """mask[reached] = 100 takes the region out of the inside plane: the plane is about to change"""
    shape = SHAPES[1]
    p = pair(_image(shape))
    p.arm()
    p.grow(_seed(shape), select=100, rides=False)
    assert len(p.surface(taken=False)) > 0
    p.check_mask()
    assert (p.mask == 100).any()


def test_click_with_its_own_thresholds_does_not_ride(ivxlib, pair):
    shape = SHAPES[1]
    p = pair(_image(shape))
    p.arm()
    p.grow(_seed(shape), t0=LO + 100, t1=HI, rides=False)
    assert len(p.surface(taken=False)) > 0
    p.check_mask()


def test_unused_ride_disarms_the_next_click(ivxlib, pair):
    p = _ridden(pair)
    p.check_mask()
    p.grow(_seed(SHAPES[1]), lo=LO - 50, rides=False)  # no surface call in between: this click does not ride
    p.grow(_seed(SHAPES[1]), lo=LO - 80, rides=False)  # ... nor the next
    assert len(p.surface(taken=False)) > 0             # (the first ride's note is for a plane that is gone)
    p.check_mask()
    p.grow(_seed(SHAPES[1]))                           # armed again
    p.surface()
    p.check_mask()
    assert p.on._ride.rides == 2 and p.on._ride.taken == 1


# ---- the switch ---------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import sys, zlib
import numpy as np
from scipy.ndimage import generate_binary_structure
from invesalius3_amd.device import DeviceVolume
shape, lo, hi = %r, %d, %d
dz, dy, dx = shape
img = np.random.default_rng(dz * dx + dy).integers(-900, 900, shape).astype(np.int16)
img[dz // 2, :, 45] = 1000
img[dz // 2, dy // 2, 2:dx - 2] = 1000
img[1:5, 1:7, 8:40] = 1000
img[0, 0, 0] = -1000
v = DeviceVolume(img)
v.timer.only = set()
out = []
for _ in range(2):
    v.zero_out_mask()
    v.threshold(lo, hi)
    v.region_grow([(45, dy // 2, dz // 2)], lo, hi, generate_binary_structure(3, 3).astype(np.uint8), fill=1, select_value=254)
    soup = v.marching_cubes(from_binary=True, download=True)
    out.append((len(soup), zlib.crc32(soup.tobytes()), zlib.crc32(v.download_mask().tobytes())))
print("RIDE", int(v._ride.enabled), v._ride.rides, v._ride.taken, *out[1])
v.close()
"""


def test_switch_off_in_a_process_of_its_own(ivxlib, pair):
    shape = SHAPES[1]
    env = dict(os.environ, IVX_MC_RIDE="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _CHILD % (shape, LO, HI)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RIDE")][-1].split()
    assert line[1:4] == ["0", "0", "0"]
    p = pair(_image(shape))
    p.arm()
    p.grow(_seed(shape))
    soup = p.surface()
    p.check_mask()
    assert [int(x) for x in line[4:]] == [len(soup), zlib.crc32(soup.tobytes()), zlib.crc32(p.mask.tobytes())]
