"""GPU parity: region growing and the write of its result in one native call (ivx_dev_flood_grow_select in csrc/k_flood.hip,
taken by DeviceVolume.region_grow) and the flood's look-ahead 0 .. 3.  Every case runs the new call on one DeviceVolume and the
two calls (ivx_dev_flood_grow, then _apply_reached's kernel) on a second one of the same input, and holds both, bit for bit,
against numpy / scipy.ndimage.label: the seeds' components of (t0 <= img <= t1) & (out != fill), out[reached] = fill,
mask[reached] = select.  Compared: download_mask(), download_out_mask(), reached_count() and the returned round count."""
import functools

import numpy as np
import pytest
from scipy.ndimage import generate_binary_structure, label

pytestmark = pytest.mark.gpu
LO, HI = 750, 3071  # (8 % of the noise is in range: below the 26-neighbour percolation threshold, many components)
SHAPES = [(16, 16, 64), (32, 32, 128), (40, 24, 192)]  # one tile; 2 x 2 x 2 tiles; partial tiles in y and z (tiles 64 x 16 x 16)
CONNS = [1, 2, 3]  # 6, 18, 26 neighbours
RING, ESCAPE = 16, 48  # entries of the counter ring (2 * BATCH); rounds after which the union-find engine takes over


def _strct(conn):
    return generate_binary_structure(3, conn).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _image(shape):
    """noise with many small in-range components, three voxel-wide lines through the volume that meet in one voxel (a region
    over every tile along each axis), and a solid block apart from them"""
    dz, dy, dx = shape
    img = np.random.default_rng(dz * dx).integers(-900, 900, shape).astype(np.int16)
    img[dz // 2, 2:dy - 2, 45] = 1000
    img[2:dz - 2, dy // 2, 45] = 1000
    img[dz // 2, dy // 2, 2:dx - 2] = 1000
    img[1:5, 1:7, 8:40] = 1000
    img[0, 0, 0] = -1000
    img.setflags(write=False)
    return img


def _seeds(shape, kind):
    """(z, y, x) seeds: the lines' crossing; that, the block and two voxels of the noise; a voxel that is out of range"""
    dz, dy, dx = shape
    if kind == "one":
        return [(dz // 2, dy // 2, 45)]
    if kind == "several":
        inr = np.argwhere((_image(shape) >= LO) & (_image(shape) <= HI))
        return [(dz // 2, dy // 2, 45), (2, 3, 20), tuple(int(v) for v in inr[len(inr) // 3]), tuple(int(v) for v in inr[-1])]
    assert kind == "out_of_range"
    return [(0, 0, 0)]


def _corridor(ntiles):
    """a voxel-wide line along y through `ntiles` tiles in an empty volume: one round per tile, no all-candidate block"""
    img = np.full((16, 16 * ntiles, 64), -1000, np.int16)
    img[8, 2:16 * ntiles - 2, 32] = 1000
    return img, [(8, 2, 32)]


def _expect(img, mask, out, seeds, t0, t1, conn, fill, select):
    """floodfill_threshold(img, seeds, t0, t1, fill, strct, out) and mask[out == fill's new voxels] = select, on copies;
    -> (mask, out, voxels reached)"""
    inr = (img >= t0) & (img <= t1)
    lab, _ = label(inr & (out != fill), _strct(conn))
    ids = {int(lab[s]) for s in seeds if inr[s]} - {0}
    reached = np.isin(lab, sorted(ids)) if ids else np.zeros(img.shape, bool)
    mask, out = mask.copy(), out.copy()
    out[reached] = fill
    if select is not None:
        mask[reached] = select
    return mask, out, int(reached.sum())


def _xyz(seeds):
    return [tuple(int(v) for v in s[::-1]) for s in seeds]


class _Pair:
    """the same input on two volumes: `new` takes ivx_dev_flood_grow_select wherever DeviceVolume does and notes the kind of
    write it handed over (None = it kept the two calls), `old` always runs the two calls"""

    def __init__(self, img, look_ahead=-1):
        from invesalius3_amd.device import DeviceVolume
        self.new, self.old = DeviceVolume(img), DeviceVolume(img)
        self.old._select = False
        self.new.timer.only = set()  # (a recorded "mask_bytes" span keeps the two calls: its own test below)
        self.new._look_ahead = look_ahead
        self.kinds = []
        inner = self.new._flood_write

        def spy(fill, select_value):
            w = inner(fill, select_value)
            self.kinds.append(None if w is None else w.kind)
            return w
        self.new._flood_write = spy
        self.img = np.asarray(img)
        self.mask = np.zeros(self.img.shape, np.uint8)
        self.out = np.zeros(self.img.shape, np.uint8)

    def each(self, f):
        return f(self.new), f(self.old)

    def threshold(self, lo=LO, hi=HI, zero_out=True):
        if zero_out:
            self.each(lambda v: v.zero_out_mask())
            self.out[...] = 0
        self.each(lambda v: v.threshold(lo, hi))
        self.mask = np.where((self.img >= lo) & (self.img <= hi), 255, 0).astype(np.uint8)

    def grow(self, seeds, conn, t0=LO, t1=HI, fill=1, select=254):
        """-> rounds, after both volumes and the expectation have taken the growing (nothing is compared yet)"""
        r_new, r_old = self.each(lambda v: v.region_grow(_xyz(seeds), t0, t1, _strct(conn), fill=fill, select_value=select))
        assert r_new == r_old, (r_new, r_old)
        self.mask, self.out, self.count = _expect(self.img, self.mask, self.out, seeds, t0, t1, conn, fill, select)
        return r_new

    def check(self):
        for v in (self.new, self.old):
            assert v.reached_count() == self.count
            assert np.array_equal(v.download_mask(), self.mask)
            assert np.array_equal(v.download_out_mask(), self.out)

    def close(self):
        self.each(lambda v: v.close())


@pytest.fixture
def pair():
    made = []

    def make(img, look_ahead=-1):
        made.append(_Pair(img, look_ahead))
        return made[-1]
    yield make
    for p in made:
        p.close()


# ---- shapes x seeds x structures: the write of the bench step (every byte of the mask from the two planes) --------------------
@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("seeds", ["one", "several", "out_of_range"])
@pytest.mark.parametrize("shape", SHAPES)
def test_shapes_seeds_structures(ivxlib, pair, shape, seeds, conn):
    p = pair(_image(shape))
    p.threshold()
    rounds = p.grow(_seeds(shape, seeds), conn)
    assert p.kinds == [ivxlib.FLOOD_WRITE_MASK_FROM_PLANES]
    p.check()
    if seeds == "out_of_range":
        # nothing floods, and the write still gives the threshold's mask: 255 * inside, everywhere
        assert rounds == 0 and p.count == 0
        assert np.array_equal(p.mask, np.where((p.img >= LO) & (p.img <= HI), 255, 0))
    else:
        assert p.count > 0 and (p.mask == 255).any()


@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("shape", SHAPES)
def test_wholly_candidate_volume(ivxlib, pair, shape, conn):
    """every voxel in range: the coarse pass floods the tiles as units and the first round starts empty"""
    p = pair(np.full(shape, 1000, np.int16))
    p.threshold()
    rounds = p.grow([(shape[0] // 2, shape[1] // 2, 7)], conn)
    assert p.kinds == [ivxlib.FLOOD_WRITE_MASK_FROM_PLANES]
    assert rounds == 0 and p.count == int(np.prod(shape))
    p.check()
    assert (p.mask == 254).all()


# ---- the end after many rounds ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("look_ahead", [-1, 0, 1, 2, 3])
def test_corridor_wraps_the_counter_ring(ivxlib, pair, look_ahead):
    """24 tiles, a round each: past the ring's 16 entries and short of the escape, with every look-ahead the same rounds"""
    img, seeds = _corridor(24)
    p = pair(img, look_ahead)
    p.threshold()
    rounds = p.grow(seeds, 3)
    print("corridor rounds", look_ahead, rounds)
    assert RING < rounds < ESCAPE
    assert p.kinds == [ivxlib.FLOOD_WRITE_MASK_FROM_PLANES]
    p.check()
    assert p.count == 16 * 24 - 4


@pytest.mark.parametrize("look_ahead", [-1, 0, 3])
def test_corridor_past_the_escape(ivxlib, pair, look_ahead):
    """64 tiles: the union-find engine finishes the flood, and the write lands behind it"""
    img, seeds = _corridor(64)
    p = pair(img, look_ahead)
    p.threshold()
    rounds = p.grow(seeds, 3)
    print("escape rounds", look_ahead, rounds)
    assert rounds >= ESCAPE
    p.check()
    assert p.count == 16 * 64 - 4


@pytest.mark.parametrize("conn", [1, 3])
@pytest.mark.parametrize("look_ahead", [0, 1, 2, 3])
def test_look_ahead_on_two_tiles_each_way(ivxlib, pair, look_ahead, conn):
    shape = SHAPES[1]
    p = pair(_image(shape), look_ahead)
    q = pair(_image(shape), -1)
    for v in (p, q):
        v.threshold()
    assert p.grow(_seeds(shape, "several"), conn) == q.grow(_seeds(shape, "several"), conn)
    p.check()
    assert np.array_equal(p.new.download_mask(), q.new.download_mask())


# ---- every kind of write, and the cases that keep the two calls --------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES[1:])
def test_apply_levels_write(ivxlib, pair, shape):
    """a threshold that wrote the mask's bytes itself: the touched chunks alone are rewritten from the planes"""
    p = pair(_image(shape))
    p.each(lambda v: setattr(v, "_mask_defer", False))
    p.threshold()
    assert not p.new._mask_pending and p.new._mask_levels == (255, None)
    p.grow(_seeds(shape, "several"), 3)
    assert p.kinds == [ivxlib.FLOOD_WRITE_APPLY_LEVELS]
    p.check()
    assert p.new._mask_levels == (255, 254) and p.new._defer_pays


@pytest.mark.parametrize("pending", [False, True])
@pytest.mark.parametrize("shape", SHAPES[1:])
def test_plain_uint8_write(ivxlib, pair, shape, pending):
    """a mask the pipeline knows nothing of (uploaded bytes), or one whose bytes are due but may not come from the planes
    (IVX_APPLY_LEVELS=0's setting): mask[reached] = select blends into bytes that have to be there before the flood's write"""
    p = pair(_image(shape))
    if pending:
        p.each(lambda v: setattr(v, "_apply_levels", False))
        p.threshold()
        assert p.new._mask_pending
    else:
        p.threshold()
        custom = np.random.default_rng(5).integers(0, 250, shape).astype(np.uint8)
        p.each(lambda v: v.mask.upload(custom))
        p.mask = custom
        assert p.new._mask_levels is None
    p.grow(_seeds(shape, "several"), 3, select=253)
    assert p.kinds == [ivxlib.FLOOD_WRITE_APPLY_U8]
    p.check()
    assert p.new._mask_pending == p.old._mask_pending is False and p.new._defer_pays == p.old._defer_pays


@pytest.mark.parametrize("shape", SHAPES[1:])
def test_no_write(ivxlib, pair, shape):
    """select_value=None: the flood alone goes through the new call; the threshold's pending bytes are written afterwards"""
    p = pair(_image(shape))
    p.threshold()
    p.grow(_seeds(shape, "one"), 3, select=None)
    assert p.kinds == [ivxlib.FLOOD_WRITE_NONE]
    p.check()
    assert (p.mask != 254).all()


@pytest.mark.parametrize("shape", SHAPES[1:])
def test_select_below_the_iso_value(ivxlib, pair, oracle, shape):
    """select_value < 127: the write from the new call, then the inside plane is taken back where reached (a second kernel,
    queued from Python as before); the surface afterwards is the oracle's"""
    p = pair(_image(shape))
    p.threshold()
    p.grow(_seeds(shape, "several"), 3, select=100)
    assert p.kinds == [ivxlib.FLOOD_WRITE_MASK_FROM_PLANES]
    for v in (p.new, p.old):
        assert v._mbits_valid and v._mask_levels is None and v._mbits_range is None
    p.check()
    soup = oracle.marching_cubes(p.mask, (1.0, 1.0, 1.0), [127.0], 0, True, True, True, 0.0, 1)
    assert len(soup) > 0
    for v in (p.new, p.old):
        assert np.array_equal(v.marching_cubes(download=True), soup)


@pytest.mark.parametrize("shape", SHAPES[1:])
def test_click_with_its_own_thresholds(ivxlib, pair, shape):
    """thresholds wider than the mask's: a candidate pass of its own, reached voxels outside the inside plane"""
    p = pair(_image(shape))
    p.threshold()
    p.grow(_seeds(shape, "one"), 3, t0=LO - 250)
    assert p.kinds == [ivxlib.FLOOD_WRITE_MASK_FROM_PLANES]
    inr = (p.img >= LO) & (p.img <= HI)
    assert ((p.mask == 254) & ~inr).any() and ((p.mask == 255) & inr).any()
    p.check()
    for v in (p.new, p.old):
        assert v._mbits_valid and v._mbits_range is None  # (the plane has taken the reached voxels in)


@pytest.mark.parametrize("shape", SHAPES[1:])
def test_fill_values_and_the_barrier(ivxlib, pair, shape):
    """fill = 2 into a zero out_mask bars nothing (new call); a second growing into the out_mask the first has left is barred
    by its voxels and writes out_mask and mask in one kernel of its own: the two calls stay"""
    p = pair(_image(shape))
    p.threshold()
    p.grow(_seeds(shape, "one"), 3, fill=2)
    assert p.kinds == [ivxlib.FLOOD_WRITE_MASK_FROM_PLANES]
    p.check()  # (download_out_mask writes the deferred bytes: out_mask is no longer known to be zero)
    first = p.out == 2
    # from the block, with thresholds under which the noise connects it to the lines: they are barred
    unbarred = _expect(p.img, p.mask, np.zeros(shape, np.uint8), [(2, 3, 20)], LO - 250, HI, 3, 2, 253)[2]
    p.grow([(2, 3, 20)], 3, t0=LO - 250, fill=2, select=253)
    assert p.kinds[-1] is None
    assert 0 < p.count < unbarred and (p.mask[first] == 254).all() and (p.mask == 253).any()
    p.check()


def test_a_recorded_span_keeps_the_two_calls(ivxlib, pair):
    """while the timer records "mask_bytes" the write stays a call of its own inside that span"""
    shape = SHAPES[1]
    p = pair(_image(shape))
    p.new.timer.only = None
    p.threshold()
    p.grow(_seeds(shape, "one"), 3)
    assert p.kinds == [None]
    p.check()
    assert len(p.new.timer.collect()["mask_bytes"]) == 1
    p.new.timer.only = {"region_grow"}
    p.threshold()
    p.grow(_seeds(shape, "several"), 3)
    assert p.kinds[-1] == ivxlib.FLOOD_WRITE_MASK_FROM_PLANES
    p.check()
    assert "mask_bytes" not in p.new.timer.collect()


def test_unknown_write_is_refused_before_the_flood(ivxlib):
    import ctypes

    L, lib = ivxlib, ivxlib.lib()
    plan = L.FloodPlan(16, 16, 64, 1, 0)
    for w in (L.FloodWrite(kind=7), L.FloodWrite(kind=L.FLOOD_WRITE_APPLY_U8, mask=None)):
        with pytest.raises(TypeError, match="flood_grow_select"):
            L.check(lib.ivx_dev_flood_grow_select(ctypes.byref(plan), L.I16, None, 0.0, 1.0, None, 0, None, None, None, None,
                                                  ctypes.byref(w), -1, None), "flood_grow_select")


# ---- repeated steps -----------------------------------------------------------------------------------------------------------
def test_three_steps_without_a_sync(ivxlib, pair, oracle):
    """threshold, growing, marching cubes three times over with nothing waited for in between (the progress line's tag and
    the counter ring are reused from step to step), each step from another seed; compared after the third"""
    shape = SHAPES[2]
    dz, dy, dx = shape
    p = pair(_image(shape))
    p.threshold()
    p.each(lambda v: v.marching_cubes())  # (the first call sizes the triangle buffer and waits for its count: not a step)
    steps = [([(2, 3, 20)], 1), (_seeds(shape, "several"), 3), ([(dz // 2, dy // 2, 45)], 2)]
    for seeds, conn in steps:
        p.threshold()
        p.grow(seeds, conn)
        nt = p.each(lambda v: v.marching_cubes())
    # (the sizing call needed the first threshold's bytes at once, so the next threshold wrote its bytes itself; from then on
    # the growing's write takes them and the thresholds leave them to it)
    assert p.kinds == [ivxlib.FLOOD_WRITE_APPLY_LEVELS] + [ivxlib.FLOOD_WRITE_MASK_FROM_PLANES] * 2
    soup = oracle.marching_cubes(p.mask, (1.0, 1.0, 1.0), [127.0], 0, True, True, True, 0.0, 1)
    assert nt == (len(soup), len(soup))
    for v in (p.new, p.old):
        v.sync()
        assert np.array_equal(v._tris.download((len(soup), 3, 3), np.float32), soup)
    p.check()


# ---- the write the flood queues itself while its lists run out ------------------------------------------------------------------
EARLY_CODE = (
    "import numpy as np\n"
    "import test_gpu_flood_select as t\n"
    "from invesalius3_amd import _lib\n"
    "shape = t.SHAPES[2]\n"
    "for early in (True, False):\n"
    "    p = t._Pair(t._image(shape) if early else t._corridor(24)[0])\n"
    "    p.threshold()\n"
    "    p.grow(t._seeds(shape, 'several') if early else t._corridor(24)[1], 3)\n"
    "    assert p.kinds == [_lib.FLOOD_WRITE_MASK_FROM_PLANES]\n"
    "    p.check()\n"
    "    p.close()\n"
    "    print('flood-done', flush=True)\n"
    "print('child-ok')\n")


@pytest.mark.parametrize("switch", ["1", "0"])
def test_early_write_is_queued_and_switched_off(ivxlib, switch):
    """IVX_FLOOD_TRACE shows the launch that looks at the next list's length on the device: queued behind the first round seen
    with a short list in an 18-tile volume, queued once and turned away in the corridor (its lists never halve again);
    IVX_FLOOD_EARLY=0 queues none; the bits are the same either way"""
    import os
    import re
    import subprocess
    import sys

    tests = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", "import sys\nsys.path[:0] = [%r, %r]\n" % (os.path.dirname(tests), tests) + EARLY_CODE],
                       env=dict(os.environ, IVX_FLOOD_TRACE="1", IVX_FLOOD_EARLY=switch), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child-ok" in r.stdout, r.stdout + r.stderr
    queued = re.findall(r"ivx flood: write queued behind round (\d+)", r.stderr)
    went = re.findall(r"ivx flood: the write behind round (\d+) went ahead", r.stderr)
    print("early write: queued behind", queued, "seen going ahead behind", went)
    if switch == "0":
        assert not queued and not went
    else:
        # (only `new` of each pair takes the call that can queue it: at most two tries in each of its two floods)
        assert 1 <= len(queued) <= 2 * 2 and set(went) <= set(queued)
