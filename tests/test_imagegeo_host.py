"""CPU: the arithmetic of the gantry-tilt correction.  csrc/imagegeo_math.h -- the text k_imagegeo.hip runs --
is built with the host compiler (tests/imagegeo_host_emu.cpp) and its int16 output is held to live scipy.ndimage.shift and
to the reference's own FixGantryTilt (tests/golden/ref_imagetools.npz) under np.array_equal; flip and swap are pinned to the
reference's output the same way, through their numpy statements."""
import os
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest
from scipy.ndimage import shift

import _imagegeo_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """tests/imagegeo_host_emu.cpp: the header the kernel includes, built with the host compiler, contraction off"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("imagegeo_emu") / "emu")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-o", exe,
                    os.path.join(HERE, "imagegeo_host_emu.cpp")], check=True)

    def run(text):
        return subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()

    def slices(s, shifts_cvals):
        h, w = s.shape
        text = "S %d %d %d\n%s\n" % (h, w, len(shifts_cvals), " ".join(str(int(v)) for v in s.ravel()))
        text += "".join("%r %d\n" % (float(sh), int(cv)) for sh, cv in shifts_cvals)
        lines = run(text)
        assert len(lines) == len(shifts_cvals)
        return [np.array(line.split(), dtype=np.int64).astype(np.int16).reshape(h, w) for line in lines]

    def volume(vol, shifts):
        d, h, w = vol.shape
        text = "V %d %d %d\n%s\n%s\n" % (d, h, w, " ".join(repr(float(v)) for v in shifts), " ".join(str(int(v)) for v in vol.ravel()))
        lines = run(text)
        assert len(lines) == 2
        return np.array(lines[0].split(), dtype=np.int64).astype(np.int16).reshape(vol.shape), [int(v) for v in lines[1].split()]

    return types.SimpleNamespace(slices=slices, volume=volume)


def test_fixture_slice_equals_scipy_at_every_shift_and_both_clamps_fire(emu):
    s = C.fixture_slice()
    got = emu.slices(s, [(sh, -1234) for sh in C.SHIFTS])
    clamped_hi = clamped_lo = False
    for sh, g in zip(C.SHIFTS, got):
        want = shift(s, (sh, 0), cval=-1234)
        assert np.array_equal(g, want), sh
        # the spline overshoots next to the two saturated regions: the float value leaves int16 and the store clamps it
        clamped_hi |= bool((g == 32767).any()) and sh not in (-19.01, -25.0)
        clamped_lo |= bool((g == -32768).any())
    assert clamped_hi and clamped_lo
    assert np.array_equal(got[0], s)  # a shift of 0 returns the input bit for bit
    for g in got[-2:]:
        assert (g == -1234).all()  # -19.01 and -25 leave no source row inside a 20-row slice
    assert (got[-3][1:] == -1234).all() and not (got[-3][0] == -1234).all()  # -19.0: row 0 reads row 19, the rest is filled


@pytest.mark.parametrize("h", [2, 3, 4])
def test_heights_where_every_tap_mirrors(emu, h):
    """Not among the shifts: 0.5 at height 2.  There the spline is the straight line through the two samples and the value is
    an exact half integer wherever they differ by an odd number, so scipy's own 1e-11 of noise decides the rounding."""
    s = C.small_slice(h)
    shifts = (0.0, -0.37, 0.3, -1.0, 1.0, -1.5, 2.0, -3.0) + ((0.5,) if h > 2 else ())
    for sh, g in zip(shifts, emu.slices(s, [(sh, 99) for sh in shifts])):
        assert np.array_equal(g, shift(s, (sh, 0), cval=99)), (h, sh)


def test_an_axis_of_length_one(emu):
    """What live scipy does, pinned: a line of one sample is not prefiltered, every tap reads that sample, so a shift of 0
    returns the slice and any other shift leaves no source row inside: all cval."""
    s = C.small_slice(1, w=7)
    g0, g1, g2 = emu.slices(s, [(0.0, 5), (0.25, 5), (-1.0, 5)])
    assert np.array_equal(shift(s, (0.0, 0), cval=5), s) and np.array_equal(g0, s)
    for sh, g in ((0.25, g1), (-1.0, g2)):
        want = shift(s, (sh, 0), cval=5)
        assert (want == 5).all() and np.array_equal(g, want)


PHANTOMS = {"disc": C.disc_phantom, "slice0": C.slice0_min_phantom, "wave": lambda: C.disc_phantom((5, 64, 64), seed=13)}


@pytest.fixture(scope="module")
def reference_file(tmp_path_factory):
    """the reference's own output: made afresh from its checkout (INVESALIUS_REFERENCE) when there is one -- in a process of
    its own, the stand-in modules stay out of this one -- and the committed golden file otherwise"""
    ref = os.environ.get("INVESALIUS_REFERENCE")
    if ref and os.path.isdir(os.path.join(ref, "invesalius")):
        out = str(tmp_path_factory.mktemp("ref_imagetools") / "ref.npz")
        subprocess.run([sys.executable, os.path.join(HERE, "golden", "make_golden_ref_imagetools.py"), out], check=True,
                       stdout=subprocess.DEVNULL)
        with np.load(out) as z:
            return {k: z[k] for k in z.files}
    return C.golden()


def test_golden_file_holds_the_fixtures_and_equals_a_fresh_run(reference_file):
    g = C.golden()
    assert sorted(g) == sorted(reference_file)
    for k in g:
        assert np.array_equal(g[k], reference_file[k]), k
    for name, make in PHANTOMS.items():
        assert np.array_equal(g["tilt_in_" + name], make())
    assert tuple(g["tilts"]) == C.TILTS and tuple(g["tilt_spacing"]) == C.PHANTOM_SPACING


@pytest.mark.parametrize("name", sorted(PHANTOMS))
@pytest.mark.parametrize("tilt", C.TILTS)
def test_whole_tool_equals_the_reference_and_live_scipy(emu, reference_file, name, tilt):
    vol = PHANTOMS[name]()
    got, cvals = emu.volume(vol, C.tilt_shifts(vol.shape[0], C.PHANTOM_SPACING, tilt))
    assert np.array_equal(got, reference_file["tilt_out_%s_%g" % (name, tilt)])
    want = vol.copy()
    want_cvals = C.scipy_fix_gantry_tilt(want, C.PHANTOM_SPACING, tilt)
    assert np.array_equal(got, want) and cvals == want_cvals
    if tilt == 0.0:
        assert np.array_equal(got, vol)


def test_the_chain_of_fill_values_is_real():
    """on the disc the spline undershoots next to the edge, the fill value falls and the next slice is filled with it; on
    the second phantom the minimum sits in slice 0 alone, which the tool never shifts, and every slice gets it"""
    vol = C.disc_phantom()
    cvals = C.scipy_fix_gantry_tilt(vol, C.PHANTOM_SPACING, C.PHANTOM_TILT)
    assert cvals[:2] == [-1024, -1024] and cvals[2] < -1200
    assert all(b <= a for a, b in zip(cvals, cvals[1:])) and len(set(cvals)) >= 5
    assert any((vol[n] == cvals[n]).any() and cvals[n] < -1024 for n in range(2, len(cvals)))  # ... and is written
    vol = C.slice0_min_phantom()
    assert set(C.scipy_fix_gantry_tilt(vol, C.PHANTOM_SPACING, C.PHANTOM_TILT)) == {-2000}
    assert (vol[1:] == -2000).any()


def test_flip_and_swap_of_the_reference_are_their_numpy_statements():
    g = C.golden()
    m, v = g["geo_in"], g["geo_version_in"]
    rev = (np.s_[::-1], np.s_[:, ::-1], np.s_[:, :, ::-1])
    for axis in range(3):
        assert np.array_equal(g["flip_out_%d" % axis], m[rev[axis]]) and np.array_equal(g["flip_version_out_%d" % axis], v[rev[axis]])
    sx, sy, sz = g["geo_spacing"]
    spacing = {"21": (sy, sx, sz), "20": (sz, sy, sx), "10": (sx, sz, sy)}
    for key, sp in spacing.items():
        a, b = int(key[0]), int(key[1])
        want = np.array(m.swapaxes(a, b))
        assert np.array_equal(g["swap_out_" + key], want) and np.array_equal(g["swap_version_out_" + key], np.array(v.swapaxes(a, b)))
        assert tuple(g["swap_spacing_" + key]) == sp
        assert tuple(g["swap_mask_shape_" + key]) == tuple(s + 1 for s in want.shape)


def test_spacing_rule_of_the_package_equals_the_reference():
    from invesalius3_amd import slice_

    g = C.golden()
    sp = tuple(g["geo_spacing"])
    for key in ("21", "20", "10"):
        a, b = int(key[0]), int(key[1])
        assert slice_.swapped_spacing(sp, (a, b)) == tuple(g["swap_spacing_" + key]) == slice_.swapped_spacing(sp, (b, a))
    assert np.array_equal(slice_.gantry_tilt_shifts(12, C.PHANTOM_SPACING, 11.5), C.tilt_shifts(12, C.PHANTOM_SPACING, 11.5))
