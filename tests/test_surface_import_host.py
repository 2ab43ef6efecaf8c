"""CPU: the surface import's host side (invesalius3_amd/surface.py) -- the parsers and writers, Merge, the affine --
against tests/_surface_import_ref.py, csrc/mesh_weld_math.h built for the host against its Python restatement, and the proof
that every weld case of tests/_surface_import_cases.py stands where it is said to.  No GPU."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import _surface_import_cases as C
import _surface_import_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
BINARY_T = (1, 2, 255, 256, 257)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """tests/mesh_weld_host_emu.cpp: the header the kernels include, built with the host compiler"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("weld_emu") / "emu")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "mesh_weld_host_emu.cpp")], check=True)

    def run(*args, stdin=b""):
        return subprocess.run([exe] + [str(a) for a in args], input=stdin, capture_output=True, check=True).stdout
    return run


@pytest.fixture()
def no_library(monkeypatch):
    """every use of libivx.so fails while this is on: what raises under it was raised before the library was touched"""
    from invesalius3_amd import _lib as L
    monkeypatch.setattr(L, "LIB_PATH", os.path.join(HERE, "no_such_dir", "libivx.so"))
    monkeypatch.setattr(L, "_lib", None)
    with pytest.raises(ImportError):
        L.lib()


def _cases():
    return {"cluster": C.cluster_case()[0], "wrap": C.wrap_case()[0], "zero": C.zero_sign_case(), "d4095": C.distinct_case(1365),
            "d4098": C.distinct_case(1366), "identical": C.identical_case(), "repeated": C.repeated_case(), "degenerate": C.degenerate_case(),
            "one": C.distinct_case(1)}


# ---- mesh_weld_math.h ---------------------------------------------------------------------------------------------------
def test_header_keys_and_hash_equal_the_restatement_on_every_case(emu):
    for name, soup in _cases().items():
        pts = np.ascontiguousarray(soup, np.float32).reshape(-1, 3)
        got = np.frombuffer(emu("k", len(pts), stdin=pts.tobytes()), np.uint32).reshape(-1, 4)
        keys = ref.keys_of(pts)
        want = np.array([k + (C.hash32(*k),) for k in keys], np.uint32)
        assert np.array_equal(got, want), name


def test_slot_counts_of_header_library_and_restatement_agree(emu):
    from invesalius3_amd import surface
    for n in (0, 1, 2, 3, 4, 5, 30, 32, 33, 2100, 4095, 4098, 2 ** 30, 2 ** 30 + 1, 2 ** 31 - 1):
        want = C.slots_for(n)
        assert int(emu("s", n)) == want == surface.weld_slots(n), n
        assert want >= 2 * n and (want & (want - 1)) == 0 and (want == 2 or want // 2 < 2 * n)
    assert int(emu("s", 2 ** 31)) == 0 and int(emu("s", -1)) == 0
    for n in (2 ** 31, -1):
        with pytest.raises(ValueError):
            surface.weld_slots(n)


def test_record_offsets_and_histogram_buckets(emu):
    for t in (0, 1, 2, 257):
        for k in (0, 4, 8):
            assert int(emu("o", t, k)) == 84 + 50 * t + 12 + 4 * k
    for p, b in ((0, 0), (1, 1), (2, 2), (3, 2), (4, 3), (7, 3), (8, 4), (16383, 14), (16384, 15), (2 ** 40, 15)):
        assert int(emu("b", p)) == b


# ---- the cases stand where they are said to (on the restatement alone) ----------------------------------------------------
def test_cluster_case_has_four_keys_on_one_home_slot():
    soup, slots = C.cluster_case()
    assert slots == C.slots_for(soup.size // 3) == 64
    assert max(len(keys) for keys in C.homes(soup, slots).values()) >= 4


def test_wrap_case_has_two_keys_on_the_last_slot():
    soup, slots = C.wrap_case()
    assert slots == C.slots_for(soup.size // 3)
    assert len(C.homes(soup, slots).get(slots - 1, ())) >= 2


def test_zero_sign_case_is_one_vertex_that_keeps_its_minus_zero():
    soup = C.zero_sign_case()
    flat = soup.reshape(-1, 3)
    assert np.signbit(flat[0, 0]) and not np.signbit(flat[3, 0]) and flat[0].tolist() == flat[3].tolist()
    v, f, c = ref.weld(soup)
    assert c == {"facets_read": 3, "vertices": 4, "facets": 3, "dropped": 0}
    assert np.signbit(v[0, 0]) and f[1, 0] == 0 and f[2, 1] == 0
    assert np.signbit(v[3, 1]) and f[2, 0] == 3  # (9, -0.0, 1) came before (9, 0.0, 1)


def test_scan_switch_cases_have_4095_and_4098_distinct_corners():
    for nt, n in ((1365, 4095), (1366, 4098)):
        soup = C.distinct_case(nt)
        assert soup.size // 3 == n and len(set(ref.keys_of(soup))) == n
        v, f, c = ref.weld(soup)
        assert c["vertices"] == n and c["dropped"] == 0 and np.array_equal(f.ravel(), np.arange(n))


def test_the_other_cases():
    v, f, c = ref.weld(C.identical_case())
    assert (c["vertices"], c["facets"], c["dropped"]) == (1, 0, 700)
    soup = C.repeated_case()
    flat, n = soup.reshape(-1, 3), soup.size // 3
    same = [j for j in range(n) if flat[j].tolist() == [-7.0, -7.0, -7.0]]
    assert same == [0, 63, 64, 255, 256, n - 1] and len(set(ref.keys_of(soup))) == n - 5
    v, f, c = ref.weld(C.degenerate_case())
    assert (c["vertices"], c["facets"], c["dropped"]) == (8, 4, 4) and v[0].tolist() == [5.0, 5.0, 5.0]
    assert 0 not in f  # the point only the dropped first facet used stays in the list, unused
    assert f.tolist() == [[1, 2, 3], [2, 3, 4], [4, 5, 6], [7, 6, 5]]


# ---- parsers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", BINARY_T)
def test_binary_stl(tmp_path, no_library, nt):
    from invesalius3_amd import surface
    soup = ref.soup_for(nt)
    path = tmp_path / "a.stl"
    path.write_bytes(ref.stl_binary_bytes(soup))
    got = surface.read_stl(path)
    assert got.dtype == np.float32 and ref.same_bits(got, soup)


def test_binary_stl_that_starts_with_solid_is_binary(tmp_path, no_library):
    from invesalius3_amd import surface
    soup = ref.soup_for(3)
    data = ref.stl_binary_bytes(soup, header=b"solid made by a writer that says solid")
    assert surface.stl_kind(data) == "binary"
    (tmp_path / "s.stl").write_bytes(data)
    assert ref.same_bits(surface.read_stl(tmp_path / "s.stl"), soup)


def test_ascii_stl_two_solids_exponents_crlf(tmp_path, no_library):
    from invesalius3_amd import surface
    (tmp_path / "a.stl").write_bytes(ref.ASCII_STL)
    assert surface.stl_kind(ref.ASCII_STL) == "ascii"
    got = surface.read_stl(tmp_path / "a.stl")
    assert ref.same_bits(got, ref.ASCII_STL_SOUP) and got[1, 2, 1] == 16777216.0 and np.signbit(got[1, 0, 1])


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian", "binary_big_endian"])
def test_ply_formats(tmp_path, no_library, fmt):
    from invesalius3_amd import surface
    (tmp_path / "a.ply").write_bytes(ref.ply_bytes(fmt))
    v, f = surface.read_ply(tmp_path / "a.ply")
    assert v.dtype == np.float32 and f.dtype == np.int32
    assert ref.same_bits(v, ref.PLY_EXPECT_VERTS) and np.array_equal(f, ref.PLY_FACES)


@pytest.mark.parametrize("order", ["<", ">"])
def test_binary_ply_of_triangles_alone_takes_the_one_read_path(tmp_path, no_library, order):
    """every face as long as the first: the reader takes the element in one structured read, and must return what the loop returns"""
    from invesalius3_amd import surface
    v, f, _ = ref.weld(ref.soup_for(300))
    fmt = "binary_little_endian" if order == "<" else "binary_big_endian"
    head = ("ply\nformat %s 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nelement face %d\n"
            "property list uchar uint vertex_index\nproperty uchar tag\nend_header\n" % (fmt, len(v), len(f))).encode()
    rec = np.zeros(len(f), np.dtype([("n", "u1"), ("i", order + "u4", (3,)), ("tag", "u1")]))
    rec["n"], rec["i"], rec["tag"] = 3, f, 9
    (tmp_path / "t.ply").write_bytes(head + v.astype(order + "f4").tobytes() + rec.tobytes())
    gv, gf = surface.read_ply(tmp_path / "t.ply")
    assert ref.same_bits(gv, v) and np.array_equal(gf, f)
    rec["n"][-1] = 2  # the last face is short: the counts disagree, the loop takes over and refuses it
    (tmp_path / "u.ply").write_bytes(head + v.astype(order + "f4").tobytes() + rec.tobytes()[:-5] + b"\x09")
    with pytest.raises(ValueError):
        surface.read_ply(tmp_path / "u.ply")


def test_every_file_error_is_raised_before_the_library_is_touched(tmp_path, no_library):
    from invesalius3_amd import surface
    good = ref.stl_binary_bytes(ref.soup_for(2))

    def stl(data):
        (tmp_path / "e.stl").write_bytes(data)
        return surface.read_stl(tmp_path / "e.stl")

    def ply(data):
        (tmp_path / "e.ply").write_bytes(data)
        return surface.read_ply(tmp_path / "e.ply")

    for bad in (good[:-1], good + b"\0", good[:100], b"", b"\0" * 83, b"facet normal 0 0 1\n"):  # truncated, trailing, neither
        with pytest.raises(ValueError):
            stl(bad)
    two = ref.ASCII_STL.replace(b"      vertex 1.5e0 0 0\r\n", b"")
    four = ref.ASCII_STL.replace(b"      vertex 1.5e0 0 0\r\n", b"      vertex 1.5e0 0 0\r\n      vertex 1 1 1\r\n")
    for bad in (two, four, ref.ASCII_STL.replace(b"1.5e0", b"abc"), ref.ASCII_STL.replace(b"endsolid second\r\n", b"facet\r\n")):
        with pytest.raises(ValueError):
            stl(bad)
    p = ref.ply_bytes("ascii")
    for bad in (p.replace(b"format ascii", b"format binary_middle_endian"), p.replace(b"property double x", b"property double u"),
                p.replace(b"vertex_indices", b"corners"), p.replace(b"-3 4 0 1 2 3", b"-3 4 0 1 2 7"), p[:-8], b"plx\n",
                p.replace(b"property double x", b"property quad x"), ref.ply_bytes("binary_big_endian")[:-3],
                p.replace(b"-4 3 3 2 4", b"-4 2 3 2")):
        with pytest.raises(ValueError):
            ply(bad)
    with pytest.raises(ValueError):
        surface.check_facet_count((2 ** 31 - 1) // 3 + 1)
    assert surface.check_facet_count((2 ** 31 - 1) // 3) == 715827882


def test_create_surface_refuses_unknown_extensions_and_empty_files(tmp_path, no_library):
    from invesalius3_amd import surface
    for name in ("a.obj", "a.3mf", "a.txt", "stl"):
        (tmp_path / name).write_bytes(ref.ASCII_STL)
        with pytest.raises(ValueError, match="File format not reconized by InVesalius"):
            surface.CreateSurfaceFromFile(tmp_path / name)
    (tmp_path / "empty.STL").write_bytes(ref.stl_binary_bytes(np.zeros((0, 3, 3), np.float32)))
    (tmp_path / "empty2.stl").write_bytes(b"solid nothing\nendsolid nothing\n")
    (tmp_path / "empty.Ply").write_bytes(b"ply\nformat ascii 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\n"
                                         b"element face 0\nproperty list uchar int vertex_indices\nend_header\n")
    for name in ("empty.STL", "empty2.stl", "empty.Ply"):
        with pytest.raises(ValueError, match="not able to import"):
            surface.CreateSurfaceFromFile(tmp_path / name)


def test_headless_refuses_two_sources_of_a_surface(tmp_path, no_library, capsys):
    """--import-surface is an alternative to --threshold / --segment / --mask / --seed; --import-world needs both a file and a project"""
    from invesalius3_amd import headless
    stl = str(tmp_path / "a.stl")
    for argv in (["--import-surface", stl, "--threshold", "1", "2"], ["case.inv3", "--import-surface", stl, "--mask", "0"],
                 ["--import-surface", stl, "--seed", "1", "2", "3"], ["--import-surface", stl, "--import-world"],
                 ["case.inv3", "--import-world"], ["--import-surface", stl, "--save", "out.inv3"], ["--stl", "out.stl"]):
        with pytest.raises(SystemExit) as e:
            headless.main(argv)
        assert e.value.code == 2, argv
    capsys.readouterr()


# ---- Merge and the writers ------------------------------------------------------------------------------------------------
def test_writers_round_trip_through_the_readers(tmp_path, no_library):
    from invesalius3_amd import surface
    from invesalius3_amd import surface_process as sp
    soup = ref.soup_for(37)
    soup[3, 1] = (-0.0, 1e-45, 3.4028234e+38)  # a minus zero, the smallest subnormal, the largest float32
    surface.write_stl_ascii(tmp_path / "w.stl", soup)
    assert surface.stl_kind((tmp_path / "w.stl").read_bytes()) == "ascii"
    assert ref.same_bits(surface.read_stl(tmp_path / "w.stl"), soup)
    sp.write_stl_binary(tmp_path / "b.stl", soup)
    assert ref.same_bits(surface.read_stl(tmp_path / "b.stl"), soup)
    v, f, _ = ref.weld(soup)
    surface.write_ply_ascii(tmp_path / "w.ply", v, f)
    gv, gf = surface.read_ply(tmp_path / "w.ply")
    assert ref.same_bits(gv, v) and np.array_equal(gf, f)


def test_merge_appends_with_id_offsets(no_library):
    from invesalius3_amd import surface
    a = ref.weld(ref.soup_for(5))[:2]
    b = ref.weld(C.degenerate_case())[:2]
    e = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    v, f = surface.Merge([a, e, b])
    assert v.dtype == np.float32 and f.dtype == np.int32
    assert ref.same_bits(v, np.concatenate([a[0], b[0]])) and np.array_equal(f, np.concatenate([a[1], b[1] + len(a[0])]))
    assert ref.same_bits(v[f], np.concatenate([a[0][a[1]], b[0][b[1]]]))
    v0, f0 = surface.Merge([])
    assert v0.shape == (0, 3) and f0.shape == (0, 3)
    with pytest.raises(ValueError):
        surface.Merge([(a[0], a[1] + len(a[0]))])


# ---- the transform --------------------------------------------------------------------------------------------------------
AFFINE = np.array([[0.9, -0.1, 0.05, 12.5], [0.1, 0.95, -0.02, -40.25], [-0.03, 0.04, 1.1, 7.0], [0, 0, 0, 1]], np.float64)


def test_affine_is_the_slice_affine_with_the_y_shift(no_library):
    from invesalius3_amd import surface
    spacing, shape = (0.5, 0.7, 1.25), (30, 41, 52)
    m = surface.world_to_invesalius_affine(AFFINE, spacing, shape)
    want = AFFINE.copy()
    want[1, 3] -= 0.7 * 40
    assert np.array_equal(m, want) and np.array_equal(m, ref.world_to_inv_affine(AFFINE, spacing, shape))
    inv = surface.world_to_invesalius_affine(AFFINE, spacing, shape, inverse=True)
    assert np.array_equal(inv, np.linalg.inv(want))


def test_reference_transform_order_and_inverse_composes_to_identity():
    """the restatement's operation order, spelled out once more with Python floats; and forward then inverse gives the input
    back within the float32 rounding of the intermediate point: |x' - x| <= 2^-23 (sum_c |Minv[r, c]| |y_c| + |x_r|) covers the
    2^-24 relative rounding of y carried through Minv, that of x' itself, and the float64 operations with room to spare"""
    pts = ref.soup_for(40).reshape(-1, 3)
    m = ref.world_to_inv_affine(AFFINE, (0.5, 0.7, 1.25), (30, 41, 52))
    y = ref.transform(pts, m)
    for i in (0, 7, 119):
        x = [float(c) for c in pts[i]]
        for r in range(3):
            want = ((float(m[r, 0]) * x[0] + float(m[r, 1]) * x[1]) + float(m[r, 2]) * x[2]) + float(m[r, 3])
            assert y[i, r] == np.float32(want)
    minv = ref.world_to_inv_affine(AFFINE, (0.5, 0.7, 1.25), (30, 41, 52), inverse=True)
    back = ref.transform(y, minv).astype(np.float64)
    y1 = np.concatenate([np.abs(y.astype(np.float64)), np.ones((len(y), 1))], axis=1)
    bound = 2.0 ** -23 * (y1 @ np.abs(minv[:3]).T + np.abs(pts.astype(np.float64)))
    assert (np.abs(back - pts.astype(np.float64)) <= bound).all()
    assert math.isfinite(float(bound.max()))
