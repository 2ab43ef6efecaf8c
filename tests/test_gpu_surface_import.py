"""GPU: surface import (csrc/k_meshweld.hip, invesalius3_amd/surface.py) -- the weld, the STL unpack and the point
transform bit for bit against tests/_surface_import_ref.py on the cases of tests/_surface_import_cases.py (which
tests/test_surface_import_host.py proves to stand where they are said to), the round trip the reference's own test pins
(tests/test_stl_export.py:72-108), the welded mesh through the existing surface kernels, and the headless driver."""
import ctypes
import json
import math

import numpy as np
import pytest

import _surface_import_cases as C
import _surface_import_ref as ref
import _surface_switch_cases as S

pytestmark = pytest.mark.gpu

CASES = {"cluster": lambda: C.cluster_case()[0], "wrap": lambda: C.wrap_case()[0], "zero_signs": C.zero_sign_case,
         "scan_4095": lambda: C.distinct_case(1365), "scan_4098": lambda: C.distinct_case(1366), "one_facet": lambda: C.distinct_case(1),
         "identical": C.identical_case, "repeated": C.repeated_case, "degenerate": C.degenerate_case}


def _equal(got, want):
    gv, gf, gc = got
    wv, wf, wc = want
    assert gv.dtype == np.float32 and gf.dtype == np.int32
    assert ref.same_bits(gv, wv), "vertices differ"
    assert gf.shape == wf.shape and np.array_equal(gf, wf), "faces differ"
    assert {k: gc[k] for k in wc} == wc, (gc, wc)


@pytest.mark.parametrize("name", list(CASES))
def test_weld_cases(ivxlib, name):
    """host form and resident form against the dict weld; the status words say what the table did"""
    from invesalius3_amd import polydata_utils as pu
    from invesalius3_amd import surface
    soup = CASES[name]()
    want = ref.weld(soup)
    got = surface.weld_soup(soup)
    _equal(got, want)
    n = soup.size // 3
    c = got[2]
    assert c["slots"] == C.slots_for(n) and sum(c["probe_histogram"]) == n
    if name == "cluster":
        assert c["max_probe"] >= 3  # four keys from one home slot take four slots
    if name == "wrap":
        assert c["max_probe"] >= 1
    if name == "identical":
        assert c["probe_histogram"][0] == n and c["max_probe"] == 0 and (c["vertices"], c["facets"]) == (1, 0)
    mesh = pu.DeviceMesh.from_soup(soup)
    try:
        v, f = mesh.download()
        _equal((v, f, mesh.weld_counts), want)
    finally:
        mesh.close()


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_a_non_finite_coordinate_at_the_last_corner_is_a_value_error(ivxlib, tmp_path, bad):
    from invesalius3_amd import polydata_utils as pu
    from invesalius3_amd import surface
    soup = C.distinct_case(90)
    soup[-1, -1, 2] = bad
    with pytest.raises(ValueError):
        surface.weld_soup(soup)
    with pytest.raises(ValueError):
        pu.DeviceMesh.from_soup(soup)
    data = ref.stl_binary_bytes(soup)
    with pytest.raises(ValueError):
        pu.DeviceMesh.from_stl_bytes(data)
    with pytest.raises(ValueError):
        surface.weld_stl_bytes(data)
    (tmp_path / "bad.stl").write_bytes(data)
    with pytest.raises(ValueError):
        surface.CreateSurfaceFromFile(tmp_path / "bad.stl")


@pytest.mark.parametrize("nt", [1, 2, 255, 256, 257])
def test_stl_unpack_equals_the_host_reader(ivxlib, tmp_path, nt):
    """the files of the host test: the unpacked soup is read_stl's, bit for bit (records alternate between 4- and 2-byte alignment;
    255 | 256 | 257 end a workgroup's span of 128 records one short, exactly, one over); then the weld from the same bytes"""
    from invesalius3_amd import _lib as L
    from invesalius3_amd import polydata_utils as pu
    from invesalius3_amd import surface
    from invesalius3_amd.device import DeviceBuffer
    data = ref.stl_binary_bytes(ref.soup_for(nt))
    (tmp_path / "a.stl").write_bytes(data)
    want = surface.read_stl(tmp_path / "a.stl")
    raw = np.frombuffer(data, np.uint8)
    file_buf, soup_buf, flag = DeviceBuffer(len(raw)), DeviceBuffer(nt * 36 + 16), DeviceBuffer(16)
    try:
        file_buf.upload(raw)
        flag.zero()
        soup_buf.zero()
        L.check(L.lib().ivx_dev_stl_unpack(file_buf.ptr, ctypes.c_int64(nt), soup_buf.ptr, flag.ptr, None), "stl_unpack")
        L.synchronize()
        assert ref.same_bits(soup_buf.download((nt, 3, 3), np.float32), want)
        assert int(flag.download((1,), np.uint32)[0]) == 0
    finally:
        for b in (file_buf, soup_buf, flag):
            b.close()
    oracle = ref.weld(want)
    _equal(surface.weld_stl_bytes(data), oracle)
    mesh = pu.DeviceMesh.from_stl_bytes(data)
    try:
        _equal(mesh.download() + (mesh.weld_counts,), oracle)
    finally:
        mesh.close()


def test_transform_points_is_the_reference_order(ivxlib):
    from invesalius3_amd import surface
    pts = ref.soup_for(120).reshape(-1, 3)
    affine = np.array([[0.9, -0.1, 0.05, 12.5], [0.1, 0.95, -0.02, -40.25], [-0.03, 0.04, 1.1, 7.0], [0, 0, 0, 1]], np.float64)
    spacing, shape = (0.5, 0.7, 1.25), (30, 41, 52)
    for inverse in (False, True):
        m = ref.world_to_inv_affine(affine, spacing, shape, inverse)
        assert ref.same_bits(surface.transform_points(pts, m), ref.transform(pts, m))
        assert ref.same_bits(surface.ConvertPolydataToInv(pts, affine, spacing, shape, inverse), ref.transform(pts, m))


# ---- the round trip -------------------------------------------------------------------------------------------------------
def _mass_bounds(verts, faces):
    """the bound of test_gpu_surface_switches.py for the four mass sums -- both sides add the same float64 terms in trees of at
    most 32 nested additions, so two results differ by at most 64 * 2^-53 * sum |term| -- and what follows for the volume
    |kx vx + ky vy + kz vz| with the exact weights k: sum |k_q| bound_q for the sums, plus the five roundings of the three
    products and two additions, each at most 2^-53 of sum |k_q v_q| (8 leaves room)"""
    from invesalius3_amd import surface_process as sp
    area, div = S.mass_terms(verts, faces)
    b = [64.0 * 2.0 ** -53 * math.fsum(np.abs(t)) for t in (area, div[:, 0], div[:, 1], div[:, 2])]
    full = sp.mass_properties_full(verts, faces)
    k, v = full[5:], full[2:5]
    vol_bound = sum(abs(k[q]) * b[1 + q] for q in range(3)) + 8.0 * 2.0 ** -53 * sum(abs(k[q] * v[q]) for q in range(3))
    return full[0], full[1], vol_bound, b[0]


def _point_set(v):
    return set(map(tuple, np.ascontiguousarray(v, np.float32).view(np.uint32).tolist()))


@pytest.fixture(scope="module")
def cube(ivxlib, tmp_path_factory):
    """marching_cubes_indexed of the 20^3 mask with a 10^3 block, and its binary STL"""
    from invesalius3_amd import surface_process as sp
    mask = np.zeros((20, 20, 20), np.uint8)
    mask[5:15, 5:15, 5:15] = 255
    v, f = sp.marching_cubes_indexed(mask, (1.0, 1.0, 1.0), [127.0])
    path = tmp_path_factory.mktemp("import") / "cube.stl"
    sp.write_stl_binary(path, v[f])
    return v, f, path


def test_round_trip_of_the_cube_keeps_points_and_cells(cube):
    from invesalius3_amd import surface
    v, f, path = cube
    imp = surface.CreateSurfaceFromFile(path)
    try:
        gv, gf = imp.mesh.download()
        assert (len(gv), len(gf)) == (len(v), len(f)) and len(v) > 0
        assert _point_set(gv) == _point_set(v) and ref.same_bits(gv[gf], v[f])
        _equal((gv, gf, imp.counts), ref.weld(v[f]))
        vol, area, vb, ab = _mass_bounds(v, f)
        print("cube: volume %.17g vs %.17g (bound %.3g), area %.17g vs %.17g (bound %.3g)" % (imp.volume, vol, vb, imp.area, area, ab))
        assert abs(imp.volume - vol) <= vb and abs(imp.area - area) <= ab
        assert imp.name == "cube" and imp.format == "stl-binary"
        assert len(imp.normals) == len(imp.normal_verts) >= len(gv) and len(imp.normal_faces) == len(gf)
    finally:
        imp.close()


def test_round_trip_of_a_thresholded_volume_against_the_python_weld(ivxlib, tmp_path):
    """here the marching-cubes count may differ (two grid edges can collide in float32): only the oracle decides"""
    from conftest import synth_volume
    from invesalius3_amd import surface
    from invesalius3_amd import surface_process as sp
    mask = np.where(synth_volume((48, 48, 48)) >= 226, 255, 0).astype(np.uint8)
    v, f = sp.marching_cubes_indexed(mask, (1.0, 1.0, 1.0), [127.0])
    assert len(f) > 1000
    sp.write_stl_binary(tmp_path / "vol.stl", v[f])
    wv, wf, wc = ref.weld(surface.read_stl(tmp_path / "vol.stl"))
    imp = surface.CreateSurfaceFromFile(tmp_path / "vol.stl")
    try:
        gv, gf = imp.mesh.download()
        _equal((gv, gf, imp.counts), (wv, wf, wc))
        vol, area, vb, ab = _mass_bounds(wv, wf)
        print("volume: %.17g vs %.17g (bound %.3g), area %.17g vs %.17g (bound %.3g)" % (imp.volume, vol, vb, imp.area, area, ab))
        assert abs(imp.volume - vol) <= vb and abs(imp.area - area) <= ab
    finally:
        imp.close()


def test_ply_and_vtp_import_and_forced_weld(cube, tmp_path):
    from invesalius3_amd import surface
    from invesalius3_amd import surface_process as sp
    v, f, _ = cube
    surface.write_ply_ascii(tmp_path / "c.PLY", v, f)
    sp.write_vtp(tmp_path / "c.vtp", v[f].reshape(-1, 3), np.arange(3 * len(f), dtype=np.int32).reshape(-1, 3))
    imp = surface.CreateSurfaceFromFile(tmp_path / "c.PLY")
    try:
        gv, gf = imp.mesh.download()
        assert ref.same_bits(gv, v) and np.array_equal(gf, f) and imp.format == "ply" and imp.counts["dropped"] == 0
    finally:
        imp.close()
    soup_mesh = surface.CreateSurfaceFromFile(tmp_path / "c.vtp")  # no weld by default: the soup as it is
    welded = surface.CreateSurfaceFromFile(tmp_path / "c.vtp", weld=True)
    try:
        assert soup_mesh.mesh.nverts == 3 * len(f) and soup_mesh.mesh.ntris == len(f)
        _equal(welded.mesh.download() + (welded.counts,), ref.weld(v[f]))
    finally:
        soup_mesh.close()
        welded.close()


def test_convert_to_inv_on_the_resident_points(cube):
    from invesalius3_amd import surface
    v, f, path = cube
    affine = np.array([[1, 0, 0, 3.5], [0, 1, 0, -2.0], [0, 0, 1, 0.25], [0, 0, 0, 1]], np.float64)
    imp = surface.CreateSurfaceFromFile(path, convert_to_inv=(affine, (1.0, 0.5, 1.0), (20, 20, 20)))
    try:
        gv, gf = imp.mesh.download()
        wv, wf, _ = ref.weld(v[f])
        assert ref.same_bits(gv, ref.transform(wv, ref.world_to_inv_affine(affine, (1.0, 0.5, 1.0), (20, 20, 20)))) and np.array_equal(gf, wf)
    finally:
        imp.close()


def test_the_welded_mesh_feeds_split_and_keep_largest(cube):
    """the imported cube and a second, shifted copy in one soup: two parts"""
    from invesalius3_amd import polydata_utils as pu
    v, f, _ = cube
    soup = np.concatenate([v[f], v[f] + np.float32(100.0)])
    mesh = pu.DeviceMesh.from_soup(soup)
    parts = largest = None
    try:
        assert mesh.nverts == 2 * len(v) and mesh.ntris == 2 * len(f)
        parts = mesh.split()
        assert parts.n == 2 and [int(t) for t in parts.table[:, 1]] == [len(f), len(f)]
        largest = mesh.keep_largest()
        lv, lf = largest.download()
        assert (len(lv), len(lf)) == (len(v), len(f)) and ref.same_bits(lv[lf], v[f])  # (a tie: the first region)
    finally:
        for m in (parts, largest, mesh):
            if m is not None:
                m.close()


def test_headless_import_largest_stl_equals_the_direct_calls(cube, tmp_path, capsys):
    from invesalius3_amd import headless, surface
    from invesalius3_amd import polydata_utils as pu
    from invesalius3_amd import surface_process as sp
    v, f, _ = cube
    both = tmp_path / "both.stl"
    extra = v[f][:40] + np.float32(100.0)  # a smaller second part
    sp.write_stl_binary(both, np.concatenate([extra, v[f]]))
    out = tmp_path / "out.stl"
    assert headless.main(["--import-surface", str(both), "--largest", "--stl", str(out)]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    mesh = pu.DeviceMesh.from_stl_bytes(both.read_bytes())
    largest = mesh.keep_largest()
    try:
        lv, lf = largest.download()
        assert ref.same_bits(surface.read_stl(out), lv[lf]) and ref.same_bits(lv[lf], v[f])
        imp = line["import"]
        assert (imp["format"], imp["facets_read"], imp["vertices"], imp["triangles"], imp["dropped"]) == \
               ("stl-binary", len(f) + 40, mesh.nverts, mesh.ntris, 0)
        assert line["largest"]["vertices"] == len(v) and line["largest"]["triangles"] == len(f) and line["largest"]["regions"] >= 2
        vol, area = sp.mass_properties(lv, lf)
        assert (line["volume"], line["area"]) == (vol, area) and imp["volume"] > 0 and imp["area"] > line["area"]
    finally:
        largest.close()
        mesh.close()
    with pytest.raises(SystemExit):
        headless.main(["--import-surface", str(both), "--threshold", "1", "2"])
    capsys.readouterr()
