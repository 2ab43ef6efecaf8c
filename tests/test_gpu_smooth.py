"""Context-aware smoothing (invesalius_rs.Mesh / ca_smoothing; mesh.rs:27-395): HIP path vs the C restatement,
bit for bit, through the reference's python surface."""
import numpy as np
import pytest

from conftest import synth_volume

pytestmark = pytest.mark.gpu

OPTS = (0.7, 3.0, 0.5, 10)  # task_navigator.py:827 defaults: angle, max distance, min weight, steps


def _mc_mesh(seed=5, shape=(28, 36, 70), iso=250.0):
    from invesalius3_amd import surface_process as sp
    img = synth_volume(shape, seed=seed)
    return sp.marching_cubes_indexed(img, (0.4785156, 0.4785156, 1.25), [iso], 0, True, True, True,
                                     float(np.iinfo(np.int16).min), 1)


@pytest.mark.parametrize("vdtype", [np.float32, np.float64])
@pytest.mark.parametrize("fdtype", [np.int64, np.uint32])
def test_ca_smoothing_matches_oracle(ivxlib, oracle, vdtype, fdtype):
    from invesalius3_amd import invesalius_rs as rs
    verts, faces = _mc_mesh()
    mesh = rs.Mesh.from_indexed(verts.astype(vdtype), faces)
    assert np.array_equal(mesh.normals, oracle.mesh_face_normals(mesh.vertices, faces))
    mesh = rs.Mesh(vertices=mesh.vertices, faces=mesh.faces.astype(fdtype), normals=mesh.normals.astype(np.float32))
    want = mesh.vertices.copy()
    oracle.context_aware_smoothing(want, mesh.faces, mesh.normals, *OPTS)
    before = mesh.vertices.copy()
    rs.ca_smoothing(mesh, *OPTS)
    assert mesh.vertices.dtype == vdtype
    assert np.array_equal(mesh.vertices, want)
    assert not np.array_equal(mesh.vertices, before)
    # copy constructor + method form
    m2 = rs.Mesh(other=rs.Mesh(vertices=before, faces=mesh.faces, normals=mesh.normals))
    m2.ca_smoothing(*OPTS)
    assert np.array_equal(m2.vertices, want)


def test_staircase_flags_weights_and_quirks(ivxlib, oracle):
    import ctypes
    from invesalius3_amd import _lib as L
    verts, faces = _mc_mesh(seed=6, shape=(12, 16, 66))
    # add isolated vertices (never in a face) and a degenerate triangle
    verts = np.concatenate([verts, np.float32([[1e3, 0, 0], [0, 1e3, 0]])])
    faces = np.concatenate([faces, np.int32([[0, 0, 1]])])
    nrm = oracle.mesh_face_normals(verts, faces)
    f4 = np.concatenate([np.full((len(faces), 1), 3), faces], axis=1).astype(np.int64)
    want = verts.copy()
    flags0, w0 = oracle.context_aware_smoothing(want, f4, nrm, *OPTS, details=True)
    got = verts.copy()
    flags = np.zeros(len(verts), np.uint8)
    w = np.zeros(len(verts), np.float64)
    L.check(L.lib().ivx_context_aware_smoothing(L.ptr(got), L.F32, ctypes.c_int64(len(got)), L.ptr(faces),
                                                ctypes.c_int64(len(faces)), L.ptr(nrm), ctypes.c_double(OPTS[0]),
                                                ctypes.c_double(OPTS[1]), ctypes.c_double(OPTS[2]), ctypes.c_int(OPTS[3]),
                                                L.ptr(flags), L.ptr(w)))
    assert np.array_equal(flags, flags0) and np.array_equal(w, w0) and np.array_equal(got, want)
    assert flags[:-2].all() and not flags[-2:].any() and np.array_equal(got[-2:], verts[-2:])
    # normals == NULL: computed on the device, same result
    got2 = verts.copy()
    L.check(L.lib().ivx_context_aware_smoothing(L.ptr(got2), L.F32, ctypes.c_int64(len(got2)), L.ptr(faces),
                                                ctypes.c_int64(len(faces)), None, ctypes.c_double(OPTS[0]),
                                                ctypes.c_double(OPTS[1]), ctypes.c_double(OPTS[2]), ctypes.c_int(OPTS[3]),
                                                None, None))
    assert np.array_equal(got2, want)


def test_vertex_3_gets_every_face(ivxlib, oracle):
    """Q-M1 on the device: vertex id 3 is a seed although no triangle touches it"""
    from invesalius3_amd import invesalius_rs as rs
    v = np.zeros((6, 3), np.float32)
    v[:, 0] = np.arange(6)
    v[:, 1] = [0, 1, 0, 7, 1, 0]
    f4 = np.array([[3, 0, 1, 2], [3, 2, 4, 5]], np.int32)
    nrm = np.array([[0, 0, 1.0], [0, 0, 1.0]])
    want = v.copy()
    flags0, w0 = oracle.context_aware_smoothing(want, f4, nrm, 0.7, 3.0, 0.5, 3, details=True)
    assert flags0[3] == 1
    rs.context_aware_smoothing(v, f4, nrm, 0.7, 3.0, 0.5, 3)
    assert np.array_equal(v, want)


def test_propagate_weights_partial_seeds_matches_oracle(ivxlib, oracle):
    from invesalius3_amd import invesalius_rs as rs
    verts, faces = _mc_mesh(seed=8, shape=(20, 24, 66))
    rng = np.random.default_rng(1)
    for frac, tmax in ((0.002, 3.0), (0.05, 1.0), (0.0, 2.0)):
        seeds = (rng.random(len(verts)) < frac).astype(np.uint8)
        w = rs.propagate_weights(verts, faces, seeds, tmax, 0.5)
        w0 = oracle.mesh_propagate_weights(verts, faces, seeds, tmax, 0.5)
        assert np.array_equal(w, w0)
        if frac:
            assert (w[seeds == 1] == 1.0).all() and 0.5 <= w.min() and (w > 0.5).sum() > seeds.sum()
        else:
            assert (w == 0.5).all()


def test_argument_errors(ivxlib):
    from invesalius3_amd import invesalius_rs as rs
    v = np.zeros((4, 3), np.float32)
    f4 = np.array([[3, 0, 1, 2]], np.int64)
    n = np.zeros((1, 3), np.float64)
    with pytest.raises(TypeError):
        rs.context_aware_smoothing(v.astype(np.float16), f4, n, 0.7, 3.0, 0.5, 1)
    with pytest.raises(TypeError):
        rs.context_aware_smoothing(v, f4.astype(np.int16), n, 0.7, 3.0, 0.5, 1)
    with pytest.raises(TypeError):
        rs.context_aware_smoothing(v, f4[:, 1:], n, 0.7, 3.0, 0.5, 1)
    with pytest.raises(IndexError):
        rs.context_aware_smoothing(v, np.array([[3, 0, 1, 9]], np.int64), n, 0.7, 3.0, 0.5, 1)
    with pytest.raises(OverflowError):
        rs.context_aware_smoothing(v, f4, n, 0.7, 3.0, 0.5, -1)
    # empty mesh: nothing to do
    rs.context_aware_smoothing(np.zeros((0, 3), np.float32), np.zeros((0, 4), np.int64), np.zeros((0, 3)), 0.7, 3.0, 0.5, 2)
    with pytest.raises(ValueError):
        rs.Mesh()


def test_high_valence_fan_spills_out_of_registers(ivxlib, oracle):
    """a 40-triangle fan: the hub's incident-face and neighbour lists are longer than the in-register fast path"""
    from invesalius3_amd import invesalius_rs as rs
    k = 40
    ang = np.linspace(0, 2 * np.pi, k, endpoint=False)
    v = np.concatenate([[[0, 0, 0.3]], np.stack([np.cos(ang), np.sin(ang), 0 * ang], 1)]).astype(np.float32)
    rng = np.random.default_rng(2)
    order = rng.permutation(k)  # faces in scrambled order: the hub's neighbours appear in that order
    f3 = np.array([[0, 1 + i, 1 + (i + 1) % k] for i in order], np.int32)
    mesh = rs.Mesh.from_indexed(v, f3)
    want = mesh.vertices.copy()
    oracle.context_aware_smoothing(want, mesh.faces, mesh.normals, *OPTS)
    rs.ca_smoothing(mesh, *OPTS)
    assert np.array_equal(mesh.vertices, want)
    # float32 vertices round the Laplacian sums away every half-step and with them the neighbour order this test is about: the
    # same fan with jittered float64 vertices, where the reference's result does depend on that order
    # (tests/test_surface_switch_cases_host.py::test_float64_fans_show_the_neighbour_order)
    import _surface_switch_cases as S
    v64, f64, _ = S.closed_fan(k, 0, seed=2, dtype=np.float64)
    mesh = rs.Mesh.from_indexed(v64, f64)
    want = mesh.vertices.copy()
    oracle.context_aware_smoothing(want, mesh.faces, mesh.normals, *OPTS)
    rs.ca_smoothing(mesh, *OPTS)
    assert mesh.vertices.dtype == np.float64 and np.array_equal(mesh.vertices, want)


def test_bench_surface_smoothing_matches_oracle_and_reports_both_times(ivxlib, oracle, capsys):
    """the 6 M-triangle class of surface the bench produces, scaled to what the CPU oracle does in a few seconds:
    bit-identical vertices, and the two wall times side by side (informational, printed with -s)"""
    import time
    from invesalius3_amd import invesalius_rs as rs
    from invesalius3_amd import surface_process as sp
    img = synth_volume((96, 160, 192), seed=51)
    img[np.random.default_rng(5).random(img.shape) < 0.01] = 2000  # debris, like the bench volume's noise fringe
    verts, faces = sp.marching_cubes_indexed(img, (0.5, 0.5, 0.5), [226.0], 0, True, True, True,
                                             float(np.iinfo(np.int16).min), 1)
    mesh = rs.Mesh.from_indexed(verts, faces)
    want = mesh.vertices.copy()
    t0 = time.perf_counter()
    oracle.context_aware_smoothing(want, mesh.faces, mesh.normals, *OPTS)
    t_cpu = time.perf_counter() - t0
    t0 = time.perf_counter()
    rs.ca_smoothing(mesh, *OPTS)
    t_gpu = time.perf_counter() - t0
    assert np.array_equal(mesh.vertices, want)
    print("ca_smoothing %d vertices / %d triangles: oracle %.3f s, host entry point (PCIe both ways) %.3f s"
          % (len(verts), len(faces), t_cpu, t_gpu))
