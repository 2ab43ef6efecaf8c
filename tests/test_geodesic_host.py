"""CPU: the restatement of the geodesic measure's rules (tests/_geodesic_ref.py) against live scipy and hand numbers,
the path checker against paths that are wrong, and the argument checks of `invesalius3_amd.measures`, which come before the
library is touched."""
import math

import numpy as np
import pytest

import _geodesic_ref as R

SQUARE = (np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.int32))


def _meshes():
    v, f = R.jittered_grid()
    yield "grid", v, f, (0, 40 * 20 + 20, len(v) - 1)
    v, f = R.jittered_grid(shift=(1000.0, 0.0, 0.0))
    yield "grid+1000", v, f, (0,)
    v, f = R.strip2(1500)
    yield "strip2x1500", v, f, (0,)
    v, f = R.fan(300)
    yield "fan", v, f, (0, 7)
    for n in (63, 64, 65, 255, 256, 257):
        v, f = R.strip(n)
        yield "strip%d" % n, v, f, (0, n - 1)
    v, f = SQUARE
    yield "square", v, f, (0, 1)
    # two components, a point no triangle uses (6) and a triangle with a repeated id
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 0, 0], [6, 0, 0], [5, 1, 0], [9, 9, 9]], np.float32)
    yield "parts", v, np.array([[0, 1, 2], [3, 4, 5], [1, 1, 2]], np.int32), (0, 3, 6)


@pytest.mark.parametrize("name,v,f,sources", [pytest.param(*m, id=m[0]) for m in _meshes()])
def test_restatements_equal_scipy(name, v, f, sources):
    for s in sources:
        want = R.scipy_dijkstra(v, f, s)
        got, pred = R.heap_dijkstra(v, f, s)
        assert np.array_equal(got, want)
        assert np.array_equal(R.bellman_ford(v, f, s), want)
        assert pred[s] == -1 and np.array_equal(pred == -1, ~np.isfinite(want) | (np.arange(len(v)) == s))


def test_unit_square_by_hand():
    v, f = SQUARE
    d, pred = R.heap_dijkstra(v, f, 0)
    assert d.tolist() == [0.0, 1.0, math.sqrt(2.0), 1.0] and pred.tolist() == [-1, 0, 0, 0]
    assert R.edges(f).tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [2, 3]]
    off, adj = R.csr(f, 4)
    assert off.tolist() == [0, 3, 5, 8, 10] and adj.tolist() == [1, 2, 3, 0, 2, 0, 1, 3, 0, 2]
    d1, _ = R.heap_dijkstra(v, f, 1)
    assert d1.tolist() == [1.0, 0.0, 1.0, 2.0]  # 1 -> 3 has no side: round either way
    R.check_path(v, f, [1, 0, 3], 1, 3, 2.0)
    R.check_path(v, f, [0, 2], 0, 2, math.sqrt(2.0))
    R.check_path(v, f, [2], 2, 2, 0.0)


def test_csr_rules():
    v, f = R.fan(300)
    off, adj = R.csr(f, len(v))
    assert off[1] == 300 and adj[:300].tolist() == list(range(1, 301)) and adj[300:303].tolist() == [0, 2, 300]
    off, adj = R.csr(np.array([[0, 1, 2], [1, 1, 2]], np.int32), 4)  # the repeated id adds nothing; point 3 is unused
    assert off.tolist() == [0, 2, 4, 6, 6] and adj.tolist() == [1, 2, 0, 2, 0, 1]


def test_check_path_rejects_wrong_paths():
    v, f = SQUARE
    with pytest.raises(AssertionError, match="no triangle side"):
        R.check_path(v, f, [1, 3], 1, 3, math.sqrt(2.0))
    with pytest.raises(AssertionError):
        R.check_path(v, f, [1, 0, 3], 1, 3, np.nextafter(2.0, 3.0))
    with pytest.raises(AssertionError, match="repeats"):
        R.check_path(v, f, [1, 0, 1, 2], 1, 2, 3.0)
    with pytest.raises(AssertionError):
        R.check_path(v, f, [0, 1], 1, 0, 1.0)


def test_measures_checks_arguments_before_the_library(monkeypatch):
    from invesalius3_amd import _lib, measures

    def touched(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "lib", touched)
    monkeypatch.setattr(_lib, "require_device", touched)
    v, f = SQUARE
    with pytest.raises(ValueError):
        measures.geodesic_path(v, f, ids=[0, 4])
    with pytest.raises(ValueError):
        measures.geodesic_path(v, f, ids=[-1, 2])
    with pytest.raises(ValueError):
        measures.geodesic_path(v, f, ids=[2])
    with pytest.raises(ValueError):
        measures.geodesic_path(v, f, points=[(0.0, 0.0, 0.0)])
    with pytest.raises(ValueError):
        measures.geodesic_path(v, f, ids=[0.5, 2.0])
    with pytest.raises(ValueError):
        measures.geodesic_path(v, np.array([[0, 1, 4]], np.int32), ids=[0, 1])
    with pytest.raises(ValueError):
        measures.geodesic_path(v, f)
    m = measures.GeodesicMeasure()
    assert m.GetValue() == 0.0 and not m.IsComplete()
    m.AddPoint(0, 0, 0)
    m.AddPoint(3, 4, 0)
    assert m.IsComplete() and not m.IsComplete(multi_point=True) and m.GetValue() == 5.0  # the straight line: no surface yet
    assert m.AddPoint(1, 1, 1) is False and m.GetNumberOfPoints() == 2
    m.finalize()
    assert m.IsComplete(multi_point=True)


def test_measures_without_a_device_is_a_runtime_error():
    from invesalius3_amd import _lib, measures

    if _lib.device_count() > 0:
        pytest.skip("GPU present")
    v, f = SQUARE
    with pytest.raises(RuntimeError):
        measures.geodesic_path(v, f, ids=[0, 2])
    with pytest.raises(RuntimeError):
        measures.geodesic_path(v, f, points=[(0, 0, 0), (1, 1, 0)])
    m = measures.GeodesicMeasure()
    with pytest.raises(RuntimeError):
        m.SetSurface(v, f)
