"""Headless driver with the geodesic measure: .inv3 -> --threshold --geodesic X Y Z X Y Z [X Y Z] gives the path that
`measures.geodesic_path` gives on the same surface made by hand, with two and with three picks, and --geodesic-npy round-trips."""
import json

import numpy as np
import pytest

import _geodesic_ref as R

pytestmark = pytest.mark.gpu

SPACING = (0.5, 0.5, 1.0)


def _run(capsys, argv):
    from invesalius3_amd import headless
    assert headless.main([str(a) for a in argv]) == 0
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def _image():
    z, y, x = np.mgrid[:26, :26, :56]
    img = np.full(z.shape, -1000, np.int16)
    for cx, r in ((8.5, 6.0), (26.5, 9.0), (46.5, 4.0)):  # three balls: middle, large, small
        img[(z - 12.5) ** 2 + (y - 12.5) ** 2 + (x - cx) ** 2 <= r * r] = 1000
    return img


def test_geodesic_two_and_three_picks(ivxlib, tmp_path, capsys):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    from invesalius3_amd import measures
    from invesalius3_amd import project as prj
    from invesalius3_amd import surface_process as sp
    img = _image()
    p = prj.Project(name="Balls", spacing=SPACING, threshold_range=(int(img.min()), int(img.max())))
    p.matrix = img
    src = tmp_path / "in.inv3"
    prj.save_inv3(src, p)
    # the surface by hand, and three picks a little off the large ball's points
    mask = np.where((img >= 226) & (img <= 3071), 255, 0).astype(np.uint8)
    verts, faces = sp.marching_cubes_indexed(mask, SPACING, [127.0], 0, True, True, True, 0.0, 1)
    e = R.edges(faces)
    ncomp, lab = connected_components(csr_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(len(verts),) * 2), directed=False)
    assert ncomp == 3
    big = np.flatnonzero(lab == np.argmax(np.bincount(lab)))
    at = [big[np.argmin(verts[big, 0])], big[np.argmax(verts[big, 0])], big[np.argmax(verts[big, 2])]]
    picks = [(verts[q].astype(np.float64) + 0.01).tolist() for q in at]
    for n in (2, 3):
        flat = [x for xyz in picks[:n] for x in xyz]
        npy = tmp_path / ("path%d.npy" % n)
        res = _run(capsys, [src, "--threshold", 226, 3071, "--geodesic", *flat, "--geodesic-npy", npy])["geodesic"]
        want = measures.geodesic_path(verts, faces, points=picks[:n])
        assert res["points"] == picks[:n] and res["point_ids"] == want.point_ids.tolist() == [int(q) for q in at[:n]]
        assert res["segment_lengths"] == want.segment_lengths and res["length_mm"] == want.length and want.length > 0.0
        assert res["path_points"] == len(want.points)
        assert np.array_equal(np.load(npy), want.points)
        for q in range(n - 1):
            R.check_path(verts, faces, want.ids[q], at[q], at[q + 1], want.segment_lengths[q])
    # a pick on another ball cannot be reached: the segment is skipped
    other = np.flatnonzero(lab != lab[big[0]])[0]
    res = _run(capsys, [src, "--threshold", 226, 3071, "--geodesic", *picks[0], *verts[other].tolist()])["geodesic"]
    assert res["path_points"] == 0 and res["length_mm"] == 0.0 and res["point_ids"] == [int(at[0]), int(other)]


def test_geodesic_arguments(tmp_path):
    from invesalius3_amd import headless
    for bad in (["--geodesic", "1", "2", "3"], ["--geodesic", "1", "2", "3", "4", "5", "6", "7"], ["--geodesic-npy", "x.npy"]):
        with pytest.raises(SystemExit):
            headless.main([str(tmp_path / "none.inv3"), "--threshold", "0", "1", *bad])
    ns = type("A", (), dict(threshold=None, segment=None, seed=None, stl=None, save=None, largest=False, smooth=False,
                            remove_nonvisible=False, surface_seed=None, split=None, crop=None, argv=[], geodesic=[0.0] * 6))
    assert not headless._render_only(ns)
    ns.geodesic = None
    assert headless._render_only(ns)
