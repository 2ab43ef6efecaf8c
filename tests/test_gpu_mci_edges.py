"""GPU: the indexed mesh of csrc/k_mci.hip and its cross-slab stitch on the cases of _mci_cases.py, held to the numpy restatement
_mci_ref.py and the C oracle's soup.  Every comparison is exact (bit patterns of the floats, ids as they are); nothing has a
tolerance.

  1. pieces        verts[faces] is the oracle soup in order; the vertices are the restated ones ARRAY FOR ARRAY, which pins the id
                   order the header of k_mci.hip promises (raster order of point words; in a word x edges, y edges, z edges, point
                   vertices) and both sides of the stitch count on; the faces are the restated ones
  2. device form   ivx_dev_mc_count / _indexed_count / _indexed_emit into guarded buffers: exact counts, nothing written past
                   them, nor past a shorter max_verts
  3. levels path   the mesh from the mask's known byte levels at rows of 62 .. 127 voxels equals the voxel path and the restatement
                   (through ivx_dev_mc_count_bits / _indexed_count_levels / _indexed_emit_levels: a resident volume takes that path
                   itself only where its rows are whole words)
  4. stitch        the C entry points rank after rank on pieces WITH samples on the iso-value (the product's Python API only ever
                   stitches 0 / 255 masks, where the point-vertex branches of k_mci_match and k_mci_gid0 never run)

Out of scope: the grid-stride loops of the kernels only take a second trip beyond 16384 workgroups x 256 lanes, i.e. with more than
4 M point words; no case here is that large."""
import ctypes

import numpy as np
import pytest

import _mci_cases as C
import _mci_ref as R
import _slab_cases as sc
from _stitch_ref import stitch_piece_meshes
from conftest import synth_volume

pytestmark = pytest.mark.gpu

S26 = np.ones((3, 3, 3), np.uint8)
GUARD = 0xA5
c64 = ctypes.c_int64
PIECES = {c["name"]: c for c in C.piece_cases()}
STITCHES = {c["name"]: c for c in C.stitch_cases()}


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rows(v):
    return np.unique(_u32(v).reshape(-1, 3), axis=0)


def _tri_rows(soup):
    t = _u32(soup).reshape(-1, 9)
    return t[np.lexsort(t.T[::-1])]


_REF = {}


def _reference(oracle, name):
    """(per-iso soups, restated verts, restated faces) of a piece case: computed once, shared, never changed"""
    if name not in _REF:
        c = PIECES[name]
        soups = [oracle.marching_cubes(c["array"], *C.args_of(c, [iso])) for iso in c["iso_values"]]
        rv, rf = R.indexed_mesh(c["array"], C.args_of(c), soups)
        for x in soups + [rv, rf]:
            x.setflags(write=False)
        _REF[name] = (soups, rv, rf)
    return _REF[name]


def _check_piece(sp, oracle, c):
    verts, faces = sp.marching_cubes_indexed(c["array"], *C.args_of(c))
    soups, rv, rf = _reference(oracle, c["name"])
    soup = np.concatenate(soups)
    assert verts.dtype == np.float32 and faces.dtype == np.int32, c["name"]
    assert verts.shape == (len(rv), 3) and faces.shape == (len(soup), 3), (c["name"], verts.shape, faces.shape, len(rv), len(soup))
    if len(soup) == 0:  # empty along an axis, or without a cell: nothing, on both sides
        assert verts.shape == (0, 3) and faces.shape == (0, 3), c["name"]
        return
    assert np.array_equal(_u32(verts[faces]), _u32(soup)), c["name"] + ": verts[faces] is not the soup"
    assert np.array_equal(_u32(verts), _u32(rv)), c["name"] + ": vertex order"   # (both iso-values' id ranges, iso 0's first)
    assert np.array_equal(faces, rf), c["name"] + ": faces"


@pytest.mark.parametrize("group", ["ints", "pad_on_iso", "pad_inside", "u16", "thin", "past_scan_block"])
def test_pieces_equal_the_restated_mesh_array_for_array(ivxlib, oracle, group):
    from invesalius3_amd import surface_process as sp
    cases = [c for c in PIECES.values() if c["group"] == group]
    assert cases
    for c in cases:
        _check_piece(sp, oracle, c)


def test_planted_on_iso_samples_after_a_large_call(ivxlib, oracle):
    """one sample on the iso-value at bit 0 / bit 63 of a word, its only crossing arriving from one known side -- after a call that
    left large workspaces behind, so that a record or base the small piece fails to write shows as the large piece's"""
    from invesalius3_amd import surface_process as sp
    big = PIECES["past_scan_block"]
    v, f = sp.marching_cubes_indexed(big["array"], *C.args_of(big))
    assert len(v) > 100000 and len(f) > 100000
    planted = [c for c in PIECES.values() if c["group"] == "planted"]
    assert {(c["point"][2], c["direction"]) for c in planted} >= {(i, d) for i in (1, 63, 64, 128) for d in C.DIRECTIONS}
    for c in planted:
        _check_piece(sp, oracle, c)


# ---- 2. the device form --------------------------------------------------------------------------------------------------------
def _params(L, a, args):
    spacing, isos, roi_start, pad_xy, pad_bottom, pad_top, pad_value, vtk_pz = args
    return L.McParams(dtype=L.DT[a.dtype], pad_xy=int(pad_xy), pad_bottom=int(pad_bottom), pad_top=int(pad_top), vtk_pz=int(vtk_pz),
                      niso=len(isos), nz=a.shape[0], ny=a.shape[1], nx=a.shape[2], roi_start=int(roi_start), pad_value=float(pad_value),
                      spacing=(ctypes.c_double * 3)(*spacing), iso=(ctypes.c_double * 2)(*(list(isos) + [0.0])[:2]))


def _device_piece(L, a, p):
    """(scratch, voxels) on the device"""
    from invesalius3_amd.device import DeviceBuffer
    nb = ctypes.c_size_t(0)
    L.check(L.lib().ivx_dev_mc_scratch_bytes(ctypes.byref(p), ctypes.byref(nb)))
    d_a = DeviceBuffer(max(a.nbytes, 16))
    d_a.upload(a)
    return DeviceBuffer(nb.value), d_a


@pytest.mark.parametrize("name", ["ints_NX64_TTT_pz1", "ints_NX65_TTT_pz1", "ints_NX65_FFF_pz0", "planted_k1_j1_x64_-x"])
def test_device_form_writes_its_counts_and_nothing_past_them(ivxlib, oracle, name):
    from invesalius3_amd import _lib as L
    from invesalius3_amd.device import DeviceBuffer
    lib, c = L.lib(), PIECES[name]
    soups, rv, rf = _reference(oracle, name)
    a, p = c["array"], _params(L, c["array"], C.args_of(c))
    d_s, d_a = _device_piece(L, a, p)
    nt, nv = c64(0), c64(0)
    L.check(lib.ivx_dev_mc_count(ctypes.byref(p), d_a.ptr, d_s.ptr, ctypes.byref(nt), None))
    L.check(lib.ivx_dev_mc_indexed_count(ctypes.byref(p), d_a.ptr, d_s.ptr, ctypes.byref(nv), None))
    assert nt.value == len(rf) > 0 and nv.value == len(rv) > 1
    d_v, d_f = DeviceBuffer((nv.value + 8) * 12), DeviceBuffer((nt.value + 8) * 12)
    guard_v = np.full((8, 3), GUARD * 0x01010101, np.uint32)
    for max_verts in (nv.value, nv.value - 1):
        for d in (d_v, d_f):
            L.check(lib.ivx_memset(d.ptr, GUARD, ctypes.c_size_t(d.nbytes), None))
        L.check(lib.ivx_dev_mc_indexed_emit(ctypes.byref(p), d_a.ptr, d_s.ptr, d_v.ptr, c64(max_verts), d_f.ptr, c64(nt.value), None))
        L.check(lib.ivx_device_synchronize())
        verts = d_v.download((nv.value + 8, 3), np.uint32)
        faces = d_f.download((nt.value + 8, 3), np.int32)
        assert np.array_equal(verts[:max_verts], _u32(rv)[:max_verts]), (name, max_verts)
        assert np.array_equal(verts[max_verts:], np.full((nv.value + 8 - max_verts, 3), GUARD * 0x01010101, np.uint32)), (name, max_verts)
        assert np.array_equal(faces[:nt.value], rf) and np.array_equal(faces[nt.value:].view(np.uint32), guard_v), (name, max_verts)
    for d in (d_s, d_a, d_v, d_f):
        d.close()


# ---- 3. the levels path --------------------------------------------------------------------------------------------------------
def _bit_plane(b):
    """a boolean (nz, ny, nx) volume as the library's bit planes: source coordinates, rows of ceil(nx / 64) uint64 words, voxel x
    at bit x & 63 of word x >> 6, zeros behind the row's end"""
    nz, ny, nx = b.shape
    wide = np.zeros((nz, ny, -(-nx // 64) * 64), np.uint8)
    wide[:, :, :nx] = b
    return np.ascontiguousarray(np.packbits(wide, axis=2, bitorder="little")).view("<u8")


def _levels_mesh(L, mask, args, select):
    """the indexed mesh of `mask` through ivx_dev_mc_count_bits, _indexed_count_levels and _indexed_emit_levels: no voxel is read, only
    the inside plane and the plane of the selected voxels, both built here from the mask's bytes"""
    from invesalius3_amd.device import DeviceBuffer
    lib, p = L.lib(), _params(L, mask, args)
    inside = _bit_plane(mask >= 127)
    sel = _bit_plane(mask == select) if select is not None else inside  # (without a second level any plane will do: v_sel = v_in)
    bufs = []
    for plane in (inside, sel):
        d = DeviceBuffer(plane.nbytes + 4096)
        d.zero()
        d.upload(plane)
        bufs.append(d)
    nb = ctypes.c_size_t(0)
    L.check(lib.ivx_dev_mc_scratch_bytes(ctypes.byref(p), ctypes.byref(nb)))
    d_s = DeviceBuffer(nb.value)
    nt, nv = c64(0), c64(0)
    L.check(lib.ivx_dev_mc_count_bits(ctypes.byref(p), bufs[0].ptr, d_s.ptr, ctypes.byref(nt), None), "mc_count_bits")
    L.check(lib.ivx_dev_mc_indexed_count_levels(ctypes.byref(p), d_s.ptr, ctypes.byref(nv), None), "mc_indexed_count_levels")
    d_v, d_f = DeviceBuffer(nv.value * 12 + 64), DeviceBuffer(nt.value * 12 + 64)
    v_sel = ctypes.c_double(float(select if select is not None else 255))
    L.check(lib.ivx_dev_mc_indexed_emit_levels(ctypes.byref(p), d_s.ptr, bufs[1].ptr, ctypes.c_double(0.0), ctypes.c_double(255.0), v_sel,
                                               d_v.ptr, nv, d_f.ptr, nt, None), "mc_indexed_emit_levels")
    L.check(lib.ivx_device_synchronize())
    out = d_v.download((nv.value, 3), np.float32), d_f.download((nt.value, 3), np.int32)
    for d in bufs + [d_s, d_v, d_f]:
        d.close()
    return out


@pytest.mark.parametrize("select", [254, None])
@pytest.mark.parametrize("dx", C.LEVELS_DX)
def test_levels_path_at_rows_about_a_word(ivxlib, oracle, monkeypatch, dx, select):
    """k_mci_vertices_levels reads the selection plane in source coordinates and the inside plane in padded ones: rows of one word
    less a bit, one word, one word and a bit, and the same about two words.  The mask is a resident volume's, after threshold and
    region growing.  DeviceVolume itself proves the byte levels only where its rows are whole words (threshold: dx % 64 == 0), so
    at the other widths its own surface call IS the voxel path and the levels path is reached through the C entry points, which
    take any width; at dx = 64 both ways to the levels path are compared."""
    from invesalius3_amd import _lib as L
    from invesalius3_amd.device import DeviceVolume
    img = synth_volume((6, 9, dx), seed=C.LEVELS_SEED)
    (lo, hi), (glo, ghi) = C.LEVELS_THRESHOLD, C.LEVELS_GROW
    z, y, x = (int(v[0]) for v in np.nonzero((img >= glo) & (img <= ghi)))
    spacing = (0.5, 0.75, 2.0)
    vol = DeviceVolume(img, spacing=spacing)
    vol.zero_out_mask()
    vol.threshold(lo, hi)
    if select is not None:
        vol.region_grow([(x, y, z)], glo, ghi, S26, fill=1, select_value=select)
    assert vol._mask_levels == ((255, select) if dx % 64 == 0 else None)
    own = vol.marching_cubes_indexed(download=True) if dx % 64 == 0 else None   # the volume's own levels path
    monkeypatch.setenv("IVX_MC_LEVELS", "0")
    v0, f0 = vol.marching_cubes_indexed(download=True)          # voxel path
    mask = vol.download_mask()
    vol.close()
    assert len(f0) > 100 and set(np.unique(mask).tolist()) == ({0, 255} if select is None else {0, 254, 255})
    if select is not None:  # the grown region crosses the seam between source words 0 and 1, or ends on it
        reach = (mask == select).any(axis=(0, 1))
        assert reach[min(63, dx - 1)] and reach[dx - 1] and (dx <= 64 or reach[64])
    args = (spacing, [127.0], 0, True, True, True, 0.0, 1)
    v1, f1 = _levels_mesh(L, mask, args, select)                 # levels path
    assert v1.shape == v0.shape and f1.shape == f0.shape
    assert np.array_equal(_u32(v1), _u32(v0)) and np.array_equal(f1, f0)
    if own is not None:
        assert np.array_equal(_u32(own[0]), _u32(v0)) and np.array_equal(own[1], f0)
    rv, rf = R.indexed_mesh(mask, args, oracle.marching_cubes(mask, *args))
    assert np.array_equal(_u32(v1), _u32(rv)) and np.array_equal(f1, rf)


# ---- 4. the stitch -------------------------------------------------------------------------------------------------------------
def stitch_chain(L, pieces):
    """The C stitch API rank after rank on the default stream, in the order SlabVolume.marching_cubes_stitched queues it on every
    rank: count, indexed count, indexed emit, stitch_top_sig into one of two alternating buffers, stitch_match against the buffer
    the rank below filled (NULL on rank 0), a device copy of the rank's (vertices, dropped) pair into vd_all[rank] -- what the
    all-gather does --, then stitch_apply.  Rank r's apply reads vd_all[0 .. r] only, and the per-stream block the indexed count
    fills is consumed by the rank's own calls before the next rank's count overwrites it.
    `pieces`: [(array, McParams)] in rank order.  -> (vd (world, 2), [per rank: dict(piece=(verts, faces) of the rank's own indexed
    mesh, verts=kept vertices, faces=faces of global ids)])"""
    from invesalius3_amd.device import DeviceBuffer
    lib, world = L.lib(), len(pieces)
    nbs = []
    for _, p in pieces:
        nb = ctypes.c_size_t(0)
        L.check(lib.ivx_dev_mc_stitch_sig_bytes(ctypes.byref(p), ctypes.byref(nb)))
        nbs.append(nb.value)
    assert len(set(nbs)) == 1  # (the ranks' planes have the same rows)
    sig = (DeviceBuffer(nbs[0] + 64), DeviceBuffer(nbs[0] + 64))
    vd, vd_all = DeviceBuffer(64), DeviceBuffer(8 * world + 64)
    vd_all.zero()
    held, ranks = [sig[0], sig[1], vd, vd_all], []
    for rank, (a, p) in enumerate(pieces):
        d_s, d_a = _device_piece(L, a, p)
        nt, nv = c64(0), c64(0)
        L.check(lib.ivx_dev_mc_count(ctypes.byref(p), d_a.ptr, d_s.ptr, ctypes.byref(nt), None), "mc_count")
        L.check(lib.ivx_dev_mc_indexed_count(ctypes.byref(p), d_a.ptr, d_s.ptr, ctypes.byref(nv), None), "mc_indexed_count")
        d_v, d_o = DeviceBuffer(nv.value * 12 + 64), DeviceBuffer(nv.value * 12 + 64)
        d_f, d_f0 = DeviceBuffer(nt.value * 12 + 64), DeviceBuffer(nt.value * 12 + 64)
        L.check(lib.ivx_dev_mc_indexed_emit(ctypes.byref(p), d_a.ptr, d_s.ptr, d_v.ptr, nv, d_f.ptr, nt, None), "mc_indexed_emit")
        L.check(lib.ivx_memcpy_d2d(d_f0.ptr, d_f.ptr, ctypes.c_size_t(nt.value * 12 + 16), None))  # the local ids, kept for the checks
        top, below = sig[rank % 2], sig[(rank + 1) % 2]
        if rank < world - 1:
            L.check(lib.ivx_dev_mc_stitch_top_sig(ctypes.byref(p), d_s.ptr, top.ptr, None), "stitch_top_sig")
        nbr = below.ptr if rank > 0 else None
        L.check(lib.ivx_dev_mc_stitch_match(ctypes.byref(p), d_s.ptr, nbr, nv, vd.ptr, None), "stitch_match")
        L.check(lib.ivx_memcpy_d2d(vd_all.at(8 * rank), vd.ptr, ctypes.c_size_t(8), None))
        L.check(lib.ivx_dev_mc_stitch_apply(ctypes.byref(p), d_s.ptr, nbr, vd_all.ptr, rank, d_v.ptr, nv, d_f.ptr, nt, d_o.ptr, None),
                "stitch_apply")
        ranks.append((nv.value, nt.value, d_v, d_o, d_f, d_f0))
        held += [d_s, d_a, d_v, d_o, d_f, d_f0]
    L.check(lib.ivx_device_synchronize())
    vds = vd_all.download((world, 2), np.uint32).astype(np.int64)
    out = []
    for rank, (nv, nt, d_v, d_o, d_f, d_f0) in enumerate(ranks):
        assert vds[rank, 0] == nv and 0 <= vds[rank, 1] <= nv
        out.append(dict(piece=(d_v.download((nv, 3), np.float32), d_f0.download((nt, 3), np.int32)),
                        verts=d_o.download((int(nv - vds[rank, 1]), 3), np.float32), faces=d_f.download((nt, 3), np.int32)))
    for d in held:
        d.close()
    return vds, out


def _slab_pieces(L, c):
    """the ranks' pieces through parallel.slab_layout / slab_mc_args -> [(array, args)]"""
    from invesalius3_amd import parallel as par
    out, fbh = [], c["fill_border_holes"]
    for rank in range(c["world"]):
        lay = par.slab_layout(rank, c["world"], c["nz"])
        m = par.slab_mc_args(lay, fbh)
        lo = lay.z_global0 - lay.hb
        a = np.ascontiguousarray(c["whole"][lo + m["z0"]:lo + m["z1"]])
        out.append((a, (c["spacing"], [c["iso"]], m["roi_start"], fbh, bool(m["pad_bottom"]), bool(m["pad_top"]), c["pad_value"],
                        int(bool(m["pad_bottom"])))))
    return out


@pytest.mark.parametrize("name", list(STITCHES))
def test_stitch_chain_with_samples_on_the_iso_value(ivxlib, oracle, name):
    from invesalius3_amd import _lib as L
    from invesalius3_amd import surface_process as sp
    c = STITCHES[name]
    world = c["world"]
    pieces = _slab_pieces(L, c)
    vds, res = stitch_chain(L, [(a, _params(L, a, args)) for a, args in pieces])
    # the ranks' own pieces are the restated ones, and their stitch by float match is what the device made by edge identity
    keys, NZs = [], []
    for (a, args), r in zip(pieces, res):
        rv, rf = R.indexed_mesh(a, args, oracle.marching_cubes(a, *args))
        assert np.array_equal(_u32(r["piece"][0]), _u32(rv)) and np.array_equal(r["piece"][1], rf)
        keys.append(R.indexed_vertices(a, args[0], args[1][0], *args[2:])[1])
        NZs.append(C.geometry(a.shape, *args[3:6])[0])
    sv, sf = stitch_piece_meshes([r["piece"] for r in res])
    dv, df = np.concatenate([r["verts"] for r in res]), np.concatenate([r["faces"] for r in res])
    assert dv.shape == sv.shape and np.array_equal(_u32(dv), _u32(sv)), "stitched vertices"
    assert df.shape == sf.shape and df.dtype == sf.dtype and np.array_equal(df, sf), "stitched faces"
    # the whole volume's indexed mesh: the same triangles and the same vertices, none twice
    wv, wf = sp.marching_cubes_indexed(c["whole"], *C.stitch_whole_args(c))
    assert len(dv) == len(wv) == len(_rows(dv)) and np.array_equal(_rows(dv), _rows(wv))
    assert len(df) == len(wf) > 0 and np.array_equal(_tri_rows(dv[df]), _tri_rows(wv[wf]))
    # the copies every rank dropped: the vertices its bottom plane shares with the top plane below it
    want = [0] + [R.shared_plane_counts(keys[r - 1], keys[r], NZs[r - 1]) for r in range(1, world)]
    assert vds[:, 1].tolist() == want
    if "want_dropped" in c:
        assert want == [0, c["want_dropped"]]
    elif not c.get("blob"):
        # on-iso samples on the shared planes: point vertices among the copies
        assert all(((k[:, 0] == 0) & (k[:, 3] == R.KIND_POINT)).any() for k in keys[1:]) and all(w > 0 for w in want[1:])
    if c.get("blob"):  # the helper itself: the product's own sharded stitch of the same mask gives the same arrays
        from invesalius3_amd.parallel import SlabVolume
        img = np.where(c["whole"] > 0, 1000, -1000).astype(np.int16)
        nz = c["nz"]

        def rank_fn(rank, comm):
            vol = SlabVolume(img[rank * nz:(rank + 1) * nz], rank, world, comm=comm, spacing=c["spacing"])
            vol.threshold(500, 3071)
            got = vol.marching_cubes_stitched(from_binary=True, download=True)
            counts = dict(vol.stitch_counts)
            vol.close()
            return got, counts

        _, prod = sc.run_ranks(world, rank_fn)
        assert np.array_equal(_u32(np.concatenate([g[1] for g, _ in prod])), _u32(dv))
        assert np.array_equal(np.concatenate([g[2] for g, _ in prod]), df)
        assert [k["dropped_copies"] for _, k in prod] == want and [k["vertices"] for _, k in prod] == vds[:, 0].tolist()
