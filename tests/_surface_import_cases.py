"""Soups that put the weld's hash table (csrc/k_meshweld.hip) where it can go wrong, built by search: the hash of
csrc/mesh_weld_math.h is restated here, and every case is searched for at the slot count the library reports for its size
(ivx_mesh_weld_slots, host only).  tests/test_surface_import_host.py proves each property on this restatement alone and checks
the restatement against the header built for the host; tests/test_gpu_surface_import.py runs the cases."""
import numpy as np

import _surface_import_ref as ref

M64 = (1 << 64) - 1


def fmix64(k: int) -> int:
    k ^= k >> 33
    k = (k * 0xFF51AFD7ED558CCD) & M64
    k ^= k >> 33
    k = (k * 0xC4CEB9FE1A85EC53) & M64
    k ^= k >> 33
    return k


def hash32(kx: int, ky: int, kz: int) -> int:
    """mesh_weld_math.h hash(): 96 key bits -> 32"""
    k = fmix64((ky << 32) | kx)
    k ^= (kz * 0x9E3779B97F4A7C15) & M64
    return fmix64(k) & 0xFFFFFFFF


def slots_for(n_corners: int) -> int:
    """mesh_weld_math.h slots(): the power of two >= 2 * corners, at least 2"""
    s = 2
    while s < 2 * n_corners:
        s <<= 1
    return s


def lib_slots(n_corners: int) -> int:
    from invesalius3_amd import surface
    return surface.weld_slots(n_corners)


def homes(soup, slots: int) -> dict:
    """home slot -> set of the distinct keys of the soup that start there"""
    out = {}
    for k in set(ref.keys_of(soup)):
        out.setdefault(hash32(*k) & (slots - 1), set()).add(k)
    return out


def _candidates(rng, n):
    return (rng.integers(-4096, 4096, (n, 3)).astype(np.float64) / 8.0).astype(np.float32)


def _points_at(slots, count, home, seed, avoid=()):
    """`count` points with different keys that all start at slot `home` (None: whichever slot fills first)"""
    rng = np.random.default_rng(seed)
    seen, by_home = set(avoid), {}
    for _ in range(200):
        pts = _candidates(rng, 4096)
        for p, k in zip(pts, ref.keys_of(pts)):
            if k in seen:
                continue
            seen.add(k)
            h = hash32(*k) & (slots - 1)
            if home is not None and h != home:
                continue
            got = by_home.setdefault(h, [])
            got.append(p)
            if len(got) == count:
                return np.array(got, np.float32)
    raise AssertionError("no %d keys found for one home slot of %d" % (count, slots))


def _fill(points, ntris, seed):
    """`ntris` triangles over `points` and as many fresh filler points as it takes for 12 different ones: triangle t takes the
    points t, t + 1, t + 5 (mod 12), so every point is used by several facets and no facet is degenerate"""
    rng = np.random.default_rng(seed)
    have = set(ref.keys_of(points))
    pool = [p for p in points]
    while len(pool) < 12:
        p = _candidates(rng, 1)[0]
        k = ref.keys_of(p[None])[0]
        if k not in have:
            have.add(k)
            pool.append(p)
    pool = np.array(pool, np.float32)
    idx = np.array([[t % 12, (t + 1) % 12, (t + 5) % 12] for t in range(ntris)])
    return np.ascontiguousarray(pool[idx])


def cluster_case(ntris=10, seed=1):
    """at least 4 different keys share one home slot: the later ones walk past the earlier ones' slots"""
    slots = lib_slots(3 * ntris)
    return _fill(_points_at(slots, 4, None, seed), ntris, seed), slots


def wrap_case(ntris=10, seed=2):
    """at least 2 different keys have the LAST slot as home: the second walks on to slot 0"""
    slots = lib_slots(3 * ntris)
    return _fill(_points_at(slots, 2, slots - 1, seed), ntris, seed), slots


def zero_sign_case():
    """(-0.0, 1, 2) first and (0.0, 1, 2) later: one vertex, and it keeps -0.0"""
    s = np.array([[[-0.0, 1, 2], [3, 4, 5], [6, 7, 8]],
                  [[0.0, 1, 2], [6, 7, 8], [9, -0.0, 1]],
                  [[9, 0.0, 1], [0.0, 1, 2], [3, 4, 5]]], np.float32)
    return s


def distinct_case(ntris):
    """3 T corners, all different: the scan of the representative flags runs over exactly 3 T ones (4095 and 4098 for T = 1365
    and 1366: either side of scan_u32.h's 4096-element block)"""
    n = 3 * ntris
    j = np.arange(n, dtype=np.float32)
    return np.stack([j, (j * 7.0) % 13.0, -j], axis=1).reshape(ntris, 3, 3)


def identical_case(ntris=700):
    return np.tile(np.array([1.5, -2.25, 3.0], np.float32), (ntris, 3, 1))


def repeated_case(ntris=100):
    """one point at corners 0, 63, 64, 255, 256 and the last, every other corner different: equal keys across wave and workgroup edges"""
    s = distinct_case(ntris).reshape(-1, 3).copy()
    s += np.float32(0.5)
    for j in (0, 63, 64, 255, 256, len(s) - 1):
        s[j] = (-7.0, -7.0, -7.0)
    return s.reshape(ntris, 3, 3)


def degenerate_case():
    """degenerate facets first, last and two adjacent ones in the middle, between good facets whose order must survive"""
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1], [2, 0, 0], [0, 2, 0], [5, 5, 5]], np.float32)
    idx = [[7, 7, 0],  # degenerate, first; its point 7 appears nowhere else and stays in the list
           [0, 1, 2], [1, 2, 3],
           [2, 3, 2], [4, 4, 4],  # adjacent degenerate facets
           [3, 4, 5], [6, 5, 4],
           [1, 6, 1]]  # degenerate, last
    return np.ascontiguousarray(p[np.array(idx)])
