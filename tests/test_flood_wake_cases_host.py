"""The cases of tests/_flood_wake_cases.py hold what their docstrings say, on the CPU: the references agree with each other
and with the oracle's flood, every contact connects exactly when a step of the structuring element says so, and the rounds
restated in numpy give the counts the GPU tests quote."""
import numpy as np
import pytest

import _flood_wake_cases as wc

S = {"26": wc.fc.structure(3), "18": wc.fc.structure(2), "6": wc.fc.structure(1), "asym": wc.asym_structure()}
PARTIAL = ((40, 40, 100), (1, 1, 0))


def _flood(fn, case, *a):
    (_, seeds, fill), = case.floods
    out = case.out0.copy()
    fn(case.img, seeds, fill, *a, out)
    return out


@pytest.mark.parametrize("key", [(), PARTIAL])
def test_contacts_connect_by_the_structuring_element(oracle, key):
    case = wc.contacts_case(*key)
    assert len(case.facts["contacts"]) == (26 if not key else 17)
    (_, seeds, fill), = case.floods
    reached_any = {}
    for name, s in S.items():
        ref = _flood(wc.propagate_flood, case, s)
        if name != "asym":
            assert np.array_equal(ref, _flood(wc.label_flood, case, {"6": 1, "18": 2, "26": 3}[name])), name
        orc = case.out0.copy()
        oracle.floodfill_threshold(case.img, seeds, wc.T0, wc.T1, fill, s, orc)
        assert np.array_equal(ref, orc), name
        body = case.img[tuple(slice(l, h + 1) for l, h in zip(case.facts["lo"], case.facts["hi"]))] == wc.VAL
        assert ref[tuple(slice(l, h + 1) for l, h in zip(case.facts["lo"], case.facts["hi"]))][body].all(), name
        ok = wc.contacts_reached(case, s)
        for d, (v, tail) in case.facts["contacts"].items():
            assert bool(ref[v]) == ok[d], (name, d)
            if name != "asym":
                assert all(bool(ref[p]) == ok[d] for p in tail), (name, d)
        reached_any[name] = sum(ok.values())
    n = len(case.facts["contacts"])
    faces = sum(1 for d in case.facts["contacts"] if sum(map(abs, d)) == 1)
    edges = sum(1 for d in case.facts["contacts"] if sum(map(abs, d)) == 2)
    assert reached_any["26"] == n and reached_any["6"] == faces and reached_any["18"] == faces + edges
    assert faces + edges < reached_any["asym"] < n  # the corner (+1, +1, +1) is the step it lacks


def test_stale_halo_bodies_are_one_component():
    case = wc.stale_halo_case()
    ref = _flood(wc.label_flood, case, 3)
    assert all(ref[v].all() for v in case.bodies.values())
    only_a1 = case.img.copy()
    only_a1[case.bodies["B1"]] = 0
    cut = wc.Case(only_a1, case.out0.copy(), case.floods)
    out = _flood(wc.label_flood, cut, 3)
    assert out[case.bodies["A1"]].all() and not out[case.bodies["A2"]].any() and not out[case.bodies["B2"]].any()


@pytest.mark.parametrize("axis", [1, 0])
def test_no_wake_case_counts(axis):
    case = wc.no_wake_case(axis)
    (_, seeds, _), = case.floods
    ref = _flood(wc.label_flood, case, 3)
    r_open = wc.model_rounds(case.img, seeds, "open")
    r_faces = wc.model_rounds(case.img, seeds, "faces")
    assert r_open[:3] == (1, 27, 27) and r_faces[:3] == (2, 28, 27)
    assert np.array_equal(r_open[3], ref != 0) and np.array_equal(r_faces[3], ref != 0)
    assert 0 < int((ref != 0).sum()) < int((case.img == wc.VAL).sum()) // 2  # one body of three


def test_chain_case_counts():
    case = wc.chain_case()
    (_, seeds, _), = case.floods
    ref = _flood(wc.label_flood, case, 3)
    assert np.array_equal(ref != 0, case.img == wc.VAL)
    tiles = {(z // wc.TZ, y // wc.TY, x // wc.TX) for z, y, x in np.argwhere(case.img == wc.VAL)}
    assert tiles == set(wc.CHAIN)
    rounds, visits, first, reached = wc.model_rounds(case.img, seeds, "open")
    assert (rounds, visits, first) == (9, 12 + 8, 12) and np.array_equal(reached, ref != 0)
    # (the rule before this one counts the same here: the tile behind a visit is closed by then, nobody can wake it)
    assert wc.model_rounds(case.img, seeds, "faces")[:3] == (rounds, visits, first)
