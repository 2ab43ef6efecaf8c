"""Host only: the arm / ride / take bookkeeping of the count that rides on a flood's mask write (invesalius3_amd/mc_ride.py)."""
from invesalius3_amd.mc_ride import RideBook


class _P:  # stands for a cached McParams object: the book compares identities
    pass


def test_arm_ride_take_and_arm_again():
    b, p = RideBook(True), _P()
    assert b.piece_to_ride() is None  # nothing rides before a surface call
    b.surface_counted(p, 0, True)
    assert b.piece_to_ride() == (p, 0)
    b.rode(7)
    assert b.piece_to_ride() is None and b.note == (p, 0, 7) and b.rides == 1
    assert b.take(p, 0, 7) and b.taken == 1 and b.note is None
    b.surface_counted(p, 0, True)
    assert b.piece_to_ride() == (p, 0)


def test_unused_ride_disarms_until_a_surface_call():
    b, p = RideBook(True), _P()
    b.surface_counted(p, 0, True)
    b.rode(1)
    assert b.piece_to_ride() is None  # the next click does not ride
    assert b.piece_to_ride() is None  # ... nor the one after
    assert not b.take(p, 0, 2)        # the plane has moved on: the surface call counts itself
    b.surface_counted(p, 0, True)
    assert b.piece_to_ride() == (p, 0) and b.rides == 1 and b.taken == 0


def test_note_matches_piece_slice_and_version_and_is_spent_once():
    p, q = _P(), _P()
    for args in ((q, 0, 3), (p, 1, 3), (p, 0, 4)):
        b = RideBook(True)
        b.surface_counted(p, 0, True)
        b.rode(3)
        assert not b.take(*args)
        assert b.note is None and not b.take(p, 0, 3)  # a refused note is gone too
    b = RideBook(True)
    b.surface_counted(p, 0, True)
    b.rode(3)
    b.drop()
    assert not b.take(p, 0, 3) and b.taken == 0


def test_not_from_the_plane_and_switched_off():
    b, p = RideBook(True), _P()
    b.surface_counted(p, 0, True)
    b.surface_counted(p, 0, False)  # a surface call that read the voxels: nothing to ride on
    assert b.piece_to_ride() is None
    off = RideBook(False)
    off.surface_counted(p, 0, True)
    assert off.piece_to_ride() is None and off.armed is None
