"""The bookkeeping of the count that rides on a flood's mask write (DeviceVolume.region_grow -> marching_cubes).  No GPU
in here: DeviceVolume drives it, tests/test_mc_ride_book.py holds it to its rules on the host.

A region growing that is followed by a surface call can have marching cubes' count done by the kernel that writes the mask's
bytes (ivx_dev_flood_grow_select_count).  That is speculation on the caller's NEXT call, so it is bounded:

  * a surface call that counted its piece from the inside plane ARMS the ride with that piece (the cached parameter object
    and the first slice); it leaves a triangle buffer behind, so the next one runs in steady state;
  * a region growing that rides SPENDS the arm and leaves a NOTE (piece, first slice, version of the inside plane);
  * the next surface call TAKES the note when it is for the same piece and the plane has the same version -- it skips its
    count -- and arms again; any other surface call counts as always, and arms with its own piece;
  * a ride nobody took is therefore followed by region growings that do not ride, until a surface call arms again: one hidden
    count wasted per streak of clicks at most;
  * the note dies with whatever counts into the marching-cubes scratch, replaces it, or rewrites the inside plane (the last
    through the version, as for DeviceVolume._prefetch).
"""
from __future__ import annotations


class RideBook:
    def __init__(self, enabled: bool = True):
        self.enabled = bool(enabled)
        self.armed = None   # (params, z0) of the piece the next region growing may count
        self.note = None    # (params, z0, plane version) of the piece a region growing has counted
        self.rides = 0      # region growings that counted
        self.taken = 0      # ... whose count a surface call used

    def piece_to_ride(self):
        """(params, z0) for a region growing that is about to run, or None"""
        return self.armed if self.enabled else None

    def rode(self, version: int):
        """the region growing's call has counted the armed piece from the plane of `version`"""
        self.note = (self.armed[0], self.armed[1], int(version))
        self.armed = None
        self.rides += 1

    def take(self, params, z0: int, version: int) -> bool:
        """a surface call for (params, z0) with the plane at `version`: is its count done?  The note is spent either way."""
        n, self.note = self.note, None
        ok = n is not None and n[0] is params and n[1] == z0 and n[2] == int(version)
        self.taken += int(ok)
        return ok

    def drop(self):
        """the marching-cubes scratch is about to hold something else (or to go)"""
        self.note = None

    def surface_counted(self, params, z0: int, from_plane: bool):
        """a surface call has a counted piece in the scratch (its own count, or the note's)"""
        self.armed = (params, z0) if (self.enabled and from_plane) else None
