// resident_ranges.h -- the host-only half of the resident-array registry: byte extents of strided views,
// containment and overlap of byte ranges, the list of host-written intervals that wait for their re-upload, and the table
// of registrations with its valid / stale / released states.  No HIP in here: ivx_runtime.hip adds the device mirror and
// the copies, tests/resident_host_emu.cpp drives the same code on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <map>
#include <vector>

namespace ivx {
namespace resident {

// Byte extent [lo, hi) of an nd-dimensional view at `p` with signed byte strides.  An axis of length 1 contributes nothing,
// whatever its stride.  Returns false for a view that cannot be served from a mirror: an empty one (nothing to serve) and
// one that repeats bytes through a zero stride on an axis longer than 1 (a broadcast view is nobody's registered memory).
static inline bool view_extent(uintptr_t p, const int64_t *shape, const int64_t *st, int nd, size_t isz, uintptr_t *lo,
                               uintptr_t *hi) {
    int64_t below = 0, above = 0;
    for (int a = 0; a < nd; a++) {
        if (shape[a] <= 0) return false;
        if (shape[a] == 1) continue;
        if (st[a] == 0) return false;
        const int64_t reach = (shape[a] - 1) * st[a];
        if (reach < 0) below += reach;
        else
            above += reach;
    }
    *lo = p + (uintptr_t)below; // (below <= 0: modular arithmetic does the subtraction)
    *hi = p + (uintptr_t)above + isz;
    return true;
}

static inline bool contains(uintptr_t lo, uintptr_t hi, uintptr_t inner_lo, uintptr_t inner_hi) {
    return inner_lo >= lo && inner_hi <= hi && inner_lo <= inner_hi;
}
static inline bool overlaps(uintptr_t a_lo, uintptr_t a_hi, uintptr_t b_lo, uintptr_t b_hi) {
    return a_lo < b_hi && b_lo < a_hi;
}

struct Interval {
    size_t lo, hi; // [lo, hi), offsets into the registered range
};

// Sorted, disjoint, non-adjacent intervals: what the host wrote (or the library wrote past the mirror) since the last refresh.
struct IntervalList {
    std::vector<Interval> v;

    void add(size_t lo, size_t hi) {
        if (lo >= hi) return;
        std::vector<Interval> out;
        out.reserve(v.size() + 1);
        bool placed = false;
        for (const Interval &i : v) {
            if (i.hi < lo) out.push_back(i);
            else if (hi < i.lo) {
                if (!placed) out.push_back(Interval{lo, hi}), placed = true;
                out.push_back(i);
            } else { // overlapping or adjacent: grow the newcomer
                lo = std::min(lo, i.lo);
                hi = std::max(hi, i.hi);
            }
        }
        if (!placed) out.push_back(Interval{lo, hi});
        v.swap(out);
    }
    size_t bytes() const {
        size_t n = 0;
        for (const Interval &i : v) n += i.hi - i.lo;
        return n;
    }
    bool empty() const { return v.empty(); }
    void clear() { v.clear(); }
};

enum State { VALID = 0, STALE = 1, RELEASED = 2 };
enum { ST_HITS = 0, ST_HIT_BYTES, ST_REFRESHES, ST_REFRESH_BYTES, ST_WRITES, ST_WRITE_BYTES, ST_INVALIDATIONS, ST_GENERATION, ST_COUNT };

struct Range {
    uintptr_t base = 0;
    size_t nbytes = 0;
    int device = 0;
    uint64_t generation = 0; // also the handle: never reused, so a released handle can only miss
    void *mirror = nullptr;  // device copy of [base, base + nbytes) (owned by ivx_runtime.hip)
    IntervalList pending;    // mirror bytes that are older than the host's
    uint64_t stats[ST_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0};

    State state() const { return pending.empty() ? VALID : STALE; }
    uintptr_t end() const { return base + nbytes; }
};

enum { RES_OK = 0, RES_EINVAL = -1 };

// The table.  Not locked: the owner serialises every call (ivx_runtime.hip holds its registry lock around each of them and
// around the copies that use what they return, which is what makes a release wait for a copy in flight).
struct Registry {
    std::map<uintptr_t, Range> by_base; // disjoint ranges, so ordered by base == ordered by end
    std::map<uint64_t, uintptr_t> by_handle;
    uint64_t next_generation = 1;

    size_t count() const { return by_base.size(); }

    // refuses empty ranges, ranges that wrap around, and any overlap with a live registration (of any device: one host
    // range has one mirror)
    int add(uintptr_t base, size_t nbytes, int device, uint64_t *handle) {
        if (!base || !nbytes || base + nbytes < base) return RES_EINVAL;
        for (const auto &kv : by_base)
            if (overlaps(base, base + nbytes, kv.second.base, kv.second.end())) return RES_EINVAL;
        Range r;
        r.base = base;
        r.nbytes = nbytes;
        r.device = device;
        r.generation = next_generation++;
        r.stats[ST_GENERATION] = r.generation;
        by_base[base] = r;
        by_handle[r.generation] = base;
        *handle = r.generation;
        return RES_OK;
    }

    Range *get(uint64_t handle) {
        auto it = by_handle.find(handle);
        return it == by_handle.end() ? nullptr : &by_base[it->second];
    }

    State state(uint64_t handle) {
        Range *r = get(handle);
        return r ? r->state() : RELEASED;
    }

    // forgets the registration (the caller frees r->mirror first)
    int release(uint64_t handle) {
        auto it = by_handle.find(handle);
        if (it == by_handle.end()) return RES_EINVAL;
        by_base.erase(it->second);
        by_handle.erase(it);
        return RES_OK;
    }

    // the registration of `device` that holds ALL of [lo, hi), or nullptr
    Range *find_containing(uintptr_t lo, uintptr_t hi, int device) {
        if (by_base.empty() || lo >= hi) return nullptr;
        auto it = by_base.upper_bound(lo);
        if (it == by_base.begin()) return nullptr;
        --it;
        Range &r = it->second;
        return (r.device == device && contains(r.base, r.end(), lo, hi)) ? &r : nullptr;
    }

    // "the host wrote [off, off + n) of this registration": EINVAL for a dead handle and for a range that leaves it
    int touch(uint64_t handle, size_t off, size_t n) {
        Range *r = get(handle);
        if (!r || off > r->nbytes || n > r->nbytes - off) return RES_EINVAL;
        r->pending.add(off, off + n);
        return RES_OK;
    }

    // The library wrote host bytes [lo, hi) without writing the mirrors (a write that no single registration of this device
    // holds completely): every registration it overlaps is stale in exactly the overlap.  Returns how many were marked.
    int invalidate(uintptr_t lo, uintptr_t hi) {
        int n = 0;
        for (auto &kv : by_base) {
            Range &r = kv.second;
            if (!overlaps(lo, hi, r.base, r.end())) continue;
            const uintptr_t a = std::max(lo, r.base), b = std::min(hi, r.end());
            r.pending.add(a - r.base, b - r.base);
            r.stats[ST_INVALIDATIONS]++;
            n++;
        }
        return n;
    }
};

} // namespace resident
} // namespace ivx
