// mc_piece.h -- what the library remembers, on the host, about the piece last COUNTED into a marching-cubes scratch block:
// one record per scratch address.  No HIP in here: k_mc.hip (triangle soup) and k_mci.hip (indexed mesh, stitch) share the one
// table below, tests/mc_piece_host_emu.cpp drives the same code on the CPU.
//
// The rules, all of them:
//   * EVERY count (ivx_dev_mc_count, _count_async, _count_bits, _count_bits_async, and through them the host forms) begins
//     with begin_count(), which resets the WHOLE record before it sets anything: the external plane, the triangle list, the
//     iso-0 / iso-1 split and the vertex split of whatever piece was counted there before are void.  A call that needs one of
//     them and does not find it refuses (IVX_EINVAL, "... must follow ..."); it never works on an older piece's value.  So a
//     scratch address that is freed and handed out again cannot see its previous owner's state either: the table keeps one
//     small record per distinct address and there is nothing to forget.
//   * the external plane: ivx_dev_mc_count_bits hands in the inside plane of iso 0 instead of having it derived into the
//     scratch; the later passes of the same piece read it in place.  There is none for iso 1.
//   * the split (number of iso-0 triangles of a two-iso piece) is set when the total is read: ivx_dev_mc_total, and the
//     counts that return the total themselves.
//   * the vertex split (number of iso-0 vertices) is set by ivx_dev_mc_indexed_count*.
//   * the pending total: the scan of a one-iso count publishes the total through a mailbox slot reserved for it; the record
//     keeps the slot's sequence number (0: none) for ivx_dev_mc_total_early and the counts that return the total.  The next
//     count on the scratch clears it with the rest; the slot itself is recycled by the ring, which the reader checks.
//   * the triangle list: ivx_dev_mc_list fills a list buffer -- a per-stream workspace that every piece on that stream shares
//     -- ahead of the emit.  The list is "ready" for a later pass when it is the same buffer that was filled for this scratch,
//     with room for at least what is asked now, and the buffer still belongs to this scratch.  A negative answer means the
//     caller fills the buffer itself next, for no one to find: the buffer loses its owner.
#pragma once
#include <stdint.h>

#include <map>
#include <mutex>

namespace ivx {

struct McPiece {
    const uint64_t *ext_bits = nullptr; // inside plane of iso 0 handed in by the caller, or nullptr: it is in the scratch
    bool has_split = false;
    uint64_t split = 0;                 // number of iso-0 triangles
    bool has_vsplit = false;
    uint32_t vsplit = 0;                // number of iso-0 vertices
    const void *list = nullptr;         // list buffer filled ahead of the emit, with room for list_cap triangles
    int64_t list_cap = 0;
    uint32_t total_seq = 0;             // mailbox number under which this count's scan publishes the total itself, or 0
};

class McPieces {
  public:
    void begin_count(const void *scratch, const uint64_t *ext_bits = nullptr) {
        std::lock_guard<std::mutex> lk(mu_);
        McPiece &r = by_scratch_[scratch];
        r = McPiece();
        r.ext_bits = ext_bits;
    }
    void set_total_seq(const void *scratch, uint32_t seq) {
        std::lock_guard<std::mutex> lk(mu_);
        by_scratch_[scratch].total_seq = seq;
    }
    // the pending mailbox number of the piece counted into `scratch`, or 0
    uint32_t total_seq(const void *scratch) {
        std::lock_guard<std::mutex> lk(mu_);
        auto it = by_scratch_.find(scratch);
        return it == by_scratch_.end() ? 0u : it->second.total_seq;
    }
    void set_split(const void *scratch, uint64_t split) {
        std::lock_guard<std::mutex> lk(mu_);
        McPiece &r = by_scratch_[scratch];
        r.has_split = true;
        r.split = split;
    }
    void set_vsplit(const void *scratch, uint32_t vsplit) {
        std::lock_guard<std::mutex> lk(mu_);
        McPiece &r = by_scratch_[scratch];
        r.has_vsplit = true;
        r.vsplit = vsplit;
    }
    bool get_split(const void *scratch, uint64_t *split) {
        std::lock_guard<std::mutex> lk(mu_);
        auto it = by_scratch_.find(scratch);
        if (it == by_scratch_.end() || !it->second.has_split) return false;
        *split = it->second.split;
        return true;
    }
    bool get_vsplit(const void *scratch, uint32_t *vsplit) {
        std::lock_guard<std::mutex> lk(mu_);
        auto it = by_scratch_.find(scratch);
        if (it == by_scratch_.end() || !it->second.has_vsplit) return false;
        *vsplit = it->second.vsplit;
        return true;
    }
    // the plane the caller handed in for iso-value `q` of the piece counted into `scratch`, or nullptr
    const uint64_t *ext_plane(const void *scratch, int q) {
        if (q != 0) return nullptr;
        std::lock_guard<std::mutex> lk(mu_);
        auto it = by_scratch_.find(scratch);
        return it == by_scratch_.end() ? nullptr : it->second.ext_bits;
    }
    void list_built(const void *scratch, const void *list, int64_t cap) {
        std::lock_guard<std::mutex> lk(mu_);
        McPiece &r = by_scratch_[scratch];
        r.list = list;
        r.list_cap = cap;
        list_owner_[list] = scratch;
    }
    // may the list pass be skipped?  (if not, the caller is about to overwrite `list`)
    bool list_ready(const void *scratch, const void *list, int64_t cap) {
        std::lock_guard<std::mutex> lk(mu_);
        auto it = by_scratch_.find(scratch);
        auto ow = list_owner_.find(list);
        const bool ok = list && it != by_scratch_.end() && it->second.list == list && cap <= it->second.list_cap &&
                        ow != list_owner_.end() && ow->second == scratch;
        if (!ok) list_owner_[list] = nullptr;
        return ok;
    }

  private:
    std::mutex mu_;
    std::map<const void *, McPiece> by_scratch_;
    std::map<const void *, const void *> list_owner_; // list buffer -> the scratch whose descriptors it holds
};

// the library's one table (one instance, whichever translation units include this header)
inline McPieces &mc_pieces() {
    static McPieces t;
    return t;
}

} // namespace ivx
