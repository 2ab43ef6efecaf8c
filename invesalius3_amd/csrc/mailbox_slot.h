// mailbox_slot.h -- the arithmetic of the GPU -> host mailbox ring (ivx_runtime.hip), host only and free of HIP, so that
// tests/mailbox_slot_host.cpp can hold it against a ring it simulates on the CPU.
//
// Sequence numbers are handed out in order 1, 2, ..., 2^32 - 1, 1, 2, ...: the counter wraps and 0 is skipped (a slot's word 63
// starts as 0, and 0 doubles as "no number reserved").  Number s lives in slot s & 63 of 64.
#pragma once
#include <stdint.h>

namespace ivx {

constexpr uint32_t MAILBOX_SLOTS = 64;

inline uint32_t mailbox_next_seq(uint32_t newest) {
    ++newest;
    return newest ? newest : 1u;
}

inline uint32_t mailbox_slot_of(uint32_t seq) { return seq & (MAILBOX_SLOTS - 1); }

// Is `seq` still the newest number handed out for its slot, `newest` being the newest number handed out at all (at or after
// `seq`, fewer than 2^32 - 128 numbers later)?  The slot's next owner is seq + 64 -- or, when that sum wraps to the skipped 0,
// seq + 128.  A `false` means the slot's words may be another message's by now: whoever still wants `seq`'s has to fetch
// them another way.
inline bool mailbox_seq_in_slot(uint32_t seq, uint32_t newest) {
    if (seq == 0) return false;
    const uint32_t d = newest - seq; // (mod 2^32: right across the wrap)
    const uint32_t next_owner = seq + MAILBOX_SLOTS == 0 ? 2 * MAILBOX_SLOTS : MAILBOX_SLOTS;
    return d < next_owner;
}

} // namespace ivx
