// csrc/mask_history_math.h built with the host compiler (tests/test_history_host.py).  One query per line on stdin:
//   H n                         -> B W literal_offset base_offset header_bytes
//   B n block                   -> word bit block_len
//   P base literal_hex bit      -> pool slot, pool byte offset
//   O offset len plane_bytes    -> block of the offset, its plane, first and last plane of [offset, offset + len)
#include <stdio.h>

#include "../invesalius3_amd/csrc/mask_history_math.h"

namespace mh = ivx_mask_history;

int main() {
    char kind;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 'H') {
            long long n;
            if (scanf("%lld", &n) != 1) return 1;
            printf("%lld %lld %lld %lld %lld\n", (long long)mh::blocks_of(n), (long long)mh::words_of(n), (long long)mh::literal_offset(n),
                   (long long)mh::base_offset(n), (long long)mh::header_bytes(n));
        } else if (kind == 'B') {
            long long n, b;
            if (scanf("%lld %lld", &n, &b) != 2) return 1;
            printf("%lld %d %d\n", (long long)mh::block_word(b), mh::block_bit(b), mh::block_len(b, n));
        } else if (kind == 'P') {
            unsigned base;
            unsigned long long lit;
            int bit;
            if (scanf("%u %llx %d", &base, &lit, &bit) != 3) return 1;
            printf("%lld %lld\n", (long long)mh::pool_slot(base, lit, bit), (long long)mh::pool_offset(base, lit, bit));
        } else if (kind == 'O') {
            long long off, len, pb;
            if (scanf("%lld %lld %lld", &off, &len, &pb) != 3) return 1;
            int64_t first, last;
            mh::planes_of_range(off, len, pb, &first, &last);
            printf("%lld %lld %lld %lld\n", (long long)mh::block_of_offset(off), (long long)mh::plane_of(off, pb), (long long)first, (long long)last);
        } else {
            return 2;
        }
    }
    return 0;
}
