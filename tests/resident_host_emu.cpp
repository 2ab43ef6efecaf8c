// resident_host_emu.cpp -- drives csrc/resident_ranges.h (the host-only half of the resident-array registry) on the CPU.
// Reads one command per line from the file named by argv[1] and answers each with one line on stdout
// (tests/test_resident_host.py writes the commands and compares the answers with numpy's own arithmetic):
//   extent P ISZ ND  N.. S..      -> "ok LO HI" | "none"            byte extent of a view
//   contains LO HI ILO IHI        -> "1" | "0"
//   reg BASE NBYTES DEV           -> "ok HANDLE" | "einval"
//   find LO HI DEV                -> "HANDLE" | "0"                 registration that holds all of [LO, HI)
//   touch HANDLE OFF N            -> "ok" | "einval"
//   write LO HI                   -> "N"                            a library write no mirror received: N ranges marked
//   pending HANDLE                -> "lo:hi lo:hi ..." | "-" | "einval"
//   refresh HANDLE                -> "BYTES" | "einval"             what a refresh would upload; empties the list
//   state HANDLE                  -> "valid" | "stale" | "released"
//   stats HANDLE                  -> eight numbers | "einval"
//   release HANDLE                -> "ok" | "einval"
//   count                         -> "N"
// All numbers are decimal.  Memory is never dereferenced: addresses are just numbers here.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "../invesalius3_amd/csrc/resident_ranges.h"

using namespace ivx::resident;

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s commands.txt\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    Registry reg;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string cmd;
        if (!(ss >> cmd) || cmd[0] == '#') continue;
        if (cmd == "extent") {
            uint64_t p, isz;
            int nd;
            int64_t shape[8], st[8];
            ss >> p >> isz >> nd;
            if (nd < 0 || nd > 8) return 2;
            for (int i = 0; i < nd; i++) ss >> shape[i];
            for (int i = 0; i < nd; i++) ss >> st[i];
            uintptr_t lo, hi;
            if (view_extent((uintptr_t)p, shape, st, nd, (size_t)isz, &lo, &hi)) printf("ok %" PRIu64 " %" PRIu64 "\n", (uint64_t)lo, (uint64_t)hi);
            else
                printf("none\n");
        } else if (cmd == "contains") {
            uint64_t a, b, c, d;
            ss >> a >> b >> c >> d;
            printf("%d\n", contains((uintptr_t)a, (uintptr_t)b, (uintptr_t)c, (uintptr_t)d) ? 1 : 0);
        } else if (cmd == "reg") {
            uint64_t base, n, h = 0;
            int dev;
            ss >> base >> n >> dev;
            if (reg.add((uintptr_t)base, (size_t)n, dev, &h) == RES_OK) printf("ok %" PRIu64 "\n", h);
            else
                printf("einval\n");
        } else if (cmd == "find") {
            uint64_t lo, hi;
            int dev;
            ss >> lo >> hi >> dev;
            Range *r = reg.find_containing((uintptr_t)lo, (uintptr_t)hi, dev);
            printf("%" PRIu64 "\n", r ? r->generation : (uint64_t)0);
        } else if (cmd == "touch") {
            uint64_t h, off, n;
            ss >> h >> off >> n;
            printf("%s\n", reg.touch(h, (size_t)off, (size_t)n) == RES_OK ? "ok" : "einval");
        } else if (cmd == "write") {
            uint64_t lo, hi;
            ss >> lo >> hi;
            printf("%d\n", reg.invalidate((uintptr_t)lo, (uintptr_t)hi));
        } else if (cmd == "pending" || cmd == "refresh" || cmd == "stats") {
            uint64_t h;
            ss >> h;
            Range *r = reg.get(h);
            if (!r) printf("einval\n");
            else if (cmd == "pending") {
                if (r->pending.empty()) printf("-");
                for (size_t i = 0; i < r->pending.v.size(); i++) printf("%s%zu:%zu", i ? " " : "", r->pending.v[i].lo, r->pending.v[i].hi);
                printf("\n");
            } else if (cmd == "refresh") {
                printf("%zu\n", r->pending.bytes());
                r->pending.clear();
            } else {
                for (int i = 0; i < ST_COUNT; i++) printf("%s%" PRIu64, i ? " " : "", r->stats[i]);
                printf("\n");
            }
        } else if (cmd == "state") {
            uint64_t h;
            ss >> h;
            const State s = reg.state(h);
            printf("%s\n", s == VALID ? "valid" : s == STALE ? "stale" : "released");
        } else if (cmd == "release") {
            uint64_t h;
            ss >> h;
            printf("%s\n", reg.release(h) == RES_OK ? "ok" : "einval");
        } else if (cmd == "count") {
            printf("%zu\n", reg.count());
        } else {
            fprintf(stderr, "unknown command: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
