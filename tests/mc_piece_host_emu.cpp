// mc_piece_host_emu.cpp -- drives csrc/mc_piece.h (what the library remembers about the piece counted into a marching-cubes
// scratch block) on the CPU.  Reads one command per line from the file named by argv[1] and answers each with one line on
// stdout (tests/test_mc_piece_host.py writes the commands and compares the answers):
//   count S [PLANE]     -> "ok"            a count begins on scratch S [with the caller's inside plane]
//   split S N           -> "ok"            the total was read: N iso-0 triangles
//   vsplit S N          -> "ok"            the indexed count ran: N iso-0 vertices
//   getsplit S          -> "N" | "none"
//   getvsplit S         -> "N" | "none"
//   plane S Q           -> "PLANE" | "0"   the caller's plane for iso-value Q
//   built S LIST CAP    -> "ok"            the list pass filled buffer LIST with room for CAP triangles
//   ready S LIST CAP    -> "1" | "0"       may a pass that reads CAP triangles from LIST skip the list pass?
// All numbers are decimal.  Memory is never dereferenced: addresses are just numbers here.
#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#include "../invesalius3_amd/csrc/mc_piece.h"

static const void *addr(uint64_t v) { return (const void *)(uintptr_t)v; }

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
    ivx::McPieces &t = ivx::mc_pieces();
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string cmd;
        uint64_t s = 0, a = 0, b = 0;
        if (!(ss >> cmd) || cmd[0] == '#') continue;
        ss >> s >> a >> b; // (missing numbers stay 0)
        if (cmd == "count") {
            t.begin_count(addr(s), (const uint64_t *)addr(a));
            printf("ok\n");
        } else if (cmd == "split") {
            t.set_split(addr(s), a);
            printf("ok\n");
        } else if (cmd == "vsplit") {
            t.set_vsplit(addr(s), (uint32_t)a);
            printf("ok\n");
        } else if (cmd == "getsplit") {
            uint64_t v;
            if (t.get_split(addr(s), &v)) printf("%" PRIu64 "\n", v);
            else
                printf("none\n");
        } else if (cmd == "getvsplit") {
            uint32_t v;
            if (t.get_vsplit(addr(s), &v)) printf("%" PRIu32 "\n", v);
            else
                printf("none\n");
        } else if (cmd == "plane") {
            printf("%" PRIu64 "\n", (uint64_t)(uintptr_t)t.ext_plane(addr(s), (int)a));
        } else if (cmd == "built") {
            t.list_built(addr(s), addr(a), (int64_t)b);
            printf("ok\n");
        } else if (cmd == "ready") {
            printf("%d\n", t.list_ready(addr(s), addr(a), (int64_t)b) ? 1 : 0);
        } else {
            fprintf(stderr, "unknown command: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
