// mailbox_slot_host.cpp -- drives csrc/mailbox_slot.h (the arithmetic of the GPU -> host mailbox ring) on the CPU.  Reads one
// command per line from the file named by argv[1] and answers each with one line on stdout (tests/test_mailbox_slot_host.py
// writes the commands and compares the answers):
//   next N              -> the sequence number handed out after N
//   slot S              -> the slot of sequence number S
//   live S NEWEST       -> "1" | "0"   is S still the newest number of its slot when NEWEST is the newest one handed out?
//   sim START STEPS     -> "ok" | "seq S newest N rule R ring Q"
//                          a ring simulated slot by slot: numbers are handed out STEPS times beginning behind START, every
//                          number takes its slot, and after each hand-out the rule is held against the ring for the last 200
//                          numbers handed out
// All numbers are decimal and unsigned 32-bit.
#include <cinttypes>
#include <cstdio>
#include <deque>
#include <fstream>
#include <sstream>
#include <string>

#include "../invesalius3_amd/csrc/mailbox_slot.h"

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
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string cmd;
        uint64_t a = 0, b = 0;
        if (!(ss >> cmd) || cmd[0] == '#') continue;
        ss >> a >> b; // (missing numbers stay 0)
        if (cmd == "next") {
            printf("%" PRIu32 "\n", ivx::mailbox_next_seq((uint32_t)a));
        } else if (cmd == "slot") {
            printf("%" PRIu32 "\n", ivx::mailbox_slot_of((uint32_t)a));
        } else if (cmd == "live") {
            printf("%d\n", ivx::mailbox_seq_in_slot((uint32_t)a, (uint32_t)b) ? 1 : 0);
        } else if (cmd == "sim") {
            uint32_t owner[ivx::MAILBOX_SLOTS] = {0};
            std::deque<uint32_t> recent;
            uint32_t newest = (uint32_t)a;
            bool ok = true;
            for (uint64_t i = 0; i < b && ok; i++) {
                newest = ivx::mailbox_next_seq(newest);
                owner[ivx::mailbox_slot_of(newest)] = newest;
                recent.push_back(newest);
                if (recent.size() > 200) recent.pop_front();
                for (uint32_t s : recent) {
                    const bool rule = ivx::mailbox_seq_in_slot(s, newest), ring = owner[ivx::mailbox_slot_of(s)] == s;
                    if (rule != ring) {
                        printf("seq %" PRIu32 " newest %" PRIu32 " rule %d ring %d\n", s, newest, (int)rule, (int)ring);
                        ok = false;
                        break;
                    }
                }
            }
            if (ok) printf("ok\n");
        } else {
            printf("unknown command\n");
        }
    }
    return 0;
}
