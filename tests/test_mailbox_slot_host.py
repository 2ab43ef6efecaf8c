"""CPU: the arithmetic of the GPU -> host mailbox ring, csrc/mailbox_slot.h built for the host (tests/mailbox_slot_host.cpp,
with the address and undefined-behaviour sanitizers): 64 slots, sequence numbers that wrap at 2^32 and skip 0, and the rule
ivx_dev_mc_total_early relies on -- is a number reserved a while ago still the newest one of its slot?"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
M = 1 << 32


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """run(commands) -> the answers, one per command"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    tmp = tmp_path_factory.mktemp("mailbox_slot")
    exe = str(tmp / "emu")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(HERE, "mailbox_slot_host.cpp")], check=True)

    def run(commands):
        src = str(tmp / "commands.txt")
        with open(src, "w") as fh:
            fh.write("\n".join(commands) + "\n")
        out = subprocess.run([exe, src], check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(out) == len(commands)
        return out
    return run


def _live(emu, pairs):
    return [int(v) for v in emu(["live %d %d" % (s % M, n % M) for s, n in pairs])]


def test_numbers_count_up_wrap_and_skip_zero(emu):
    assert emu(["next 0", "next 1", "next 63", "next %d" % (M - 2), "next %d" % (M - 1)]) == ["1", "2", "64", str(M - 1), "1"]
    assert emu(["slot 1", "slot 63", "slot 64", "slot 65", "slot %d" % (M - 1), "slot %d" % (M - 64)]) == ["1", "63", "0", "1", "63", "0"]


@pytest.mark.parametrize("seq", [1, 5, 64, 1000, 12345 * 64 + 63])
def test_a_number_keeps_its_slot_for_63_later_numbers(emu, seq):
    """distance 0 and 63: still there; distance 64: the slot's next owner has been handed out; and never again after that"""
    assert _live(emu, [(seq, seq), (seq, seq + 1), (seq, seq + 63), (seq, seq + 64), (seq, seq + 65), (seq, seq + 127),
                       (seq, seq + 128), (seq, seq + 10 ** 6)]) == [1, 1, 1, 0, 0, 0, 0, 0]


def test_no_number_reserved(emu):
    """0 is "none": never in a slot, whatever the newest number"""
    assert _live(emu, [(0, 0), (0, 1), (0, 63), (0, 64), (0, M - 1)]) == [0, 0, 0, 0, 0]


def test_across_the_wrap(emu):
    """the newest number is small again while the reserved one is just below 2^32"""
    seq = M - 16  # slot 48; its next owner is the number 48
    assert _live(emu, [(seq, M - 1), (seq, 1), (seq, 47), (seq, 48), (seq, 49), (seq, 200)]) == [1, 1, 1, 0, 0, 0]
    seq = M - 1   # slot 63; next owner 63
    assert _live(emu, [(seq, seq), (seq, 1), (seq, 62), (seq, 63), (seq, 64)]) == [1, 1, 1, 0, 0]


def test_the_skipped_zero_leaves_slot_0_alone_for_a_round(emu):
    """2^32 - 64 sits in slot 0 and the number that would follow it there is 0, which is never handed out: the slot's next owner
    is 64, i.e. 128 later.  Its neighbours 2^32 - 65 and 2^32 - 63 follow the ordinary rule."""
    seq = M - 64
    assert _live(emu, [(seq, seq), (seq, M - 1), (seq, 1), (seq, 63), (seq, 64), (seq, 65), (seq, 128)]) == [1, 1, 1, 1, 0, 0, 0]
    assert _live(emu, [(M - 65, M - 2), (M - 65, M - 1), (M - 65, 1)]) == [1, 0, 0]
    assert _live(emu, [(M - 63, M - 1), (M - 63, 1), (M - 63, 2)]) == [1, 0, 0]


def test_the_rule_is_what_a_ring_does(emu):
    """hand numbers out one by one, let each take its slot, and hold the rule against the ring after every step: from the start,
    and across the wrap"""
    assert emu(["sim 0 1000", "sim %d 1000" % (M - 400), "sim %d 400" % (M - 64), "sim %d 300" % (M - 1)]) == ["ok"] * 4
