"""CPU: the host-only record of the piece counted into a marching-cubes scratch block, csrc/mc_piece.h built for the host
(tests/mc_piece_host_emu.cpp, with the address and undefined-behaviour sanitizers) -- when a triangle list built ahead may be
reused, and that a count voids everything known about the piece counted into that scratch before."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
A, B = 4096, 8192          # two scratch blocks
LIST, OTHER = 65536, 131072  # two list buffers
PLANE = 1 << 20


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """run(commands) -> the answers, one per command, from a fresh table"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    tmp = tmp_path_factory.mktemp("mc_piece_emu")
    exe = str(tmp / "emu")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(HERE, "mc_piece_host_emu.cpp")], check=True)

    def run(commands):
        src = str(tmp / "commands.txt")
        with open(src, "w") as fh:
            fh.write("\n".join(commands) + "\n")
        out = subprocess.run([exe, src], check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(out) == len(commands)
        return out
    return run


def test_a_list_is_ready_for_its_scratch_up_to_its_capacity(emu):
    got = emu(["ready %d %d 10" % (A, LIST),                      # nothing built yet
               "count %d" % A, "built %d %d 100" % (A, LIST),
               "ready %d %d 100" % (A, LIST), "ready %d %d 1" % (A, LIST),
               "ready %d %d 100" % (A, OTHER),                    # another buffer
               "ready %d %d 100" % (A, LIST),                     # (asking about OTHER did not touch LIST)
               "ready %d %d 101" % (A, LIST)])                    # more than was built
    assert got == ["0", "ok", "ok", "1", "1", "0", "1", "0"]


def test_a_negative_answer_voids_the_buffers_owner(emu):
    """the caller of a refused `ready` fills the buffer itself, for nobody to find"""
    got = emu(["count %d" % A, "built %d %d 100" % (A, LIST),
               "ready %d %d 101" % (A, LIST),                     # too large: refused, LIST is about to be overwritten
               "ready %d %d 100" % (A, LIST), "ready %d %d 1" % (A, LIST)])
    assert got == ["ok", "ok", "0", "0", "0"]


def test_a_count_voids_the_list(emu):
    got = emu(["count %d" % A, "built %d %d 100" % (A, LIST), "ready %d %d 100" % (A, LIST),
               "count %d" % A, "ready %d %d 100" % (A, LIST),
               "built %d %d 50" % (A, LIST), "ready %d %d 50" % (A, LIST), "count %d %d" % (A, PLANE), "ready %d %d 50" % (A, LIST)])
    assert got == ["ok", "ok", "1", "ok", "0", "ok", "1", "ok", "0"]


def test_another_scratch_takes_the_buffer_over(emu):
    got = emu(["count %d" % A, "built %d %d 100" % (A, LIST), "count %d" % B, "ready %d %d 100" % (A, LIST),  # B's count leaves A alone
               "built %d %d 80" % (B, LIST),
               "ready %d %d 80" % (B, LIST),
               "ready %d %d 100" % (A, LIST),                      # A's descriptors are gone: refused, and LIST loses its owner
               "ready %d %d 80" % (B, LIST)])
    assert got == ["ok", "ok", "ok", "1", "ok", "1", "0", "0"]


def test_a_count_voids_split_vertex_split_and_plane(emu):
    got = emu(["getsplit %d" % A, "getvsplit %d" % A, "plane %d 0" % A,
               "count %d %d" % (A, PLANE), "split %d 1234567890123" % A, "vsplit %d 4000000000" % A,
               "getsplit %d" % A, "getvsplit %d" % A, "plane %d 0" % A,
               "count %d" % A,
               "getsplit %d" % A, "getvsplit %d" % A, "plane %d 0" % A,
               "split %d 0" % A, "getsplit %d" % A, "getvsplit %d" % A,  # a split of zero triangles is a split
               "count %d %d" % (A, PLANE), "getsplit %d" % A, "plane %d 0" % A])
    assert got == ["none", "none", "0",
                   "ok", "ok", "ok",
                   "1234567890123", "4000000000", str(PLANE),
                   "ok",
                   "none", "none", "0",
                   "ok", "0", "none",
                   "ok", "none", str(PLANE)]


def test_the_callers_plane_is_for_iso_0_only(emu):
    got = emu(["count %d %d" % (A, PLANE), "plane %d 0" % A, "plane %d 1" % A, "plane %d 0" % B])
    assert got == ["ok", str(PLANE), "0", "0"]


def test_two_scratches_do_not_see_each_other(emu):
    got = emu(["count %d %d" % (A, PLANE), "split %d 7" % A, "vsplit %d 8" % A, "built %d %d 100" % (A, LIST),
               "count %d" % B,
               "getsplit %d" % B, "getvsplit %d" % B, "plane %d 0" % B, "ready %d %d 1" % (B, OTHER),
               "split %d 70" % B, "vsplit %d 80" % B,
               "getsplit %d" % A, "getvsplit %d" % A, "plane %d 0" % A, "ready %d %d 100" % (A, LIST),
               "count %d" % A, "getsplit %d" % B, "getvsplit %d" % B])
    assert got == ["ok", "ok", "ok", "ok",
                   "ok",
                   "none", "none", "0", "0",
                   "ok", "ok",
                   "7", "8", str(PLANE), "1",
                   "ok", "70", "80"]
