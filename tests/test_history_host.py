"""CPU: the mask edit history's bookkeeping against the reference's own EditionHistory (tests/golden/ref_history.npz), and the
format arithmetic of csrc/mask_history_math.h, compiled for the host, against the numpy restatement (tests/_history_ref.py)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _history_ref as R

NS = (1, 63, 64, 65, 4095, 4096, 4097, 64 * 4096 * 64 - 1, 64 * 4096 * 64, 64 * 4096 * 64 + 1)
PLANES = (1, 63, 64, 110, 4096)


@pytest.mark.parametrize("name", R.script_names())
def test_restated_bookkeeping_equals_the_reference_at_every_step(name):
    fx = R.fixture()
    R.replay(name, lambda size, publish: R.NumpyHistory(size, publish), np.zeros(fx["init_" + name].shape, np.uint8))


def test_fixture_covers_what_it_claims():
    fx = R.fixture()
    assert set(R.script_names()) >= {"orientations", "no_slices", "scroll_only", "double_step", "overflow", "truncation", "clear"}
    assert int(fx["size_overflow"]) == 3 and fx["len_overflow"].max() == 7  # the reference keeps size * 2 + 1 nodes
    notes = [str(s) for s in fx["notes"]]
    assert len(notes) == 2 and all("IndexError" in s for s in notes)  # the stated deviation: the reference dies, we do nothing
    # a scroll-only undo: the index and the matrix stay, the only message is the scroll
    import json
    msgs = json.loads(str(fx["msg_scroll_only"]))
    script = json.loads(str(fx["script_scroll_only"]))
    only = [i for i, (op, m) in enumerate(zip(script, msgs)) if op[0] in ("undo", "redo") and len(m) == 1 and m[0][0][0] == "Set scroll position"]
    assert only, "no scroll-only step in the fixture"
    for i in only:
        assert fx["idx_scroll_only"][i] == fx["idx_scroll_only"][i - 1]
        assert np.array_equal(fx["mat_scroll_only"][i], fx["mat_scroll_only"][i - 1])
    # the double step: one call moves the index by two
    d = np.abs(np.diff(fx["idx_double_step"]))
    assert (d == 2).any()


def test_empty_history_does_nothing():
    sent = []
    h = R.NumpyHistory(publish=lambda *a, **k: sent.append(a))
    del sent[:]
    m = np.arange(24, dtype=np.uint8).reshape(2, 3, 4)
    h.undo(m)
    h.redo(m)
    assert not sent and h.index == -1 and np.array_equal(m.reshape(-1), np.arange(24))


@pytest.mark.parametrize("n", (1, 63, 64, 65, 4095, 4096, 4097, 274625))
def test_restated_codec_round_trips(n):
    rng = np.random.default_rng(n)
    runs = np.repeat(np.array([0, 1, 2, 253, 254, 255], np.uint8)[rng.integers(0, 6, n // 40 + 2)], 40)[:n].copy()
    runs[rng.integers(0, n, max(n // 500, 1))] = 7
    for x in (np.zeros(n, np.uint8), np.full(n, 255, np.uint8), rng.integers(0, 256, n).astype(np.uint8), runs):
        header, pool, nlit = R.encode(x)
        assert header.size == R.layout(n)[4] and pool.size == 64 * nlit
        assert np.array_equal(R.decode(header, pool, n), x)
    assert R.encode(np.zeros(n, np.uint8))[2] == 0
    assert R.encode(rng.integers(0, 256, n).astype(np.uint8))[2] <= R.layout(n)[0]


@pytest.fixture(scope="module")
def host_emu(tmp_path_factory):
    """tests/mask_history_host_emu.cpp: the header the kernels include, built with the host compiler"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("mask_history_emu") / "emu")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(os.path.dirname(__file__), "mask_history_host_emu.cpp")],
                   check=True)

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
        got = [tuple(int(v) for v in line.split()) for line in out.splitlines()]
        assert len(got) == len(lines)
        return got

    return run


def test_header_layout_equals_the_restatement(host_emu):
    got = host_emu(["H %d" % n for n in NS])
    for n, g in zip(NS, got):
        assert g == R.layout(n), n
    # the header is a pure function of n and its arrays are aligned for their element types
    for n, (B, W, off_lit, off_base, total) in zip(NS, got):
        assert off_lit % 8 == 0 and off_base % 4 == 0 and off_lit >= B and total == off_lit + 12 * W


def _blocks_of_interest(n):
    B = R.cdiv(n, 64)
    return sorted({b for b in (0, 1, 62, 63, 64, 65, 4095, 4096, 4097, B - 2, B - 1) if 0 <= b < B})


def test_block_to_word_bit_and_length(host_emu):
    rows = [(n, b) for n in NS for b in _blocks_of_interest(n)]
    got = host_emu(["B %d %d" % r for r in rows])
    for (n, b), g in zip(rows, got):
        assert g == (b // 64, b % 64, min(64, n - 64 * b)), (n, b)


def test_pool_offsets_equal_the_restatement(host_emu):
    """the slot the kernels compute for a literal block == its rank among the literal blocks of the encoded stream"""
    rng = np.random.default_rng(5)
    rows, want = [], []
    for n in (65, 4097, 274625):
        x = np.repeat(rng.integers(0, 3, R.cdiv(n, 64)).astype(np.uint8), 64)[:n].copy()
        x[rng.integers(0, n, n // 90 + 1)] = 200
        header, pool, nlit = R.encode(x)
        B, W, off_lit, off_base, _ = R.layout(n)
        literal, base = header[off_lit:off_base].view(np.uint64), header[off_base:].view(np.uint32)
        rank = 0
        for b in range(B):
            if (int(literal[b >> 6]) >> (b & 63)) & 1:
                rows.append("P %d %x %d" % (base[b >> 6], int(literal[b >> 6]), b & 63))
                want.append((rank, 64 * rank))
                rank += 1
        assert rank == nlit
    rows += ["P 7 ffffffffffffffff 63", "P 0 8000000000000000 63", "P 4294967295 1 0"]
    want += [(70, 4480), (0, 0), (4294967295, 64 * 4294967295)]
    assert host_emu(rows) == want


def test_plane_of_offset(host_emu):
    rows = []
    for n in NS:
        for pb in PLANES:
            for off in sorted({0, 1, pb - 1, pb, pb + 1, 63, 64, 65, n - 1, max(n - 17, 0), (n // 2 // 64) * 64 + 48}):
                if 0 <= off < n:
                    rows.append((off, min(16, n - off), pb))
    got = host_emu(["O %d %d %d" % r for r in rows])
    for (off, ln, pb), g in zip(rows, got):
        assert g == (off // 64, off // pb, off // pb, (off + ln - 1) // pb), (off, ln, pb)
    # and the restatement's changed planes use the same rule
    old = np.zeros(500, np.uint8)
    new = old.copy()
    new[[109, 330]] = 1
    assert np.nonzero(R.changed_planes(old, new, 110))[0].tolist() == [0, 3]
