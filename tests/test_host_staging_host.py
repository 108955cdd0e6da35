"""csrc/host_staging.hpp -- where the arrays of a synchronous *_host call lie in
the staging buffer -- compiled with the host compiler
(tools/host_staging_host_test.cpp).  The rules: inputs first in registration
order, outputs after the input total, a NULL array takes no space, an int32
array of B elements occupies (B + 1) / 2 8-byte words and only its 4 B bytes
are the caller's, at most 16 arrays.  The expected byte offsets and word totals
below are written out by hand from those rules; nothing here computes them
from a second copy of the code."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")

CASES = {}


def case(name, arrays, words, regions):
    """arrays: (in|out, present, elem_bytes, count); words: (in, out, total);
    regions: per array (what add returned, byte offset, bytes)."""
    assert name not in CASES and len(arrays) == len(regions)
    CASES[name] = (" ".join("%s %d %d %d" % a for a in arrays), arrays, words, regions)


# drc_qpid_host on the FR3 (nv = na = 7) at B = 3, every array given:
# q, qdot 21 words, xt 36, xdt 18, xi 36, xdi 18 = 150; qdd, tau 21, status and iters 2 words each
case("qpid_fr3_b3",
     [("in", 1, 8, 21), ("in", 1, 8, 21), ("in", 1, 8, 36), ("in", 1, 8, 18), ("in", 1, 8, 36), ("in", 1, 8, 18),
      ("out", 1, 8, 21), ("out", 1, 8, 21), ("out", 1, 4, 3), ("out", 1, 4, 3)],
     (150, 46, 196),
     [(0, 0, 168), (1, 168, 168), (2, 336, 288), (3, 624, 144), (4, 768, 288), (5, 1056, 144),
      (6, 1200, 168), (7, 1368, 168), (8, 1536, 12), (9, 1552, 12)])
# ... without x_init, xdot_init and iters
case("qpid_fr3_b3_nulls",
     [("in", 1, 8, 21), ("in", 1, 8, 21), ("in", 1, 8, 36), ("in", 1, 8, 18), ("in", 0, 8, 36), ("in", 0, 8, 18),
      ("out", 1, 8, 21), ("out", 1, 8, 21), ("out", 1, 4, 3), ("out", 0, 4, 3)],
     (96, 44, 140),
     [(0, 0, 168), (1, 168, 168), (2, 336, 288), (3, 624, 144), (-1, 0, 0), (-1, 0, 0),
      (4, 768, 168), (5, 936, 168), (6, 1104, 12), (-1, 0, 0)])
# drc_qpid_stages_host on the FR3 at B = 1: `pair` (int32) between double arrays
case("qpid_stages_fr3_b1",
     [("in", 1, 8, 7), ("in", 1, 8, 7), ("in", 1, 8, 12), ("in", 1, 8, 6), ("in", 0, 8, 12), ("in", 0, 8, 6),
      ("out", 1, 8, 12), ("out", 1, 8, 42), ("out", 1, 8, 8), ("out", 1, 8, 8), ("out", 1, 4, 1), ("out", 1, 8, 6),
      ("out", 1, 8, 42), ("out", 1, 8, 8), ("out", 1, 8, 14)],
     (32, 141, 173),
     [(0, 0, 56), (1, 56, 56), (2, 112, 96), (3, 208, 48), (-1, 0, 0), (-1, 0, 0),
      (4, 256, 96), (5, 352, 336), (6, 688, 64), (7, 752, 64), (8, 816, 4), (9, 824, 48),
      (10, 872, 336), (11, 1208, 64), (12, 1272, 112)])
# an int32 array of B elements takes (B + 1) / 2 words; the double array after it stays on a word
case("int32_b1", [("in", 1, 8, 5), ("out", 1, 4, 1), ("out", 1, 8, 1), ("out", 1, 4, 1)], (5, 3, 8),
     [(0, 0, 40), (1, 40, 4), (2, 48, 8), (3, 56, 4)])
case("int32_b2", [("in", 1, 8, 5), ("out", 1, 4, 2), ("out", 1, 8, 2), ("out", 1, 4, 2)], (5, 4, 9),
     [(0, 0, 40), (1, 40, 8), (2, 48, 16), (3, 64, 8)])
case("int32_b3", [("in", 1, 8, 5), ("out", 1, 4, 3), ("out", 1, 8, 3), ("out", 1, 4, 3)], (5, 7, 12),
     [(0, 0, 40), (1, 40, 12), (2, 56, 24), (3, 80, 12)])
case("no_arrays", [], (0, 0, 0), [])
case("all_null", [("in", 0, 8, 7), ("out", 0, 4, 3)], (0, 0, 0), [(-1, 0, 0), (-1, 0, 0)])
# the outputs lie after the input total whatever the registration order
case("outputs_registered_first", [("out", 1, 8, 4), ("in", 1, 8, 3), ("out", 1, 4, 1)], (3, 5, 8),
     [(0, 24, 32), (1, 0, 24), (2, 56, 4)])
# the 17th array is refused (-2) and takes nothing; a NULL array still is -1
case("full", [("in", 1, 8, 1)] * 16 + [("in", 1, 8, 1), ("out", 1, 8, 1), ("out", 0, 8, 1)], (16, 0, 16),
     [(i, 8 * i, 8) for i in range(16)] + [(-2, 0, 0), (-2, 0, 0), (-1, 0, 0)])


def build(tmp, flags):
    assert shutil.which(CXX), "no host C++ compiler"
    exe = str(tmp / "host_staging")
    subprocess.check_call([CXX, "-std=c++17", "-Wall", "-Werror"] + flags +
                          [os.path.join(ROOT, "tools", "host_staging_host_test.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    exe = build(tmp_path_factory.mktemp("host_staging"), ["-O1"])
    names = list(CASES)
    r = subprocess.run([exe], input="".join(CASES[n][0] + "\n" for n in names), capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-500:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(names)
    return dict(zip(names, lines))


def parse(line):
    tok = line.split()
    return tuple(int(t) for t in tok[:3]), [tuple(int(v) for v in t.split(":")) for t in tok[3:]]


@pytest.mark.parametrize("name", list(CASES))
def test_layout(answers, name):
    query, arrays, words, regions = CASES[name]
    got_words, got = parse(answers[name])
    assert got_words == words, (query, answers[name])
    assert got == regions, (query, answers[name])


@pytest.mark.parametrize("name", list(CASES))
def test_regions_disjoint_aligned_outputs_after_inputs(answers, name):
    _, arrays, _, _ = CASES[name]
    (in_words, out_words, total), got = parse(answers[name])
    assert total == in_words + out_words
    spans = []
    for (kind, present, elem, count), (ret, off, nbytes) in zip(arrays, got):
        if ret < 0:
            assert not present or len(spans) == 16
            continue
        assert present and nbytes == elem * count
        assert off % 8 == 0                                   # every array, so every double array, on a whole word
        if kind == "in":
            assert off + nbytes <= 8 * in_words
        else:
            assert 8 * in_words <= off and off + nbytes <= 8 * total
        spans.append((off, off + nbytes))
    spans.sort()
    for (_, end), (start, _) in zip(spans, spans[1:]):
        assert end <= start
    outs = [off for (kind, _, _, _), (ret, off, _) in zip(arrays, got) if kind == "out" and ret >= 0]
    if outs:
        assert min(outs) == 8 * in_words                      # the outputs start at the input total
