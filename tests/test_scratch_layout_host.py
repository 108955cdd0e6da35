"""csrc/scratch_layout.hpp -- where every region of the per-stream device
scratch lies and how many bytes a call's layout takes -- compiled with the host
compiler (tools/scratch_layout_host_test.cpp) and checked against the rules
the header states.

Grid: nv in {1, 6, 7, 10, 16}, na in {nv, nv - 3} where positive, record
lengths {1, 15, 16, 17, 300} (the stride rounds to 16), B in {1, 2, 63, 64, 65,
2049, 65536}; for the seeds scratch T in {1, 3, 64}, S in {1, 2, 5} and
nobst in {0, 1, 4}; every combination of a layout's flags.  The program itself
checks that measuring (no base) and carving (a heap block of exactly `bytes`)
take the same steps, that every struct member is the region of its name, and
that every region holds its own tag after all were filled.

The byte count and every offset of the whole grid are pinned in
tests/golden/scratch_layout_parent.txt, recorded from the size formulas and
address expressions that api.cpp spelled out per launch path before the
layouts had a header: `WHAT | bytes | offset ...`, -1 where no address is
formed.  The reach layout is no row of that file: it is the reach-path layout
followed by wp [B] int32 (drc_qpik_reach_batch runs as a reach path of one
waypoint), and test_reach_is_reach_path_then_wp holds every reach case to the
pinned reach_path case of the same nv, na, B and persistent."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")
GOLDEN = os.path.join(ROOT, "tests", "golden", "scratch_layout_parent.txt")

NV, RLEN, BATCH = (1, 6, 7, 10, 16), (1, 15, 16, 17, 300), (1, 2, 63, 64, 65, 2049, 65536)
TARGETS, SEEDS, NOBST = (1, 3, 64), (1, 2, 5), (0, 1, 4)
NV_NA = [(nv, na) for nv in NV for na in (nv, nv - 3) if na > 0]
FLAGS = {"qpik": ("stages", "auto_order"), "qpid": ("stages", "whole_body"), "osf": (), "dyn_list": (),
         "rollout": ("qdot_traj",), "reach": ("persistent",), "reach_path": ("persistent",),
         "seeds": ("persistent", "ob_expand")}


def expected_cases():
    """The grid (module docstring) as {layout: set of parameter tuples}, flags last."""
    bits = lambda n: list(itertools.product((0, 1), repeat=n))
    dims = {"qpik": itertools.product(RLEN, BATCH), "osf": itertools.product(NV, BATCH), "dyn_list": [(b,) for b in BATCH],
            "qpid": [(nv, na, r, b) for (nv, na) in NV_NA for r in RLEN for b in BATCH],
            "seeds": [(nv, na, n, t, s) for (nv, na) in NV_NA for n in NOBST for t in TARGETS for s in SEEDS]}
    for k in ("rollout", "reach", "reach_path"):
        dims[k] = [(nv, na, b) for (nv, na) in NV_NA for b in BATCH]
    return {k: {tuple(d) + f for d in dims[k] for f in bits(len(FLAGS[k]))} for k in FLAGS}


def parse(text):
    cases = []
    for ln in text.splitlines():
        what, nbytes, regions = (x.strip() for x in ln.split("|"))
        t = what.split()
        par = dict((k, int(v)) for k, v in (x.split("=") for x in t[1:]))
        regs = []
        for r in regions.split():
            name, elem, off, n, carved = r.split(":")
            regs.append((name, int(elem), int(off), int(n), int(carved)))
        cases.append(dict(what=what, layout=t[0], par=par, bytes=int(nbytes), regions=regs))
    return cases


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    assert shutil.which(CXX), "no host C++ compiler"
    exe = os.path.join(str(tmp_path_factory.mktemp("scratch_layout")), "scratch_layout_host")
    subprocess.check_call([CXX, "-O1", "-std=c++17", "-Wall", "-Werror",
                           os.path.join(ROOT, "tools", "scratch_layout_host_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-500:])
    return parse(r.stdout)


def test_grid(cases):
    got = {}
    for c in cases:
        got.setdefault(c["layout"], []).append(tuple(c["par"].values()))
    want = expected_cases()
    assert sorted(got) == sorted(want)
    for k in want:
        assert len(got[k]) == len(set(got[k])) and set(got[k]) == want[k], k


def off_regions(c):
    """The regions whose condition is off in this case."""
    p, k = c["par"], c["layout"]
    on = lambda names, flag: set(names) if flag else set()
    if k == "qpik":
        return on(["rec"], p["stages"]) | on(["order", "hot", "hot_flag"], not p["auto_order"])
    if k == "qpid":
        return {"rec", "M", "g", "g_joint"} if p["stages"] else on(["g_joint"], not p["whole_body"])
    if k == "rollout":
        return on(["eta"], p["qdot_traj"])
    if k in ("reach", "reach_path"):
        return on(["pose", "dist", "xt", "xdt"], p["persistent"])
    if k == "seeds":
        return on(["eta"], not p["persistent"]) | on(["pose"], not (p["ob_expand"] and p["nobst"]))
    return set()


def test_rules(cases):
    for c in cases:
        regs, nbytes = c["regions"], c["bytes"]
        off = off_regions(c)
        for name, elem, o, n, carved in regs:
            assert o % elem == 0 and 0 <= o and o + n * elem <= nbytes, (c["what"], name)
            if name in off:
                assert n == 0 and carved == -1, (c["what"], name)
            else:
                assert n > 0 and carved == o, (c["what"], name)
        live = sorted((o, o + n * elem, name) for name, elem, o, n, _ in regs if n)
        for a, b in zip(live, live[1:]):
            assert a[1] <= b[0], (c["what"], a, b)
        end = max((e for _, e, _ in live), default=0)
        if c["layout"] == "qpik":   # the order arrays' 8-byte boundary is part of the count with or without them
            assert nbytes == (end if c["par"]["auto_order"] else (end + 7) // 8 * 8), c["what"]
            order = [r for r in regs if r[0] == "order"][0]
            assert order[2] % 8 == 0
        else:
            assert nbytes == end, c["what"]


def test_offsets_and_sizes_unchanged(cases):
    with open(GOLDEN) as fh:
        want = [ln.rstrip("\n") for ln in fh if not ln.startswith("#")]
    got = ["%s | %d | %s" % (c["what"], c["bytes"], " ".join(str(r[4]) for r in c["regions"])) for c in cases
           if c["layout"] != "reach"]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w


def test_reach_is_reach_path_then_wp(cases):
    key = lambda c: tuple(sorted(c["par"].items()))
    path = {key(c): c for c in cases if c["layout"] == "reach_path"}
    reach = [c for c in cases if c["layout"] == "reach"]
    assert len(reach) == len(path) > 0
    for c in reach:
        p = path[key(c)]                          # (pinned by test_offsets_and_sizes_unchanged)
        B = c["par"]["B"]
        assert c["regions"][:-1] == p["regions"], c["what"]
        assert c["regions"][-1] == ("wp", 4, p["bytes"], B, p["bytes"]), c["what"]
        assert c["bytes"] == p["bytes"] + 4 * B, c["what"]
