"""CPU check of the offset convolution's weight-gradient work split: the host program tests/conv3_wgrad_plan_main.cpp walks
csrc/conv3_wgrad_plan.h -- the very footprints, d ranges, workgroup map and workspace offsets csrc/conv3_wgradx.hip runs -- under
the address and undefined-behaviour sanitizers (a stand-alone program, nothing is preloaded).  It exits non-zero unless every token
is the centre of exactly one (workgroup, step, lane slot), every plane a step reads is a zero plane or lies in the workgroup's own
sample, and every workspace slab has one writer inside the reported size; the grids it prints for the benched shapes are held to
the plan's target here."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_on_the_host(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "conv3_wgrad_plan_main")
    cmd = [cxx, "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "conv3_wgrad_plan_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "every token once, every plane in its sample, every slab one writer" in r.stdout
    rows = re.findall(r"benched (\d+) (\d+) (\d+) (\d+) Cin (\d+) items (\d+): grid (\d+) x (\d+) = (\d+) workgroups, tw (\d+), (\d+) d ranges",
                      r.stdout)
    got = {tuple(int(v) for v in row[:6]): tuple(int(v) for v in row[6:]) for row in rows}
    assert set(got) == {(2, 32, 32, 32, 96, 2), (2, 32, 32, 32, 96, 4), (2, 16, 16, 16, 192, 4), (2, 8, 8, 8, 384, 12), (2, 8, 8, 8, 384, 4)}
    for (B, D, H, W, Cin, items), (gx, gy, wgs, tw, nranges) in got.items():
        assert gy == items and gx * gy == wgs and tw == (16 if W >= 12 else 8)
        # two workgroups per CU, or every d range already down to the 4 planes below which priming two planes undoes the saving
        assert wgs >= 512 or nranges == max(1, D // 4), (B, D, H, W, Cin, items, wgs, nranges)
        assert nranges == 1 or D // nranges >= 4
    # the two 32^3 launches, the 16^3 one and the twelve-item 8^3 one
    assert got[(2, 32, 32, 32, 96, 2)][2] == 512 and got[(2, 32, 32, 32, 96, 4)][2] == 512
    assert got[(2, 16, 16, 16, 192, 4)][2] == 512 and got[(2, 8, 8, 8, 384, 12)][2] == 384
