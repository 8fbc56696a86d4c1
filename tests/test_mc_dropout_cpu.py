"""The Monte-Carlo pose heads without a GPU: Philox4x32-10 against known answers, csrc/philox.h compiled by the host compiler
against the numpy statement (tests/mc_dropout_ref.py), the mask's statistics, the launcher's limits (checked before any launch)
and the host side of mc_dropout.McDropout."""
import os
import re

import numpy as np
import pytest

import mc_dropout_ref as R
from conftest import ROOT

# (counter, key) -> output: the Random123 known-answer vectors of philox4x32_10
KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


def _hex(words) -> str:
    return " ".join(f"{int(v):08x}" for v in words)


def test_philox_known_answers():
    for ctr, key, want in KAT:
        assert _hex(R.philox4x32_10(*ctr, *key)) == want


def test_philox_vectorised_equals_scalar():
    """The helper broadcasts: a grid of (k, s) equals the calls one by one."""
    k, s = np.arange(5).reshape(1, -1), np.arange(3).reshape(-1, 1)
    grid = R.mask_words(77, 2, 9, R.NODE_TAG, k, s)
    assert grid.shape == (3, 5, 4)
    for si in range(3):
        for ki in range(5):
            assert (grid[si, ki] == R.mask_words(77, 2, 9, R.NODE_TAG, ki, si)).all()


def test_header_on_the_host_equals_numpy(tmp_path):
    """csrc/philox.h is plain C++: the host compiler builds tests/philox_check.cpp with -Wall -Wextra -Werror; the program prints
    the three known answers and the mask words of its tuples, which must be the numpy helper's."""
    import shutil
    import subprocess
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "philox_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "philox_check.cpp")],
                   check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    out = run.stdout
    assert "philox: ok" in out
    kats = re.findall(r"^kat (.+)$", out, re.M)
    assert kats == [want for _, _, want in KAT]
    masks = re.findall(r"^mask (\d+) (\d+) (\d+) (\d+) (\d+) (\d+) : (.+)$", out, re.M)
    assert len(masks) >= 5
    for a, b, k, s, draw, seed, words in masks:
        assert _hex(R.mask_words(int(seed), int(draw), int(a), int(b), int(k), int(s))) == words, (a, b, k, s, draw, seed)
    # source and target are not interchangeable, and the node tag is no edge
    by = {tuple(int(v) for v in m[:6]): m[6] for m in masks}
    assert by[(7, 3, 1, 1, 0, 0)] != by[(3, 7, 1, 1, 0, 0)]


@pytest.mark.parametrize("p", [0.5, 0.1, 0.9])
def test_mask_statistics(p):
    """2^20 mask elements (64 node rows x 4096 columns x 4 samples) of a fixed seed: the kept fraction is within 5 binomial
    standard deviations of 1 - T / 2^32, and the masks of two samples, of two draws and of a node row against an edge row with the
    same first id agree on a fraction within 5 sigma of what independent masks give, q^2 + (1 - q)^2."""
    rows, d, S, seed = 64, 4096, 4, 20261020
    n = rows * d * S
    assert n == 2 ** 20
    q = 1.0 - R.threshold(p) / 2.0 ** 32
    a = np.arange(rows)
    tag = np.full(rows, R.NODE_TAG)
    m0 = R.mask(seed, 0, a, tag, d, S, p)
    assert m0.shape == (S, rows, d)
    assert abs(m0.mean() - q) <= 5.0 * np.sqrt(q * (1.0 - q) / n), (m0.mean(), q)
    agree = q * q + (1.0 - q) ** 2

    def independent(x, y):
        return abs((x == y).mean() - agree) <= 5.0 * np.sqrt(agree * (1.0 - agree) / x.size)
    assert independent(m0[0], m0[1]) and independent(m0[2], m0[3])                 # two samples
    assert independent(m0, R.mask(seed, 1, a, tag, d, S, p))                        # two draws
    assert independent(m0, R.mask(seed, 0, a, a + 1, d, S, p))                      # node tag against an edge (a, a + 1)
    assert independent(m0, R.mask(seed + 1, 0, a, tag, d, S, p))                    # two seeds


def test_threshold_and_scale():
    assert R.threshold(0.5) == 2 ** 31 and R.threshold(0.25) == 2 ** 30
    assert R.threshold(0.1) == int(np.floor(0.1 * 2.0 ** 32)) < 2 ** 32
    assert float(R.scale_f32(0.5)) == 2.0


def test_symbols_are_declared_and_built():
    from relpose_gnn_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "relpose_gnn_hip.h")).read()
    for name in ("rpg_pose_heads_mc_f32", "rpg_mc_advance"):
        assert name in _lib.SYMBOLS and re.search(r"\b" + name + r"\s*\(", hdr) and hasattr(_lib.lib(), name)
    assert "mc_heads.hip" in build.SOURCES
    assert "posenet.py:1073-1086" in open(os.path.join(ROOT, "relpose-gnn_amd", "csrc", "mc_heads.hip")).read()


def test_launcher_limits_are_checked_before_any_launch():
    """Every limit of the header returns RPG_ERR_BAD_ARG from the host-side check: no kernel is launched, so this runs without a
    GPU (the pointers are placeholders that nothing dereferences)."""
    from relpose_gnn_amd import _lib
    lib, P = _lib.lib(), 4096

    def call(r=4, d=64, p=0.5, s=8, off=0, x=P, state=P, mean=P, var=P):
        return lib.rpg_pose_heads_mc_f32(x, P, P, r, d, p, s, 0, state, None, None, off, mean, var, None, None)
    bad = _lib.RPG_ERR_BAD_ARG
    for p in (0.0, 1.0, -0.1, 1.5, float("nan")):
        assert call(p=p) == bad, p
    for s in (0, -1, 1025):
        assert call(s=s) == bad, s
    assert call(d=6) == bad and call(d=0) == bad and call(d=4 * 65536) == bad
    assert call(r=0) == bad and call(off=-1) == bad and call(off=2 ** 31 - 3) == bad and call(off=2 ** 40) == bad
    assert call(x=None) == bad and call(state=None) == bad and call(mean=None) == bad and call(var=None) == bad
    assert call(x=P + 4) == bad                                                    # 16-byte alignment
    assert lib.rpg_mc_advance(None, None) == bad
    with pytest.raises(ValueError):
        _lib.check(call(p=1.0), "pose_heads_mc")


def test_mc_dropout_host_side():
    from relpose_gnn_amd.mc_dropout import McDropout, McSpread
    m = McDropout()
    assert (m.samples, m.seed, m.last, m.node_base) == (16, 0, None, 0)
    m.node_base = 48                       # no device state yet: kept for the state's creation
    m.reset(7)
    assert m.node_base == 48 and m._init == [7, 48]
    m.reset(2 ** 32 + 5)                   # the draw counter is 32 bits and wraps
    assert m._init[0] == 5
    for bad in (0, 1025, -3):
        with pytest.raises(ValueError):
            McDropout(samples=bad)
    with pytest.raises(ValueError):
        McDropout(seed=-1)
    with pytest.raises(ValueError):
        McDropout(seed=2 ** 64)
    with pytest.raises(ValueError):
        m.node_base = 2 ** 31
    assert McSpread._fields == ("abs_var", "rel_var")
