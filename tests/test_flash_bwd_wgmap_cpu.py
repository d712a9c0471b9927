"""The workgroup map of the flash backward's pass 1, checked on the CPU:
tests/flash_bwd_wgmap_check.cpp includes the header the kernel includes
(deepspeed_amd/ops/csrc/flash_bwd_wgmap.h), is compiled here with the host
compiler and prints (key block, bh) for every workgroup id of a launch.

Workgroups are dealt to the 8 XCDs round-robin by id, so id % 8 labels the ids
that share an L2. Checked for key-block counts 1, 2, 7, 8, 9, 32, 33 and
B * Hk in 1, 3, 8, 32 (and 12: complete rounds of 8 plus a ragged tail):
  * the map is a bijection onto (key block, bh): a missed pair would leave
    rows of dk / dv unwritten, a repeated one is wasted work;
  * all key blocks of a bh have one id % 8, for every bh when B * Hk is a
    multiple of 8 and for the bh in complete rounds of 8 otherwise (the tail
    is spread over the XCDs on purpose: see the header);
  * within a bh, ascending id gives ascending key block: block 0, the one
    with the most q steps under the causal mask, starts first.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "deepspeed_amd", "ops", "csrc")
NXCD = 8
NKB = (1, 2, 7, 8, 9, 32, 33)
NBH = (1, 3, 8, 32)
CASES = [(nkb, nbh) for nkb in NKB for nbh in NBH + (12,)]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("wgmap") / "flash_bwd_wgmap_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC,
                    os.path.join(HERE, "flash_bwd_wgmap_check.cpp"),
                    "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def maps(checker):
    out = {}
    for nkb, nbh in CASES:
        r = subprocess.run([checker, str(nkb), str(nbh)], capture_output=True,
                           text=True, check=True)
        rows = [tuple(int(w) for w in line.split())
                for line in r.stdout.splitlines()]
        assert [row[0] for row in rows] == list(range(nkb * nbh))
        out[nkb, nbh] = [(kb, bh) for _, kb, bh in rows]
    return out


def test_kernel_uses_the_header_under_test():
    src = open(os.path.join(CSRC, "attention_bwd.hip")).read()
    assert '#include "flash_bwd_wgmap.h"' in src
    assert "bwd_wgmap::wg_index(" in src


@pytest.mark.parametrize("nkb,nbh", CASES)
def test_bijection_onto_key_block_and_bh(maps, nkb, nbh):
    m = maps[nkb, nbh]
    assert sorted(m) == [(kb, bh) for kb in range(nkb) for bh in range(nbh)]


@pytest.mark.parametrize("nkb,nbh", CASES)
def test_a_bh_stays_on_one_residue_mod_8(maps, nkb, nbh):
    m = maps[nkb, nbh]
    full = nbh // NXCD * NXCD
    residues = {}
    for i, (kb, bh) in enumerate(m):
        residues.setdefault(bh, set()).add(i % NXCD)
    for bh in range(full):
        assert len(residues[bh]) == 1, (bh, residues[bh])
    if nbh >= NXCD and nbh % NXCD == 0:
        assert all(len(r) == 1 for r in residues.values())
        # and the 8 bh of a round take the 8 residues: no XCD is left idle
        for r0 in range(0, nbh, NXCD):
            assert set().union(*(residues[bh] for bh in
                                 range(r0, r0 + NXCD))) == set(range(NXCD))


@pytest.mark.parametrize("nkb,nbh", CASES)
def test_heaviest_key_block_first_within_a_bh(maps, nkb, nbh):
    m = maps[nkb, nbh]
    for bh in range(nbh):
        assert [kb for kb, b in m if b == bh] == list(range(nkb))


@pytest.mark.parametrize("nkb", NKB)
def test_few_bh_in_flight_per_residue(maps, nkb):
    """One residue class walks ALL key blocks of a bh before the next bh."""
    m = maps[nkb, 32]
    for x in range(NXCD):
        seq = [bh for i, (kb, bh) in enumerate(m) if i % NXCD == x]
        assert seq == [bh for bh in range(x, 32, NXCD) for _ in range(nkb)]
