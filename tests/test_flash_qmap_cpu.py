"""The workgroup map of the two q-outer flash kernels (flash_fwd_v6_kernel of
attention.hip and pass 2, flash_bwd_dq_kernel, of attention_bwd.hip), checked
on the CPU: tests/flash_qmap_check.cpp includes the header the kernels include
(deepspeed_amd/ops/csrc/flash_bwd_wgmap.h), is compiled here with the host
compiler and prints (q block, bh) for every workgroup id of a launch.

Workgroups are dealt to the 8 XCDs round-robin by id, so id % 8 labels the ids
that share an XCD. Under the causal mask q block i runs i + 1 key steps (in
units of one q block of keys), and a call ends with its heaviest XCD. Checked
for q-block counts 1, 2, 7, 8, 9, 16, 32, 33 and B * Hq in 1, 3, 8, 12, 32, 128:
  * the map is a bijection onto (q block, bh): a missed pair would leave rows
    of out / dq unwritten, a repeated one is wasted work;
  * all q blocks of a bh in a complete round of 8 have one id % 8, and the 8 bh
    of a round take the 8 residues;
  * within a bh, ascending id gives DESCENDING q block: the last block, the
    one with the most key steps under the causal mask, starts first;
  * for B * Hq a multiple of 8 every residue gets the same sum of causal
    steps. The plain (q block, bh) grids the kernels had do not, whenever the
    block count is even: the test computes the same sum over them, and holds
    the flagship's figures (16 forward blocks: 10 .. 24 per bh, mean 17; 32
    pass 2 blocks: 52 .. 80, mean 66).
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "deepspeed_amd", "ops", "csrc")
NXCD = 8
NQB = (1, 2, 7, 8, 9, 16, 32, 33)
NBH = (1, 3, 8, 12, 32, 128)
CASES = [(nqb, nbh) for nqb in NQB for nbh in NBH]
FULL_CASES = [(nqb, nbh) for nqb, nbh in CASES if nbh % NXCD == 0]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("qmap") / "flash_qmap_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC,
                    os.path.join(HERE, "flash_qmap_check.cpp"),
                    "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def maps(checker):
    out = {}
    for nqb, nbh in CASES:
        r = subprocess.run([checker, str(nqb), str(nbh)], capture_output=True,
                           text=True, check=True)
        rows = [tuple(int(w) for w in line.split())
                for line in r.stdout.splitlines()]
        assert [row[0] for row in rows] == list(range(nqb * nbh))
        out[nqb, nbh] = [(qb, bh) for _, qb, bh in rows]
    return out


def plain_forward(nqb, nbh):
    """The (q block, bh) grid: x = q block, y = bh, linear id = x + nqb * y."""
    return [(i % nqb, i // nqb) for i in range(nqb * nbh)]


def plain_pass2(nqb, nbh):
    """The same grid with the q block reversed (heaviest first)."""
    return [(nqb - 1 - i % nqb, i // nqb) for i in range(nqb * nbh)]


def causal_steps_per_residue(m):
    steps = [0] * NXCD
    for i, (qb, _) in enumerate(m):
        steps[i % NXCD] += qb + 1
    return steps


@pytest.mark.parametrize("name", ("attention.hip", "attention_bwd.hip"))
def test_kernels_use_the_function_under_test(name):
    src = open(os.path.join(CSRC, name)).read()
    assert '#include "flash_bwd_wgmap.h"' in src
    assert "bwd_wgmap::q_index(blockIdx.x, " in src
    kernel = {"attention.hip": "flash_fwd_v6_kernel",
              "attention_bwd.hip": "flash_bwd_dq_kernel"}[name]
    body = src.split("__global__ void " + kernel + "(")[1]
    body = body.split("__global__ void ")[0]
    assert "bwd_wgmap::q_index(blockIdx.x, " in body
    assert "blockIdx.y" not in body and "gridDim" not in body


@pytest.mark.parametrize("nqb,nbh", CASES)
def test_bijection_onto_q_block_and_bh(maps, nqb, nbh):
    m = maps[nqb, nbh]
    assert sorted(m) == [(qb, bh) for qb in range(nqb) for bh in range(nbh)]


@pytest.mark.parametrize("nqb,nbh", CASES)
def test_a_bh_of_a_complete_round_stays_on_one_residue_mod_8(maps, nqb, nbh):
    m = maps[nqb, nbh]
    full = nbh // NXCD * NXCD
    residues = {}
    for i, (qb, bh) in enumerate(m):
        residues.setdefault(bh, set()).add(i % NXCD)
    for bh in range(full):
        assert len(residues[bh]) == 1, (bh, residues[bh])
    # the 8 bh of a round take the 8 residues: no XCD is left idle
    for r0 in range(0, full, NXCD):
        assert set().union(*(residues[bh] for bh in
                             range(r0, r0 + NXCD))) == set(range(NXCD))


@pytest.mark.parametrize("nqb,nbh", CASES)
def test_heaviest_q_block_first_within_a_bh(maps, nqb, nbh):
    m = maps[nqb, nbh]
    for bh in range(nbh):
        assert [qb for qb, b in m if b == bh] == list(range(nqb - 1, -1, -1))


@pytest.mark.parametrize("nqb,nbh", FULL_CASES)
def test_every_residue_gets_the_same_causal_steps(maps, nqb, nbh):
    steps = causal_steps_per_residue(maps[nqb, nbh])
    assert sum(steps) == nbh * nqb * (nqb + 1) // 2
    assert len(set(steps)) == 1, steps


@pytest.mark.parametrize("nqb,nbh", [c for c in FULL_CASES
                                     if c[0] > 1 and c[0] % 2 == 0])
@pytest.mark.parametrize("plain", (plain_forward, plain_pass2))
def test_the_plain_grid_does_not(plain, nqb, nbh):
    m = plain(nqb, nbh)
    assert sorted(m) == [(qb, bh) for qb in range(nqb) for bh in range(nbh)]
    steps = causal_steps_per_residue(m)
    assert len(set(steps)) > 1, steps


def test_the_flagship_figures_of_the_plain_grids():
    """B 4, 32 q heads, S 4096: 16 forward blocks of 256 rows, 32 pass 2
    blocks of 128. Steps per bh on the lightest and heaviest residue."""
    fwd = causal_steps_per_residue(plain_forward(16, 128))
    assert (min(fwd) // 128, max(fwd) // 128, sum(fwd) // 128 / 8) == \
        (10, 24, 17.0)           # x 4 key tiles of 64: 40, 96, mean 68
    p2 = causal_steps_per_residue(plain_pass2(32, 128))
    assert (min(p2) // 128, max(p2) // 128, sum(p2) // 128 / 8) == \
        (52, 80, 66.0)
