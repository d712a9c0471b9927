"""Layout proof of the flash backward's one-image-per-tile LDS layout, on the
CPU: tests/flash_bwd_layout_check.cpp includes the header the kernels include
(deepspeed_amd/ops/csrc/flash_bwd_layout.h), is compiled here with the host
compiler and emulates the row reads and the hardware transposed reads on an
image filled the way the DMA fills it. The Q and dO images of pass 1 and the
K and V images of pass 2 all go through these same functions, so one run per
head dim covers them.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "deepspeed_amd", "ops", "csrc")
# conflict degree the header's comment documents: 1 = conflict-free, for the
# transposed read (per 32-lane half) and the row read (per 16-lane group)
DOCUMENTED = {64: (1, 1), 128: (1, 1)}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("layout") / "flash_bwd_layout_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC,
                    os.path.join(HERE, "flash_bwd_layout_check.cpp"),
                    "-o", exe], check=True)
    return exe


def _run(exe, mutant):
    r = subprocess.run([exe, str(mutant)], capture_output=True, text=True)
    rows = {}
    for line in r.stdout.splitlines():
        w = line.split()
        rows[int(w[1])] = dict(frag=w[3], addr=w[5], tr=int(w[7]),
                               row=int(w[9]))
    return r.returncode, rows


def test_kernel_includes_the_header_under_test():
    src = open(os.path.join(CSRC, "attention_bwd.hip")).read()
    assert '#include "flash_bwd_layout.h"' in src
    for fn in ("bwd_layout::img_off<DH>", "bwd_layout::tr_read_addr<DH>",
               "bwd_layout::dma_src_byte<DH>"):
        assert fn in src, fn


def test_fragments_addresses_and_conflicts(checker):
    code, rows = _run(checker, 0)
    assert sorted(rows) == [64, 128]
    for d, r in rows.items():
        assert r["frag"] == "ok", (d, r)
        assert r["addr"] == "ok", (d, r)
        assert (r["tr"], r["row"]) == DOCUMENTED[d], (d, r)
    assert code == 0


@pytest.mark.parametrize("mutant", [1, 2], ids=["xor_dropped_on_one_row_class",
                                                "8_byte_halves_swapped"])
def test_one_edge_mutant_fails_the_fragment_check(checker, mutant):
    code, rows = _run(checker, mutant)
    assert code == 1
    for d, r in rows.items():
        assert r["addr"] == "ok", (d, r)  # in bounds and aligned: no fault,
        assert r["frag"] == "bad", (d, r)  # just wrong data
