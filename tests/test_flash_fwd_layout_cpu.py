"""Layout proof of the flash forward's LDS images, on the CPU:
tests/flash_fwd_layout_check.cpp includes the header the kernel includes
(deepspeed_amd/ops/csrc/flash_fwd_layout.h), is compiled here with the host
compiler and emulates K's row reads and V's hardware transposed reads on
images filled the way the DMA fills them.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "deepspeed_amd", "ops", "csrc")
# conflict degree the header's comment documents: 1 = conflict-free, for V's
# transposed read (per 32-lane half) and K's row read (per 16-lane group);
# last, the 2-way row read of the ((row&7)<<4) swizzle the header replaced
DOCUMENTED = {64: (1, 1, 2), 128: (1, 1, 2)}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("layout") / "flash_fwd_layout_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC,
                    os.path.join(HERE, "flash_fwd_layout_check.cpp"),
                    "-o", exe], check=True)
    return exe


def _run(exe, mutant):
    r = subprocess.run([exe, str(mutant)], capture_output=True, text=True)
    rows = {}
    for line in r.stdout.splitlines():
        w = line.split()
        rows[int(w[1])] = dict(frag=w[3], addr=w[5], tr=int(w[7]),
                               row=int(w[9]), old_row=int(w[11]))
    return r.returncode, rows


def test_kernel_includes_the_header_under_test():
    src = open(os.path.join(CSRC, "attention.hip")).read()
    assert '#include "flash_fwd_layout.h"' in src
    assert '#include "lds_tr_read.h"' in src
    for fn in ("fwd_layout::k_row_read_addr<DH>",
               "fwd_layout::v_tr_lane_base<DH>", "v_tr_step<DH>",
               "fwd_layout::k_dma_src_byte<DH>",
               "fwd_layout::v_dma_src_byte<DH>", "fwd_layout::dma_row<DH>"):
        assert fn in src, fn
    # the transposed-read helpers exist once, shared with the backward
    bwd = open(os.path.join(CSRC, "attention_bwd.hip")).read()
    assert '#include "lds_tr_read.h"' in bwd
    for text in (src, bwd):
        assert "ds_read_b64_tr_b16 %0" not in text


def test_fragments_addresses_and_conflicts(checker):
    code, rows = _run(checker, 0)
    assert sorted(rows) == [64, 128]
    for d, r in rows.items():
        assert r["frag"] == "ok", (d, r)
        assert r["addr"] == "ok", (d, r)
        assert (r["tr"], r["row"], r["old_row"]) == DOCUMENTED[d], (d, r)
    assert code == 0


@pytest.mark.parametrize("mutant", [1, 2], ids=["xor_dropped_on_one_row_class",
                                                "8_byte_halves_swapped"])
def test_one_edge_mutant_fails_the_fragment_check(checker, mutant):
    code, rows = _run(checker, mutant)
    assert code == 1
    for d, r in rows.items():
        assert r["addr"] == "ok", (d, r)  # in bounds and aligned: no fault,
        assert r["frag"] == "bad", (d, r)  # just wrong data
