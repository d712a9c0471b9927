// Prints the workgroup map of the two q-outer flash kernels (the forward and
// the backward's pass 2), from the header the kernels include: one line
// "id qb bh" per workgroup id of an nqb x nbh launch. Usage:
// flash_qmap_check <nqb> <nbh>. The properties are asserted by
// tests/test_flash_qmap_cpu.py.
#include <cstdio>
#include <cstdlib>

#include "flash_bwd_wgmap.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const int nqb = std::atoi(argv[1]);
  const int nbh = std::atoi(argv[2]);
  for (int id = 0; id < nqb * nbh; ++id) {
    const bwd_wgmap::QIndex w = bwd_wgmap::q_index(id, nqb, nbh);
    std::printf("%d %d %d\n", id, w.qb, w.bh);
  }
  return 0;
}
