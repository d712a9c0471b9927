// Prints the workgroup map of the flash backward's pass 1, from the header the
// kernel includes: one line "id kb bh" per workgroup id of an nkb x nbh
// launch. Usage: flash_bwd_wgmap_check <nkb> <nbh>. The properties are
// asserted by tests/test_flash_bwd_wgmap_cpu.py.
#include <cstdio>
#include <cstdlib>

#include "flash_bwd_wgmap.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const int nkb = std::atoi(argv[1]);
  const int nbh = std::atoi(argv[2]);
  for (int id = 0; id < nkb * nbh; ++id) {
    const bwd_wgmap::WgIndex w = bwd_wgmap::wg_index(id, nkb, nbh);
    std::printf("%d %d %d\n", id, w.kb, w.bh);
  }
  return 0;
}
