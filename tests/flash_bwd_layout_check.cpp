// Host-only proof of the flash backward LDS image layout. Includes the SAME
// header the kernels include (deepspeed_amd/ops/csrc/flash_bwd_layout.h) and
// emulates, on an image filled through the DMA source map with distinct
// values:
//   - the 16-byte row read, against the A operand T[16*rt + l15][32*ks +
//     8*l4 + j];
//   - the transposed read (per 16-lane group, lane 4q+p addresses row q,
//     columns 4p .. 4p+3; lane i receives column i, row q in element q),
//     against T^T[16*dt + l15][k], k = 4*l4 + j (j < 4), 16 + 4*l4 + j - 4;
//   - bounds and alignment of every address;
//   - the bank conflict degree, bank = (a/4) mod 64: per 32-lane half for
//     the transposed read, per ds_read_b128 lane group for the row read.
//
// usage: flash_bwd_layout_check [mutant]
//   mutant 0 (default) the header's addresses
//   mutant 1 transposed read without the XOR on rows with (row & 7) == 5
//   mutant 2 transposed read with the two 8-byte halves of a chunk swapped
// Prints one line per head dim: "D <d> frag <ok|bad> addr <ok|bad> tr_conflict
// <n> row_conflict <n>"; exit status 1 when a fragment or an address is wrong.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "flash_bwd_layout.h"

namespace L = bwd_layout;

static int g_mutant = 0;

template <int DH>
static int tr_addr(int lane, int dt, int hf) {
  const int l15 = lane & 15, l4 = lane >> 4;
  const int q = l15 >> 2, p = l15 & 3;
  const int row = 16 * hf + 4 * l4 + q;
  if (g_mutant == 1 && (row & 7) == 5) return row * (DH * 2) + 32 * dt + 8 * p;
  if (g_mutant == 2) return L::img_off<DH>(row, 32 * dt + 8 * (p ^ 1));
  return L::tr_read_addr<DH>(lane, dt, hf);
}

// max number of distinct dwords that one bank serves within a lane group
static int conflict_degree(const std::vector<int>& lanes,
                           const std::vector<int>& addr, int bytes) {
  std::map<int, std::set<int>> per_bank;
  for (int l : lanes)
    for (int b = 0; b < bytes; b += 4)
      per_bank[((addr[l] + b) / 4) % 64].insert((addr[l] + b) / 4);
  size_t worst = 0;
  for (auto& kv : per_bank) worst = kv.second.size() > worst ? kv.second.size() : worst;
  return (int)worst;
}

template <int DH>
static bool check() {
  constexpr int IMG = L::TS * DH * 2;
  std::vector<unsigned short> lds(IMG / 2, 0xffff);
  std::vector<int> written(IMG / 2, 0);
  auto T = [](int row, int col) { return (unsigned short)(row * DH + col); };

  // fill as the kernel does: LDS-linear 16-byte pieces, swizzled source
  for (int linear = 0; linear < IMG; linear += 16) {
    const int row = L::dma_row<DH>(linear);
    const int src = L::dma_src_byte<DH>(linear);
    for (int e = 0; e < 8; ++e) {
      lds[linear / 2 + e] = T(row, src / 2 + e);
      written[linear / 2 + e]++;
    }
  }
  bool frag_ok = true, addr_ok = true;
  for (int w : written) frag_ok &= (w == 1);
  // the fill and img_off agree
  for (int row = 0; row < L::TS; ++row)
    for (int col = 0; col < DH; ++col)
      frag_ok &= lds[L::img_off<DH>(row, col * 2) / 2] == T(row, col);

  int tr_conf = 0, row_conf = 0;
  // ---- row reads --------------------------------------------------------
  static const int groups[4][16] = {
      {0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
      {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
      {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
      {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
  for (int rt = 0; rt < 2; ++rt)
    for (int ks = 0; ks < DH / 32; ++ks) {
      std::vector<int> addr(64);
      for (int lane = 0; lane < 64; ++lane) {
        const int a = addr[lane] = L::row_read_addr<DH>(lane, rt, ks);
        addr_ok &= a >= 0 && a + 16 <= IMG && a % 16 == 0;
        if (!(a >= 0 && a + 16 <= IMG)) continue;
        const int l15 = lane & 15, l4 = lane >> 4;
        for (int j = 0; j < 8; ++j)
          frag_ok &= lds[a / 2 + j] == T(16 * rt + l15, 32 * ks + 8 * l4 + j);
      }
      for (auto& g : groups) {
        const int c = conflict_degree(std::vector<int>(g, g + 16), addr, 16);
        row_conf = c > row_conf ? c : row_conf;
      }
    }
  // ---- transposed reads -------------------------------------------------
  for (int dt = 0; dt < DH / 16; ++dt) {
    unsigned short frag[64][8];
    for (int hf = 0; hf < 2; ++hf) {
      std::vector<int> addr(64);
      for (int lane = 0; lane < 64; ++lane) {
        const int a = addr[lane] = tr_addr<DH>(lane, dt, hf);
        addr_ok &= a >= 0 && a + 8 <= IMG && a % 8 == 0;
      }
      if (!addr_ok) break;
      for (int lane = 0; lane < 64; ++lane) {
        const int g = lane >> 4, i = lane & 15;
        for (int q = 0; q < 4; ++q)  // column i of row q: lane 4q + i/4
          frag[lane][4 * hf + q] =
              lds[addr[16 * g + 4 * q + (i >> 2)] / 2 + (i & 3)];
      }
      for (int half = 0; half < 2; ++half) {
        std::vector<int> lanes;
        for (int l = 32 * half; l < 32 * half + 32; ++l) lanes.push_back(l);
        const int c = conflict_degree(lanes, addr, 8);
        tr_conf = c > tr_conf ? c : tr_conf;
      }
    }
    if (!addr_ok) break;
    for (int lane = 0; lane < 64; ++lane) {
      const int l15 = lane & 15, l4 = lane >> 4;
      for (int j = 0; j < 8; ++j) {
        const int k = j < 4 ? 4 * l4 + j : 16 + 4 * l4 + j - 4;
        frag_ok &= frag[lane][j] == T(k, 16 * dt + l15);
      }
    }
  }
  std::printf("D %d frag %s addr %s tr_conflict %d row_conflict %d\n", DH,
              frag_ok ? "ok" : "bad", addr_ok ? "ok" : "bad", tr_conf,
              row_conf);
  return frag_ok && addr_ok;
}

int main(int argc, char** argv) {
  if (argc > 1) g_mutant = std::atoi(argv[1]);
  bool ok = check<64>();
  ok &= check<128>();
  return ok ? 0 : 1;
}
