// Host-only proof of the flash forward's LDS image layout. Includes the SAME
// header the kernel includes (deepspeed_amd/ops/csrc/flash_fwd_layout.h) and
// emulates, on K and V images filled through the DMA source maps with
// distinct values:
//   - K's 16-byte row read, against the A operand of S^T = K Q^T in lane
//     (l31, hi): K[32*mt + l31][16*ks + 8*hi + j];
//   - V's transposed reads (per 16-lane group, lane 4q+p addresses row q,
//     columns 4p .. 4p+3; lane i receives column i, row q in element q),
//     against the A operand of O^T += V^T P^T in lane (l31, hi):
//     V[16*ks + 8*hi + j][32*mt + l31], j = 0..7 (the P fragment's k order);
//   - bounds and alignment of every address, and that the fill writes every
//     byte of an image exactly once;
//   - the bank conflict degree, bank = (a/4) mod 64: per 32-lane half for
//     the transposed read, per ds_read_b128 lane group for the row read. For
//     the record it also counts the row read under the ((row&7)<<4) swizzle
//     this layout replaced.
//
// usage: flash_fwd_layout_check [mutant]
//   mutant 0 (default) the header's addresses
//   mutant 1 transposed read without the XOR on rows with (row & 3) == 1
//            (D 128) / (row & 3) == 2 (D 64)
//   mutant 2 transposed read with the two 8-byte halves of a chunk swapped
// Prints one line per head dim: "D <d> frag <ok|bad> addr <ok|bad> tr_conflict
// <n> row_conflict <n> old_row_conflict <n>"; exit status 1 when a fragment or
// an address is wrong.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <vector>

#include "flash_fwd_layout.h"

namespace L = fwd_layout;

static int g_mutant = 0;

template <int DH>
static int tr_addr(int lane, int mt, int ks, int hf) {
  const int l15 = lane & 15, g = lane >> 4;
  const int hi = g >> 1, dh = g & 1;
  const int q = l15 >> 2, p = l15 & 3;
  const int row = 16 * ks + 8 * hi + 4 * hf + q;
  const int byte = 64 * mt + 32 * dh + 8 * p;
  if (g_mutant == 1 && (row & 3) == (DH == 128 ? 1 : 2))
    return row * (DH * 2) + byte;
  if (g_mutant == 2) return L::v_off<DH>(row, byte ^ 8);
  return L::v_tr_read_addr<DH>(lane, mt, ks, hf);
}

// max number of distinct dwords that one bank serves within a lane group
static int conflict_degree(const std::vector<int>& lanes,
                           const std::vector<int>& addr, int bytes) {
  std::map<int, std::set<int>> per_bank;
  for (int l : lanes)
    for (int b = 0; b < bytes; b += 4)
      per_bank[((addr[l] + b) / 4) % 64].insert((addr[l] + b) / 4);
  size_t worst = 0;
  for (auto& kv : per_bank)
    worst = kv.second.size() > worst ? kv.second.size() : worst;
  return (int)worst;
}

static const int kGroups[4][16] = {
    {0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
    {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
    {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
    {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};

static int b128_degree(const std::vector<int>& addr) {
  int worst = 0;
  for (auto& g : kGroups) {
    const int c = conflict_degree(std::vector<int>(g, g + 16), addr, 16);
    worst = c > worst ? c : worst;
  }
  return worst;
}

template <int DH>
static bool check() {
  constexpr int IMG = L::KT * DH * 2;
  auto T = [](int row, int col) { return (unsigned short)(row * DH + col); };
  bool frag_ok = true, addr_ok = true;

  // fill as the kernel does: LDS-linear 16-byte pieces, swizzled source
  std::vector<unsigned short> kimg(IMG / 2, 0xffff), vimg(IMG / 2, 0xffff);
  std::vector<int> kw(IMG / 2, 0), vw(IMG / 2, 0);
  for (int linear = 0; linear < IMG; linear += 16) {
    const int row = L::dma_row<DH>(linear);
    const int ksrc = L::k_dma_src_byte<DH>(linear);
    const int vsrc = L::v_dma_src_byte<DH>(linear);
    addr_ok &= row >= 0 && row < L::KT;
    addr_ok &= ksrc >= 0 && ksrc + 16 <= DH * 2 && ksrc % 16 == 0;
    addr_ok &= vsrc >= 0 && vsrc + 16 <= DH * 2 && vsrc % 16 == 0;
    if (!addr_ok) break;
    for (int e = 0; e < 8; ++e) {
      kimg[linear / 2 + e] = T(row, ksrc / 2 + e);
      vimg[linear / 2 + e] = T(row, vsrc / 2 + e);
      kw[linear / 2 + e]++;
      vw[linear / 2 + e]++;
    }
  }
  for (int w : kw) frag_ok &= (w == 1);
  for (int w : vw) frag_ok &= (w == 1);
  // the fill and the offset functions agree
  for (int row = 0; row < L::KT && addr_ok; ++row)
    for (int col = 0; col < DH; ++col) {
      frag_ok &= kimg[L::k_off<DH>(row, col * 2) / 2] == T(row, col);
      frag_ok &= vimg[L::v_off<DH>(row, col * 2) / 2] == T(row, col);
    }

  int tr_conf = 0, row_conf = 0, old_row_conf = 0;
  // ---- K row reads --------------------------------------------------------
  for (int mt = 0; mt < 2 && addr_ok; ++mt)
    for (int ks = 0; ks < DH / 16; ++ks) {
      std::vector<int> addr(64), old_addr(64);
      for (int lane = 0; lane < 64; ++lane) {
        const int a = addr[lane] = L::k_row_read_addr<DH>(lane, mt, ks);
        const int l31 = lane & 31, hi = lane >> 5;
        const int row = 32 * mt + l31;
        old_addr[lane] =
            row * (DH * 2) + (((16 * ks + 8 * hi) * 2) ^ ((row & 7) << 4));
        const bool in = a >= 0 && a + 16 <= IMG;
        addr_ok &= in && a % 16 == 0;
        if (!in) continue;
        for (int j = 0; j < 8; ++j)
          frag_ok &= kimg[a / 2 + j] == T(row, 16 * ks + 8 * hi + j);
      }
      const int c = b128_degree(addr), o = b128_degree(old_addr);
      row_conf = c > row_conf ? c : row_conf;
      old_row_conf = o > old_row_conf ? o : old_row_conf;
    }
  // ---- V transposed reads -------------------------------------------------
  for (int mt = 0; mt < DH / 32 && addr_ok; ++mt)
    for (int ks = 0; ks < 4 && addr_ok; ++ks) {
      unsigned short frag[64][8];
      for (int hf = 0; hf < 2; ++hf) {
        std::vector<int> addr(64);
        for (int lane = 0; lane < 64; ++lane) {
          const int a = addr[lane] = tr_addr<DH>(lane, mt, ks, hf);
          addr_ok &= a >= 0 && a + 8 <= IMG && a % 8 == 0;
        }
        if (!addr_ok) break;
        for (int lane = 0; lane < 64; ++lane) {
          const int g = lane >> 4, i = lane & 15;
          for (int q = 0; q < 4; ++q)  // column i of row q: lane 4q + i/4
            frag[lane][4 * hf + q] =
                vimg[addr[16 * g + 4 * q + (i >> 2)] / 2 + (i & 3)];
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
        const int l31 = lane & 31, hi = lane >> 5;
        for (int j = 0; j < 8; ++j)
          frag_ok &= frag[lane][j] == T(16 * ks + 8 * hi + j, 32 * mt + l31);
      }
    }
  std::printf(
      "D %d frag %s addr %s tr_conflict %d row_conflict %d "
      "old_row_conflict %d\n",
      DH, frag_ok ? "ok" : "bad", addr_ok ? "ok" : "bad", tr_conf, row_conf,
      old_row_conf);
  return frag_ok && addr_ok;
}

int main(int argc, char** argv) {
  if (argc > 1) g_mutant = std::atoi(argv[1]);
  bool ok = check<64>();
  ok &= check<128>();
  return ok ? 0 : 1;
}
