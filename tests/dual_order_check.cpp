// Stand-alone check of csrc/dual_order.hpp (built and run by test_dual_order_host.py with the host compiler under
// -fsanitize=address,undefined): for every grid and order, dual_tile is a bijection of the dispatch indices onto the
// gx x gy tiles, order 0 is the formula the sweep always had, and xcd_unmap inverts xcd_remap (the partial row).
#include <cstdio>
#include <vector>

#include "dual_order.hpp"

// the x-fastest order as k_dual_lds_2d computed it from blockIdx before dual_order.hpp, written out again here
static int old_remap(int b, int nblocks) {
  const int per = nblocks >> 3, full = per << 3;
  return b >= full ? b : (b & 7) * per + (b >> 3);
}

int main() {
  std::vector<int> gxs, gys;
  for (int g = 1; g <= 40; ++g) gxs.push_back(g);
  gxs.push_back(64);
  gxs.push_back(512);
  for (int g = 1; g <= 8; ++g) gys.push_back(g);
  gys.push_back(32);
  const int bands[] = {0, 1, 2, 4};
  long checked = 0;
  int bad = 0;
  for (int gx : gxs)
    for (int gy : gys)
      for (int band : bands) {
        std::vector<int> hit((size_t)gx * gy, 0);
        for (int by = 0; by < gy; ++by)
          for (int bx = 0; bx < gx; ++bx) {
            const int L = bx + gx * by;
            const pdhg::DualTile t = pdhg::dual_tile(L, gx, gy, band);
            if (t.xt < 0 || t.xt >= gx || t.ys < 0 || t.ys >= gy) {
              if (bad++ < 10) printf("out of range: gx %d gy %d band %d L %d -> (%d, %d)\n", gx, gy, band, L, t.xt, t.ys);
              continue;
            }
            ++hit[(size_t)t.ys * gx + t.xt];
            if (band == 0 && (t.xt != old_remap(bx, gx) || t.ys != by)) {
              if (bad++ < 10) printf("order 0 differs: gx %d gy %d L %d -> (%d, %d)\n", gx, gy, L, t.xt, t.ys);
            }
            // the partial row: the block index that ran this tile under the x-fastest order
            const int ub = pdhg::xcd_unmap(t.xt, gx);
            if (ub < 0 || ub >= gx || old_remap(ub, gx) != t.xt) {
              if (bad++ < 10) printf("xcd_unmap: gx %d tile %d -> block %d\n", gx, t.xt, ub);
            }
            // banded part: workgroup L (XCD L % 8) runs a tile of that XCD's contiguous x range
            if (band > 0 && L < (gx >> 3) * 8 * gy && t.xt / (gx >> 3) != (L & 7)) {
              if (bad++ < 10) printf("band: gx %d gy %d band %d L %d -> x tile %d of another XCD\n", gx, gy, band, L, t.xt);
            }
            ++checked;
          }
        for (size_t i = 0; i < hit.size(); ++i)
          if (hit[i] != 1) {
            if (bad++ < 10)
              printf("gx %d gy %d band %d: tile (%d, %d) covered %d times\n", gx, gy, band, (int)(i % gx), (int)(i / gx), hit[i]);
          }
      }
  // band order, XB = 1, C3's fp64 grid: the 32 first slots of XCD 0 are the 32 strips of x tile 0
  for (int s = 0; s < 32; ++s) {
    const pdhg::DualTile t = pdhg::dual_tile(8 * s, 512, 32, 1);
    if (t.xt != 0 || t.ys != s) {
      if (bad++ < 10) printf("C3 band: slot %d -> (%d, %d)\n", s, t.xt, t.ys);
    }
  }
  printf("%ld tiles checked, %d bad\n", checked, bad);
  return bad ? 1 : 0;
}
