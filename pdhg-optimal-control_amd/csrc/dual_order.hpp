// Which (x tile, y strip) of the dual sweep's launch grid a workgroup runs (k_dual_lds_2d).  Plain C++: a host
// program can include this file without the HIP kernels (tests/test_dual_order_host.py does).
//
// The hardware hands out workgroups in linear order L = blockIdx.x + gridDim.x * blockIdx.y, round-robin over the
// 8 XCDs: workgroup L runs on XCD L % 8 as that XCD's slot L / 8, and the workgroups resident at one moment are a
// run of consecutive L.
//
// band = 0 (x-fastest, the order the sweep always had): tile = (xcd_remap(blockIdx.x), blockIdx.y).  The resident
// workgroups are different x tiles of ONE y strip: the chip streams every array as strip-wide runs (1 KiB in fp64
// FR) at a pitch of one grid row, so the address bits between the strip width and the row length are the same for
// every request in flight.
//
// band = XB > 0 (band order): XCD c owns the contiguous x tiles [c gx/8, (c+1) gx/8) and walks them in bands of XB
// tiles x gy/XB strips, y strips fastest, then the XB tiles, then the band's strip groups, then the next band.  With
// XB = 1 the gy workgroups an XCD starts together cover whole grid rows (RX rows x ny contiguous per array and
// step), a band's strip-edge exchange (p.ey) stays inside one L2, and the next band's halo rows x0-1 are the rows
// that L2 read last.  XB = 2 / 4 trade row coverage for x-halo sharing inside a band.
//
// Both are bijections of [0, gx gy) onto the tiles for every grid: the x tiles past the last multiple of 8 (all of
// them when gx < 8) are run x-fastest by the workgroups after the banded part, as xcd_remap leaves its tail in place;
// an XB that does not divide both gx/8 and gy is halved until it does.  Speed only, never correctness.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PDHG_HD __host__ __device__ __forceinline__
#else
#define PDHG_HD inline
#endif

namespace pdhg {

// XCD-aware block index remap: hardware deals consecutive workgroups round-robin
// over the 8 XCDs; remap so each XCD walks a contiguous range of logical blocks
// (neighbouring tiles share that XCD's L2).  Speed only, never correctness.
PDHG_HD int xcd_remap(int b, int nblocks) {
  const int per = nblocks >> 3;            // blocks per XCD in the full part
  const int full = per << 3;
  if (b >= full) return b;                 // tail keeps identity mapping
  return (b & 7) * per + (b >> 3);
}

// its inverse: the block index b with xcd_remap(b, nblocks) == t
PDHG_HD int xcd_unmap(int t, int nblocks) {
  const int per = nblocks >> 3;
  const int full = per << 3;
  if (t >= full) return t;
  return (t % per) * 8 + t / per;
}

struct DualTile {
  int xt, ys;   // x tile in [0, gx), y strip in [0, gy)
};

// linear dispatch index L in [0, gx gy) -> tile; band: 0 = x-fastest, XB > 0 = band order (see above)
PDHG_HD DualTile dual_tile(int L, int gx, int gy, int band) {
  if (band <= 0) return DualTile{xcd_remap(L % gx, gx), L / gx};
  const int per = gx >> 3, full = per << 3;   // x tiles per XCD, banded x tiles
  const int nband = full * gy;
  if (L >= nband) {                           // tail tiles [full, gx): x-fastest
    const int rem = gx - full, l = L - nband;
    return DualTile{full + l % rem, l / rem};
  }
  int xb = band;
  while (xb > 1 && (per % xb != 0 || gy % xb != 0)) xb >>= 1;
  const int c = L & 7, s = L >> 3;            // XCD, its slot in [0, per gy)
  const int ysub = gy / xb;                   // strips per band
  const int grp = s / gy, in = s % gy;        // group of gy slots = one band of xb tiles x ysub strips
  const int xband = grp / xb, sg = grp % xb;  // x band of the XCD, strip group inside it
  return DualTile{c * per + xband * xb + in / ysub, sg * ysub + in % ysub};
}

}  // namespace pdhg
