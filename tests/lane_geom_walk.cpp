// mind_amd/csrc/lane_geom.h compiled alone, on the CPU, with a main of its own (tests/test_lane_host.py builds it with the address and
// undefined-behaviour sanitizers and feeds it the edge cases): lg_cum and lg_box_lanes over the lanes and poses read from stdin, every
// number a C99 hexadecimal float, so that nothing is lost on the way in or out.  Built with -ffp-contract=off (the header's contract).
//   in:  P, lane_off[P + 1], verts[2 V], cos_flow, bound, off, n, then n rows (x, y, cos, sin)
//   out: n rows: margin, then (lat, s, along, across, lane, edge) of `any` and of `flow`
#include <cmath>
#include <cstdio>
#include <vector>
#include "lane_geom.h"

int main() {
  int P = 0, n = 0;
  if (std::scanf("%d", &P) != 1 || P < 1) return 2;
  std::vector<int> off((size_t)P + 1);
  for (int &o : off)
    if (std::scanf("%d", &o) != 1) return 2;
  const int V = off[P];
  std::vector<double> verts((size_t)V * 2), cum((size_t)V);
  for (double &v : verts)
    if (std::scanf("%la", &v) != 1) return 2;
  double cos_flow, bound, boff;
  if (std::scanf("%la %la %la %d", &cos_flow, &bound, &boff, &n) != 4) return 2;
  lg_cum(verts.data(), off.data(), P, cum.data());
  for (int i = 0; i < n; ++i) {
    double x, y, c, s;
    if (std::scanf("%la %la %la %la", &x, &y, &c, &s) != 4) return 2;
    lg_out o[2];
    const double m = lg_box_lanes(x, y, c, s, boff, cos_flow, bound, verts.data(), off.data(), P, cum.data(), o);
    std::printf("%a", m);
    for (int k = 0; k < 2; ++k) std::printf(" %a %a %a %a %d %d", o[k].lat, o[k].s, o[k].along, o[k].across, o[k].lane, o[k].edge);
    std::printf("\n");
  }
  return 0;
}
