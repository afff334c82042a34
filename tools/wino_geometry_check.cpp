// Sweeps the host-side launch geometry the Winograd translation units share (csrc/conv_wino_common.h: the persistent
// grid of the forward / data-gradient launches, the slab split of the weight gradients, the work share) over every CU
// budget, column-block count, tile-block count and chunk count the planners can pass, and checks its invariants.  Needs
// no device.  A stand-alone program, so that the code can run under the sanitizers:
//
//   hipcc -std=c++17 -O1 -g -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer \
//       -c tools/wino_geometry_check.cpp -o /tmp/wino_geometry_check.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined -o /tmp/wino_geometry_check /tmp/wino_geometry_check.o
//   /tmp/wino_geometry_check        # exit status 0 and "ok", no sanitizer report
#include <cstdio>

#include "../image-generation_amd/csrc/conv_wino_common.h"

using namespace dvg;

static long g_bad = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      if (g_bad++ < 20) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                     \
  } while (0)

int main() {
  long n = 0;
  for (int cus = 0; cus <= 300; ++cus)
    for (int ny = 1; ny <= 16; ++ny) {
      const int budget = wino_cu_budget(cus, ny);
      CHECK(budget >= ny && budget <= 256 && (cus <= 0 || cus > 256 || cus < ny || budget == cus), "cus=%d ny=%d budget=%d", cus, ny, budget);
      for (int nblk = 1; nblk <= 4096; ++nblk, ++n) {
        const int gx = wino_grid_width(cus, ny, nblk);
        CHECK(gx >= 1 && gx <= nblk && gx * ny <= (budget > ny ? budget : ny), "cus=%d ny=%d nblk=%d gx=%d", cus, ny, nblk, gx);
        // the static deal's shrunken grid keeps the round count, and no narrower grid does
        const int gs = wino_grid_static(gx, nblk), rounds = (nblk + gx - 1) / gx;
        CHECK(gs >= 1 && gs <= gx && (nblk + gs - 1) / gs == rounds, "cus=%d ny=%d nblk=%d gx=%d static=%d", cus, ny, nblk, gx, gs);
        CHECK(gs == 1 || (nblk + gs - 2) / (gs - 1) > rounds, "cus=%d ny=%d nblk=%d gx=%d static=%d is not the narrowest", cus, ny, nblk, gx, gs);
        // what the launchers call: the full width under the dynamic deal (three rounds or more), else the shrunken grid
        for (int may_deal = 0; may_deal <= 1; ++may_deal) {
          const WinoGridPlan p = wino_grid_plan(cus, ny, nblk, may_deal != 0);
          CHECK(p.dynamic == (may_deal && nblk >= 3 * gx) && p.gx == (p.dynamic ? gx : gs), "cus=%d ny=%d nblk=%d may_deal=%d plan=(%d, %d)",
                cus, ny, nblk, may_deal, p.gx, (int)p.dynamic);
          CHECK(p.gx >= 1 && p.gx <= nblk && p.gx * ny <= (budget > ny ? budget : ny) && (nblk + p.gx - 1) / p.gx == rounds,
                "cus=%d ny=%d nblk=%d may_deal=%d plan gx=%d", cus, ny, nblk, may_deal, p.gx);
        }
        const float share = wino_work_share((unsigned)(gx * ny));
        CHECK(share > 0.f && share <= 1.f, "cus=%d ny=%d nblk=%d share=%f", cus, ny, nblk, (double)share);
      }
    }
  // workgroups per slab: every product of channel tiles and position groups the weight-gradient shapes give, and odd ones
  const int wgs_list[] = {1, 2, 3, 4, 6, 8, 16, 24, 32, 64, 128, 256, 512};
  for (int wgs : wgs_list)
    for (int cus = 0; cus <= 300; ++cus)
      for (int chunks = 1; chunks <= 8192; ++chunks, ++n) {
        const WinoSlabs s = wino_slab_split(chunks, wgs, cus);
        CHECK(s.want >= 1 && s.per >= 1 && s.nsplit >= 1 && s.nsplit <= s.want, "chunks=%d wgs=%d cus=%d want=%d per=%d nsplit=%d",
              chunks, wgs, cus, s.want, s.per, s.nsplit);
        CHECK((long)(s.nsplit - 1) * s.per < chunks && chunks <= (long)s.nsplit * s.per, "chunks=%d wgs=%d cus=%d per=%d nsplit=%d: not a cover",
              chunks, wgs, cus, s.per, s.nsplit);
        CHECK((long)s.want * s.per >= chunks, "chunks=%d wgs=%d cus=%d want=%d per=%d", chunks, wgs, cus, s.want, s.per);
        CHECK(s.want == 1 || (s.want <= chunks / 8 && (long)s.want * wgs <= cus), "chunks=%d wgs=%d cus=%d want=%d: deeper than 8 chunks, within the budget",
              chunks, wgs, cus, s.want);
      }
  std::printf("%s: %ld geometries, %ld failed checks\n", g_bad ? "FAILED" : "ok", n, g_bad);
  return g_bad ? 1 : 0;
}
