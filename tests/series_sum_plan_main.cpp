// Stand-alone driver of paos_amd/csrc/series_sum_plan.h for tests/test_series_sum_plan_host.py (built with the sanitizers
// there).  stdin: lines "size <frames> <nx> <ny>", "fits <doubles>", "ranges <frames>" or "tiles <npix> <threads>".
// stdout, per line: "size <0|1> <doubles>", "fits <0|1>", "ranges : <t0> <nt> ; ..." or "tiles <count>".
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "../paos_amd/csrc/series_sum_plan.h"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    in >> what;
    if (what == "size") {
      int frames = 0, nx = 0, ny = 0;
      in >> frames >> nx >> ny;
      size_t doubles = 0;
      const bool ok = paos::series_sum_size(frames, nx, ny, &doubles);
      std::printf("size %d %llu\n", ok ? 1 : 0, (unsigned long long)doubles);
    } else if (what == "fits") {
      unsigned long long doubles = 0;
      in >> doubles;
      std::printf("fits %d\n", paos::series_sum_fits((size_t)doubles) ? 1 : 0);
    } else if (what == "ranges") {
      int frames = 0;
      in >> frames;
      std::printf("ranges :");
      paos::SeriesSumRange r{0, 0};
      int count = 0;
      while (paos::series_sum_next_range(frames, &r)) {
        if (++count > 100) return 2;  // (a walk that does not end)
        std::printf(" %d %d ;", r.t0, r.nt);
      }
      std::printf("\n");
    } else if (what == "tiles") {
      unsigned long long npix = 0;
      int threads = 0;
      in >> npix >> threads;
      std::printf("tiles %u\n", paos::series_sum_tiles((size_t)npix, threads));
    } else if (!what.empty()) {
      return 1;
    }
  }
  return 0;
}
