// Stand-alone driver of paos_amd/csrc/series_plan.h for tests/test_series_plan_host.py (built with the sanitizers there).
// stdin: lines "plan <batch> <frames> <npix> <cap>" or "cap <fallback> [<text of the environment variable>]".
// stdout, per line: "plan <items> <frames> <bytes> : <t0> <nt> <i0> <ni> ; ..." or "cap <bytes>".
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "../paos_amd/csrc/series_plan.h"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    in >> what;
    if (what == "plan") {
      int batch = 0, frames = 0;
      unsigned long long npix = 0, cap = 0;
      in >> batch >> frames >> npix >> cap;
      const paos::SeriesPlan p = paos::series_plan(batch, frames, (size_t)npix, (size_t)cap);
      std::printf("plan %d %d %llu :", p.items, p.frames, (unsigned long long)paos::series_plan_bytes(p, (size_t)npix));
      paos::SeriesChunk c{0, 0, 0, 0};
      int count = 0;
      while (paos::series_next_chunk(p, batch, frames, &c)) {
        if (++count > 200000) return 2;  // (a plan that does not end)
        std::printf(" %d %d %d %d ;", c.t0, c.nt, c.i0, c.ni);
      }
      std::printf("\n");
    } else if (what == "cap") {
      unsigned long long fallback = 0;
      std::string text;
      in >> fallback;
      const bool given = static_cast<bool>(in >> text);
      std::printf("cap %llu\n", (unsigned long long)paos::series_cap_bytes(given ? text.c_str() : nullptr, (size_t)fallback));
    } else if (!what.empty()) {
      return 1;
    }
  }
  return 0;
}
