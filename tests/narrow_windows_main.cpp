// narrow_windows_main.cpp -- drives pick_narrow of paos_amd/csrc/pass_program.h from stdin for
// tests/test_narrow_windows_host.py: does a launch take the narrow-window variant of its central-half build?  Compiled with
// the address and undefined-behaviour sanitizers; no GPU, no library.  Any number of questions, each:
//   launch N BATCH CENTRAL SWITCH COUNT      grid size, items, FrugalBuild::central, PAOS_NARROW_WINDOWS, passes in the launch
//   then per item: ACTIVE POS_LO POS_HI SPOS_LO SPOS_HI   loads of the launch's first pass, stores of its last one
// An inactive item is inactive in every pass.  The passes between the first and the last (COUNT = 3) and the fields the
// decision must not read -- the stores of the first pass and the loads of the last one of a launch of several -- span whole lines.
// Output per question: "narrow 0" or "narrow 1".
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "../paos_amd/csrc/pass_program.h"
#include "../paos_amd/csrc/pass_records.h"

int main() {
  std::string cmd;
  while (std::cin >> cmd) {
    if (cmd != "launch") return 2;
    PlanDims d{};
    FrugalBuild b{};
    int count = 0;
    std::cin >> d.n >> d.batch >> b.central >> d.narrow_windows >> count;
    if (!std::cin || count < 1 || count > 3 || d.batch < 1) return 2;
    d.br = 4; d.precision = PAOS_F64; d.central_half = 1;
    std::vector<LoweredPass> low(count);
    for (LoweredPass& lp : low) {
      lp.ok = true;
      lp.items.assign(d.batch, FrugalItem{});
    }
    for (int it = 0; it < d.batch; ++it) {
      double active, pos_lo, pos_hi, spos_lo, spos_hi;
      std::cin >> active >> pos_lo >> pos_hi >> spos_lo >> spos_hi;
      if (!std::cin) return 2;
      for (int k = 0; k < count; ++k) {
        FrugalItem& fi = low[k].items[it];
        fi.active = active;
        fi.line_lo = 0.0; fi.line_hi = (double)d.n;
        fi.pos_lo = k == 0 ? pos_lo : 0.0; fi.pos_hi = k == 0 ? pos_hi : (double)d.n;
        fi.spos_lo = k == count - 1 ? spos_lo : 0.0; fi.spos_hi = k == count - 1 ? spos_hi : (double)d.n;
      }
    }
    Launch g;
    g.count = count;
    for (int k = 0; k < count; ++k) g.lp[k] = &low[k];
    std::printf("narrow %d\n", pick_narrow(d, g, b));
  }
  return 0;
}
