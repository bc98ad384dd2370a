// item_groups_main.cpp -- drives paos_amd/csrc/item_groups.h from stdin for tests/test_item_groups_host.py (compiled with
// the address and undefined-behaviour sanitizers; no GPU, no library).  Doubles travel as the 16 hex digits of their bits, so
// that a NaN's payload and the sign of a zero arrive as they were sent.  Commands, one per line:
//   groups B STRIDE SKIP   then B rows "PART V.."        -> goff / glen / members of group_items (joins: same_record)
//   maps B STRIDE ENABLE SKIP SHARE   then B rows "V.."  -> goff / glen / members of map_groups
//   subs B STRIDE ENABLE SKIP SHARE   then B rows "KEY V.." (items with one KEY start from one field)
//                                                        -> lead / same, then subs / goff / glen / members of split_by_map
//   reps B STRIDE   then B rows "FLAG V.."               -> power_of / compute
//   sameas B SELF   then one row of B values              -> valid 0 | 1
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "../paos_amd/csrc/item_groups.h"

static double read_bits() {
  std::string tok;
  std::cin >> tok;
  const uint64_t u = std::stoull(tok, nullptr, 16);
  double d;
  std::memcpy(&d, &u, sizeof d);
  return d;
}

static void print(const char* name, const std::vector<double>& v) {
  std::printf("%s", name);
  for (double x : v) std::printf(" %d", (int)x);
  std::printf("\n");
}

static void print(const ItemGroups& g) {
  print("goff", g.goff);
  print("glen", g.glen);
  print("members", g.members);
}

int main() {
  std::string cmd;
  while (std::cin >> cmd) {
    int batch = 0;
    std::cin >> batch;
    if (cmd == "sameas") {
      int self = 0;
      std::cin >> self;
      std::vector<double> same_as(batch);
      for (double& s : same_as) s = read_bits();
      std::printf("valid %d\n", same_as_valid(same_as.data(), batch, self != 0) ? 1 : 0);
      continue;
    }
    int stride = 0, enable = 0, skip = -1, share = 1;
    std::cin >> stride;
    if (cmd == "groups") std::cin >> skip;
    if (cmd == "maps" || cmd == "subs") std::cin >> enable >> skip >> share;
    const bool tagged = cmd != "maps";  // a leading integer per row: PART, KEY or FLAG
    std::vector<double> tag(batch, 0.0), rec((size_t)batch * stride);
    for (int i = 0; i < batch; ++i) {
      if (tagged) std::cin >> tag[i];
      for (int k = 0; k < stride; ++k) rec[(size_t)i * stride + k] = read_bits();
    }
    const double* r = rec.data();
    if (cmd == "groups") {
      print(group_items(
          batch, [&](int j, int i) { return same_record(r + (size_t)j * stride, r + (size_t)i * stride, stride, skip); },
          [&](int i) { return tag[i] != 0.0; }));
    } else if (cmd == "maps") {
      print(map_groups(batch, r, stride, enable, skip, share != 0));
    } else if (cmd == "subs") {
      ItemGroups g = group_items(batch, [&](int j, int i) { return tag[j] == tag[i]; }, [](int) { return true; });
      std::vector<double> lead, same;
      group_leaders(g, lead, same);
      print("lead", lead);
      print("same", same);
      print("subs", split_by_map(g, r, stride, enable, skip, share != 0));
      print(g);
    } else if (cmd == "reps") {
      std::vector<double> power_of, compute;
      power_representatives(batch, r, stride, tag.data(), power_of, compute);
      print("power_of", power_of);
      print("compute", compute);
    } else {
      std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
