// arena_layout_main.cpp -- drives paos_amd/csrc/arena_layout.h from stdin for tests/test_arena_layout_host.py (compiled with
// the address and undefined-behaviour sanitizers; no GPU, no library).  The program plays the part of context.hip: one slab
// of CAP doubles in ordinary memory, written where the layout says (so that a block past the slab's end is an error the
// sanitizer reports), a switch of slabs is a rewind, a growth a larger slab.  First line: CAP.  Then one command per line:
//   batch          -> a new batch object                      (prints nothing)
//   begin TOTAL    -> "begin fits|switch|grow CAP HEAD"       room for TOTAL doubles in one slab, before the first block
//   add COUNT      -> "add OFFSET HEAD" | "add switch OFFSET HEAD" (it went to a fresh slab) | "add refused closed|room|size"
//   commit         -> "commit FIRST COUNT" | "commit none"    the range one copy would move
//   drop           -> "drop"                                  an error path: nothing pending any more
//   state          -> "state HEAD SENT PENDING"
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "../paos_amd/csrc/arena_layout.h"

int main() {
  size_t cap = 0;
  std::cin >> cap;
  ArenaLayout lay;
  lay.cap = cap;
  std::vector<double> slab(cap, 0.0);
  ArenaBatchState st;
  double stamp = 1.0;  // every block is filled with a value of its own
  std::string cmd;
  while (std::cin >> cmd) {
    if (cmd == "batch") {
      st = ArenaBatchState{};
    } else if (cmd == "begin") {
      size_t total = 0;
      std::cin >> total;
      const ArenaRoom room = lay.room(total);
      if (room == ARENA_SWITCH) lay.rewind();
      if (room == ARENA_GROW) {
        lay.cap = lay.grown(total);
        lay.rewind();
        slab.assign(lay.cap, 0.0);
      }
      st.reserved = true;
      std::printf("begin %s %zu %zu\n", room == ARENA_FITS ? "fits" : (room == ARENA_SWITCH ? "switch" : "grow"), lay.cap, lay.head);
    } else if (cmd == "add") {
      size_t count = 0;
      std::cin >> count;
      if (!st.may_add()) { std::printf("add refused closed\n"); continue; }
      if (count > lay.cap) { std::printf("add refused size\n"); continue; }
      bool switched = false;
      if (!lay.fits(count)) {
        if (!st.may_switch()) { std::printf("add refused room\n"); continue; }
        size_t first = 0, n = 0;
        lay.take(&first, &n);  // (context.hip copies what is pending before it leaves a slab)
        lay.rewind();
        switched = true;
      }
      const size_t at = lay.place(count);
      for (size_t k = 0; k < count; ++k) slab.data()[at + k] = stamp;  // (past the end: the sanitizer stops the program)
      stamp += 1.0;
      std::printf("add %s%zu %zu\n", switched ? "switch " : "", at, lay.head);
    } else if (cmd == "commit") {
      st.closed = true;
      size_t first = 0, count = 0;
      if (lay.take(&first, &count)) std::printf("commit %zu %zu\n", first, count);
      else std::printf("commit none\n");
    } else if (cmd == "drop") {
      lay.drop();
      std::printf("drop\n");
    } else if (cmd == "state") {
      std::printf("state %zu %zu %d\n", lay.head, lay.sent, lay.pending() ? 1 : 0);
    } else {
      std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
