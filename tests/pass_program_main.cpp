// pass_program_main.cpp -- drives paos_amd/csrc/pass_program.h (on the records of pass_records.h) from stdin for
// tests/test_pass_program_host.py: the planning steps of a pass program in the order passes.hip runs them, with the record
// sets assigned the way a fresh context would (distinct apertures get distinct sets, in program order; eight sets, the
// least recently used one is overwritten).  Compiled with the address and undefined-behaviour sanitizers and without FMA
// contraction; no GPU, no library.  Doubles travel as the 16 hex digits of their bits.  Any number of programs, each:
//   program
//   dims N BATCH BR PRECISION CENTRAL_HALF
//   switches LINE_TABLES FUSE_PAIRS COMPACT_GRID ENV_PRUNE STAGE_PROGRAM BATCHED_RECORDS PSF_ZERO_REUSE CTX_PRUNE
//   final MODE                       0 the field, 1 the PSF instead, 2 the field and its power
//   psfmem AXIS [LO HI per item]     what the PSF buffer is known to hold (AXIS -1: nothing, no windows follow)
//   entry ROWS STALE COLS            flags; then [BATCH][2] row windows if ROWS, [BATCH][2] column windows if COLS
//   blocks NB                        then NB * BATCH * 5 doubles
//   passes NP                        then per pass: AXIS FFT1 FFT2 NPRE NMID NPOST and (KIND FLAGS BLOCK) per operator
// Output per program: "program", "phases RC" (non-zero: nothing else), "flags ...", "batched Q..", per pass "pass ..." and per
// item "item ...", per launch "launch ...", "psfmem ..." -- see the printf calls.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "../paos_amd/csrc/pass_program.h"
#include "../paos_amd/csrc/pass_records.h"

static double read_bits() {
  std::string tok;
  std::cin >> tok;
  const uint64_t u = std::stoull(tok, nullptr, 16);
  double d;
  std::memcpy(&d, &u, sizeof d);
  return d;
}

static void expect(const char* word) {
  std::string tok;
  std::cin >> tok;
  if (tok != word) {
    std::fprintf(stderr, "expected '%s', got '%s'\n", word, tok.c_str());
    std::exit(2);
  }
}

// the record sets of a fresh context (passes.hip: assign_mask_set, without the device buffers)
struct RecordSet {
  std::vector<double> key;
  unsigned long long used = 0;
  int line_lo = 0, line_hi = 0;
};
constexpr int kSets = 8;

static void assign_set(const PlanDims& d, RecordSet* sets, unsigned long long& clock, int axis, LoweredPass& lp, const double* blocks) {
  std::vector<double> key;
  key.push_back((double)axis);
  const double* ap = blocks + (size_t)lp.mask_block * d.batch * FP_STRIDE;
  key.insert(key.end(), ap, ap + (size_t)2 * d.batch * FP_STRIDE);
  key.insert(key.end(), lp.mask_shared.begin(), lp.mask_shared.end());
  int hit = -1, victim = 0;
  for (int k = 0; k < kSets; ++k) {
    if (!sets[k].key.empty() && sets[k].key.size() == key.size() && !std::memcmp(sets[k].key.data(), key.data(), key.size() * sizeof(double))) hit = k;
    if (sets[k].used < sets[victim].used) victim = k;
  }
  const int k = hit >= 0 ? hit : victim;
  sets[k].used = ++clock;
  if (hit < 0) sets[k].key = key;
  lp.mask_set = k;
  lp.mask_render = hit < 0;
}

int main() {
  std::string cmd;
  while (std::cin >> cmd) {
    if (cmd != "program") return 2;
    PlanDims d{};
    PlanSwitches sw;
    int mode = 0, known_axis = -1, has_rows = 0, stale = 0, has_cols = 0, n_blocks = 0, n_passes = 0;
    expect("dims");
    std::cin >> d.n >> d.batch >> d.br >> d.precision >> d.central_half;
    expect("switches");
    std::cin >> sw.line_tables >> sw.fuse_pairs >> sw.compact_grid >> sw.env_prune >> sw.stage_program >> sw.batched_records >>
        sw.psf_zero_reuse >> sw.ctx_prune;
    expect("final");
    std::cin >> mode;
    expect("psfmem");
    std::cin >> known_axis;
    std::vector<double> zero_lo, zero_hi;
    if (known_axis >= 0)
      for (int it = 0; it < d.batch; ++it) { zero_lo.push_back(read_bits()); zero_hi.push_back(read_bits()); }
    expect("entry");
    std::cin >> has_rows >> stale >> has_cols;
    std::vector<double> rows, cols;
    for (int k = 0; has_rows && k < 2 * d.batch; ++k) rows.push_back(read_bits());
    for (int k = 0; has_cols && k < 2 * d.batch; ++k) cols.push_back(read_bits());
    expect("blocks");
    std::cin >> n_blocks;
    std::vector<double> blocks((size_t)n_blocks * d.batch * FP_STRIDE);
    for (double& v : blocks) v = read_bits();
    expect("passes");
    std::cin >> n_passes;
    std::vector<paos_pass> passes(n_passes);
    for (paos_pass& p : passes) {
      p = paos_pass{};
      std::cin >> p.axis >> p.fft1 >> p.fft2 >> p.n_pre >> p.n_mid >> p.n_post;
      if (p.n_pre > PAOS_MAX_PW || p.n_mid > PAOS_MAX_PW || p.n_post > PAOS_MAX_PW) return 2;
      for (int l = 0; l < 3; ++l) {
        paos_pw_op* ops = l == 0 ? p.pre : (l == 1 ? p.mid : p.post);
        for (int o = 0; o < op_list(p, l).count; ++o) std::cin >> ops[o].kind >> ops[o].flags >> ops[o].block;
      }
    }
    if (!std::cin) return 2;
    const double* entry_rows = has_rows ? rows.data() : nullptr;
    const double* entry_cols = has_cols && stale ? cols.data() : nullptr;  // (paos_run_program: columns with stale rows only)

    std::printf("program\n");
    const int phases = check_phase_args(d, passes.data(), n_passes, blocks.data(), n_blocks);
    std::printf("phases %d\n", phases);
    if (phases) continue;
    // lower + assign sets
    RecordSet sets[kSets];
    unsigned long long clock = 0;
    std::vector<LoweredPass> low(n_passes);
    bool all_frugal = n_passes > 0;
    for (int q = 0; q < n_passes; ++q) {
      low[q].ok = lower_frugal(d, passes[q], blocks.data(), low[q]);
      if (low[q].ok && low[q].mask_block >= 0) assign_set(d, sets, clock, passes[q].axis, low[q], blocks.data());
      all_frugal = all_frugal && low[q].ok;
    }
    // plan
    const bool pruned = all_frugal && sw.env_prune && sw.ctx_prune;
    if (pruned) plan_pruning(d, passes.data(), n_passes, blocks.data(), low, entry_rows, stale != 0, entry_cols);
    for (LoweredPass& lp : low) {
      if (!lp.ok || lp.mask_block < 0) continue;
      record_window(d, lp);
      RecordSet& ms = sets[lp.mask_set];
      if (!lp.mask_render && !(ms.line_lo <= lp.mask_lo && ms.line_hi >= lp.mask_hi)) lp.mask_render = true;
      if (lp.mask_render) { ms.line_lo = lp.mask_lo; ms.line_hi = lp.mask_hi; }
    }
    const bool zero_first = stale && entry_rows && entry_zero_first(d, pruned, low, entry_rows, entry_cols);
    // what the plan's store mode needs
    const int store = last_pass_store(low, mode);
    if (store == 1) psf_zero_fill(d, sw, passes[n_passes - 1].axis, low[n_passes - 1].items, known_axis, zero_lo, zero_hi);
    const std::vector<int> batched = batched_renderings(sw, all_frugal, low);
    std::vector<char> rendered_first(n_passes, 0);
    for (int q : batched) { low[q].mask_render = false; rendered_first[q] = 1; }
    // the launches
    std::vector<int> launch_of;
    std::vector<Launch> launches = form_launches(d, sw, passes.data(), n_passes, low, all_frugal && pruned, launch_of);
    for (Launch& g : launches) {
      if (!g.lp[0]->ok) continue;
      decide_tables(d, sw, g);
      finish_launch(d, sw, g, g.q + g.count == n_passes ? store : 0);
    }
    std::printf("flags all_frugal %d pruned %d zero_first %d store %d staged_whole %d\n", all_frugal ? 1 : 0, pruned ? 1 : 0, zero_first ? 1 : 0, store,
                stage_whole_program(d, sw, all_frugal, n_passes) ? 1 : 0);
    std::printf("batched");
    for (int q : batched) std::printf(" %d", q);
    std::printf("\n");
    for (int q = 0; q < n_passes; ++q) {
      const LoweredPass& lp = low[q];
      std::printf("pass %d ok %d axis %d kpre %d kmid %d nfft %d mask_block %d mask_slot %d set %d render %d window %d %d\n", q, lp.ok ? 1 : 0, passes[q].axis,
                  lp.kpre, lp.kmid, lp.nfft, lp.mask_block, lp.mask_slot, lp.mask_set, lp.mask_render || rendered_first[q] ? 1 : 0, lp.mask_lo, lp.mask_hi);
      for (int it = 0; lp.ok && it < d.batch; ++it) {
        const FrugalItem& f = lp.items[it];
        std::printf("item %d %d active %d lines %d %d fill %d loads %d %d stores %d %d\n", q, it, f.active != 0.0 ? 1 : 0, (int)f.line_lo, (int)f.line_hi,
                    f.line_fill != 0.0 ? 1 : 0, (int)f.pos_lo, (int)f.pos_hi, (int)f.spos_lo, (int)f.spos_hi);
      }
    }
    for (size_t k = 0; k < launches.size(); ++k) {
      const Launch& g = launches[k];
      if (!g.lp[0]->ok) continue;
      int rec[kBuildFields];
      build_to_ints(g.build, rec);
      std::printf("launch %d pass %d count %d tables %d build", (int)k, g.q, g.count, g.tables ? 1 : 0);
      for (int v : rec) std::printf(" %d", v);
      std::printf(" grid %u %u tag %d bytes %.17g lines %.17g\n", g.live_lo, g.live_hi, g.tag, g.bytes, g.lines);
    }
    if (store == 1) {
      std::printf("psfmem");
      for (int it = 0; it < d.batch; ++it) std::printf(" %d %d", (int)zero_lo[it], (int)zero_hi[it]);
      std::printf("\n");
    }
  }
  return 0;
}
