// pass_program.h -- what a pass program launches, decided in plain C++: lowering a pass for the frugal kernels (lower_frugal),
// the pruning of dead lines across a program (plan_pruning), which passes share a launch (form_launches), whose slots read
// tables (decide_tables), the build a launch takes (pick_build), its grid window and what the launch timer is told
// (finish_launch), and the rules around them: the bound of the phase arguments, the record window of a pass, when the entry
// windows must be zeroed first, what the last pass may store, which zeros a PSF store still owes, when the record renderings
// may go in one batch.  Of a context it reads five ints (PlanDims) and the values of the environment switches
// (PlanSwitches): no HIP, nothing launched, so that a plain C++ program can test it (tests/pass_program_main.cpp).
// passes.hip includes it (compiled without FMA contraction: lower_frugal's bound must not be contracted), assigns the record
// sets -- they live in the context's store -- and does everything that touches the device.
#pragma once
#include "../../include/paos_hip.h"

#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "pass_records.h"

#pragma GCC visibility push(hidden)  // internal to the library, like everything host.h declares

using namespace paos;

struct PlanDims {
  int n, batch, br;  // grid size, items, block height of the layout
  int precision;     // PAOS_F64 / PAOS_F32
  int central_half;  // the context takes the central-half builds (PAOS_CENTRAL_HALF when it was created)
  int narrow_windows = 1;  // ... and their narrow-window variant (PAOS_NARROW_WINDOWS likewise)
};
// The environment switches the planning reads (true: the default path), and the context's own pruning switch.
struct PlanSwitches {
  bool line_tables = true;      // PAOS_LINE_TABLES=0: every slot evaluates
  bool fuse_pairs = true;       // PAOS_FUSE_PAIRS=0: one pass per launch
  bool compact_grid = true;     // PAOS_COMPACT_GRID=0 launches the full grid (dead workgroups exit in their prologue)
  bool env_prune = true;        // PAOS_NO_PRUNE=1 processes every tile (A/B tests of the dead-line pruning)
  bool stage_program = true;    // PAOS_STAGE_PROGRAM=0: each launch stages its own records and tables
  bool batched_records = true;  // PAOS_BATCHED_RECORDS=0: aperture records rendered in place, one launch per aperture
  bool psf_zero_reuse = true;   // PAOS_PSF_ZERO_REUSE=0: a PSF store writes the zeros of all its dead tiles
  bool ctx_prune = true;        // paos_ctx_set_pruning
};

// the three operator lists of a pass: 0 in front of the first transform, 1 between the two, 2 behind the second
struct OpList {
  const paos_pw_op* ops;
  int count;
};
inline OpList op_list(const paos_pass& p, int l) {
  return l == 0 ? OpList{p.pre, p.n_pre} : (l == 1 ? OpList{p.mid, p.n_mid} : OpList{p.post, p.n_post});
}
inline bool is_phase(const paos_pw_op& op) { return op.kind == PAOS_PW_QPHASE_CENTRED || op.kind == PAOS_PW_QPHASE_NATURAL; }

// The device sincos has no huge-argument path: bound every enabled phase operator of a program.
enum PhaseCheck { PHASES_OK = 0, PHASE_BLOCK_OUT_OF_RANGE, PHASE_TOO_LARGE };
inline PhaseCheck check_phase_args(const PlanDims& d, const paos_pass* passes, int n_passes, const double* blocks, int n_blocks) {
  for (int i = 0; i < n_passes; ++i)
    for (int l = 0; l < 3; ++l) {
      const OpList ol = op_list(passes[i], l);
      for (int o = 0; o < ol.count && o < PAOS_MAX_PW; ++o) {
        const paos_pw_op& op = ol.ops[o];
        if (!is_phase(op)) continue;
        if (op.block < 0 || op.block >= n_blocks) return PHASE_BLOCK_OUT_OF_RANGE;
        for (int it = 0; it < d.batch; ++it) {
          const double* p = blocks + ((size_t)op.block * d.batch + it) * FP_STRIDE;
          if (p[FP_ENABLE] == 0.0) continue;
          const double hx = 0.5 * d.n * p[FP_SX], hy = 0.5 * d.n * p[FP_SY];
          double arg = std::fabs(p[FP_COEF]) * (hx * hx + hy * hy);
          if (op.flags & PAOS_PWF_MUL2PI) arg *= 6.283185307179586;
          if (!(arg < kMaxPhaseArg)) return PHASE_TOO_LARGE;
        }
      }
    }
  return PHASES_OK;
}

// Express pass p as   load | sign*scale*K phases | FFT | sign*scale*K phases | [FFT] | store.
inline bool lower_frugal(const PlanDims& d, const paos_pass& p, const double* blocks /*host*/, LoweredPass& lp) {
  std::vector<FrugalItem>& items = lp.items;
  int &kpre = lp.kpre, &kmid = lp.kmid, &nfft = lp.nfft, &mask_block = lp.mask_block, &mask_slot = lp.mask_slot;
  std::vector<double>& mask_shared = lp.mask_shared;
  std::vector<int>& mask_rep = lp.mask_rep;
  if (p.axis != 0 && p.axis != 1) return false;
  if (p.fft1 < 0 || p.n_post != 0) return false;
  const OpList lists[2] = {op_list(p, 0), op_list(p, 1)};
  int k[2] = {0, 0};
  mask_block = -1; mask_slot = -1;
  for (int l = 0; l < 2; ++l)
    for (int o = 0; o < lists[l].count; ++o) {
      const int kind = lists[l].ops[o].kind;
      if (is_phase(lists[l].ops[o])) {
        ++k[l];
        for (int it = 0; it < d.batch; ++it) {  // the kernels fold the sign into the coefficient: it must be +-1
          const double* q = blocks + ((size_t)lists[l].ops[o].block * d.batch + it) * FP_STRIDE;
          if (q[FP_ENABLE] != 0.0 && std::fabs(q[FP_SGN]) != 1.0) return false;
        }
      }
      else if (kind == PAOS_PW_MASK) {
        if (mask_block >= 0) return false;  // one aperture per pass (one set of line records)
        mask_block = lists[l].ops[o].block; mask_slot = l;
      } else if (kind != PAOS_PW_SIGN && kind != PAOS_PW_SCALE) return false;
    }
  if (k[0] > kFrugalMaxPre || k[1] > kFrugalMaxMid) return false;
  if (mask_block >= 0) {  // can this aperture be held as per-line records along the pass axis?
    for (int it = 0; it < d.batch; ++it) {
      const double* q = blocks + ((size_t)mask_block * d.batch + it) * FP_STRIDE;
      const double* q2 = blocks + ((size_t)(mask_block + 1) * d.batch + it) * FP_STRIDE;
      if (q[0] == 0.0) continue;
      const double a = q[3], b = q[4], theta = q2[0], obsc = q2[1], subpix = q2[2], shape = q2[3];
      if (theta != 0.0 || !(a > 0.0) || !(b > 0.0)) return false;
      if (shape == PAOS_SHAPE_ELLIPSE) {
        // longest partial run near the tips of the ellipse: ~ 2 a sqrt(3 / b) along rows
        const double along = p.axis == 0 ? a : b, across = p.axis == 0 ? b : a;
        if (!(across >= 2.0) || 2.0 * along * std::sqrt(3.0 / across) + 8.0 > kMaskW) return false;
      } else {
        const int sp = (int)subpix;
        if (obsc != 0.0 || sp <= 0 || (sp & (sp - 1)) != 0) return false;
      }
    }
  }
  kpre = k[0]; kmid = k[1]; nfft = p.fft2 >= 0 ? 2 : 1;
  items.assign(d.batch, FrugalItem{});
  mask_shared.assign(d.batch, 0.0);
  mask_rep.assign(d.batch, -1);
  auto blk = [&](int b, int it) { return blocks + ((size_t)b * d.batch + it) * FP_STRIDE; };
  for (int it = 0; it < d.batch; ++it) {
    FrugalItem& fi = items[it];
    const double* c1 = blk(p.fft1, it);
    fi.fft1_on = c1[FC_ENABLE] != 0.0; fi.fft1_inv = c1[FC_INVERSE] != 0.0;
    if (p.fft2 >= 0) { const double* c2 = blk(p.fft2, it); fi.fft2_on = c2[FC_ENABLE] != 0.0; fi.fft2_inv = c2[FC_INVERSE] != 0.0; }
    bool active = fi.fft1_on != 0.0 || fi.fft2_on != 0.0;
    FrugalSlot* slots[2] = {&fi.pre, &fi.mid};
    FrugalPhase* phases[2] = {fi.pre_ph, fi.mid_ph};
    int sign_bits[2] = {0, 0};
    for (int l = 0; l < 2; ++l) {
      slots[l]->sign_on = 0.0; slots[l]->scale = 1.0;
      sign_bits[l] = 0;
      slots[l]->mask_on = 0.0; slots[l]->w_in = 1.0; slots[l]->w_out = 0.0;
      slots[l]->lines = nullptr; slots[l]->vals = nullptr;
      int j = 0;
      for (int o = 0; o < lists[l].count; ++o) {
        const paos_pw_op& op = lists[l].ops[o];
        const double* q = blk(op.block, it);
        const bool on = q[FP_ENABLE] != 0.0;
        active = active || on;
        if (op.kind == PAOS_PW_MASK) {
          const double* q2 = blk(op.block + 1, it);
          slots[l]->mask_on = on ? 1.0 : 0.0;
          const bool obsc = q2[1] != 0.0 && q2[3] == PAOS_SHAPE_ELLIPSE;
          slots[l]->w_in = obsc ? 0.0 : 1.0; slots[l]->w_out = obsc ? 1.0 : 0.0;
          // items with the same aperture on the same sampling (a Monte-Carlo batch: one wavelength, many
          // wavefront-error draws) share one set of line records: only the first of them is rendered
          int rep = it;
          for (int j = 0; j < it; ++j)
            if (!std::memcmp(blk(op.block, j), q, FP_STRIDE * sizeof(double)) &&
                !std::memcmp(blk(op.block + 1, j), q2, FP_STRIDE * sizeof(double))) { rep = j; break; }
          mask_shared[it] = rep != it ? 1.0 : 0.0;
          mask_rep[it] = rep;  // the record set is chosen later (passes.hip: assign_mask_set): pointers are filled in there
        } else if (op.kind == PAOS_PW_SIGN) {
          // bit 0: (-1)^position along the line, bit 1: (-1)^line; the checkerboard flips both
          if (on) {
            const bool x_only = op.flags & PAOS_PWF_X_ONLY, y_only = op.flags & PAOS_PWF_Y_ONLY;
            const int along = p.axis == 0 ? (y_only ? 0 : 1) : (x_only ? 0 : 1);
            const int across = p.axis == 0 ? (x_only ? 0 : 1) : (y_only ? 0 : 1);
            sign_bits[l] ^= along | (across << 1);
          }
        }
        else if (op.kind == PAOS_PW_SCALE) { if (on) slots[l]->scale *= q[FP_COEF]; }
        else {
          FrugalPhase& ph = phases[l][j++];
          ph.natural = op.kind == PAOS_PW_QPHASE_NATURAL ? 1.0 : 0.0;
          // the sign rides on the coefficient: exp(i sgn m2 fl(coef s)) = exp(i m2 fl((sgn coef) s)), sgn = +-1
          if (on) { ph.sx = q[FP_SX]; ph.sy = q[FP_SY]; ph.coef = q[FP_COEF] * q[FP_SGN]; ph.sgn = 1.0; ph.m2 = (op.flags & PAOS_PWF_MUL2PI) ? 6.283185307179586 : 1.0; }
          else { ph.sx = ph.sy = 0.0; ph.coef = 0.0; ph.sgn = 1.0; ph.m2 = 1.0; }  // exp(i 0) = 1 exactly
        }
      }
      // frugal_slot: 1 = (-1)^(line + position), 2 = (-1)^position, 3 = (-1)^line
      slots[l]->sign_on = sign_bits[l] == 3 ? 1.0 : (sign_bits[l] == 1 ? 2.0 : (sign_bits[l] == 2 ? 3.0 : 0.0));
    }
    fi.active = active ? 1.0 : 0.0;
    fi.line_lo = 0.0; fi.line_hi = (double)d.n; fi.line_fill = 0.0; fi.pos_lo = 0.0; fi.pos_hi = (double)d.n;
    fi.spos_lo = 0.0; fi.spos_hi = (double)d.n;
  }
  // The KPRE = 0 shapes take the slot in front of the first transform to be empty (frugal_slot: PLAIN).  The
  // rare pass that has a sign, a scale or an aperture there but no phase runs on the KPRE = 1 shape; its
  // phase record is all zeros: exp(i 0) = 1 exactly.
  if (kpre == 0)
    for (const FrugalItem& fi : items)
      if (fi.active != 0.0 && (fi.pre.sign_on != 0.0 || fi.pre.scale != 1.0 || fi.pre.mask_on != 0.0)) { kpre = 1; break; }
  return true;
}

// ---- pruning of dead lines (pass_records.h: FrugalItem::line_lo ...) ------------------------------

// Lines (rows for a row pass, columns for a column pass) outside the returned range get weight
// exactly 0 from the aperture of this pass: photutils' bounding box, ixmin = floor(c - e + 0.5),
// ixmax = ceil(c + e + 0.5) (pointwise.h: make_box; theta = 0 here), widened by one pixel and then
// rounded outward to whole block rows so that a tile is either wholly dead or processed.
inline bool mask_live_range(const PlanDims& d, const double* q, const double* q2, int axis, int* lo, int* hi) {
  if (q[0] == 0.0 || q2[0] != 0.0 || q2[1] != 0.0) return false;  // off, tilted, or an obscuration (outside weight 1)
  const double centre = axis == 0 ? q[2] : q[1];
  double ext = axis == 0 ? q[4] : q[3];
  if (q2[3] != PAOS_SHAPE_ELLIPSE) ext = ext / 2.0;
  if (!std::isfinite(centre) || !std::isfinite(ext) || !(ext > 0.0)) return false;
  const double a = std::floor(centre - ext + 0.5) - 1.0, b = std::ceil(centre + ext + 0.5) + 1.0;
  const int n = d.n;
  int l = a < 0.0 ? 0 : (a > n ? n : (int)a), h = b < 0.0 ? 0 : (b > n ? n : (int)b);
  const int br = d.br;
  l = (l / br) * br;
  h = ((h + br - 1) / br) * br;
  if (h > n) h = n;
  if (l >= h) { l = 0; h = br; }  // aperture off the grid along this axis: keep one block row live
  *lo = l; *hi = h;
  return true;
}

struct LineRange { int lo, hi; };

// Fill in the pruning fields of a whole program.  Per item the planner carries, forwards, the BOX outside which the
// field is known to be zero -- rows [r.lo, r.hi) x columns [c.lo, c.hi); physically (zeros in memory: what a stand-alone
// aperture leaves, passed in through entry_rows) or virtually (tiles that were skipped hold stale data that STANDS for
// zeros) -- and, backwards, the box of each pass's output that the next pass reads at all:
//   forwards   a pass keeps dead lines dead; its transforms spread the live positions over the whole line; an aperture
//              riding on it clips both ranges to its bounding box (positions: unless a transform follows it);
//   backwards  a pass processes the lines that are alive AND wanted, loads the live positions of those lines and stores
//              the positions the next pass reads; what it reads is what the pass in front of it has to deliver.
// Every load therefore falls inside what the previous pass stored (or is known to be zero and not loaded), and nothing
// else is ever looked at: tiles nobody processes keep whatever they held.  The last pass an item takes part in delivers
// the whole grid: it stores every position of its lines and writes zeros to the dead ones (line_fill).
// Round 4: the box (both axes at once, and the backward half) is what lets the separable pass programs (passes.py:
// SeparableCompiler) run an aperture-to-aperture stretch on the live rows and the wanted columns only; for the
// operator-by-operator programs it yields the ranges of round 2's one-axis planner and round 3's "stores nobody reads".
inline void plan_pruning(const PlanDims& d, const paos_pass* passes, int n_passes, const double* blocks,
                         std::vector<LoweredPass>& low, const double* entry_rows, bool entry_stale, const double* entry_cols) {
  const int n = d.n, br = d.br;
  // never empty, always inside `a`: an aperture off the live range keeps one block row of `a` (which it then zeroes)
  auto meet = [br](LineRange a, LineRange b) {
    LineRange r{a.lo > b.lo ? a.lo : b.lo, a.hi < b.hi ? a.hi : b.hi};
    if (r.lo >= r.hi) { r.lo = a.lo; r.hi = a.lo + br < a.hi ? a.lo + br : a.hi; }
    return r;
  };
  std::vector<int> act;
  std::vector<LineRange> lines, loads;
  for (int it = 0; it < d.batch; ++it) {
    act.clear();
    for (int q = 0; q < n_passes; ++q)
      if (low[q].items[it].active != 0.0) act.push_back(q);
    if (act.empty()) continue;
    LineRange box[2] = {{0, n}, {0, n}};  // [0]: rows, [1]: columns
    bool clean = false;                   // rows outside box[0] are zeros in memory and nothing has touched them
    LineRange rows0{0, n};
    if (entry_rows) {
      int l = (int)entry_rows[2 * it], h = (int)entry_rows[2 * it + 1];
      l = l < 0 ? 0 : (l / br) * br;
      h = h > n ? n : ((h + br - 1) / br) * br;
      if (h > n) h = n;
      if (l < h && (l > 0 || h < n)) { box[0] = {l, h}; clean = !entry_stale; }
      rows0 = box[0];
    }
    if (entry_cols && entry_stale) {
      // (round 5: paos_start_box) the columns outside stand for zeros too, inside the live rows: the first pass loads the box
      // only, and every later pass reads what its predecessor stored -- nobody ever looks at them
      int l = (int)entry_cols[2 * it], h = (int)entry_cols[2 * it + 1];
      l = l < 0 ? 0 : (l / br) * br;
      h = h > n ? n : ((h + br - 1) / br) * br;
      if (h > n) h = n;
      if (l < h && (l > 0 || h < n)) box[1] = {l, h};
    }
    // forwards
    lines.assign(act.size(), LineRange{0, n});
    loads.assign(act.size(), LineRange{0, n});
    for (size_t k = 0; k < act.size(); ++k) {
      const int q = act[k], ax = passes[q].axis;
      const FrugalItem& fi = low[q].items[it];
      LineRange& L = box[ax];      // along the lines of this pass (rows for a row pass)
      LineRange& P = box[1 - ax];  // along the positions of a line
      LineRange ml{0, n}, mp{0, n};
      bool masked = false;
      if (low[q].mask_block >= 0) {
        const double* mq = blocks + ((size_t)low[q].mask_block * d.batch + it) * FP_STRIDE;
        const double* mq2 = blocks + ((size_t)(low[q].mask_block + 1) * d.batch + it) * FP_STRIDE;
        masked = mask_live_range(d, mq, mq2, ax, &ml.lo, &ml.hi) && mask_live_range(d, mq, mq2, 1 - ax, &mp.lo, &mp.hi);
      }
      if (masked) L = meet(L, ml);
      lines[k] = L;
      LineRange pos = P;
      if (masked && low[q].mask_slot == 0) pos = meet(pos, mp);  // in front of the first transform: no need to load what it zeroes
      loads[k] = pos;
      if (fi.fft1_on != 0.0) pos = {0, n};
      if (masked && low[q].mask_slot == 1) pos = meet(pos, mp);
      if (low[q].nfft >= 2 && fi.fft2_on != 0.0) pos = {0, n};
      P = pos;
    }
    // backwards
    LineRange want[2] = {{0, n}, {0, n}};
    for (size_t k = act.size(); k-- > 0;) {
      const int q = act[k], ax = passes[q].axis;
      FrugalItem& fi = low[q].items[it];
      const LineRange proc = meet(lines[k], want[ax]);
      fi.line_lo = proc.lo; fi.line_hi = proc.hi;
      fi.pos_lo = loads[k].lo; fi.pos_hi = loads[k].hi;
      fi.spos_lo = want[1 - ax].lo; fi.spos_hi = want[1 - ax].hi;
      want[ax] = proc;
      want[1 - ax] = loads[k];
    }
    // zeros nobody has written: the last pass writes them
    for (size_t k = 0; k < act.size(); ++k) {
      const FrugalItem& fi = low[act[k]].items[it];
      if (passes[act[k]].axis != 0 || (int)fi.line_lo != rows0.lo || (int)fi.line_hi != rows0.hi || fi.spos_lo > 0.0 ||
          fi.spos_hi < (double)n)
        clean = false;
    }
    FrugalItem& last = low[act.back()].items[it];
    if ((last.line_lo > 0.0 || last.line_hi < (double)n) && !clean) last.line_fill = 1.0;
  }
}

// Which lines' aperture records does a pass read?  Those of its live tiles only: a workgroup whose lines are dead
// for its item (frugal_pass_kernel: outside [line_lo, line_hi), bounds that are multiples of the tile height)
// leaves before it looks at a record.  Only these lines are rendered (a quarter of them behind a clear aperture at
// zoom 4), and a set found in the context's store is good only if it was rendered that far.
inline void record_window(const PlanDims& d, LoweredPass& lp) {
  double lo = (double)d.n, hi = 0.0;
  for (const FrugalItem& fi : lp.items) {
    if (fi.active == 0.0) continue;
    lo = fi.line_lo < lo ? fi.line_lo : lo;
    hi = fi.line_hi > hi ? fi.line_hi : hi;
  }
  const bool window = hi > lo;
  lp.mask_lo = window ? (int)lo : 0;
  lp.mask_hi = window ? (int)hi : d.n;
}

// Entry rows that merely stand for zeros must become zeros wherever the program will not consume them: everywhere when
// the planner is off, and for an item no pass of the program touches ...
inline bool entry_zero_first(const PlanDims& d, bool pruned, const std::vector<LoweredPass>& low, const double* entry_rows,
                             const double* entry_cols) {
  bool need = !pruned;
  for (int it = 0; it < d.batch && !need; ++it) {
    bool active = false;
    for (const LoweredPass& lp : low) active = active || lp.items[it].active != 0.0;
    need = !active;
  }
  // ... and for an item whose window is empty: the planner takes an empty window for no window at all (plan_pruning),
  // so its first pass would load every line of stale data
  const double* windows[2] = {entry_rows, entry_cols};
  for (int w = 0; w < 2 && !need; ++w)
    for (int it = 0; windows[w] && it < d.batch && !need; ++it) {
      const int br = d.br, l = ((int)windows[w][2 * it] / br) * br;
      int h = (((int)windows[w][2 * it + 1] + br - 1) / br) * br;
      if (h > d.n) h = d.n;
      need = l >= h;
    }
  return need;
}

// What the last pass of a program stores besides or instead of the field (FrugalBuild::store) when the caller wants
// `final_mode`: 1, the PSF instead of the field -- |u|^2 and its per-workgroup sums (frugal_pass.h: STORE) -- when the pass runs
// on the frugal kernels in a shape built for it and every item takes part; 2, the field AND the sums of |u|^2 of its tiles
// (FrugalArgs::pow_partial), likewise (the shapes built with STORE = 2).  0: the program runs as usual and the caller's
// sweep or reduction follows it.
inline int last_pass_store(const std::vector<LoweredPass>& low, int final_mode) {
  if (final_mode == 0 || low.empty()) return 0;
  const LoweredPass& last = low.back();
  bool ok = last.ok && last.kpre <= 1 && (final_mode == 2 || last.kmid <= 1);
  if (ok)
    for (const FrugalItem& fi : last.items) ok = ok && fi.active != 0.0;
  return ok ? final_mode : 0;
}

// Dead tiles of a PSF-storing pass write PSF zeros (line_fill) -- unless the buffer already holds zeros there: the previous
// storing pass had the same live lines (the next batch of a sweep, the next Monte-Carlo batch).
// Round 4: per item.  What the buffer may still hold of the previous storing pass lies inside that pass's live
// lines [zero_lo, zero_hi); only dead tiles of THIS pass that meet them write zeros (the range travels in
// the item's -- here otherwise unused -- store-position fields).  A walked sweep changes the sampling at the
// image plane from batch to batch, so the live lines are never the same twice, but they move by a few lines.
// known_axis: the axis of the previous storing pass (-1: nothing known); zero_lo / zero_hi: its live lines in, this
// pass's out.
inline void psf_zero_fill(const PlanDims& d, const PlanSwitches& sw, int axis, std::vector<FrugalItem>& last, int known_axis,
                          std::vector<double>& zero_lo, std::vector<double>& zero_hi) {
  const bool known = sw.psf_zero_reuse && known_axis == axis && (int)zero_lo.size() == d.batch;
  zero_lo.resize(d.batch); zero_hi.resize(d.batch);
  for (int it = 0; it < d.batch; ++it) {
    const double old_lo = known ? zero_lo[it] : 0.0, old_hi = known ? zero_hi[it] : (double)d.n;
    const bool covered = old_lo >= last[it].line_lo && old_hi <= last[it].line_hi;  // every old line is rewritten
    last[it].line_fill = covered ? 0.0 : 1.0;
    last[it].spos_lo = covered ? 0.0 : old_lo;
    last[it].spos_hi = covered ? (double)d.n : old_hi;
    zero_lo[it] = last[it].line_lo; zero_hi[it] = last[it].line_hi;
  }
}

// The aperture line records a program has to render (not found in the context's kept sets) go in ONE launch per shape, in
// front of the first pass -- when every rendering goes to a set no EARLIER pass of this program reads (always, unless a
// program carries more distinct apertures than there are sets; then each is rendered in place, right before its pass).
// Returns the passes whose records are rendered in the batch; empty: each in place.
inline std::vector<int> batched_renderings(const PlanSwitches& sw, bool all_frugal, const std::vector<LoweredPass>& low) {
  std::vector<int> todo;
  bool safe = sw.batched_records && all_frugal;
  for (int q = 0; q < (int)low.size() && safe; ++q) {
    if (low[q].mask_block < 0) continue;
    if (low[q].mask_render) {
      for (int r = 0; r < q; ++r) safe = safe && !(low[r].mask_block >= 0 && low[r].mask_set == low[q].mask_set);
      todo.push_back(q);
    }
  }
  if (!safe || todo.size() <= 1) todo.clear();
  return todo;
}

// Do all phases of the pass vary along its lines only (the row / column factors of the separable programs)?  Then their
// factors come from tables by position (pass_records.h: FrugalSlot::table).  complex128 only (the complex64 slots use the
// hardware sin / cos).
inline bool phases_along_lines(const PlanSwitches& sw, int axis, const LoweredPass& lp, bool or_none = false) {
  if (!sw.line_tables || (lp.kpre + lp.kmid == 0 && !or_none)) return false;
  const int counts[2] = {lp.kpre, lp.kmid};
  for (int l = 0; l < 2; ++l)
    for (const FrugalItem& fi : lp.items) {
      if (fi.active == 0.0) continue;
      const FrugalPhase* ph = l == 0 ? fi.pre_ph : fi.mid_ph;
      for (int j = 0; j < counts[l]; ++j)
        if ((axis == 0 ? ph[j].sy : ph[j].sx) != 0.0) return false;
    }
  return true;
}

// Can the launch of a pass along `axis` go on with the next pass of the program (frugal_pass.h: LONG builds)?  Same axis, both on
// table slots with phases in every slot, a two-transform pass in front, and every item takes both or neither, on the same lines.
inline bool can_fuse_pair(const PlanDims& d, const PlanSwitches& sw, int axis, const LoweredPass& lp, int axis2, const LoweredPass& lp2) {
  if (!sw.fuse_pairs) return false;
  if (!lp.ok || !lp2.ok || axis != axis2 || lp.nfft != 2) return false;
  // (an aperture may ride on either pass -- the second one's slots read their line records themselves -- but the two must not
  // share a record set that the second would have to re-render between them: sets are assigned per pass, in program order)
  if (lp.mask_block >= 0 && lp2.mask_block >= 0 && lp.mask_set == lp2.mask_set) return false;
  // (a slot without phases takes part with a table of ones: (v 1) f is v f bit for bit)
  if (!phases_along_lines(sw, axis, lp, true) || !phases_along_lines(sw, axis2, lp2, true)) return false;
  for (int it = 0; it < d.batch; ++it) {
    const FrugalItem &f1 = lp.items[it], &f2 = lp2.items[it];
    if ((f1.active != 0.0) != (f2.active != 0.0)) return false;
    if (f1.active != 0.0 && (f1.line_lo != f2.line_lo || f1.line_hi != f2.line_hi || f1.line_fill != 0.0)) return false;
  }
  return true;
}

// One launch of a pass program: a pass and the one or two behind it that ride along (can_fuse_pair), and everything that is
// decided about it before it runs.
struct Launch {
  LoweredPass* lp[3] = {nullptr, nullptr, nullptr};
  int q = 0, count = 1, axis = 0;
  bool tables = false;   // its slots read their phase factors from tables (decide_tables)
  size_t item_base = 0;  // index of its first item record in the staged array (passes.hip: stage_groups)
  // finish_launch:
  int store = 0;                       // FrugalBuild::store
  FrugalBuild build{};                 // the build it takes
  int narrow = 0;                      // ... and whether it launches the narrow-window variant of that build (pick_narrow)
  unsigned live_lo = 0, live_hi = 0;   // the grid covers the workgroups of these lines only (0, 0: all lines)
  int tag = 0;                         // for the launch timer: what the launch skips
  double bytes = 0.0, lines = 0.0;     // ... the bytes the plan has it move, the line transforms it runs
  const LoweredPass& last() const { return *lp[count - 1]; }  // the pass whose stores leave the launch
};

// The launches of the program: a pass, or two / three consecutive passes of one row / column chain (can_fuse_pair) -- where
// every pass runs on the frugal kernels under the pruning plan.  launch_of[q]: the launch that starts at pass q (-1: q rides).
inline std::vector<Launch> form_launches(const PlanDims& d, const PlanSwitches& sw, const paos_pass* passes, int n_passes,
                                         std::vector<LoweredPass>& low, bool fusable, std::vector<int>& launch_of) {
  std::vector<Launch> launches;
  launch_of.assign(n_passes, -1);
  for (int q = 0; q < n_passes;) {
    Launch g;
    g.q = q; g.axis = passes[q].axis; g.lp[0] = &low[q];
    if (low[q].ok && fusable) {
      const bool pair = q + 1 < n_passes && can_fuse_pair(d, sw, passes[q].axis, low[q], passes[q + 1].axis, low[q + 1]);
      // (and a third: the five-transform chains -- ptp, stw, ptp -- that end a SYN20-like prescription)
      const bool triple = pair && q + 2 < n_passes && can_fuse_pair(d, sw, passes[q + 1].axis, low[q + 1], passes[q + 2].axis, low[q + 2]) &&
                          !(low[q].mask_block >= 0 && low[q + 2].mask_block >= 0 && low[q].mask_set == low[q + 2].mask_set);
      g.count = triple ? 3 : (pair ? 2 : 1);
      for (int k = 1; k < g.count; ++k) g.lp[k] = &low[q + k];
    }
    launch_of[q] = (int)launches.size();
    launches.push_back(g);
    q += g.count;
  }
  return launches;
}

// Item records and phase tables of a whole program are staged once, in front of its first launch, when every pass runs on
// the frugal kernels (a table per operator slot of every pass: 2 MiB each at 4096^2 x 32; a program that would need more
// than 1 GiB of them -- hundreds of passes -- stages launch by launch, on six tables).
inline bool stage_whole_program(const PlanDims& d, const PlanSwitches& sw, bool all_frugal, int n_passes) {
  const size_t table_bytes = (size_t)2 * n_passes * d.batch * d.n * 2 * sizeof(double);  // (entries of cx<double>)
  return all_frugal && sw.stage_program && table_bytes <= (size_t(1) << 30);
}

// Does the launch run on table slots?  All phases of all its passes along the lines; a fused launch always does.
inline void decide_tables(const PlanDims& d, const PlanSwitches& sw, Launch& g) {
  // (complex64: a slot evaluates its factors with the hardware sin / cos for less than the table's loads cost -- measured: dense
  // launches 2.03 -> 2.41 ms with tables -- so only the fused groups, whose one build reads tables, use them)
  g.tables = g.count > 1 || (d.precision == PAOS_F64 && phases_along_lines(sw, g.axis, *g.lp[0]));
  if (g.tables && g.count == 1) {
    // (a single pass over most of the grid is bound by HBM, and the table's reads are traffic too: dense launches
    // 3.75 ms evaluated, 3.85-4.0 with tables -- tables where the pass works on at most half of the lines)
    double lines = 0.0, active = 0.0;
    for (const FrugalItem& fi : g.lp[0]->items)
      if (fi.active != 0.0) { lines += fi.line_hi - fi.line_lo; active += 1.0; }
    if (active > 0.0 && lines > 0.5 * active * d.n) g.tables = false;
  }
}

// Is there a build of this name in the family of the dims?
inline bool build_exists(const PlanDims& d, const FrugalBuild& b) {
  return dispatch_family(d.precision, d.n, false, [&](auto t, auto n) { return frugal_built<decltype(t), decltype(n)::value>(b); });
}

// THE place that says which build a launch takes: from the passes it runs, whether their slots read tables (decide_tables)
// and what it stores (FrugalBuild::store) to the name of the build.
inline FrugalBuild pick_build(const PlanDims& d, const Launch& g) {
  const LoweredPass& lp = *g.lp[0];
  const LoweredPass *next = g.lp[1], *next2 = g.lp[2];
  FrugalBuild b{};
  b.axis = g.axis;
  // The table builds take "has phases" for the number of phases -- their slots read one factor --, and a fused launch runs on
  // the one build whose slots all read tables (a slot without phases: a table of ones).
  b.kpre = next ? 1 : (g.tables && lp.kpre > 1 ? 1 : lp.kpre);
  b.kmid = next ? 1 : (g.tables && lp.kmid > 1 ? 1 : lp.kmid);
  b.nfft = lp.nfft >= 2 ? 2 : 1;
  b.store = g.store;
  b.tab = g.tables ? 1 : 0;
  b.fuse = next2 ? 2 + next2->nfft : (next ? next->nfft : 0);
  // The PSF- and power-storing launches take neither of the builds below: their sums are laid out per two-line tile.
  if (!g.tables || g.store != 0) return b;
  // light: a single table pass whose every item loads and stores at most half of its positions -- one-line workgroups.
  // central: every active item of the FIRST pass loads positions of the central half only -- the central-half build of the
  // shape.  Per launch, not per item: one item outside sends the whole launch to the ordinary build.  (There is no device-side
  // guard: frugal_pass.h, CH.)
  bool light = !next, central = d.central_half, any = false;
  for (const FrugalItem& fi : lp.items) {
    if (fi.active == 0.0) continue;
    any = true;
    light = light && 2.0 * (fi.pos_hi - fi.pos_lo) <= (double)d.n && 2.0 * (fi.spos_hi - fi.spos_lo) <= (double)d.n;
    central = central && 4.0 * fi.pos_lo >= (double)d.n && 4.0 * fi.pos_hi <= 3.0 * (double)d.n;
  }
  // ... where there is one (the central-half builds run on one-line workgroups: a fused launch, or a light pass)
  b.one_line = light ? 1 : 0;
  if (!build_exists(d, b)) b.one_line = 0;
  b.central = central && any ? 1 : 0;
  if (!build_exists(d, b)) b.central = 0;
  return b;
}

// Does the launch take the narrow-window variant of its central-half build (frugal_pass.h: CH = 2)?  A property of the launch,
// not of the build's name: the build is a central-half one, the context's switch is on, every active item of the FIRST pass
// loads positions of [5 n / 16, 11 n / 16) only, and every active item of the pass whose stores leave the launch stores
// positions of that window only.  Per launch, like `central`: one item outside either window keeps the whole launch on the
// central-half kernel.  (There is no device-side guard on either side: frugal_pass.h, CH.)
inline int pick_narrow(const PlanDims& d, const Launch& g, const FrugalBuild& b) {
  if (b.central != 1 || !d.narrow_windows) return 0;
  const double lo = 5.0 * (double)d.n, hi = 11.0 * (double)d.n;
  bool any = false;
  for (const FrugalItem& fi : g.lp[0]->items) {
    if (fi.active == 0.0) continue;
    any = true;
    if (!(16.0 * fi.pos_lo >= lo && 16.0 * fi.pos_hi <= hi)) return 0;
  }
  for (const FrugalItem& fo : g.last().items) {
    if (fo.active == 0.0) continue;
    if (!(16.0 * fo.spos_lo >= lo && 16.0 * fo.spos_hi <= hi)) return 0;
  }
  return any ? 1 : 0;
}

// Everything else that is decided about a launch once its tables flag and what it stores are known: its build, the lines
// its grid has to cover, and the launch timer's figures.
inline void finish_launch(const PlanDims& d, const PlanSwitches& sw, Launch& g, int store) {
  g.store = store;
  g.build = pick_build(d, g);
  g.narrow = pick_narrow(d, g, g.build);
  const bool store_psf = store == 1;
  const LoweredPass& lp = *g.lp[0];
  {  // the lines some item still works on: the grid need not cover the others when their tiles have nothing to write
    double lo = (double)d.n, hi = 0.0;
    bool fill = false;
    // (a fused pair: the lines are the same for both passes, what is stored and filled is the second pass's business)
    for (const FrugalItem& fi : g.last().items) {
      if (fi.active == 0.0) continue;
      lo = fi.line_lo < lo ? fi.line_lo : lo;
      hi = fi.line_hi > hi ? fi.line_hi : hi;
      if (fi.line_fill != 0.0 && store_psf) {  // dead tiles write PSF zeros inside [spos_lo, spos_hi) only (psf_zero_fill)
        lo = fi.spos_lo < lo ? fi.spos_lo : lo;
        hi = fi.spos_hi > hi ? fi.spos_hi : hi;
      } else {
        fill = fill || fi.line_fill != 0.0;
      }
    }
    g.live_lo = g.live_hi = 0;
    if (sw.compact_grid && !fill && hi > lo && (lo > 0.0 || hi < (double)d.n)) {
      g.live_lo = (unsigned)lo;
      g.live_hi = (unsigned)hi;
    }
  }
  // for the launch timer: what does this launch skip?  bit 0: whole tiles of dead lines, bit 1: loads of dead
  // positions, bit 2: stores nobody reads, bit 3: it stores the PSF instead of the field
  const double elem = d.precision == PAOS_F64 ? 16.0 : 8.0;
  g.tag = store_psf ? 8 : 0;
  g.bytes = 0.0;
  g.lines = 0.0;
  if (g.count > 1) g.tag |= g.count > 2 ? 32 : 16;  // bit 4: the launch ran two passes of the program, bit 5: three
  for (int it = 0; it < d.batch; ++it) {
    const FrugalItem& fi = lp.items[it];
    const FrugalItem& fo = g.last().items[it];  // the pass whose stores leave the launch
    if (fi.active == 0.0) continue;
    if (fi.line_lo > 0.0 || fi.line_hi < (double)d.n) g.tag |= 1;
    if (fi.pos_lo > 0.0 || fi.pos_hi < (double)d.n) g.tag |= 2;
    if (!store_psf && (fo.spos_lo > 0.0 || fo.spos_hi < (double)d.n)) g.tag |= 4;
    // what the plan has this launch move: its live lines' loaded and stored positions (the PSF store: doubles, every position)
    g.bytes += (fi.line_hi - fi.line_lo) * ((fi.pos_hi - fi.pos_lo) * elem + (store_psf ? (double)d.n * 8.0 : (fo.spos_hi - fo.spos_lo) * elem));
    // ... and compute: every live line goes through the transforms that are switched on for this item, in every pass of the launch
    for (int k = 0; k < g.count; ++k) {
      const FrugalItem& fk = g.lp[k]->items[it];
      g.lines += (fi.line_hi - fi.line_lo) * ((fk.fft1_on != 0.0 ? 1.0 : 0.0) + (g.lp[k]->nfft >= 2 && fk.fft2_on != 0.0 ? 1.0 : 0.0));
    }
  }
}

#pragma GCC visibility pop
