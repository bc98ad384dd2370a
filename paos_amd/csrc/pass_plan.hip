// pass_plan.hip -- the host-only half of a pass program: lowering a pass for the frugal kernels (lower_frugal) and
// planning which lines, loads and stores of a whole program are dead (plan_pruning).  Launches nothing.
#include "host.h"

#include <cmath>
#include <cstring>

// Express pass p as   load | sign*scale*K phases | FFT | sign*scale*K phases | [FFT] | store.
bool lower_frugal(const paos_ctx* c, const paos_pass& p, const double* blocks /*host*/, LoweredPass& lp) {
  std::vector<FrugalItem>& items = lp.items;
  int &kpre = lp.kpre, &kmid = lp.kmid, &nfft = lp.nfft, &mask_block = lp.mask_block, &mask_slot = lp.mask_slot;
  std::vector<double>& mask_shared = lp.mask_shared;
  std::vector<int>& mask_rep = lp.mask_rep;
  if (p.axis != 0 && p.axis != 1) return false;
  if (p.fft1 < 0 || p.n_post != 0) return false;
  const paos_pw_op* lists[2] = {p.pre, p.mid};
  const int counts[2] = {p.n_pre, p.n_mid};
  int k[2] = {0, 0};
  mask_block = -1; mask_slot = -1;
  for (int l = 0; l < 2; ++l)
    for (int o = 0; o < counts[l]; ++o) {
      const int kind = lists[l][o].kind;
      if (kind == PAOS_PW_QPHASE_CENTRED || kind == PAOS_PW_QPHASE_NATURAL) {
        ++k[l];
        for (int it = 0; it < c->batch; ++it) {  // the kernels fold the sign into the coefficient: it must be +-1
          const double* q = blocks + ((size_t)lists[l][o].block * c->batch + it) * FP_STRIDE;
          if (q[FP_ENABLE] != 0.0 && std::fabs(q[FP_SGN]) != 1.0) return false;
        }
      }
      else if (kind == PAOS_PW_MASK) {
        if (mask_block >= 0) return false;  // one aperture per pass (one set of line records)
        mask_block = lists[l][o].block; mask_slot = l;
      } else if (kind != PAOS_PW_SIGN && kind != PAOS_PW_SCALE) return false;
    }
  if (k[0] > kFrugalMaxPre || k[1] > kFrugalMaxMid) return false;
  if (mask_block >= 0) {  // can this aperture be held as per-line records along the pass axis?
    for (int it = 0; it < c->batch; ++it) {
      const double* q = blocks + ((size_t)mask_block * c->batch + it) * FP_STRIDE;
      const double* q2 = blocks + ((size_t)(mask_block + 1) * c->batch + it) * FP_STRIDE;
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
  items.assign(c->batch, FrugalItem{});
  mask_shared.assign(c->batch, 0.0);
  mask_rep.assign(c->batch, -1);
  auto blk = [&](int b, int it) { return blocks + ((size_t)b * c->batch + it) * FP_STRIDE; };
  for (int it = 0; it < c->batch; ++it) {
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
      for (int o = 0; o < counts[l]; ++o) {
        const paos_pw_op& op = lists[l][o];
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
          mask_rep[it] = rep;  // the record set is chosen later (assign_mask_set): pointers are filled in there
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
    fi.line_lo = 0.0; fi.line_hi = (double)c->n; fi.line_fill = 0.0; fi.pos_lo = 0.0; fi.pos_hi = (double)c->n;
    fi.spos_lo = 0.0; fi.spos_hi = (double)c->n;
  }
  // The KPRE = 0 shapes take the slot in front of the first transform to be empty (frugal_slot: PLAIN).  The
  // rare pass that has a sign, a scale or an aperture there but no phase runs on the KPRE = 1 shape; its
  // phase record is all zeros: exp(i 0) = 1 exactly.
  if (kpre == 0)
    for (const FrugalItem& fi : items)
      if (fi.active != 0.0 && (fi.pre.sign_on != 0.0 || fi.pre.scale != 1.0 || fi.pre.mask_on != 0.0)) { kpre = 1; break; }
  return true;
}

// ---- pruning of dead lines (frugal_pass.h: FrugalItem::line_lo ...) ------------------------------
namespace {

// Lines (rows for a row pass, columns for a column pass) outside the returned range get weight
// exactly 0 from the aperture of this pass: photutils' bounding box, ixmin = floor(c - e + 0.5),
// ixmax = ceil(c + e + 0.5) (pointwise.h: make_box; theta = 0 here), widened by one pixel and then
// rounded outward to whole block rows so that a tile is either wholly dead or processed.
bool mask_live_range(const paos_ctx* c, const double* q, const double* q2, int axis, int* lo, int* hi) {
  if (q[0] == 0.0 || q2[0] != 0.0 || q2[1] != 0.0) return false;  // off, tilted, or an obscuration (outside weight 1)
  const double centre = axis == 0 ? q[2] : q[1];
  double ext = axis == 0 ? q[4] : q[3];
  if (q2[3] != PAOS_SHAPE_ELLIPSE) ext = ext / 2.0;
  if (!std::isfinite(centre) || !std::isfinite(ext) || !(ext > 0.0)) return false;
  const double a = std::floor(centre - ext + 0.5) - 1.0, b = std::ceil(centre + ext + 0.5) + 1.0;
  const int n = c->n;
  int l = a < 0.0 ? 0 : (a > n ? n : (int)a), h = b < 0.0 ? 0 : (b > n ? n : (int)b);
  const int br = c->br;
  l = (l / br) * br;
  h = ((h + br - 1) / br) * br;
  if (h > n) h = n;
  if (l >= h) { l = 0; h = br; }  // aperture off the grid along this axis: keep one block row live
  *lo = l; *hi = h;
  return true;
}

struct LineRange { int lo, hi; };

}  // namespace

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
void plan_pruning(const paos_ctx* c, const paos_pass* passes, int n_passes, const double* blocks,
                  std::vector<LoweredPass>& low, const double* entry_rows, bool entry_stale, const double* entry_cols) {
  const int n = c->n, br = c->br;
  // never empty, always inside `a`: an aperture off the live range keeps one block row of `a` (which it then zeroes)
  auto meet = [br](LineRange a, LineRange b) {
    LineRange r{a.lo > b.lo ? a.lo : b.lo, a.hi < b.hi ? a.hi : b.hi};
    if (r.lo >= r.hi) { r.lo = a.lo; r.hi = a.lo + br < a.hi ? a.lo + br : a.hi; }
    return r;
  };
  std::vector<int> act;
  std::vector<LineRange> lines, loads;
  for (int it = 0; it < c->batch; ++it) {
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
        const double* mq = blocks + ((size_t)low[q].mask_block * c->batch + it) * FP_STRIDE;
        const double* mq2 = blocks + ((size_t)(low[q].mask_block + 1) * c->batch + it) * FP_STRIDE;
        masked = mask_live_range(c, mq, mq2, ax, &ml.lo, &ml.hi) && mask_live_range(c, mq, mq2, 1 - ax, &mp.lo, &mp.hi);
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
