// passes.hip -- pass programs: which kernel runs each pass, the aperture line records that ride on the frugal passes, the
// staging of item records and phase tables, the launches, and the reference's primitives as programs (paos_ptp / stw / wts).
#include "frugal_launch.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "phase_tables.h"

namespace {

int check_ops(paos_ctx* c, const paos_pw_op* ops, int count, int n_blocks) {
  if (count < 0 || count > PAOS_MAX_PW) return fail(c, PAOS_EINVAL, "too many pointwise operators in a pass");
  for (int o = 0; o < count; ++o) {
    if (ops[o].kind < PAOS_PW_SIGN || ops[o].kind > PAOS_PW_MASK) return fail(c, PAOS_EINVAL, "unknown pointwise operator");
    if (ops[o].block < 0 || ops[o].block >= n_blocks) return fail(c, PAOS_EINVAL, "operator block index out of range");
    if (ops[o].kind == PAOS_PW_MASK && ops[o].block + 1 >= n_blocks) return fail(c, PAOS_EINVAL, "an aperture operator needs two parameter blocks");
  }
  return PAOS_OK;
}

// Separable phase tables with an exact rounding correction (fft_kernels.h: table_phase) replace
// the per-pixel sincos by ~25 fp64 instructions + one L2-resident 16-byte load.  Measured on
// MI355X (round 1) the extra loads cost more than the arithmetic they save at 2 waves/SIMD
// (90 vs 97 wavefronts/s), so the path is opt-in: PAOS_PHASE_TABLES=1.
bool use_tables() {
  static const bool on = env_is("PAOS_PHASE_TABLES", '1');
  return on;
}

// ---- frugal path (N >= 1024, complex128): compile-time pass shapes, <= 128 VGPRs ---------------
// PAOS_NO_FRUGAL=1 keeps every pass on the generic kernel (A/B tests).
bool use_frugal() {
  static const bool on = !env_is("PAOS_NO_FRUGAL", '1');
  return on;
}

bool frugal_sizes(const paos_ctx* c) {
  // instantiated for complex128 at N >= 1024 and complex64 at N >= 2048
  return use_frugal() && c->n >= (c->precision == PAOS_F64 ? 1024 : 2048);
}

int ensure_mask_store(paos_ctx* c) {
  if (!c->mask_overflow) {
    HIPCHK(c, hipMalloc(&c->mask_overflow, sizeof(int)));
    HIPCHK(c, hipMemsetAsync(c->mask_overflow, 0, sizeof(int), c->stream));
  }
  return PAOS_OK;
}

// Pick the record set pass `lp` reads -- one that already holds its aperture, or the least recently used one, to
// be rendered -- and point the items' slots at it.  Called for the passes of a program in order, before anything is
// launched: launches follow in the same order on one stream, so a set re-used further down the program is
// overwritten only after the pass that read it.
int assign_mask_set(paos_ctx* c, const paos_pass& p, LoweredPass& lp, const double* blocks) {
  std::vector<double> key;
  key.reserve((size_t)2 * c->batch * FP_STRIDE + c->batch + 3);
  key.push_back((double)p.axis);
  key.push_back((double)(mask_render_mode() + (mask_rect_blocks() ? 0 : 8)));  // (the renderers give the same records bit for bit -- and a test that says so must render twice)
  const double* ap = blocks + (size_t)lp.mask_block * c->batch * FP_STRIDE;
  key.insert(key.end(), ap, ap + (size_t)2 * c->batch * FP_STRIDE);  // the two consecutive block sets
  key.insert(key.end(), lp.mask_shared.begin(), lp.mask_shared.end());
  int hit = -1, victim = 0;
  for (int k = 0; k < paos_ctx::kMaskSets; ++k) {
    const paos_ctx::MaskSet& ms = c->mask_sets[k];
    if (!ms.key.empty() && ms.key.size() == key.size() && !std::memcmp(ms.key.data(), key.data(), key.size() * sizeof(double))) hit = k;
    if (ms.used < c->mask_sets[victim].used) victim = k;
  }
  const int k = hit >= 0 ? hit : victim;
  paos_ctx::MaskSet& ms = c->mask_sets[k];
  if (!ms.lines) {
    // (every set of the context at the first use of any: a sweep walks through all of them within two or three programs, and an
    // allocation of this size in the middle of a later program stalls the stream -- a five-step bench run behind ONE warm-up step
    // measured 7 % low for it)
    for (paos_ctx::MaskSet& m2 : c->mask_sets) {
      if (m2.lines) continue;
      HIPCHK(c, hipMalloc(&m2.lines, (size_t)c->batch * c->n * sizeof(MaskLine)));
      HIPCHK(c, hipMalloc(&m2.vals, (size_t)c->batch * c->n * 2 * kMaskW * sizeof(double)));
    }
  }
  ms.used = ++c->mask_clock;
  lp.mask_set = k;
  lp.mask_render = hit < 0;
  lp.mask_shapes = 0;  // which of the two renderers have anything to do (the other one's launch would only exit)
  for (int it = 0; it < c->batch; ++it) {
    const double* a1 = ap + (size_t)it * FP_STRIDE;
    const double* a2 = a1 + (size_t)c->batch * FP_STRIDE;
    if (a1[0] != 0.0 && (it >= (int)lp.mask_shared.size() || lp.mask_shared[it] == 0.0)) lp.mask_shapes |= (int)a2[3] == 0 ? 1 : 2;
  }
  if (hit < 0) { ms.key = std::move(key); ++c->mask_rendered; } else ++c->mask_hits;
  for (int it = 0; it < c->batch; ++it) {
    if (lp.mask_rep[it] < 0) continue;
    FrugalSlot& sl = lp.mask_slot == 0 ? lp.items[it].pre : lp.items[it].mid;
    sl.lines = ms.lines + (size_t)lp.mask_rep[it] * c->n;
    sl.vals = ms.vals + (size_t)lp.mask_rep[it] * c->n * 2 * kMaskW;
  }
  return PAOS_OK;
}

void forget_mask_sets(paos_ctx* c) {  // after a failed program: what the sets hold is no longer known
  for (auto& ms : c->mask_sets) ms.key.clear();
}

MaskRender mask_job(paos_ctx* c, const paos_pass& p, const LoweredPass& lp, const double* ap, const double* dshared) {
  const int line0 = lp.mask_lo, line_end = lp.mask_hi > lp.mask_lo ? lp.mask_hi : c->n;
  return MaskRender{ap, dshared, lp.mask_set, p.axis, line0, line_end, lp.mask_shapes};
}

// Do all phases of the pass vary along its lines only (the row / column factors of the separable programs)?  Then their
// factors come from tables by position (frugal_pass.h: FrugalSlot::table).  complex128 only (the complex64 slots use the
// hardware sin / cos).  PAOS_LINE_TABLES=0: every slot evaluates.
bool phases_along_lines(const paos_ctx* c, const paos_pass& p, const LoweredPass& lp, bool or_none = false) {
  static const bool want = !env_is("PAOS_LINE_TABLES", '0');
  if (!want || (lp.kpre + lp.kmid == 0 && !or_none)) return false;
  const int counts[2] = {lp.kpre, lp.kmid};
  for (int l = 0; l < 2; ++l)
    for (const FrugalItem& fi : lp.items) {
      if (fi.active == 0.0) continue;
      const FrugalPhase* ph = l == 0 ? fi.pre_ph : fi.mid_ph;
      for (int j = 0; j < counts[l]; ++j)
        if ((p.axis == 0 ? ph[j].sy : ph[j].sx) != 0.0) return false;
    }
  return true;
}

// Can the launch of pass `p` go on with the next pass `p2` of the program (frugal_pass.h: LONG builds)?  Same axis, both on
// table slots with phases in every slot, a two-transform pass in front, and every item takes both or neither, on the same lines.  PAOS_FUSE_PAIRS=0: never.
bool can_fuse_pair(const paos_ctx* c, const paos_pass& p, const LoweredPass& lp, const paos_pass& p2, const LoweredPass& lp2) {
  if (env_is("PAOS_FUSE_PAIRS", '0')) return false;
  if (!lp.ok || !lp2.ok || p.axis != p2.axis || lp.nfft != 2) return false;
  // (an aperture may ride on either pass -- the second one's slots read their line records themselves -- but the two must not
  // share a record set that the second would have to re-render between them: sets are assigned per pass, in program order)
  if (lp.mask_block >= 0 && lp2.mask_block >= 0 && lp.mask_set == lp2.mask_set) return false;
  // (a slot without phases takes part with a table of ones: (v 1) f is v f bit for bit)
  if (!phases_along_lines(c, p, lp, true) || !phases_along_lines(c, p2, lp2, true)) return false;
  for (int it = 0; it < c->batch; ++it) {
    const FrugalItem &f1 = lp.items[it], &f2 = lp2.items[it];
    if ((f1.active != 0.0) != (f2.active != 0.0)) return false;
    if (f1.active != 0.0 && (f1.line_lo != f2.line_lo || f1.line_hi != f2.line_hi || f1.line_fill != 0.0)) return false;
  }
  return true;
}

// launch a pass that lower_frugal accepted -- and, with `next`, the pass behind it in the same launch (can_fuse_pair)
// One launch of a pass program: a pass and the one or two behind it that ride along (can_fuse_pair).
struct FusedGroup {
  LoweredPass* lp[3] = {nullptr, nullptr, nullptr};
  int q = 0, count = 1, axis = 0;
  bool tables = false;   // its slots read their phase factors from tables
  size_t item_base = 0;  // index of its first item record in the staged array
};

// Stage the launches `groups`: decide which of them run on table slots (all phases of all their passes along the lines;
// a fused group always does), point their slots at tables of the context's store, copy the item records of all of them to
// the device in ONE transfer and build all tables with ONE launch -- in front of the program's first launch, so that
// nothing but the pass kernels themselves stands between two passes (round 4: a copy and a table launch in front of
// every pass cost ~50 us of an 1.3 ms launch).  The records join the caller's batch `ab` (round 17: the block table and the
// renderings' vectors of a program travel in the same transfer); the table launch, launch_staged_tables, follows the
// batch's commit.  st->items: the device array; groups[g].item_base indexes it.
struct StagedTables {
  const FrugalItem* items = nullptr;
  const PhaseSlotDesc* descs = nullptr;
  unsigned count = 0;  // table descriptors: slots with phases
};
int stage_groups(paos_ctx* c, ArenaBatch& ab, std::vector<FusedGroup>& groups, StagedTables* st) {
  std::vector<FrugalItem> blob;
  std::vector<PhaseSlotDesc> descs;
  int slots = 0;
  for (FusedGroup& g : groups) {
    paos_pass axis_only{};
    axis_only.axis = g.axis;
    // (complex64: a slot evaluates its factors with the hardware sin / cos for less than the table's loads cost -- measured: dense
    // launches 2.03 -> 2.41 ms with tables -- so only the fused groups, whose one build reads tables, use them)
    g.tables = g.count > 1 || (c->precision == PAOS_F64 && phases_along_lines(c, axis_only, *g.lp[0]));
    if (g.tables && g.count == 1) {
      // (a single pass over most of the grid is bound by HBM, and the table's reads are traffic too: dense launches
      // 3.75 ms evaluated, 3.85-4.0 with tables -- tables where the pass works on at most half of the lines)
      double lines = 0.0, active = 0.0;
      for (const FrugalItem& fi : g.lp[0]->items)
        if (fi.active != 0.0) { lines += fi.line_hi - fi.line_lo; active += 1.0; }
      if (active > 0.0 && lines > 0.5 * active * c->n) g.tables = false;
    }
    if (g.tables) slots += 2 * g.count;
  }
  if (slots > c->ptab_slots) {
    if (c->ptab) { HIPCHK(c, hipStreamSynchronize(c->stream)); (void)hipFree(c->ptab); c->ptab = nullptr; c->ptab_slots = 0; }
    HIPCHK(c, hipMalloc(&c->ptab, (size_t)slots * c->batch * c->n * sizeof(cx<double>)));
    c->ptab_slots = slots;
  }
  int slot = 0;
  for (FusedGroup& g : groups) {
    g.item_base = blob.size();
    for (int k = 0; k < g.count; ++k) {
      LoweredPass& l = *g.lp[k];
      const int counts[2] = {l.kpre, l.kmid};
      for (int s = 0; s < 2; ++s) {
        // (in a fused group a slot without phases rides with a table of ones)
        const bool has = g.tables && (counts[s] > 0 || g.count > 1);
        for (int it = 0; it < c->batch; ++it)
          (s == 0 ? l.items[it].pre : l.items[it].mid).table = has ? c->ptab + ((size_t)slot * c->batch + it) * c->n : nullptr;
        if (has) descs.push_back(PhaseSlotDesc{(int)blob.size(), s, counts[s], g.axis});
        if (g.tables) ++slot;
      }
      blob.insert(blob.end(), l.items.begin(), l.items.end());
    }
  }
  static_assert(sizeof(FrugalItem) % sizeof(double) == 0 && sizeof(PhaseSlotDesc) == 2 * sizeof(double), "records of doubles");
  const size_t item_doubles = blob.size() * sizeof(FrugalItem) / sizeof(double);
  std::vector<double> flat(item_doubles + 2 * descs.size());
  std::memcpy(flat.data(), blob.data(), item_doubles * sizeof(double));
  if (!descs.empty()) std::memcpy(flat.data() + item_doubles, descs.data(), descs.size() * sizeof(PhaseSlotDesc));
  const double* dflat = nullptr;
  int rc = ab.add(flat.data(), flat.size(), &dflat);
  if (rc) return rc;
  st->items = reinterpret_cast<const FrugalItem*>(dflat);
  st->descs = reinterpret_cast<const PhaseSlotDesc*>(dflat + item_doubles);
  st->count = (unsigned)descs.size();
  return PAOS_OK;
}
// the tables of what stage_groups staged, behind the commit of its batch
int launch_staged_tables(paos_ctx* c, const StagedTables& st) {
  if (st.count == 0) return PAOS_OK;
  const PhaseTableArgs ta{st.items, reinterpret_cast<const cx<double>*>(c->tw), st.descs, c->n, c->precision == PAOS_F64 ? 0 : 1};
  hipLaunchKernelGGL(phase_table_kernel<0>, dim3(c->n / 256, c->batch, st.count), dim3(256), 0, c->stream, ta);
  HIPCHK(c, hipGetLastError());
  return PAOS_OK;
}

// Is there a build of this name in the context's family (frugal_launch.h: frugal_built)?
bool build_exists(const paos_ctx* c, const FrugalBuild& b) {
  if (c->precision != PAOS_F64) return c->n == 2048 ? frugal_built<float, 2048>(b) : frugal_built<float, 4096>(b);
  return c->n == 1024 ? frugal_built<double, 1024>(b) : (c->n == 2048 ? frugal_built<double, 2048>(b) : frugal_built<double, 4096>(b));
}

// THE place that says which build a launch takes: from the passes it runs (`lp` and the one or two that ride along), whether
// their slots read tables (stage_groups) and what it stores (FrugalBuild::store) to the name of the build.
FrugalBuild pick_build(const paos_ctx* c, int axis, const LoweredPass& lp, const LoweredPass* next, const LoweredPass* next2, bool tables,
                       int store) {
  FrugalBuild b{};
  b.axis = axis;
  // The table builds take "has phases" for the number of phases -- their slots read one factor --, and a fused launch runs on
  // the one build whose slots all read tables (a slot without phases: a table of ones).
  b.kpre = next ? 1 : (tables && lp.kpre > 1 ? 1 : lp.kpre);
  b.kmid = next ? 1 : (tables && lp.kmid > 1 ? 1 : lp.kmid);
  b.nfft = lp.nfft >= 2 ? 2 : 1;
  b.store = store;
  b.tab = tables ? 1 : 0;
  b.fuse = next2 ? 2 + next2->nfft : (next ? next->nfft : 0);
  // The PSF- and power-storing launches take neither of the builds below: their sums are laid out per two-line tile.
  if (!tables || store != 0) return b;
  // light: a single table pass whose every item loads and stores at most half of its positions -- one-line workgroups.
  // central: every active item of the FIRST pass loads positions of the central half only -- the central-half build of the
  // shape.  Per launch, not per item: one item outside sends the whole launch to the ordinary build.  (There is no device-side
  // guard: frugal_pass.h, CH.)
  bool light = !next, central = c->central_half, any = false;
  for (const FrugalItem& fi : lp.items) {
    if (fi.active == 0.0) continue;
    any = true;
    light = light && 2.0 * (fi.pos_hi - fi.pos_lo) <= (double)c->n && 2.0 * (fi.spos_hi - fi.spos_lo) <= (double)c->n;
    central = central && 4.0 * fi.pos_lo >= (double)c->n && 4.0 * fi.pos_hi <= 3.0 * (double)c->n;
  }
  // ... where there is one (the central-half builds run on one-line workgroups: a fused launch, or a light pass)
  b.one_line = light ? 1 : 0;
  if (!build_exists(c, b)) b.one_line = 0;
  b.central = central && any ? 1 : 0;
  if (!build_exists(c, b)) b.central = 0;
  return b;
}

int launch_lowered(paos_ctx* c, const paos_pass& p, LoweredPass& lp, const double* dblocks, bool store_psf = false,
                   bool sum_power = false, LoweredPass* next = nullptr, LoweredPass* next2 = nullptr,
                   const FrugalItem* staged = nullptr, bool staged_tables = false) {
  LoweredPass* const last = next2 ? next2 : next;  // the pass whose stores leave the launch (nullptr: this one)
  for (LoweredPass* l : {&lp, next, next2}) {  // render the records along the pass axis, right before the pass (every pass of a chain)
    if (!l || l->mask_block < 0 || !l->mask_render) continue;
    const double* ap = dblocks + (size_t)l->mask_block * c->batch * FP_STRIDE;
    const double* dshared = nullptr;
    int rcs = arena_push(c, l->mask_shared.data(), l->mask_shared.size(), &dshared);
    if (rcs) return rcs;
    const MaskRender job = mask_job(c, p, *l, ap, dshared);  // (a pair runs along one axis)
    if ((rcs = render_mask_records(c, &job, 1))) return rcs;
    l->mask_render = false;
  }
  // The item records (with the pointers to their slots' phase tables) and the tables themselves: staged for the whole
  // program in front of its first launch (stage_groups: one copy, one table launch), or here for this launch alone.
  bool tables = staged_tables;
  const FrugalItem* ditems_f = staged;
  if (!ditems_f) {
    FusedGroup g;
    g.lp[0] = &lp; g.lp[1] = next; g.lp[2] = next2; g.count = next2 ? 3 : (next ? 2 : 1);
    g.axis = p.axis;
    std::vector<FusedGroup> one{g};
    ArenaBatch ab(c);  // (inside the program's reservation: no begin)
    StagedTables st;
    int rcg = stage_groups(c, ab, one, &st);
    if (rcg || (rcg = ab.commit()) || (rcg = launch_staged_tables(c, st))) return rcg;
    tables = one[0].tables;
    ditems_f = st.items + one[0].item_base;
  }
  const double* ditems = reinterpret_cast<const double*>(ditems_f);
  FrugalArgs a{c->field, c->tw, reinterpret_cast<const FrugalItem*>(ditems), c->pitch, c->item_stride, nullptr, nullptr, nullptr};
  if (store_psf) { a.psf = c->psf; a.psf_partial = c->psf_partial; }
  if (sum_power) a.pow_partial = c->pow_partial;
  a.dyn_scale = c->dyn_scale;
  {  // the lines some item still works on: the grid need not cover the others when their tiles have nothing to write
    // PAOS_COMPACT_GRID=0 launches the full grid (dead workgroups exit in their prologue)
    static const bool want = !env_is("PAOS_COMPACT_GRID", '0');
    double lo = (double)c->n, hi = 0.0;
    bool fill = false;
    // (a fused pair: the lines are the same for both passes, what is stored and filled is the second pass's business)
    const std::vector<FrugalItem>& out_items = last ? last->items : lp.items;
    for (const FrugalItem& fi : out_items) {
      if (fi.active == 0.0) continue;
      lo = fi.line_lo < lo ? fi.line_lo : lo;
      hi = fi.line_hi > hi ? fi.line_hi : hi;
      if (fi.line_fill != 0.0 && store_psf) {  // dead tiles write PSF zeros inside [spos_lo, spos_hi) only (run_passes_impl)
        lo = fi.spos_lo < lo ? fi.spos_lo : lo;
        hi = fi.spos_hi > hi ? fi.spos_hi : hi;
      } else {
        fill = fill || fi.line_fill != 0.0;
      }
    }
    a.live_lo = a.live_hi = a.wg0 = 0;
    if (want && !fill && hi > lo && (lo > 0.0 || hi < (double)c->n)) {
      a.live_lo = (unsigned)lo;
      a.live_hi = (unsigned)hi;
    }
  }
  // for the launch timer: what does this launch skip?  bit 0: whole tiles of dead lines, bit 1: loads of dead
  // positions, bit 2: stores nobody reads, bit 3: it stores the PSF instead of the field
  c->prof_next_tag = store_psf ? 8 : 0;
  c->prof_next_bytes = 0.0;
  c->prof_next_lines = 0.0;
  if (next) c->prof_next_tag |= next2 ? 32 : 16;  // bit 4: the launch ran two passes of the program, bit 5: three
  for (int it = 0; it < c->batch; ++it) {
    const FrugalItem& fi = lp.items[it];
    const FrugalItem& fo = last ? last->items[it] : fi;  // the pass whose stores leave the launch
    if (fi.active == 0.0) continue;
    if (fi.line_lo > 0.0 || fi.line_hi < (double)c->n) c->prof_next_tag |= 1;
    if (fi.pos_lo > 0.0 || fi.pos_hi < (double)c->n) c->prof_next_tag |= 2;
    if (!store_psf && (fo.spos_lo > 0.0 || fo.spos_hi < (double)c->n)) c->prof_next_tag |= 4;
    // what the plan has this launch move: its live lines' loaded and stored positions (the PSF store: doubles, every position)
    c->prof_next_bytes += (fi.line_hi - fi.line_lo) * ((fi.pos_hi - fi.pos_lo) * (double)elem_bytes(c) +
                                                        (store_psf ? (double)c->n * 8.0 : (fo.spos_hi - fo.spos_lo) * (double)elem_bytes(c)));
    // ... and compute: every live line goes through the transforms that are switched on for this item, in every pass of the launch
    for (const LoweredPass* l : {(const LoweredPass*)&lp, (const LoweredPass*)next, (const LoweredPass*)next2}) {
      if (!l) continue;
      const FrugalItem& fk = l->items[it];
      c->prof_next_lines += (fi.line_hi - fi.line_lo) * ((fk.fft1_on != 0.0 ? 1.0 : 0.0) + (l->nfft >= 2 && fk.fft2_on != 0.0 ? 1.0 : 0.0));
    }
  }
  const FrugalBuild b = pick_build(c, p.axis, lp, next, next2, tables, store_psf ? 1 : (sum_power ? 2 : 0));
  // PAOS_DUMP_PASSES=1: on stderr, the build the launch takes and one line per pass it runs (what item 0's two slots carry)
  static const bool dump = env_is("PAOS_DUMP_PASSES", '1');
  {  // paos_pass_builds: the record the family function gets, in launch order
    const int rec[9] = {b.axis, b.kpre, b.kmid, b.nfft, b.store, b.tab, b.fuse, b.one_line, b.central};
    c->pass_builds.insert(c->pass_builds.end(), rec, rec + 9);
  }
  if (dump) {
    std::fprintf(stderr, "build axis %d kpre %d kmid %d nfft %d store %d tab %d fuse %d one_line %d central %d n %d %s\n", b.axis, b.kpre, b.kmid,
                 b.nfft, b.store, b.tab, b.fuse, b.one_line, b.central, c->n, c->precision == PAOS_F64 ? "fp64" : "fp32");
    for (const LoweredPass* l : {(const LoweredPass*)&lp, (const LoweredPass*)next, (const LoweredPass*)next2}) {
      if (!l || l->items.empty()) continue;
      const FrugalItem& f = l->items[0];  // ("+pass": rides in the launch of the pass above it)
      std::fprintf(stderr, "%spass axis %d kpre %d kmid %d nfft %d | pre: sign %g scale %g mask %g | fft1 on %g inv %g | mid: sign %g scale %g mask %g | "
                   "fft2 on %g inv %g | lines [%g, %g) fill %g loads [%g, %g) stores [%g, %g)\n", l == &lp ? "" : "+", p.axis, l->kpre, l->kmid, l->nfft,
                   f.pre.sign_on, f.pre.scale, f.pre.mask_on, f.fft1_on, f.fft1_inv, f.mid.sign_on, f.mid.scale, f.mid.mask_on, f.fft2_on, f.fft2_inv,
                   f.line_lo, f.line_hi, f.line_fill, f.pos_lo, f.pos_hi, f.spos_lo, f.spos_hi);
    }
  }
  if (c->precision == PAOS_F64) {
    switch (c->n) {
      case 1024: return paos_frugal_d1024(c, b, a);
      case 2048: return paos_frugal_d2048(c, b, a);
      default: return paos_frugal_d4096(c, b, a);
    }
  }
  switch (c->n) {
    case 2048: return paos_frugal_f2048(c, b, a);
    default: return paos_frugal_f4096(c, b, a);
  }
}

int launch_one_pass(paos_ctx* c, const paos_pass& p, const double* dblocks, int n_blocks,
                    const int* table_of_op /* [3][PAOS_MAX_PW], -1 = none */) {
  int rc;
  if ((rc = check_ops(c, p.pre, p.n_pre, n_blocks))) return rc;
  if ((rc = check_ops(c, p.mid, p.n_mid, n_blocks))) return rc;
  if ((rc = check_ops(c, p.post, p.n_post, n_blocks))) return rc;
  if (p.fft1 >= n_blocks || p.fft2 >= n_blocks) return fail(c, PAOS_EINVAL, "transform control block out of range");
  {  // at most one aperture operator per pass: its weight map is rendered right before it
    const paos_pw_op* lists3[3] = {p.pre, p.mid, p.post};
    const int counts3[3] = {p.n_pre, p.n_mid, p.n_post};
    int nmask = 0;
    for (int l = 0; l < 3; ++l)
      for (int o = 0; o < counts3[l]; ++o)
        if (lists3[l][o].kind == PAOS_PW_MASK) {
          if (++nmask > 1) return fail(c, PAOS_EINVAL, "one aperture operator per pass");
          int rcm = render_mask_weights(c, dblocks + (size_t)lists3[l][o].block * c->batch * FP_STRIDE);
          if (rcm) return rcm;
        }
  }
  PassArgs a{};
  a.field = c->field; a.tw = c->tw; a.blocks = dblocks; a.tables = c->tables; a.mask = c->mask; a.batch = c->batch;
  a.fft1 = p.fft1; a.fft2 = p.fft2; a.n_pre = p.n_pre; a.n_mid = p.n_mid; a.n_post = p.n_post;
  static_assert(sizeof(PwOp) == sizeof(paos_pw_op), "ABI op layout");
  std::memcpy(a.pre, p.pre, sizeof(a.pre));
  std::memcpy(a.mid, p.mid, sizeof(a.mid));
  std::memcpy(a.post, p.post, sizeof(a.post));
  PwOp* lists[3] = {a.pre, a.mid, a.post};
  const int counts[3] = {a.n_pre, a.n_mid, a.n_post};
  int feat = 0;
  for (int l = 0; l < 3; ++l)
    for (int o = 0; o < PAOS_MAX_PW; ++o) {
      lists[l][o].flags &= (1 << kTableShift) - 1;
      const int t = table_of_op[l * PAOS_MAX_PW + o];
      if (t >= 0) { lists[l][o].flags |= (t + 1) << kTableShift; feat = 3; }
      if (o < counts[l] && lists[l][o].kind == PWK_MASK) feat = 3;
    }
  a.pitch = c->pitch; a.item_stride = c->item_stride;
  if (p.axis == 0 || p.axis == 1) return generic_pass(c, p.axis, a, feat);
  if (p.axis != -1) return fail(c, PAOS_EINVAL, "pass axis must be 0, 1 or -1");
  if (p.fft1 >= 0 || p.fft2 >= 0 || p.n_mid || p.n_post)
    return fail(c, PAOS_EINVAL, "a transform-free pass carries its operators in the pre list");
  return pointwise_pass(c, a);
}

// PAOS_NO_PRUNE=1 processes every tile (A/B tests of the dead-line pruning).
bool use_pruning() {
  static const bool on = !env_is("PAOS_NO_PRUNE", '1');
  return on;
}

// entry_rows / entry_stale: see paos_program_opts.  final_ticket != nullptr: the caller wants |u|^2 and its sum of
// the field the program ends with, not the field.
int run_passes_impl(paos_ctx* c, const paos_pass* passes, int n_passes, const double* blocks, int n_blocks,
                    const double* entry_rows, bool entry_stale, int* final_ticket, int final_mode, const double* entry_cols) {
  if (c) c->pass_builds.clear();  // (paos_pass_builds: the launches of THIS program)
  if (!c || !passes || !blocks || n_passes < 0 || n_blocks < 1) return fail(c, PAOS_EINVAL, "bad pass program");
  c->norm2_of_field = false;  // (set again at the end when the last pass sums the power of what it stores)
  // A program that ends on the PSF gives the field up for it: the free power-ticket slot it will need is checked
  // BEFORE anything is launched (found full afterwards, the context held neither field nor ticket).
  if (int rcr = final_ticket ? power_ring_full(c) : PAOS_OK) return rcr;
  // The device sincos has no huge-argument path: bound every enabled phase operator here.
  for (int i = 0; i < n_passes; ++i) {
    const paos_pw_op* lists[3] = {passes[i].pre, passes[i].mid, passes[i].post};
    const int counts[3] = {passes[i].n_pre, passes[i].n_mid, passes[i].n_post};
    for (int l = 0; l < 3; ++l)
      for (int o = 0; o < counts[l] && o < PAOS_MAX_PW; ++o) {
        const paos_pw_op& op = lists[l][o];
        if (op.kind != PAOS_PW_QPHASE_CENTRED && op.kind != PAOS_PW_QPHASE_NATURAL) continue;
        if (op.block < 0 || op.block >= n_blocks) return fail(c, PAOS_EINVAL, "operator block index out of range");
        for (int it = 0; it < c->batch; ++it) {
          const double* p = blocks + ((size_t)op.block * c->batch + it) * FP_STRIDE;
          if (p[FP_ENABLE] == 0.0) continue;
          const double hx = 0.5 * c->n * p[FP_SX], hy = 0.5 * c->n * p[FP_SY];
          double arg = std::fabs(p[FP_COEF]) * (hx * hx + hy * hy);
          if (op.flags & PAOS_PWF_MUL2PI) arg *= 6.283185307179586;
          if (!(arg < kMaxPhaseArg))
            return fail(c, PAOS_EUNSUPPORTED, "quadratic phase exceeds 1e12 rad at the grid corner (or is not finite)");
        }
      }
  }
  const double* dblocks = nullptr;
  // everything this program pushes stays live until its last pass has run: the block table and,
  // per pass, one FrugalItem record per batch item (each push is rounded up to 16 doubles)
  // plus, for a pass that carries an aperture, the [batch] "shares its line records" vector (launch_lowered)
  // ... and two table descriptors (stage_groups)
  const size_t per_pass = (((size_t)c->batch * sizeof(FrugalItem) / sizeof(double) + 15) & ~size_t(15)) +
                          (((size_t)c->batch + 15) & ~size_t(15)) + 16;
  // ... and the two windows of zero_outside_box.  Round 17: the block table, the vectors of the batched renderings and the
  // staged records are ONE batch, copied once in front of the program's first launch that reads any of them; whatever is
  // pushed launch by launch behind that (arena_push: a copy of its own) still lies inside this reservation.
  ArenaBatch ab(c);
  int rc = ab.begin((size_t)n_blocks * c->batch * FP_STRIDE + 16 + (size_t)n_passes * per_pass + 2 * arena_rounded((size_t)2 * c->batch));
  if (rc) return rc;
  rc = ab.add(blocks, (size_t)n_blocks * c->batch * FP_STRIDE, &dblocks);
  if (rc) return rc;
  // Lower every pass for the frugal kernels first; when the whole program runs on them, plan the
  // pruning of dead lines across it (look-ahead), then launch.
  std::vector<LoweredPass> low(n_passes);
  bool all_frugal = !use_tables() && frugal_sizes(c) && n_passes > 0;
  if (!use_tables() && frugal_sizes(c)) {
    if ((rc = ensure_mask_store(c))) return rc;
    for (int q = 0; q < n_passes; ++q) {
      LoweredPass& lp = low[q];
      lp.ok = lower_frugal(c, passes[q], blocks, lp);
      if (lp.ok && lp.mask_block >= 0 && (rc = assign_mask_set(c, passes[q], lp, blocks))) return rc;
      all_frugal = all_frugal && lp.ok;
    }
  }
  if (c->dyn_pending) {
    // a stop's scaling is waiting: the first pass takes it along in its middle slot when it is a frugal pass every item
    // takes part in; otherwise the field gets it now
    bool ride = n_passes > 0 && low[0].ok;
    if (ride)
      for (const FrugalItem& fi : low[0].items) ride = ride && fi.active != 0.0;
    if (ride) ++c->deferred_rode;
    if (!ride && (rc = settle_scale(c))) return rc;
  }
  const bool pruned = all_frugal && use_pruning() && c->prune;
  if (pruned) plan_pruning(c, passes, n_passes, blocks, low, entry_rows, entry_stale, entry_cols);
  // Which lines' aperture records does each pass read?  Those of its live tiles only: a workgroup whose lines are dead
  // for its item (frugal_pass_kernel: outside [line_lo, line_hi), bounds that are multiples of the tile height)
  // leaves before it looks at a record.  Only these lines are rendered (a quarter of them behind a clear aperture at
  // zoom 4), and a set found in the context's store is good only if it was rendered that far.
  {
    for (int q = 0; q < n_passes; ++q) {
      LoweredPass& lp = low[q];
      if (!lp.ok || lp.mask_block < 0) continue;
      double lo = (double)c->n, hi = 0.0;
      for (const FrugalItem& fi : lp.items) {
        if (fi.active == 0.0) continue;
        lo = fi.line_lo < lo ? fi.line_lo : lo;
        hi = fi.line_hi > hi ? fi.line_hi : hi;
      }
      const bool window = hi > lo;
      lp.mask_lo = window ? (int)lo : 0;
      lp.mask_hi = window ? (int)hi : c->n;
      paos_ctx::MaskSet& ms = c->mask_sets[lp.mask_set];
      if (!lp.mask_render && !(ms.line_lo <= lp.mask_lo && ms.line_hi >= lp.mask_hi)) {
        lp.mask_render = true;  // found, but rendered for a narrower window than this pass reads
        --c->mask_hits; ++c->mask_rendered;
      }
      if (lp.mask_render) { ms.line_lo = lp.mask_lo; ms.line_hi = lp.mask_hi; }
    }
  }
  if (entry_stale && entry_rows) {
    // Rows that merely stand for zeros must become zeros wherever the program will not consume them: everywhere when
    // the planner is off, and for an item no pass of the program touches.
    bool need = !pruned;
    for (int it = 0; it < c->batch && !need; ++it) {
      bool active = false;
      for (int q = 0; q < n_passes; ++q) active = active || low[q].items[it].active != 0.0;
      need = !active;
    }
    // ... and for an item whose window is empty: the planner takes an empty window for no window at all (plan_pruning),
    // so its first pass would load every line of stale data
    const double* windows[2] = {entry_rows, entry_cols};
    for (int w = 0; w < 2 && !need; ++w)
      for (int it = 0; windows[w] && it < c->batch && !need; ++it) {
        const int br = c->br, l = ((int)windows[w][2 * it] / br) * br;
        int h = (((int)windows[w][2 * it + 1] + br - 1) / br) * br;
        if (h > c->n) h = c->n;
        need = l >= h;
      }
    if (need) {
      // (all items at once: the ones the planner handles lose nothing but a little time, and the planner was told
      // "stale", which is also right for zeros)
      if ((rc = entry_cols ? zero_outside_box(c, entry_rows, entry_cols) : zero_outside_rows(c, entry_rows))) return rc;
    }
  }
  // The PSF instead of the field: the last pass stores |u|^2 and its per-workgroup sums (frugal_pass.h: STORE) when
  // it runs on the frugal kernels in a shape built for it and every item takes part; otherwise the program runs as
  // usual and the intensity sweep follows.
  bool fused_store = false, fused_power = false;
  int power_groups = 0;
  if (final_ticket && final_mode == 2) {
    // The field is kept AND its power is wanted (a saved surface, run.py:218-223 callers): the last pass sums |u|^2 of
    // its tiles while it stores them (FrugalArgs::pow_partial) -- when it runs on the frugal kernels and every item
    // takes part; otherwise the ordinary reduction follows the program.
    fused_power = n_passes > 0 && low[n_passes - 1].ok && low[n_passes - 1].kpre <= 1;  // (the shapes built with STORE = 2)
    if (fused_power)
      for (const FrugalItem& fi : low[n_passes - 1].items) fused_power = fused_power && fi.active != 0.0;
    if (fused_power) {
      power_groups = c->n / frugal_tile_lines(c, passes[n_passes - 1].axis);
      if (c->pow_nparts < c->n / 2) {  // (sized for the finest tiling of either axis)
        if (c->pow_partial) (void)hipFree(c->pow_partial);
        c->pow_partial = nullptr; c->pow_nparts = 0;
        HIPCHK(c, hipMalloc(&c->pow_partial, (size_t)c->batch * (c->n / 2) * sizeof(double)));
        c->pow_nparts = c->n / 2;
      }
      // dead tiles and workgroups that are not launched at all contribute nothing: zeros
      HIPCHK(c, hipMemsetAsync(c->pow_partial, 0, (size_t)c->batch * power_groups * sizeof(double), c->stream));
    }
  }
  if (final_ticket && final_mode != 2) {
    if (!c->psf) HIPCHK(c, hipMalloc(&c->psf, (size_t)c->batch * c->item_stride * sizeof(double)));
    c->otf_valid = false;  // a new PSF: the transfer functions computed from the previous one are stale
    fused_store = n_passes > 0 && low[n_passes - 1].ok && low[n_passes - 1].kpre <= 1 && low[n_passes - 1].kmid <= 1;
    if (fused_store)
      for (const FrugalItem& fi : low[n_passes - 1].items) fused_store = fused_store && fi.active != 0.0;
    if (fused_store) {
      const int groups = c->n / frugal_tile_lines(c, passes[n_passes - 1].axis);
      if (c->psf_nparts < groups) {
        if (c->psf_partial) (void)hipFree(c->psf_partial);
        c->psf_partial = nullptr; c->psf_nparts = 0;
        c->psf_zero_axis = -1;
        HIPCHK(c, hipMalloc(&c->psf_partial, (size_t)c->batch * groups * sizeof(double)));
        c->psf_nparts = groups;
      }
      // dead tiles of the storing pass write PSF zeros (line_fill) -- unless the buffer already holds zeros there:
      // the previous storing pass had the same live lines (the next batch of a sweep, the next Monte-Carlo batch)
      static const bool reuse = !env_is("PAOS_PSF_ZERO_REUSE", '0');
      const int axis = passes[n_passes - 1].axis;
      std::vector<FrugalItem>& last = low[n_passes - 1].items;
      // Round 4: per item.  What the buffer may still hold of the previous storing pass lies inside that pass's live
      // lines [psf_zero_lo, psf_zero_hi); only dead tiles of THIS pass that meet them write zeros (the range travels in
      // the item's -- here otherwise unused -- store-position fields).  A walked sweep changes the sampling at the
      // image plane from batch to batch, so the live lines are never the same twice, but they move by a few lines.
      const bool known = reuse && c->psf_zero_axis == axis && (int)c->psf_zero_lo.size() == c->batch;
      c->psf_zero_lo.resize(c->batch); c->psf_zero_hi.resize(c->batch);
      for (int it = 0; it < c->batch; ++it) {
        const double old_lo = known ? c->psf_zero_lo[it] : 0.0, old_hi = known ? c->psf_zero_hi[it] : (double)c->n;
        const bool covered = old_lo >= last[it].line_lo && old_hi <= last[it].line_hi;  // every old line is rewritten
        last[it].line_fill = covered ? 0.0 : 1.0;
        last[it].spos_lo = covered ? 0.0 : old_lo;
        last[it].spos_hi = covered ? (double)c->n : old_hi;
        c->psf_zero_lo[it] = last[it].line_lo; c->psf_zero_hi[it] = last[it].line_hi;
      }
      c->psf_zero_axis = -1;  // set again below once the pass is on the stream
    }
  }
  // The aperture line records this program has to render (not found in the context's kept sets): all of them in ONE
  // launch per shape, in front of the first pass -- when every rendering goes to a set no EARLIER pass of this program
  // reads (always, unless a program carries more distinct apertures than there are sets; then each is rendered in place,
  // right before its pass).  PAOS_BATCHED_RECORDS=0: in place, one launch per aperture, as before.
  std::vector<MaskRender> renderings;
  {
    static const bool want = !env_is("PAOS_BATCHED_RECORDS", '0');
    std::vector<int> todo;
    bool safe = want && all_frugal;
    for (int q = 0; q < n_passes && safe; ++q) {
      if (low[q].mask_block < 0) continue;
      if (low[q].mask_render) {
        for (int r = 0; r < q; ++r) safe = safe && !(low[r].mask_block >= 0 && low[r].mask_set == low[q].mask_set);
        todo.push_back(q);
      }
    }
    if (safe && todo.size() > 1) {  // (launched below, behind the commit)
      for (int q : todo) {
        LoweredPass& lp = low[q];
        const double* dshared = nullptr;
        if ((rc = ab.add(lp.mask_shared.data(), lp.mask_shared.size(), &dshared))) return rc;
        renderings.push_back(mask_job(c, passes[q], lp, dblocks + (size_t)lp.mask_block * c->batch * FP_STRIDE, dshared));
        lp.mask_render = false;
      }
    }
  }
  // The launches of the program: a pass, or two / three consecutive passes of one row / column chain (can_fuse_pair).
  // When every pass runs on the frugal kernels their item records and phase tables are staged here, once, for all of
  // them (stage_groups); otherwise each launch stages its own.  PAOS_STAGE_PROGRAM=0: each launch stages its own.
  std::vector<FusedGroup> groups;
  std::vector<int> group_of(n_passes, -1);
  const FrugalItem* staged_items = nullptr;
  StagedTables staged;
  {
    for (int q = 0; q < n_passes;) {
      FusedGroup g;
      g.q = q; g.axis = passes[q].axis; g.lp[0] = &low[q];
      if (low[q].ok && all_frugal && pruned) {
        const bool pair = q + 1 < n_passes && can_fuse_pair(c, passes[q], low[q], passes[q + 1], low[q + 1]);
        // (and a third: the five-transform chains -- ptp, stw, ptp -- that end a SYN20-like prescription)
        const bool triple = pair && q + 2 < n_passes && can_fuse_pair(c, passes[q + 1], low[q + 1], passes[q + 2], low[q + 2]) &&
                            !(low[q].mask_block >= 0 && low[q + 2].mask_block >= 0 && low[q].mask_set == low[q + 2].mask_set);
        g.count = triple ? 3 : (pair ? 2 : 1);
        for (int k = 1; k < g.count; ++k) g.lp[k] = &low[q + k];
      }
      group_of[q] = (int)groups.size();
      groups.push_back(g);
      q += g.count;
    }
    // (a table per operator slot of every pass: 2 MiB each at 4096^2 x 32; a program that would need more than 1 GiB of
    // them -- hundreds of passes -- stages launch by launch, on six tables)
    const size_t table_bytes = (size_t)2 * n_passes * c->batch * c->n * sizeof(cx<double>);
    if (all_frugal && !env_is("PAOS_STAGE_PROGRAM", '0') && table_bytes <= (size_t(1) << 30)) {
      if ((rc = stage_groups(c, ab, groups, &staged))) return rc;
      staged_items = staged.items;
    }
  }
  // THE copy of the program, in front of its first launch that reads a block: the record renderings, the table kernel, or
  // the first pass.  (What ran above -- a settled stop scale, zeroed windows -- reads none of this batch.)
  if ((rc = ab.commit())) return rc;
  for (size_t at = 0; at < renderings.size(); at += kMaskRenders)
    if ((rc = render_mask_records(c, renderings.data() + at, (int)std::min<size_t>(kMaskRenders, renderings.size() - at)))) return rc;
  if ((rc = launch_staged_tables(c, staged))) return rc;
  // Walk the program in chunks whose phase operators fit the table store: fill the tables of
  // a chunk with one small launch, then run its passes.
  int i = 0;
  while (i < n_passes) {
    TableArgs ta{};
    ta.blocks = dblocks; ta.tables = c->tables; ta.batch = c->batch; ta.n = c->n; ta.count = 0;
    std::vector<int> assign;  // per pass of the chunk: [3][PAOS_MAX_PW]
    int j = i;
    for (; j < n_passes; ++j) {
      const paos_pass& p = passes[j];
      const paos_pw_op* lists[3] = {p.pre, p.mid, p.post};
      const int counts[3] = {p.n_pre, p.n_mid, p.n_post};
      int need = 0;
      for (int l = 0; l < 3; ++l)
        for (int o = 0; o < counts[l] && o < PAOS_MAX_PW; ++o)
          need += (lists[l][o].kind == PAOS_PW_QPHASE_CENTRED || lists[l][o].kind == PAOS_PW_QPHASE_NATURAL);
      if (use_tables() && ta.count + need > kMaxTables) {
        if (j == i) return fail(c, PAOS_EINVAL, "one pass needs more phase tables than the store holds");
        break;
      }
      const size_t base = assign.size();
      assign.resize(base + 3 * PAOS_MAX_PW, -1);
      if (!use_tables()) continue;
      for (int l = 0; l < 3; ++l)
        for (int o = 0; o < counts[l] && o < PAOS_MAX_PW; ++o) {
          const paos_pw_op& op = lists[l][o];
          if (op.kind != PAOS_PW_QPHASE_CENTRED && op.kind != PAOS_PW_QPHASE_NATURAL) continue;
          if (op.block < 0 || op.block >= n_blocks) return fail(c, PAOS_EINVAL, "operator block index out of range");
          ta.jobs[ta.count] = {op.block, op.kind, op.flags & PAOS_PWF_MUL2PI};
          assign[base + l * PAOS_MAX_PW + o] = ta.count++;
        }
    }
    if (ta.count > 0) {
      if (!c->tables) {  // opt-in feature: allocate on first use
        HIPCHK(c, hipMalloc(&c->tables, (size_t)kMaxTables * c->batch * 2 * c->n * sizeof(cx<double>)));
        ta.tables = c->tables;
      }
      const dim3 grid((2 * c->n + 255) / 256, c->batch, ta.count);
      hipLaunchKernelGGL(phase_table_kernel, grid, dim3(256), 0, c->stream, ta);
      HIPCHK(c, hipGetLastError());
    }
    for (int q = i; q < j; ++q) {
      if (low[q].ok) {
        // (a group of up to three passes of one row / column chain runs in ONE launch: frugal_pass.h, LONG builds)
        const FusedGroup& g = groups[group_of[q]];
        const int last = q + g.count - 1;
        if (last >= j) return fail(c, PAOS_EINVAL, "a fused group crosses a table chunk");
        if ((rc = launch_lowered(c, passes[q], low[q], dblocks, fused_store && last == n_passes - 1, fused_power && last == n_passes - 1,
                                 g.lp[1], g.lp[2], staged_items ? staged_items + g.item_base : nullptr, g.tables))) return rc;
        q = last;
        if (c->dyn_pending) {  // (first launch of the program) the stop's factor has gone into the field: ones again for the next
          if ((rc = dyn_scale_reset(c))) return rc;
        }
        continue;
      }
      if ((rc = launch_one_pass(c, passes[q], dblocks, n_blocks, &assign[(size_t)(q - i) * 3 * PAOS_MAX_PW]))) return rc;
    }
    i = j;
  }
  if (final_ticket && final_mode == 2) {
    // (the fallback: a generic-kernel pass, or an item that sat the last pass out)
    const int rcp = fused_power ? take_power_ticket(c, c->pow_partial, power_groups, nullptr, final_ticket) : paos_norm2_enqueue(c, final_ticket);
    if (rcp == PAOS_OK) c->norm2_of_field = true;  // c->norm2 = the power of every item's field as stored
    return rcp;
  }
  if (final_ticket) {
    if (fused_store) {
      c->psf_zero_axis = passes[n_passes - 1].axis;  // every launch of the program went through
      return take_power_ticket(c, c->psf_partial, c->n / frugal_tile_lines(c, passes[n_passes - 1].axis), nullptr, final_ticket);
    }
    return psf_keep_power_impl(c, final_ticket);
  }
  return PAOS_OK;
}

}  // namespace

int run_passes(paos_ctx* c, const paos_pass* passes, int n_passes, const double* blocks, int n_blocks, const double* entry_rows,
               bool entry_stale, int* final_ticket, int final_mode, const double* entry_cols) {
  const int rc = arena_settled(c, run_passes_impl(c, passes, n_passes, blocks, n_blocks, entry_rows, entry_stale, final_ticket, final_mode, entry_cols));
  if (rc != PAOS_OK && c) forget_mask_sets(c);  // a program that stopped half way: which records were rendered is moot
  return rc;
}

// How ellipse records are rendered (read per call: tests switch it).  PAOS_MASK_SCAN=1: the chunk scan of rounds 2-3 (0);
// PAOS_MASK_PAIRS=0: one line per wave through two 32-pixel windows (1), =1: two lines per wave through 16-pixel windows
// where they fit (2); default: four lines per wave through 8-pixel windows where they fit (3).
int mask_render_mode() {
  if (env_is("PAOS_MASK_SCAN", '1')) return 0;
  return env_is("PAOS_MASK_PAIRS", '0') ? 1 : (env_is("PAOS_MASK_PAIRS", '1') ? 2 : 3);
}
// ... and rectangle records: 64 lines per wave from one column profile (round 5); PAOS_MASK_RECT_BLOCKS=0: one line per wave
bool mask_rect_blocks() {
  return !env_is("PAOS_MASK_RECT_BLOCKS", '0');
}

namespace {

// ---- the reference's primitives as pass programs --------------------------------------
struct Program {
  std::vector<paos_pass> passes;
  std::vector<double> blocks;
  int batch;
  explicit Program(int b) : batch(b) {}
  // block set with the enable flags of `src` (stride FP_STRIDE) and the given payload
  int add_block(const double* src, double v1, double v2, double v3, double v4, bool copy) {
    const int id = (int)(blocks.size() / ((size_t)batch * FP_STRIDE));
    for (int i = 0; i < batch; ++i) {
      const double* s = src + (size_t)i * FP_STRIDE;
      if (copy) blocks.insert(blocks.end(), s, s + FP_STRIDE);
      else blocks.insert(blocks.end(), {s[FP_ENABLE], v1, v2, v3, v4});
    }
    return id;
  }
  paos_pass& add_pass(int axis, int fft1, int fft2) {
    paos_pass p{};
    p.axis = axis; p.fft1 = fft1; p.fft2 = fft2;
    passes.push_back(p);
    return passes.back();
  }
};
void push(paos_pw_op* list, int& count, int kind, int block, int flags = 0) { list[count++] = {kind, flags, block}; }

enum FftOp { OP_PTP, OP_STW, OP_WTS };

int fft_op(paos_ctx* c, FftOp op, const double* params, int inverse) {
  if (!c || !params) return fail(c, PAOS_EINVAL, "null argument");
  Program g(c->batch);
  const double inv_n = 1.0 / c->n;
  const int par = g.add_block(params, 0, 0, 0, 0, true);
  const int scl = g.add_block(params, 0, 0, inv_n, 0, false);
  if (op == OP_PTP) {
    const int fwd = g.add_block(params, 0, 0, 0, 0, false), inv = g.add_block(params, 1, 0, 0, 0, false);
    g.add_pass(0, fwd, -1);
    { paos_pass& p = g.add_pass(1, fwd, inv); push(p.mid, p.n_mid, PAOS_PW_QPHASE_NATURAL, par); push(p.mid, p.n_mid, PAOS_PW_SCALE, scl); }
    { paos_pass& p = g.add_pass(0, inv, -1); push(p.mid, p.n_mid, PAOS_PW_SCALE, scl); }
  } else {
    const int ctl = g.add_block(params, inverse ? 1.0 : 0.0, 0, 0, 0, false);
    paos_pass& r = g.add_pass(0, ctl, -1);
    push(r.pre, r.n_pre, PAOS_PW_SIGN, par);
    if (op == OP_WTS) push(r.pre, r.n_pre, PAOS_PW_QPHASE_CENTRED, par);
    paos_pass& q = g.add_pass(1, ctl, -1);
    push(q.mid, q.n_mid, PAOS_PW_SIGN, par);
    if (op == OP_STW) push(q.mid, q.n_mid, PAOS_PW_QPHASE_CENTRED, par);
    push(q.mid, q.n_mid, PAOS_PW_SCALE, scl);
  }
  return run_passes(c, g.passes.data(), (int)g.passes.size(), g.blocks.data(),
                    (int)(g.blocks.size() / ((size_t)c->batch * FP_STRIDE)));
}

}  // namespace

extern "C" {

int paos_run_program(paos_ctx* c, const paos_pass* passes, int n_passes, const double* blocks, int n_blocks,
                     const paos_program_opts* opts) {
  if (c) (void)hipSetDevice(c->device);
  if (!opts) return run_passes(c, passes, n_passes, blocks, n_blocks);
  if (c && opts->live_rows) {
    int rc = check_rows(c, opts->live_rows);
    if (rc) return rc;
  }
  if (opts->final_intensity && !opts->power_ticket) return fail(c, PAOS_EINVAL, "final_intensity needs a place for the power ticket");
  if (opts->final_intensity < 0 || opts->final_intensity > 2) return fail(c, PAOS_EINVAL, "final_intensity: 0, 1 (PSF instead of the field) or 2 (field + its power)");
  const bool stale = opts->live_rows && opts->rows_stale != 0;
  if (c && opts->live_cols && stale) {
    int rc = check_rows(c, opts->live_cols);
    if (rc) return rc;
  }
  return run_passes(c, passes, n_passes, blocks, n_blocks, opts->live_rows, stale,
                    opts->final_intensity ? opts->power_ticket : nullptr, opts->final_intensity == 2 ? 2 : 1,
                    stale ? opts->live_cols : nullptr);
}

int paos_frugal_built(int precision, int n, const int* record) {
  if (!record) return -PAOS_EINVAL;  // (negative: PAOS_EINVAL itself is 1, "built")
  const FrugalBuild b{record[0], record[1], record[2], record[3], record[4], record[5], record[6], record[7], record[8]};
  if (precision == PAOS_F64) {
    if (n == 1024) return frugal_built<double, 1024>(b) ? 1 : 0;
    if (n == 2048) return frugal_built<double, 2048>(b) ? 1 : 0;
    if (n == 4096) return frugal_built<double, 4096>(b) ? 1 : 0;
  } else if (precision == PAOS_F32) {
    if (n == 2048) return frugal_built<float, 2048>(b) ? 1 : 0;
    if (n == 4096) return frugal_built<float, 4096>(b) ? 1 : 0;
  }
  return -PAOS_EINVAL;
}

int paos_pass_builds(paos_ctx* c, int* records, int capacity, int* count) {
  if (!c || !count || capacity < 0 || (capacity > 0 && !records)) return fail(c, PAOS_EINVAL, "bad pass-builds request");
  const int have = (int)(c->pass_builds.size() / 9);
  *count = have;
  if (have > 0 && capacity > 0) std::memcpy(records, c->pass_builds.data(), (size_t)(have < capacity ? have : capacity) * 9 * sizeof(int));
  return PAOS_OK;
}

int paos_phase(paos_ctx* c, const double* params, int mul2pi) {
  SETTLE_SCALE(c);
  if (c) (void)hipSetDevice(c->device);  // one process may drive several GPUs
  if (!c || !params) return fail(c, PAOS_EINVAL, "null argument");
  Program g(c->batch);
  const int par = g.add_block(params, 0, 0, 0, 0, true);
  paos_pass& p = g.add_pass(-1, -1, -1);
  push(p.pre, p.n_pre, PAOS_PW_QPHASE_CENTRED, par, mul2pi ? PAOS_PWF_MUL2PI : 0);
  return run_passes(c, g.passes.data(), 1, g.blocks.data(), 1);
}

int paos_run_passes(paos_ctx* c, const paos_pass* passes, int n_passes, const double* blocks, int n_blocks) {
  if (c) (void)hipSetDevice(c->device);  // one process may drive several GPUs
  return run_passes(c, passes, n_passes, blocks, n_blocks);
}

int paos_run_passes_live(paos_ctx* c, const paos_pass* passes, int n_passes, const double* blocks, int n_blocks,
                         const double* live_rows) {
  if (c) (void)hipSetDevice(c->device);
  if (c && live_rows)
    for (int i = 0; i < c->batch; ++i)
      if (!(live_rows[2 * i] >= 0.0) || !(live_rows[2 * i + 1] <= (double)c->n) || !(live_rows[2 * i] <= live_rows[2 * i + 1]))
        return fail(c, PAOS_EINVAL, "live row range must satisfy 0 <= lo <= hi <= n");
  return run_passes(c, passes, n_passes, blocks, n_blocks, live_rows);
}

int paos_ptp(paos_ctx* c, const double* params) {
  if (c) (void)hipSetDevice(c->device);  // one process may drive several GPUs
  return fft_op(c, OP_PTP, params, 0);
}
int paos_stw(paos_ctx* c, const double* params, int inverse) {
  if (c) (void)hipSetDevice(c->device);  // one process may drive several GPUs
  return fft_op(c, OP_STW, params, inverse);
}
int paos_wts(paos_ctx* c, const double* params, int inverse) {
  if (c) (void)hipSetDevice(c->device);  // one process may drive several GPUs
  return fft_op(c, OP_WTS, params, inverse);
}

}  // extern "C"
