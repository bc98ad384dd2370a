// passes.hip -- pass programs: the record sets of the apertures that ride on the frugal passes, the staging of item records
// and phase tables, the launches, and the reference's primitives as programs (paos_ptp / stw / wts).  What a program
// launches -- which kernel runs each pass, which passes share a launch, the build it takes -- is planned in pass_program.h.
#include "frugal_launch.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "pass_program.h"
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
  if (!c->block_stats) {
    HIPCHK(c, hipMalloc(&c->block_stats, 3 * sizeof(unsigned long long)));
    HIPCHK(c, hipMemsetAsync(c->block_stats, 0, 3 * sizeof(unsigned long long), c->stream));
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

MaskRender mask_job(paos_ctx* c, int axis, const LoweredPass& lp, const double* ap, const double* dshared) {
  const int line0 = lp.mask_lo, line_end = lp.mask_hi > lp.mask_lo ? lp.mask_hi : c->n;
  return MaskRender{ap, dshared, lp.mask_set, axis, line0, line_end, lp.mask_shapes};
}

// What the planner (pass_program.h) reads of a context ...
PlanDims plan_dims(const paos_ctx* c) {
  return PlanDims{c->n, c->batch, c->br, c->precision, c->central_half ? 1 : 0, c->narrow_windows ? 1 : 0};
}
// ... and of the environment: read once per process, except the two that tests switch (host.h: env_is)
PlanSwitches plan_switches(const paos_ctx* c) {
  static const bool line_tables = !env_is("PAOS_LINE_TABLES", '0'), compact_grid = !env_is("PAOS_COMPACT_GRID", '0'),
                    env_prune = !env_is("PAOS_NO_PRUNE", '1'), batched_records = !env_is("PAOS_BATCHED_RECORDS", '0'),
                    psf_zero_reuse = !env_is("PAOS_PSF_ZERO_REUSE", '0');
  PlanSwitches sw;
  sw.line_tables = line_tables;
  sw.fuse_pairs = !env_is("PAOS_FUSE_PAIRS", '0');
  sw.compact_grid = compact_grid;
  sw.env_prune = env_prune;
  sw.stage_program = !env_is("PAOS_STAGE_PROGRAM", '0');
  sw.batched_records = batched_records;
  sw.psf_zero_reuse = psf_zero_reuse;
  sw.ctx_prune = c->prune;
  return sw;
}

// Stage the launches `groups`: point the slots of those that run on table slots (decide_tables) at tables of the context's
// store, copy the item records of all of them to
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
int stage_groups(paos_ctx* c, ArenaBatch& ab, std::vector<Launch>& groups, StagedTables* st) {
  std::vector<FrugalItem> blob;
  std::vector<PhaseSlotDesc> descs;
  int slots = 0;
  for (const Launch& g : groups)
    if (g.tables) slots += 2 * g.count;
  if (slots > c->ptab_slots) {
    if (c->ptab) { HIPCHK(c, hipStreamSynchronize(c->stream)); (void)hipFree(c->ptab); c->ptab = nullptr; c->ptab_slots = 0; }
    HIPCHK(c, hipMalloc(&c->ptab, (size_t)slots * c->batch * c->n * sizeof(cx<double>)));
    c->ptab_slots = slots;
  }
  int slot = 0;
  for (Launch& g : groups) {
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

// One launch of a program, as planned (pass_program.h: Launch).  staged: its item records in the array the program staged
// in front of its first launch, or nullptr.
int launch_lowered(paos_ctx* c, const Launch& g, const double* dblocks, const FrugalItem* staged) {
  for (int k = 0; k < g.count; ++k) {  // render the records along the pass axis, right before the pass (every pass of a chain)
    LoweredPass* l = g.lp[k];
    if (l->mask_block < 0 || !l->mask_render) continue;
    const double* ap = dblocks + (size_t)l->mask_block * c->batch * FP_STRIDE;
    const double* dshared = nullptr;
    int rcs = arena_push(c, l->mask_shared.data(), l->mask_shared.size(), &dshared);
    if (rcs) return rcs;
    const MaskRender job = mask_job(c, g.axis, *l, ap, dshared);  // (a chain runs along one axis)
    if ((rcs = render_mask_records(c, &job, 1))) return rcs;
    l->mask_render = false;
  }
  // The item records (with the pointers to their slots' phase tables) and the tables themselves: staged for the whole
  // program in front of its first launch (stage_groups: one copy, one table launch), or here for this launch alone.
  if (!staged) {
    std::vector<Launch> one{g};
    ArenaBatch ab(c);  // (inside the program's reservation: no begin)
    StagedTables st;
    int rcg = stage_groups(c, ab, one, &st);
    if (rcg || (rcg = ab.commit()) || (rcg = launch_staged_tables(c, st))) return rcg;
    staged = st.items + one[0].item_base;
  }
  FrugalArgs a{c->field, c->tw, staged, c->pitch, c->item_stride, nullptr, nullptr, nullptr};
  if (g.store == 1) { a.psf = c->psf; a.psf_partial = c->psf_partial; }
  if (g.store == 2) a.pow_partial = c->pow_partial;
  a.dyn_scale = c->dyn_scale;
  a.live_lo = g.live_lo; a.live_hi = g.live_hi; a.wg0 = 0;
  c->prof_next_tag = g.tag;
  c->prof_next_bytes = g.bytes;
  c->prof_next_lines = g.lines;
  const FrugalBuild& b = g.build;
  {  // paos_pass_builds: the record the family function gets, in launch order
    int rec[kBuildFields];
    build_to_ints(b, rec);
    c->pass_builds.insert(c->pass_builds.end(), rec, rec + kBuildFields);
  }
  // PAOS_DUMP_PASSES=1: on stderr, the build the launch takes and one line per pass it runs (what item 0's two slots carry)
  static const bool dump = env_is("PAOS_DUMP_PASSES", '1');
  if (dump) {
    std::fprintf(stderr, "build axis %d kpre %d kmid %d nfft %d store %d tab %d fuse %d one_line %d central %d n %d %s\n", b.axis, b.kpre, b.kmid,
                 b.nfft, b.store, b.tab, b.fuse, b.one_line, b.central, c->n, c->precision == PAOS_F64 ? "fp64" : "fp32");
    for (int k = 0; k < g.count; ++k) {
      const LoweredPass* l = g.lp[k];
      if (l->items.empty()) continue;
      const FrugalItem& f = l->items[0];  // ("+pass": rides in the launch of the pass above it)
      std::fprintf(stderr, "%spass axis %d kpre %d kmid %d nfft %d | pre: sign %g scale %g mask %g | fft1 on %g inv %g | mid: sign %g scale %g mask %g | "
                   "fft2 on %g inv %g | lines [%g, %g) fill %g loads [%g, %g) stores [%g, %g)\n", k == 0 ? "" : "+", g.axis, l->kpre, l->kmid, l->nfft,
                   f.pre.sign_on, f.pre.scale, f.pre.mask_on, f.fft1_on, f.fft1_inv, f.mid.sign_on, f.mid.scale, f.mid.mask_on, f.fft2_on, f.fft2_inv,
                   f.line_lo, f.line_hi, f.line_fill, f.pos_lo, f.pos_hi, f.spos_lo, f.spos_hi);
    }
  }
  // (a pass is lowered only in a context of one of the families: frugal_sizes)
  return dispatch_family(c->precision, c->n, (int)PAOS_EUNSUPPORTED,
                         [&](auto t, auto n) { return frugal_family<decltype(t), decltype(n)::value>(c, b, a, g.narrow != 0); });
}

int launch_one_pass(paos_ctx* c, const paos_pass& p, const double* dblocks, int n_blocks,
                    const int* table_of_op /* [3][PAOS_MAX_PW], -1 = none */) {
  int rc;
  for (int l = 0; l < 3; ++l)
    if ((rc = check_ops(c, op_list(p, l).ops, op_list(p, l).count, n_blocks))) return rc;
  if (p.fft1 >= n_blocks || p.fft2 >= n_blocks) return fail(c, PAOS_EINVAL, "transform control block out of range");
  int nmask = 0;  // at most one aperture operator per pass: its weight map is rendered right before it
  for (int l = 0; l < 3; ++l) {
    const OpList ol = op_list(p, l);
    for (int o = 0; o < ol.count; ++o)
      if (ol.ops[o].kind == PAOS_PW_MASK) {
        if (++nmask > 1) return fail(c, PAOS_EINVAL, "one aperture operator per pass");
        int rcm = render_mask_weights(c, dblocks + (size_t)ol.ops[o].block * c->batch * FP_STRIDE);
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
  int feat = 0;
  for (int l = 0; l < 3; ++l)
    for (int o = 0; o < PAOS_MAX_PW; ++o) {
      lists[l][o].flags &= (1 << kTableShift) - 1;
      const int t = table_of_op[l * PAOS_MAX_PW + o];
      if (t >= 0) { lists[l][o].flags |= (t + 1) << kTableShift; feat = 3; }
      if (o < op_list(p, l).count && lists[l][o].kind == PWK_MASK) feat = 3;
    }
  a.pitch = c->pitch; a.item_stride = c->item_stride;
  if (p.axis == 0 || p.axis == 1) return generic_pass(c, p.axis, a, feat);
  if (p.axis != -1) return fail(c, PAOS_EINVAL, "pass axis must be 0, 1 or -1");
  if (p.fft1 >= 0 || p.fft2 >= 0 || p.n_mid || p.n_post)
    return fail(c, PAOS_EINVAL, "a transform-free pass carries its operators in the pre list");
  return pointwise_pass(c, a);
}

// ---- a pass program, step by step (run_passes_impl): what the steps hand to each other -------------------------------
struct ProgramRun {
  paos_ctx* c;
  const paos_pass* passes;
  int n_passes;
  const double* blocks;  // host
  int n_blocks;
  PlanDims d;
  PlanSwitches sw;
  ArenaBatch ab;                    // THE copy of the program: the block table, the renderings' vectors, the staged records
  const double* dblocks = nullptr;  // the block table on the device
  std::vector<LoweredPass> low;
  bool all_frugal = false, pruned = false;
  int store = 0;         // what the last pass stores on the way out (pass_program.h: last_pass_store)
  int power_groups = 0;  // store = 2: the per-workgroup sums of an item
  std::vector<MaskRender> renderings;  // the record renderings that go in one batch, in front of the first pass
  std::vector<Launch> launches;
  std::vector<int> launch_of;
  StagedTables staged;   // items != nullptr: records and tables of the whole program were staged in front of its first launch
  ProgramRun(paos_ctx* c_, const paos_pass* passes_, int n_passes_, const double* blocks_, int n_blocks_)
      : c(c_), passes(passes_), n_passes(n_passes_), blocks(blocks_), n_blocks(n_blocks_), d(plan_dims(c_)), sw(plan_switches(c_)), ab(c_) {}
};

int validate_program(paos_ctx* c, const paos_pass* passes, int n_passes, const double* blocks, int n_blocks, const int* final_ticket) {
  if (c) c->pass_builds.clear();  // (paos_pass_builds: the launches of THIS program)
  if (!c || !passes || !blocks || n_passes < 0 || n_blocks < 1) return fail(c, PAOS_EINVAL, "bad pass program");
  c->norm2_of_field = false;  // (set again at the end when the last pass sums the power of what it stores)
  // A program that ends on the PSF gives the field up for it: the free power-ticket slot it will need is checked
  // BEFORE anything is launched (found full afterwards, the context held neither field nor ticket).
  if (int rcr = final_ticket ? power_ring_full(c) : PAOS_OK) return rcr;
  switch (check_phase_args(plan_dims(c), passes, n_passes, blocks, n_blocks)) {
    case PHASE_BLOCK_OUT_OF_RANGE: return fail(c, PAOS_EINVAL, "operator block index out of range");
    case PHASE_TOO_LARGE: return fail(c, PAOS_EUNSUPPORTED, "quadratic phase exceeds 1e12 rad at the grid corner (or is not finite)");
    default: return PAOS_OK;
  }
}

// Everything the program pushes stays live until its last pass has run: the block table and,
// per pass, one FrugalItem record per batch item (each push is rounded up to 16 doubles)
// plus, for a pass that carries an aperture, the [batch] "shares its line records" vector (launch_lowered)
// ... and two table descriptors (stage_groups)
// ... and the two windows of zero_outside_box.  Round 17: the block table, the vectors of the batched renderings and the
// staged records are ONE batch, copied once in front of the program's first launch that reads any of them; whatever is
// pushed launch by launch behind that (arena_push: a copy of its own) still lies inside this reservation.
int open_batch(ProgramRun& r) {
  paos_ctx* c = r.c;
  const size_t per_pass = (((size_t)c->batch * sizeof(FrugalItem) / sizeof(double) + 15) & ~size_t(15)) +
                          (((size_t)c->batch + 15) & ~size_t(15)) + 16;
  int rc = r.ab.begin((size_t)r.n_blocks * c->batch * FP_STRIDE + 16 + (size_t)r.n_passes * per_pass + 2 * arena_rounded((size_t)2 * c->batch));
  if (rc) return rc;
  return r.ab.add(r.blocks, (size_t)r.n_blocks * c->batch * FP_STRIDE, &r.dblocks);
}

// Lower every pass for the frugal kernels first, so that the planner can look ahead across the program, and give every
// pass that carries an aperture a record set of the context's store, in program order.
int lower_and_assign_sets(ProgramRun& r) {
  paos_ctx* c = r.c;
  r.low.resize(r.n_passes);
  r.all_frugal = !use_tables() && frugal_sizes(c) && r.n_passes > 0;
  if (use_tables() || !frugal_sizes(c)) return PAOS_OK;
  int rc = ensure_mask_store(c);
  if (rc) return rc;
  for (int q = 0; q < r.n_passes; ++q) {
    LoweredPass& lp = r.low[q];
    lp.ok = lower_frugal(r.d, r.passes[q], r.blocks, lp);
    if (lp.ok && lp.mask_block >= 0 && (rc = assign_mask_set(c, r.passes[q], lp, r.blocks))) return rc;
    r.all_frugal = r.all_frugal && lp.ok;
  }
  return PAOS_OK;
}

// A stop's scaling is waiting: the first pass takes it along in its middle slot when it is a frugal pass every item
// takes part in; otherwise the field gets it now.
int settle_stop(ProgramRun& r) {
  paos_ctx* c = r.c;
  if (!c->dyn_pending) return PAOS_OK;
  bool ride = r.n_passes > 0 && r.low[0].ok;
  if (ride)
    for (const FrugalItem& fi : r.low[0].items) ride = ride && fi.active != 0.0;
  if (ride) ++c->deferred_rode;
  return ride ? PAOS_OK : settle_scale(c);
}

// When the whole program runs on the frugal kernels, plan the pruning of dead lines across it (look-ahead); then the lines
// whose aperture records each pass reads (record_window): a set found in the context's store is good only if it was rendered
// that far.
void plan_lines(ProgramRun& r, const double* entry_rows, bool entry_stale, const double* entry_cols) {
  paos_ctx* c = r.c;
  r.pruned = r.all_frugal && r.sw.env_prune && r.sw.ctx_prune;
  if (r.pruned) plan_pruning(r.d, r.passes, r.n_passes, r.blocks, r.low, entry_rows, entry_stale, entry_cols);
  for (LoweredPass& lp : r.low) {
    if (!lp.ok || lp.mask_block < 0) continue;
    record_window(r.d, lp);
    paos_ctx::MaskSet& ms = c->mask_sets[lp.mask_set];
    if (!lp.mask_render && !(ms.line_lo <= lp.mask_lo && ms.line_hi >= lp.mask_hi)) {
      lp.mask_render = true;  // found, but rendered for a narrower window than this pass reads
      --c->mask_hits; ++c->mask_rendered;
    }
    if (lp.mask_render) { ms.line_lo = lp.mask_lo; ms.line_hi = lp.mask_hi; }
  }
}

// What the store mode of the last pass needs on the device: the buffers of its sums, zeroed where dead tiles and workgroups
// that are not launched contribute nothing, and the PSF buffer itself -- and, for a PSF store, which zeros it still owes.
int prepare_store(ProgramRun& r, int final_mode) {
  paos_ctx* c = r.c;
  r.store = last_pass_store(r.low, final_mode);
  if (final_mode == 2 && r.store == 2) {
    r.power_groups = c->n / frugal_tile_lines(c, r.passes[r.n_passes - 1].axis);
    if (c->pow_nparts < c->n / 2) {  // (sized for the finest tiling of either axis)
      if (c->pow_partial) (void)hipFree(c->pow_partial);
      c->pow_partial = nullptr; c->pow_nparts = 0;
      HIPCHK(c, hipMalloc(&c->pow_partial, (size_t)c->batch * (c->n / 2) * sizeof(double)));
      c->pow_nparts = c->n / 2;
    }
    // dead tiles and workgroups that are not launched at all contribute nothing: zeros
    HIPCHK(c, hipMemsetAsync(c->pow_partial, 0, (size_t)c->batch * r.power_groups * sizeof(double), c->stream));
  }
  if (final_mode != 1) return PAOS_OK;
  if (!c->psf) HIPCHK(c, hipMalloc(&c->psf, (size_t)c->batch * c->item_stride * sizeof(double)));
  c->otf_valid = c->ee_valid = false;  // a new PSF: the transfer functions and energy curves computed from the previous one are stale
  if (r.store != 1) return PAOS_OK;
  const int axis = r.passes[r.n_passes - 1].axis, groups = c->n / frugal_tile_lines(c, axis);
  if (c->psf_nparts < groups) {
    if (c->psf_partial) (void)hipFree(c->psf_partial);
    c->psf_partial = nullptr; c->psf_nparts = 0;
    c->psf_zero_axis = -1;
    HIPCHK(c, hipMalloc(&c->psf_partial, (size_t)c->batch * groups * sizeof(double)));
    c->psf_nparts = groups;
  }
  psf_zero_fill(r.d, r.sw, axis, r.low[r.n_passes - 1].items, c->psf_zero_axis, c->psf_zero_lo, c->psf_zero_hi);
  c->psf_zero_axis = -1;  // set again once the pass is on the stream (hand_out_ticket)
  return PAOS_OK;
}

// The record renderings that go in ONE launch per shape (batched_renderings): their vectors join the program's batch, the
// launches follow its commit.  Every other rendering happens in place, right before its pass (launch_lowered).
int batch_renderings(ProgramRun& r) {
  for (int q : batched_renderings(r.sw, r.all_frugal, r.low)) {
    LoweredPass& lp = r.low[q];
    const double* dshared = nullptr;
    int rc = r.ab.add(lp.mask_shared.data(), lp.mask_shared.size(), &dshared);
    if (rc) return rc;
    r.renderings.push_back(mask_job(r.c, r.passes[q].axis, lp, r.dblocks + (size_t)lp.mask_block * r.c->batch * FP_STRIDE, dshared));
    lp.mask_render = false;
  }
  return PAOS_OK;
}

// The launches of the program, each with its tables flag, its build, its grid window and its timer figures; when every
// pass runs on the frugal kernels their item records and phase tables are staged here, once, for all of them
// (stage_groups); otherwise each launch stages its own.
int plan_and_stage_launches(ProgramRun& r) {
  r.launches = form_launches(r.d, r.sw, r.passes, r.n_passes, r.low, r.all_frugal && r.pruned, r.launch_of);
  for (Launch& g : r.launches) {
    if (!g.lp[0]->ok) continue;  // (a pass on the generic kernel: launch_one_pass)
    decide_tables(r.d, r.sw, g);
    finish_launch(r.d, r.sw, g, g.q + g.count == r.n_passes ? r.store : 0);
  }
  if (!stage_whole_program(r.d, r.sw, r.all_frugal, r.n_passes)) return PAOS_OK;
  return stage_groups(r.c, r.ab, r.launches, &r.staged);
}

// Walk the program in chunks whose phase operators fit the table store of the generic kernel (PAOS_PHASE_TABLES=1; without
// it the whole program is one chunk): fill the tables of a chunk with one small launch, then run its passes.
int launch_chunks(ProgramRun& r) {
  paos_ctx* c = r.c;
  int rc;
  int i = 0;
  while (i < r.n_passes) {
    TableArgs ta{};
    ta.blocks = r.dblocks; ta.tables = c->tables; ta.batch = c->batch; ta.n = c->n; ta.count = 0;
    std::vector<int> assign;  // per pass of the chunk: [3][PAOS_MAX_PW]
    int j = i;
    for (; j < r.n_passes; ++j) {
      const paos_pass& p = r.passes[j];
      int need = 0;
      for (int l = 0; l < 3; ++l)
        for (int o = 0; o < op_list(p, l).count && o < PAOS_MAX_PW; ++o) need += is_phase(op_list(p, l).ops[o]);
      if (use_tables() && ta.count + need > kMaxTables) {
        if (j == i) return fail(c, PAOS_EINVAL, "one pass needs more phase tables than the store holds");
        break;
      }
      const size_t base = assign.size();
      assign.resize(base + 3 * PAOS_MAX_PW, -1);
      if (!use_tables()) continue;
      for (int l = 0; l < 3; ++l)
        for (int o = 0; o < op_list(p, l).count && o < PAOS_MAX_PW; ++o) {
          const paos_pw_op& op = op_list(p, l).ops[o];
          if (!is_phase(op)) continue;
          if (op.block < 0 || op.block >= r.n_blocks) return fail(c, PAOS_EINVAL, "operator block index out of range");
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
      if (!r.low[q].ok) {
        if ((rc = launch_one_pass(c, r.passes[q], r.dblocks, r.n_blocks, &assign[(size_t)(q - i) * 3 * PAOS_MAX_PW]))) return rc;
        continue;
      }
      // (a group of up to three passes of one row / column chain runs in ONE launch: frugal_pass.h, LONG builds)
      const Launch& g = r.launches[r.launch_of[q]];
      const int last = q + g.count - 1;
      if (last >= j) return fail(c, PAOS_EINVAL, "a fused group crosses a table chunk");
      if ((rc = launch_lowered(c, g, r.dblocks, r.staged.items ? r.staged.items + g.item_base : nullptr))) return rc;
      q = last;
      if (c->dyn_pending) {  // (first launch of the program) the stop's factor has gone into the field: ones again for the next
        if ((rc = dyn_scale_reset(c))) return rc;
      }
    }
    i = j;
  }
  return PAOS_OK;
}

// The ticket of the power the caller asked for: of the sums the last pass left, or -- the fallback: a generic-kernel pass, or
// an item that sat the last pass out -- of the reduction or the intensity sweep that follows the program.
int hand_out_ticket(ProgramRun& r, int final_mode, int* final_ticket) {
  paos_ctx* c = r.c;
  if (final_mode == 2) {
    const int rcp = r.store == 2 ? take_power_ticket(c, c->pow_partial, r.power_groups, nullptr, final_ticket) : paos_norm2_enqueue(c, final_ticket);
    if (rcp == PAOS_OK) c->norm2_of_field = true;  // c->norm2 = the power of every item's field as stored
    return rcp;
  }
  if (r.store != 1) return psf_keep_power_impl(c, final_ticket);
  c->psf_zero_axis = r.passes[r.n_passes - 1].axis;  // every launch of the program went through
  return take_power_ticket(c, c->psf_partial, c->n / frugal_tile_lines(c, r.passes[r.n_passes - 1].axis), nullptr, final_ticket);
}

// entry_rows / entry_stale: see paos_program_opts.  final_ticket != nullptr: the caller wants |u|^2 and its sum of
// the field the program ends with, not the field (final_mode 1), or the field and the sum (2).
int run_passes_impl(paos_ctx* c, const paos_pass* passes, int n_passes, const double* blocks, int n_blocks,
                    const double* entry_rows, bool entry_stale, int* final_ticket, int final_mode, const double* entry_cols) {
  int rc = validate_program(c, passes, n_passes, blocks, n_blocks, final_ticket);
  if (rc) return rc;
  final_mode = final_ticket ? (final_mode == 2 ? 2 : 1) : 0;
  ProgramRun r(c, passes, n_passes, blocks, n_blocks);
  if ((rc = open_batch(r)) || (rc = lower_and_assign_sets(r)) || (rc = settle_stop(r))) return rc;
  plan_lines(r, entry_rows, entry_stale, entry_cols);
  if (entry_stale && entry_rows && entry_zero_first(r.d, r.pruned, r.low, entry_rows, entry_cols)) {
    // (all items at once: the ones the planner handles lose nothing but a little time, and the planner was told
    // "stale", which is also right for zeros)
    if ((rc = entry_cols ? zero_outside_box(c, entry_rows, entry_cols) : zero_outside_rows(c, entry_rows))) return rc;
  }
  if ((rc = prepare_store(r, final_mode)) || (rc = batch_renderings(r)) || (rc = plan_and_stage_launches(r))) return rc;
  // THE copy of the program, in front of its first launch that reads a block: the record renderings, the table kernel, or
  // the first pass.  (What ran above -- a settled stop scale, zeroed windows -- reads none of this batch.)
  if ((rc = r.ab.commit())) return rc;
  for (size_t at = 0; at < r.renderings.size(); at += kMaskRenders)
    if ((rc = render_mask_records(c, r.renderings.data() + at, (int)std::min<size_t>(kMaskRenders, r.renderings.size() - at)))) return rc;
  if ((rc = launch_staged_tables(c, r.staged)) || (rc = launch_chunks(r))) return rc;
  return final_mode ? hand_out_ticket(r, final_mode, final_ticket) : PAOS_OK;
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
// where they fit (2); PAOS_MASK_BLOCKS=0: four lines per wave through 8-pixel windows where they fit (3); default: blocks of
// 64 lines per wave, the exact overlap on the undecided window pixels only (4, round 24: mask_blocks_kernel).
int mask_render_mode() {
  if (env_is("PAOS_MASK_SCAN", '1')) return 0;
  if (env_is("PAOS_MASK_PAIRS", '0')) return 1;
  if (env_is("PAOS_MASK_PAIRS", '1')) return 2;
  return env_is("PAOS_MASK_BLOCKS", '0') ? 3 : 4;  // 4 (round 24): blocks of 64 lines per wave in front of the cascade
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
  const FrugalBuild b = build_from_ints(record);
  return dispatch_family(precision, n, -(int)PAOS_EINVAL, [&](auto t, auto size) { return frugal_built<decltype(t), decltype(size)::value>(b) ? 1 : 0; });
}

int paos_pass_builds(paos_ctx* c, int* records, int capacity, int* count) {
  if (!c || !count || capacity < 0 || (capacity > 0 && !records)) return fail(c, PAOS_EINVAL, "bad pass-builds request");
  const int have = (int)(c->pass_builds.size() / kBuildFields);
  *count = have;
  if (have > 0 && capacity > 0) std::memcpy(records, c->pass_builds.data(), (size_t)(have < capacity ? have : capacity) * kBuildFields * sizeof(int));
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
