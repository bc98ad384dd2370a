// paos_hip.hip -- the pointwise entry points of the C ABI (include/paos_hip.h): every launch of a kernel of pointwise.h: the start field, apertures and stops, power sums and their
// tickets, PSF keep / fetch / metrics, import / export, phase maps, PSD screens, Zernike surfaces, pupils, Gram sums, and
// what the pass programs need of them (aperture line records and weight maps, the deferred stop scale).  The header's
// non-template kernels can be compiled once only, so this is the one unit that includes it.
#include "host.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "item_groups.h"
#include "pointwise.h"

namespace {

int pw_blocks(const paos_ctx* c) {
  const size_t total = (size_t)c->item_stride;
  size_t b = (total + kPwThreads - 1) / kPwThreads;
  return (int)(b < 2048 ? b : 2048);
}

// ---- a stop whose scaling is left to the next pass (paos_stop_defer_last_power) ---------------------------------------
__global__ void dyn_scale_set_kernel(double* dyn, const double* norm2, const double* enable, int batch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < batch) dyn[i] = (!enable || enable[i] != 0.0) ? 1.0 / sqrt(norm2[i]) : 1.0;  // stop_scale_kernel's own expression
}
__global__ void dyn_scale_reset_kernel(double* dyn, int batch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < batch) dyn[i] = 1.0;
}
template <typename T>
__global__ void scale_by_kernel(cx<T>* field, const double* dyn, unsigned item_stride) {
  const int item = blockIdx.y;
  const double s = dyn[item];
  if (s == 1.0) return;
  cx<T>* f = field + (size_t)item * item_stride;
  for (size_t m = (size_t)blockIdx.x * blockDim.x + threadIdx.x; m < item_stride; m += (size_t)gridDim.x * blockDim.x)
    f[m] = {(T)__dmul_rn((double)f[m].x, s), (T)__dmul_rn((double)f[m].y, s)};
}

}  // namespace

int dyn_scale_reset(paos_ctx* c) {
  hipLaunchKernelGGL(dyn_scale_reset_kernel, dim3((c->batch + 255) / 256), dim3(256), 0, c->stream, c->dyn_scale, c->batch);
  HIPCHK(c, hipGetLastError());
  c->dyn_pending = false;
  return PAOS_OK;
}

// Whatever is about to read or rewrite the field other than a pass program that can take the factor along: the stop's
// scaling is applied now, by the sweep make_stop would have run (same factor, same products: bit-identical).
int settle_scale(paos_ctx* c, bool field_is_overwritten) {
  if (!c->dyn_pending) return PAOS_OK;
  ++c->deferred_settled;
  if (!field_is_overwritten) {
    const dim3 grid(pw_blocks(c), c->batch), block(kPwThreads);
    dispatch_layout(c, [&](auto t, auto) {
      using T = decltype(t);
      hipLaunchKernelGGL(scale_by_kernel<T>, grid, block, 0, c->stream, (cx<T>*)c->field, c->dyn_scale, c->item_stride);
    });
  }
  return dyn_scale_reset(c);
}

// one launch per shape that occurs for `count` renderings (blockIdx.z), the grid sized for the widest line window
static_assert(kMaskRenders == kMaskJobs, "a call's renderings go out in one launch per shape");
int render_mask_records(paos_ctx* c, const MaskRender* renders, int count) {
  MaskJobs jobs{};
  for (int j = 0; j < count; ++j) {
    const MaskRender& r = renders[j];
    const paos_ctx::MaskSet& ms = c->mask_sets[r.set];
    jobs.job[j] = MaskJob{r.params, r.shared, ms.lines, ms.vals, r.axis, r.line0, r.line_end, r.shapes};
  }
  jobs.batch_stride = c->batch * (int)FP_STRIDE; jobs.param_stride = (int)FP_STRIDE; jobs.n = c->n; jobs.overflow = c->mask_overflow;
  const int mode = mask_render_mode();
  jobs.windows = mode != 0 ? 1 : 0;
  jobs.pairs = mode >= 2 ? std::min(mode, 3) - 1 : 0;  // (mode 4, blocks of lines: the lines it hands over go two per wave first)
  jobs.rect_blocks = mask_rect_blocks() ? 1 : 0;
  int widest = 0, shapes = 0;
  for (int j = 0; j < count; ++j) {
    widest = std::max(widest, jobs.job[j].line_end - jobs.job[j].line0);
    shapes |= jobs.job[j].shapes;
  }
  const dim3 block(256);
  // (ellipses: a wave renders four / two lines, the grid covers a quarter / half as many waves)
  const int per_wg = 4 * (jobs.pairs >= 2 ? 4 : (jobs.pairs ? 2 : 1));
  constexpr int block_per_wg = kMaskBlockLines * kMaskWaves;  // (round 24) ... or a block of 64
  if ((shapes & 1) && mode == 4)
    hipLaunchKernelGGL(mask_blocks_kernel, dim3((widest + block_per_wg - 1) / block_per_wg, c->batch, count), block, 0, c->stream, jobs, c->block_stats);
  else if (shapes & 1)
    hipLaunchKernelGGL(mask_lines_kernel<0>, dim3((widest + per_wg - 1) / per_wg, c->batch, count), block, 0, c->stream, jobs);
  const int rect_per_wg = 4 * (jobs.rect_blocks ? 64 : 1);
  if (shapes & 2) hipLaunchKernelGGL(mask_lines_kernel<1>, dim3((widest + rect_per_wg - 1) / rect_per_wg, c->batch, count), block, 0, c->stream, jobs);
  HIPCHK(c, hipGetLastError());
  return PAOS_OK;
}

// The weight map of the aperture whose two parameter block sets start at `ap`, for EVERY item, into c->mask: what a
// PWK_MASK operator of a pass on the generic kernels multiplies by (rendered right before the pass).
int render_mask_weights(paos_ctx* c, const double* ap) {
  if (!c->mask) HIPCHK(c, hipMalloc(&c->mask, (size_t)c->batch * c->item_stride * sizeof(double)));
  const dim3 grid(pw_blocks(c), c->batch), block(kPwThreads);
  const double* ap2 = ap + (size_t)c->batch * FP_STRIDE;  // the next block set
  dispatch_layout(c, [&](auto t, auto br) {  // both shapes: each takes the items that have it
    using T = decltype(t);
    constexpr int BRV = decltype(br)::value;
    hipLaunchKernelGGL((aperture_kernel<T, BRV, Lay<T>::BC, 0>), grid, block, 0, c->stream, (cx<T>*)nullptr, ap, ap2, FP_STRIDE, c->n, c->pitch, c->item_stride, c->mask, 1);
    hipLaunchKernelGGL((aperture_kernel<T, BRV, Lay<T>::BC, 1>), grid, block, 0, c->stream, (cx<T>*)nullptr, ap, ap2, FP_STRIDE, c->n, c->pitch, c->item_stride, c->mask, 1);
  });
  HIPCHK(c, hipGetLastError());
  return PAOS_OK;
}

// a transform-free pass: its operators, pixel by pixel
int pointwise_pass(paos_ctx* c, const PassArgs& a) {
  const dim3 grid(pw_blocks(c), c->batch), block(kPwThreads);
  dispatch_layout(c, [&](auto t, auto br) {
    hipLaunchKernelGGL((pointwise_kernel<decltype(t), decltype(br)::value, Lay<decltype(t)>::BC>), grid, block, 0, c->stream, a, c->n);
  });
  HIPCHK(c, hipGetLastError());
  return PAOS_OK;
}

namespace {

// The phase-map kernels form fl(fl(2 pi w) / wl): a finite map value can overflow there (|w| near 1e308, or any w over a
// tiny wavelength), and sincos(inf) would write NaN into the field.  |.| and both roundings are monotone, so the map's
// largest |w| decides for the whole map.
const char* const kPhaseMapOverflow = "the phase argument 2 pi w / wl of the map's largest value is not finite";
bool phase_map_argument_finite(double wmax, double wl) { return std::isfinite((6.283185307179586 * wmax) / wl); }

// groups of items with one wfe map share its evaluation (start_impl, zernike_apply); PAOS_SHARE_WFE=0: never
bool share_wfe_maps() {
  static const bool on = !env_is("PAOS_SHARE_WFE", '0');
  return on;
}

// stage 1 of a power reduction: per-workgroup sums of |u|^2 of the field (inside the windows, of the enabled items) into c->partial
void norm2_partial_launch(paos_ctx* c, const double* enable, const double* rows = nullptr, const double* cols = nullptr) {
  dispatch_layout(c, [&](auto t, auto br) {
    using T = decltype(t);
    hipLaunchKernelGGL((norm2_partial_kernel<T, decltype(br)::value, Lay<T>::BC>), dim3(c->nparts, c->batch), dim3(kPwThreads), 0, c->stream,
                       (const cx<T>*)c->field, c->partial, c->n, c->pitch, c->item_stride, enable, 1, rows, cols);
  });
}

// field *= 1 / sqrt(c->norm2) for the enabled items
void stop_scale_launch(paos_ctx* c, const double* enable) {
  dispatch_layout(c, [&](auto t, auto) {
    using T = decltype(t);
    hipLaunchKernelGGL(stop_scale_kernel<T>, dim3(pw_blocks(c), c->batch), dim3(kPwThreads), 0, c->stream, (cx<T>*)c->field, c->norm2,
                       c->item_stride, enable, 1);
  });
}

}  // namespace

// ---- the ring of power tickets ----------------------------------------------------------------------------------------
// refuses while the slot the next ticket would take is still out (for the entry points that must refuse before they launch)
int power_ring_full(paos_ctx* c) {
  if (c->norm_busy[next_norm_slot(c)])  // the oldest ticket has not been fetched
    return fail(c, PAOS_EINVAL, "64 power reductions outstanding: fetch earlier tickets (paos_norm2_fetch) first");
  return PAOS_OK;
}

// partial sums -> c->norm2 (item i: the sums of item source[i], if given) -> the pinned slot of a new ticket
int take_power_ticket(paos_ctx* c, const double* partial, int nparts, const double* source, int* ticket) {
  if (int rc = power_ring_full(c)) return rc;
  const int slot = next_norm_slot(c);
  hipLaunchKernelGGL(norm2_final_kernel, dim3(c->batch), dim3(kPwThreads), 0, c->stream, partial, c->norm2, nparts, (const double*)nullptr, 1, source);
  HIPCHK(c, hipGetLastError());
  c->norm_busy[slot] = true;
  c->norm_slot = (slot + 1) % kNormSlots;
  HIPCHK(c, hipMemcpyAsync(c->norm2_host + (size_t)slot * c->batch, c->norm2, (size_t)c->batch * sizeof(double),
                           hipMemcpyDeviceToHost, c->stream));
  *ticket = slot;
  return PAOS_OK;
}

extern "C" {

int paos_fill(paos_ctx* c, double re, double im) {
  DROP_SCALE(c);
  if (c) (void)hipSetDevice(c->device);  // one process may drive several GPUs
  if (!c) return fail(c, PAOS_EINVAL, "null context");
  const size_t total = (size_t)c->item_stride * c->batch;
  // padding blocks are filled too; they are never read by any operator
  dispatch_layout(c, [&](auto t, auto) {
    using T = decltype(t);
    hipLaunchKernelGGL(fill_kernel<T>, dim3(2048), dim3(kPwThreads), 0, c->stream, (cx<T>*)c->field, total, (T)re, (T)im);
  });
  HIPCHK(c, hipGetLastError());
  return PAOS_OK;
}

// The Zernike surface right behind the start, applied while the start field is written (paos_start_zernike_box)
struct StartZernike {
  int nmax, kdim, param_stride;
  const double *table, *params;
  int* power_ticket;  // optional: the power of the start field itself, as paos_norm2_enqueue_box would sum it
};
static int zernike_check(paos_ctx* c, int nmax, int kdim, const double* table, const double* params, int param_stride);

// What a start keeps from call to call (paos_ctx::start_key, start_partial_key).  PAOS_START_POWER_MEMO=0: nothing.
static bool start_memo_on() {
  static const bool memo = !env_is("PAOS_START_POWER_MEMO", '0');
  return memo;
}
static bool same_key(const std::vector<double>& a, const std::vector<double>& b) {
  return a.size() == b.size() && !std::memcmp(a.data(), b.data(), a.size() * sizeof(double));
}
static void start_forget(paos_ctx* c) {
  c->start_key.clear();
  c->start_partial_key.clear();
}

// check, group, upload (one copy), find or evaluate the power sums, launch, keep the sums
static int start_body(paos_ctx* c, double re, double im, int shape, const double* aperture, const double* stop,
                      const double* write_rows, const double* write_cols, const StartZernike* zk) {
  if (c) (void)hipSetDevice(c->device);
  if (!c || !aperture) return fail(c, PAOS_EINVAL, "null argument");
  if (shape != PAOS_SHAPE_ELLIPSE && shape != PAOS_SHAPE_RECT) return fail(c, PAOS_EINVAL, "unknown aperture shape");
  int rc;
  if (zk) {
    if ((rc = zernike_check(c, zk->nmax, zk->kdim, zk->table, zk->params, zk->param_stride))) return rc;
    if (zk->power_ticket && (rc = power_ring_full(c))) return rc;
  }
  const int batch = c->batch;
  std::vector<double> flags(batch, 0.0);
  bool any_stop = false;
  if (stop)
    for (int i = 0; i < batch; ++i) { flags[i] = stop[i] != 0.0 ? 1.0 : 0.0; any_stop |= flags[i] != 0.0; }
  // items with identical aperture records (a wavelength sweep at the entrance pupil, a Monte-Carlo batch)
  // have identical power sums: stage 1 runs for the first of them, stage 2 sums ITS partials for all
  std::vector<double> power_of, compute;
  power_representatives(batch, aperture, AP_STRIDE, flags.data(), power_of, compute);
  if (write_rows && (rc = check_rows(c, write_rows))) return rc;
  std::vector<double> wc;
  if (write_cols) {
    if (!write_rows) return fail(c, PAOS_EINVAL, "a column window needs a row window");
    if ((rc = check_rows(c, write_cols))) return rc;
    wc = rounded_cols(c, write_cols);
  }
  // groups of items that start from the same field (start_write_kernel): PAOS_SHARE_START=0: never
  static const bool share_start = !env_is("PAOS_SHARE_START", '0');
  ItemGroups groups = group_items(
      batch,
      [&](int j, int i) {
        return share_start && flags[j] == flags[i] && same_record(aperture + (size_t)j * AP_STRIDE, aperture + (size_t)i * AP_STRIDE, AP_STRIDE) &&
               (!write_rows || same_record(write_rows + 2 * j, write_rows + 2 * i, 2)) &&
               (!write_cols || same_record(write_cols + 2 * j, write_cols + 2 * i, 2));
      },
      [](int) { return true; });
  // ... and, with a Zernike surface riding on the write, inside each of them the groups of items with one wfe map: records equal
  // in everything but the wavelength (zernike_apply's rule, PAOS_SHARE_WFE); items without a Zernike record form one more
  std::vector<double> lead, same, subs;
  const bool want_power = zk && zk->power_ticket;  // one sum per group of identical start fields (paos_norm2_enqueue_box: same_as)
  if (zk) {
    group_leaders(groups, lead, same);  // (of the groups of identical start fields, before they are split)
    subs = split_by_map(groups, zk->params, zk->param_stride, ZP_ENABLE, ZP_INV_WL, share_wfe_maps());
  }
  // every block of the call in one slab, one copy in front of the first launch
  const size_t zt_count = zk ? (size_t)(zk->nmax + 1) * zk->kdim * 3 : 0, zp_count = zk ? (size_t)batch * zk->param_stride : 0;
  size_t total = arena_rounded((size_t)batch * AP_STRIDE) + 3 * arena_rounded(batch) + arena_rounded(groups.goff.size()) +
                 arena_rounded(groups.glen.size()) + arena_rounded(groups.members.size());
  if (write_rows) total += arena_rounded((size_t)2 * batch);
  if (write_cols) total += arena_rounded(wc.size());
  if (zk) total += arena_rounded(zt_count) + arena_rounded(zp_count) + arena_rounded(subs.size());
  if (want_power) total += 2 * arena_rounded(batch);
  ArenaBatch ab(c);
  if ((rc = ab.begin(total))) return rc;
  const double *dp = nullptr, *ds = nullptr, *dcompute = nullptr, *dpower_of = nullptr, *drows = nullptr, *dcols = nullptr;
  if ((rc = ab.add(aperture, (size_t)batch * AP_STRIDE, &dp))) return rc;
  if ((rc = ab.add(flags.data(), flags.size(), &ds))) return rc;
  if ((rc = ab.add(compute.data(), compute.size(), &dcompute))) return rc;
  if ((rc = ab.add(power_of.data(), power_of.size(), &dpower_of))) return rc;
  if (write_rows && (rc = ab.add(write_rows, (size_t)2 * batch, &drows))) return rc;
  if (write_cols && (rc = ab.add(wc.data(), wc.size(), &dcols))) return rc;
  const double *dzt = nullptr, *dzp = nullptr, *dsubs = nullptr, *dlead = nullptr, *dsame = nullptr;
  if (zk) {
    if ((rc = ab.add(zk->table, zt_count, &dzt))) return rc;
    if ((rc = ab.add(zk->params, zp_count, &dzp))) return rc;
    if ((rc = ab.add(subs.data(), subs.size(), &dsubs))) return rc;
    if (want_power) {
      if ((rc = ab.add(lead.data(), lead.size(), &dlead))) return rc;
      if ((rc = ab.add(same.data(), same.size(), &dsame))) return rc;
    }
  }
  const double *dgoff = nullptr, *dglen = nullptr, *dmembers = nullptr;
  if ((rc = ab.add(groups.goff.data(), groups.goff.size(), &dgoff))) return rc;
  if ((rc = ab.add(groups.glen.data(), groups.glen.size(), &dglen))) return rc;
  if ((rc = ab.add(groups.members.data(), groups.members.size(), &dmembers))) return rc;
  if ((rc = ab.commit())) return rc;
  // The power sums of a start with stops, into c->norm2: those of the last start if that had the same shape, constant,
  // aperture records and stop flags (paos_ctx::start_key), else the launch evaluates them and they are kept.  The key is
  // set BEHIND the launches that fill the sums: a start that fails in between leaves no key at all (start_impl).
  const bool memo = start_memo_on();
  std::vector<double> key, pkey;
  if (memo && (any_stop || want_power)) {
    key.reserve(3 + (size_t)batch * (AP_STRIDE + 1));
    key.push_back((double)shape); key.push_back(re); key.push_back(im);
    key.insert(key.end(), aperture, aperture + (size_t)batch * AP_STRIDE);
    key.insert(key.end(), flags.begin(), flags.end());
  }
  bool power_found = false;
  if (any_stop) {
    power_found = memo && c->start_norm2 && same_key(key, c->start_key);
    if (power_found) HIPCHK(c, hipMemcpyAsync(c->norm2, c->start_norm2, (size_t)batch * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    else c->start_key.clear();
  }
  // ... and the per-workgroup sums of the power of the start field inside its box: those of the last start with the same
  // key, row windows, rounded column windows and sharing (paos_ctx::start_partial), else the launch evaluates them THERE
  bool partial_found = false;
  double* partial = c->partial;
  if (want_power && memo) {
    pkey = key;
    pkey.insert(pkey.end(), write_rows, write_rows + (size_t)2 * batch);
    pkey.insert(pkey.end(), wc.begin(), wc.end());
    pkey.insert(pkey.end(), lead.begin(), lead.end());
    pkey.insert(pkey.end(), same.begin(), same.end());
    partial_found = c->start_partial && same_key(pkey, c->start_partial_key);
    if (!partial_found) c->start_partial_key.clear();
    if (!c->start_partial) HIPCHK(c, hipMalloc(&c->start_partial, (size_t)batch * c->nparts * sizeof(double)));
    partial = c->start_partial;
  }
  const dim3 block(kPwThreads), sweep(pw_blocks(c), batch), parts(c->nparts, batch);
  dispatch_layout(c, [&](auto t, auto br) {
    using T = decltype(t);
    constexpr int BRV = decltype(br)::value, BC = Lay<T>::BC;
    dispatch_either<0, 1>(shape == PAOS_SHAPE_ELLIPSE, [&](auto s) {
      constexpr int S = decltype(s)::value;
      if (any_stop && !power_found) {
        hipLaunchKernelGGL((start_power_kernel<T, BRV, BC, S>), parts, block, 0, c->stream, dp, c->n, c->pitch, c->item_stride, re, im,
                           c->partial, dcompute);
        hipLaunchKernelGGL(norm2_final_kernel, dim3(batch), block, 0, c->stream, c->partial, c->norm2, c->nparts, ds, 1, dpower_of);
      }
      if (!zk) {
        hipLaunchKernelGGL((start_write_kernel<T, BRV, BC, S>), sweep, block, 0, c->stream, (cx<T>*)c->field, dp, c->n, c->pitch,
                           c->item_stride, re, im, (const double*)c->norm2, ds, drows, dgoff, dglen, dmembers, dcols);
        return;
      }
      // (orders up to 8 run on the unrolled build, like zernike_kernel) ... and the power of the start field from the
      // weights, before the reduction behind it rewrites c->norm2
      dispatch_either<8, 0>(zk->nmax <= 8, [&](auto nc) {
        hipLaunchKernelGGL((zernike_start_write_kernel<T, BRV, BC, S, decltype(nc)::value>), sweep, block, 0, c->stream, (cx<T>*)c->field,
                           dp, c->n, c->pitch, c->item_stride, re, im, (const double*)c->norm2, ds, drows, dcols, dgoff, dglen, dsubs,
                           dmembers, dzt, dzp, zk->param_stride, zk->nmax, zk->kdim);
      });
      if (want_power && !partial_found)
        hipLaunchKernelGGL((start_norm2_partial_kernel<T, BRV, BC, S>), parts, block, 0, c->stream, partial, dp, c->n, c->pitch,
                           c->item_stride, re, im, (const double*)c->norm2, ds, dlead, drows, dcols);
    });
  });
  HIPCHK(c, hipGetLastError());
  if (any_stop && !power_found && memo) {  // keep the sums just evaluated (c->norm2 is rewritten by every reduction)
    if (!c->start_norm2) HIPCHK(c, hipMalloc(&c->start_norm2, (size_t)batch * sizeof(double)));
    HIPCHK(c, hipMemcpyAsync(c->start_norm2, c->norm2, (size_t)batch * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    c->start_key = std::move(key);
  }
  if (want_power && !partial_found && memo) c->start_partial_key = std::move(pkey);
  if (want_power) return take_power_ticket(c, partial, c->nparts, dsame, zk->power_ticket);
  return PAOS_OK;
}

// a start that fails keeps nothing: neither key may point at sums of another start, or at sums that were never written
static int start_impl(paos_ctx* c, double re, double im, int shape, const double* aperture, const double* stop,
                      const double* write_rows, const double* write_cols = nullptr, const StartZernike* zk = nullptr) {
  const int rc = arena_settled(c, start_body(c, re, im, shape, aperture, stop, write_rows, write_cols, zk));
  if (rc != PAOS_OK && c) start_forget(c);
  return rc;
}

int paos_start(paos_ctx* c, double re, double im, int shape, const double* aperture, const double* stop) {
  return paos_start_box(c, re, im, shape, aperture, stop, nullptr, nullptr);
}

int paos_start_rows(paos_ctx* c, double re, double im, int shape, const double* aperture, const double* stop,
                    const double* write_rows) {
  return paos_start_box(c, re, im, shape, aperture, stop, write_rows, nullptr);
}

int paos_start_box(paos_ctx* c, double re, double im, int shape, const double* aperture, const double* stop,
                   const double* write_rows, const double* write_cols) {
  DROP_SCALE(c);
  return start_impl(c, re, im, shape, aperture, stop, write_rows, write_cols);
}

int paos_start_zernike_box(paos_ctx* c, double re, double im, int shape, const double* aperture, const double* stop,
                           const double* write_rows, const double* write_cols, int nmax, int kdim, const double* table,
                           const double* params, int param_stride, int* power_ticket) {
  DROP_SCALE(c);
  if (c && (!write_rows || !write_cols)) return fail(c, PAOS_EINVAL, "paos_start_zernike_box: null window");
  const StartZernike zk{nmax, kdim, param_stride, table, params, power_ticket};
  return start_impl(c, re, im, shape, aperture, stop, write_rows, write_cols, &zk);
}

int paos_zero_outside_box(paos_ctx* c, const double* live_rows, const double* live_cols) {
  SETTLE_SCALE(c);
  if (c) (void)hipSetDevice(c->device);
  if (!c || !live_rows) return fail(c, PAOS_EINVAL, "null argument");
  int rc = check_rows(c, live_rows);
  if (rc) return rc;
  if (live_cols && (rc = check_rows(c, live_cols))) return rc;
  return arena_settled(c, zero_outside_box(c, live_rows, live_cols));
}

int paos_zero_outside_rows(paos_ctx* c, const double* live_rows) { return paos_zero_outside_box(c, live_rows, nullptr); }

int paos_import(paos_ctx* c, int item, const void* host) {
  SETTLE_SCALE(c);
  if (c) (void)hipSetDevice(c->device);  // one process may drive several GPUs
  if (!c || !host || item < 0 || item >= c->batch) return fail(c, PAOS_EINVAL, "bad item or null buffer");
  const size_t bytes = (size_t)c->n * c->n * 16;
  HIPCHK(c, hipMemcpyAsync(c->staging, host, bytes, hipMemcpyHostToDevice, c->stream));
  dispatch_layout(c, [&](auto t, auto br) {
    using T = decltype(t);
    hipLaunchKernelGGL((import_kernel<T, decltype(br)::value, Lay<T>::BC>), dim3(pw_blocks(c)), dim3(kPwThreads), 0, c->stream,
                       (cx<T>*)c->field + (size_t)item * c->item_stride, (const cx<double>*)c->staging, c->n, c->pitch);
  });
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the host buffer is only borrowed
  return PAOS_OK;
}

static int export_impl(paos_ctx* c, int item, int what, void* host_out, bool pinned) {
  if (!c || !host_out || item < 0 || item >= c->batch || what < 0 || what > 3)
    return fail(c, PAOS_EINVAL, "bad item/what or null buffer");
  dispatch_layout(c, [&](auto t, auto br) {
    using T = decltype(t);
    hipLaunchKernelGGL((export_kernel<T, decltype(br)::value, Lay<T>::BC>), dim3(pw_blocks(c)), dim3(kPwThreads), 0, c->stream,
                       (const cx<T>*)c->field + (size_t)item * c->item_stride, (double*)c->staging, c->n, c->pitch, what);
  });
  HIPCHK(c, hipGetLastError());
  const size_t bytes = (size_t)c->n * c->n * (what == PAOS_WHAT_FIELD ? 16 : 8);
  if (pinned) {  // one DMA into page-locked memory
    HIPCHK(c, hipMemcpyAsync(host_out, c->staging, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  } else {
    int rc = copy_to_host(c, host_out, c->staging, bytes);
    if (rc) return rc;
  }
  return check_mask_overflow(c);
}

int paos_export(paos_ctx* c, int item, int what, void* host_out) {
  SETTLE_SCALE(c);
  if (c) (void)hipSetDevice(c->device);  // one process may drive several GPUs
  return export_impl(c, item, what, host_out, false);
}

int paos_export_pinned(paos_ctx* c, int item, int what, void* pinned_out) {
  SETTLE_SCALE(c);
  if (c) (void)hipSetDevice(c->device);
  return export_impl(c, item, what, pinned_out, true);
}

int paos_psf_keep(paos_ctx* c) {
  SETTLE_SCALE(c);
  if (c) (void)hipSetDevice(c->device);
  if (!c) return fail(c, PAOS_EINVAL, "null context");
  if (!c->psf) HIPCHK(c, hipMalloc(&c->psf, (size_t)c->batch * c->item_stride * sizeof(double)));
  c->psf_zero_axis = -1;  // the whole buffer is rewritten
  c->otf_valid = c->ee_valid = false;  // ... and the transfer functions and energy curves computed from the previous PSFs are stale
  const dim3 grid(pw_blocks(c), c->batch), block(kPwThreads);
  dispatch_layout(c, [&](auto t, auto br) {
    using T = decltype(t);
    hipLaunchKernelGGL((intensity_kernel<T, decltype(br)::value, Lay<T>::BC>), grid, block, 0, c->stream, (const cx<T>*)c->field,
                       c->psf, c->n, c->pitch, c->item_stride);
  });
  HIPCHK(c, hipGetLastError());
  return PAOS_OK;
}

int paos_psf_fetch(paos_ctx* c, int item, double* host_out) {
  if (c) (void)hipSetDevice(c->device);
  if (!c || !host_out || item < 0 || item >= c->batch) return fail(c, PAOS_EINVAL, "bad item or null buffer");
  if (!c->psf) return fail(c, PAOS_EINVAL, "no PSF kept (paos_psf_keep)");
  // the PSF buffer is blocked like the field: row-major through the staging buffer
  dispatch_layout(c, [&](auto t, auto br) {
    hipLaunchKernelGGL((psf_unblock_kernel<decltype(br)::value, Lay<decltype(t)>::BC>), dim3(pw_blocks(c)), dim3(kPwThreads), 0, c->stream,
                       (const double*)c->psf + (size_t)item * c->item_stride, (double*)c->staging, c->n, c->pitch);
  });
  HIPCHK(c, hipGetLastError());
  return copy_to_host(c, host_out, c->staging, (size_t)c->n * c->n * sizeof(double));
}

static int aperture_launch(paos_ctx* c, int shape, const double* dp, int nitems, double* mask_out) {
  const dim3 grid(pw_blocks(c), nitems), block(kPwThreads);
  dispatch_layout(c, [&](auto t, auto br) {
    using T = decltype(t);
    dispatch_either<0, 1>(shape == PAOS_SHAPE_ELLIPSE, [&](auto s) {
      hipLaunchKernelGGL((aperture_kernel<T, decltype(br)::value, Lay<T>::BC, decltype(s)::value>), grid, block, 0, c->stream,
                         mask_out ? (cx<T>*)nullptr : (cx<T>*)c->field, dp, (const double*)nullptr, AP_STRIDE, c->n, c->pitch,
                         c->item_stride, mask_out, 0);
    });
  });
  HIPCHK(c, hipGetLastError());
  return PAOS_OK;
}

int paos_aperture(paos_ctx* c, int shape, const double* params) {
  SETTLE_SCALE(c);
  if (c) (void)hipSetDevice(c->device);  // one process may drive several GPUs
  if (!c || !params) return fail(c, PAOS_EINVAL, "null argument");
  if (shape != PAOS_SHAPE_ELLIPSE && shape != PAOS_SHAPE_RECT) return fail(c, PAOS_EINVAL, "unknown aperture shape");
  const double* dp = nullptr;
  int rc = arena_push(c, params, (size_t)c->batch * AP_STRIDE, &dp);
  if (rc) return rc;
  return aperture_launch(c, shape, dp, c->batch, nullptr);
}

int paos_aperture_render(paos_ctx* c, int shape, const double* params1, double* host_mask) {
  if (c) (void)hipSetDevice(c->device);  // one process may drive several GPUs
  if (!c || !params1 || !host_mask) return fail(c, PAOS_EINVAL, "null argument");
  if (shape != PAOS_SHAPE_ELLIPSE && shape != PAOS_SHAPE_RECT) return fail(c, PAOS_EINVAL, "unknown aperture shape");
  const double* dp = nullptr;
  int rc = arena_push(c, params1, AP_STRIDE, &dp);
  if (rc) return rc;
  rc = aperture_launch(c, shape, dp, 1, (double*)c->staging);
  if (rc) return rc;
  return copy_to_host(c, host_mask, c->staging, (size_t)c->n * c->n * 8);
}

// a stop's optional [batch] enable flags, on the device (null: every item)
static int push_enable(paos_ctx* c, const double* enable, const double** den) {
  *den = nullptr;
  return enable ? arena_push(c, enable, (size_t)c->batch, den) : PAOS_OK;
}

static int norm2_launch(paos_ctx* c, const double* den) {
  norm2_partial_launch(c, den);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(norm2_final_kernel, dim3(c->batch), dim3(kPwThreads), 0, c->stream, c->partial, c->norm2, c->nparts, den, 1);
  HIPCHK(c, hipGetLastError());
  return PAOS_OK;
}

int paos_make_stop(paos_ctx* c, const double* enable) {
  SETTLE_SCALE(c);
  if (c) (void)hipSetDevice(c->device);  // one process may drive several GPUs
  if (!c) return fail(c, PAOS_EINVAL, "null context");
  const double* den;
  int rc = push_enable(c, enable, &den);
  if (rc || (rc = norm2_launch(c, den))) return rc;
  stop_scale_launch(c, den);
  HIPCHK(c, hipGetLastError());
  return PAOS_OK;
}

int paos_stop_scale_last_power(paos_ctx* c, const double* enable) {
  if (!c) return fail(c, PAOS_EINVAL, "null context");
  // something has touched the field or c->norm2 since the program summed the power (or no program did): reduce now
  if (!c->norm2_of_field) return paos_make_stop(c, enable);
  SETTLE_SCALE(c);  // (clears norm2_of_field: behind the stop c->norm2 no longer is the field's power)
  (void)hipSetDevice(c->device);
  const double* den;
  if (int rc = push_enable(c, enable, &den)) return rc;
  stop_scale_launch(c, den);
  HIPCHK(c, hipGetLastError());
  return PAOS_OK;
}

int paos_stop_defer_last_power(paos_ctx* c, const double* enable) {
  if (!c) return fail(c, PAOS_EINVAL, "null context");
  // (a second stop with nothing in between lands here too: the first one consumed the flag, so this one reduces the
  // field as it then is -- make_stop settles the first one's factor first)
  if (!c->norm2_of_field) return paos_make_stop(c, enable);
  (void)hipSetDevice(c->device);
  SETTLE_SCALE(c);  // (clears norm2_of_field)
  const double* den;
  if (int rc = push_enable(c, enable, &den)) return rc;
  hipLaunchKernelGGL(dyn_scale_set_kernel, dim3((c->batch + 255) / 256), dim3(256), 0, c->stream, c->dyn_scale, c->norm2, den, c->batch);
  HIPCHK(c, hipGetLastError());
  c->dyn_pending = true;
  return PAOS_OK;
}

int paos_psf_metrics(paos_ctx* c, int nr, const double* radii_px, double cx_px, double cy_px, double* host_out) {
  SETTLE_SCALE(c);
  if (c) (void)hipSetDevice(c->device);  // one process may drive several GPUs
  if (!c || !host_out || nr < 0 || nr > kMaxRadii || (nr > 0 && !radii_px)) return fail(c, PAOS_EINVAL, "bad metrics request");
  // (a negative radius would act as |r| once squared, a NaN one would count nothing)
  for (int k = 0; k < nr; ++k)
    if (!(radii_px[k] >= 0.0) || !std::isfinite(radii_px[k])) return fail(c, PAOS_EINVAL, "radii must be finite and >= 0");
  if (!std::isfinite(cx_px) || !std::isfinite(cy_px)) return fail(c, PAOS_EINVAL, "the centre must be finite");
  const int nvals = 4 + nr, nblocks = 512;
  if (!c->metric_partial) {
    HIPCHK(c, hipMalloc(&c->metric_partial, (size_t)c->batch * nblocks * (4 + kMaxRadii) * sizeof(double)));
    HIPCHK(c, hipMalloc(&c->metric_out, (size_t)c->batch * (4 + kMaxRadii) * sizeof(double)));
    HIPCHK(c, hipHostMalloc(&c->metric_host, (size_t)c->batch * (4 + kMaxRadii) * sizeof(double)));
  }
  MetricArgs a{};
  a.field = c->field; a.partial = c->metric_partial; a.n = c->n; a.nr = nr; a.pitch = c->pitch;
  a.item_stride = c->item_stride; a.cx = cx_px; a.cy = cy_px;
  for (int k = 0; k < nr; ++k) a.r2[k] = radii_px[k] * radii_px[k];
  const dim3 grid(nblocks, c->batch), block(kPwThreads);
  dispatch_layout(c, [&](auto t, auto br) {
    hipLaunchKernelGGL((psf_metrics_kernel<decltype(t), decltype(br)::value, Lay<decltype(t)>::BC>), grid, block, 0, c->stream, a);
  });
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(psf_metrics_final_kernel, dim3(c->batch), dim3(64), 0, c->stream, c->metric_partial, c->metric_out, nblocks, nvals);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(c->metric_host, c->metric_out, (size_t)c->batch * nvals * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::memcpy(host_out, c->metric_host, (size_t)c->batch * nvals * sizeof(double));
  return check_mask_overflow(c);
}

int paos_norm2_enqueue(paos_ctx* c, int* ticket) {
  SETTLE_SCALE(c);
  if (c) (void)hipSetDevice(c->device);  // one process may drive several GPUs
  if (!c || !ticket) return fail(c, PAOS_EINVAL, "null argument");
  if (int rc = power_ring_full(c)) return rc;
  norm2_partial_launch(c, nullptr);
  HIPCHK(c, hipGetLastError());
  return take_power_ticket(c, c->partial, c->nparts, nullptr, ticket);
}

}  // extern "C"

int psf_keep_power_impl(paos_ctx* c, int* ticket) {
  if (int rc = power_ring_full(c)) return rc;
  if (!c->psf) HIPCHK(c, hipMalloc(&c->psf, (size_t)c->batch * c->item_stride * sizeof(double)));
  c->psf_zero_axis = -1;  // the whole buffer is rewritten
  c->otf_valid = c->ee_valid = false;  // ... and the transfer functions and energy curves computed from the previous PSFs are stale
  const dim3 grid(c->nparts, c->batch), block(kPwThreads);
  dispatch_layout(c, [&](auto t, auto br) {
    using T = decltype(t);
    hipLaunchKernelGGL((intensity_power_kernel<T, decltype(br)::value, Lay<T>::BC>), grid, block, 0, c->stream, (const cx<T>*)c->field,
                       c->psf, c->partial, c->n, c->pitch, c->item_stride);
  });
  HIPCHK(c, hipGetLastError());
  return take_power_ticket(c, c->partial, c->nparts, nullptr, ticket);
}

// rows outside [lo, hi) of every item := 0 (whole block rows, which are contiguous in memory)
int zero_outside_rows(paos_ctx* c, const double* live_rows) {
  const size_t eb = elem_bytes(c);
  for (int i = 0; i < c->batch; ++i) {
    const int br = c->br;
    int lo = ((int)live_rows[2 * i] / br) * br, hi = (((int)live_rows[2 * i + 1] + br - 1) / br) * br;
    if (hi > c->n) hi = c->n;
    if (lo >= hi) { lo = 0; hi = 0; }
    char* base = (char*)c->field + (size_t)i * c->item_stride * eb;
    const size_t row_bytes = (size_t)c->pitch / br * eb;  // one row's share of a block row
    if (lo > 0) HIPCHK(c, hipMemsetAsync(base, 0, (size_t)lo * row_bytes, c->stream));
    if (hi < c->n) HIPCHK(c, hipMemsetAsync(base + (size_t)hi * row_bytes, 0, (size_t)(c->n - hi) * row_bytes, c->stream));
  }
  return PAOS_OK;
}

// ... and outside the columns [lo, hi) of the rows in between (round 5: a sweep over the field; this is the rare path --
// something wants to read a field that was started inside its aperture's box only)
int zero_outside_box(paos_ctx* c, const double* live_rows, const double* live_cols) {
  if (!live_cols) return zero_outside_rows(c, live_rows);
  const double *drows = nullptr, *dcols = nullptr;
  int rc;
  const std::vector<double> lc = rounded_cols(c, live_cols);
  // (no begin: inside a pass program the program's reservation holds these two as well)
  ArenaBatch ab(c);
  if ((rc = ab.add(live_rows, (size_t)2 * c->batch, &drows))) return rc;
  if ((rc = ab.add(lc.data(), lc.size(), &dcols))) return rc;
  if ((rc = ab.commit())) return rc;
  const dim3 grid(pw_blocks(c), c->batch), block(kPwThreads);
  dispatch_layout(c, [&](auto t, auto br) {
    using T = decltype(t);
    hipLaunchKernelGGL((zero_outside_box_kernel<T, decltype(br)::value, Lay<T>::BC>), grid, block, 0, c->stream, (cx<T>*)c->field, c->n,
                       c->pitch, c->item_stride, drows, dcols);
  });
  HIPCHK(c, hipGetLastError());
  return PAOS_OK;
}

extern "C" {

int paos_psf_keep_power(paos_ctx* c, int* ticket) {
  SETTLE_SCALE(c);
  if (c) (void)hipSetDevice(c->device);
  if (!c || !ticket) return fail(c, PAOS_EINVAL, "null argument");
  return psf_keep_power_impl(c, ticket);
}

static int norm2_enqueue_rows_impl(paos_ctx* c, const double* live_rows, const double* same_as, int* ticket,
                                   const double* live_cols = nullptr) {
  if (c) (void)hipSetDevice(c->device);
  if (!c || !ticket || !live_rows) return fail(c, PAOS_EINVAL, "null argument");
  int rc = check_rows(c, live_rows);
  if (rc) return rc;
  if ((rc = power_ring_full(c))) return rc;
  const double *drows = nullptr, *dlead = nullptr, *dsame = nullptr, *dcols = nullptr;
  const size_t nb = (size_t)c->batch;
  ArenaBatch ab(c);
  if ((rc = ab.begin((live_cols ? 2 : 1) * arena_rounded(2 * nb) + (same_as ? 2 : 0) * arena_rounded(nb)))) return rc;
  if ((rc = ab.add(live_rows, 2 * nb, &drows))) return rc;
  if (live_cols) {
    const std::vector<double> lc = rounded_cols(c, live_cols);
    if ((rc = ab.add(lc.data(), lc.size(), &dcols))) return rc;
  }
  if (same_as) {  // items whose fields the caller knows to be copies of another item's: summed once
    if (!same_as_valid(same_as, c->batch, true)) return fail(c, PAOS_EINVAL, "same_as must name an item that stands for itself");
    std::vector<double> lead(c->batch);
    for (int i = 0; i < c->batch; ++i) {
      const int j = (int)same_as[i];
      if (live_rows[2 * i] != live_rows[2 * j] || live_rows[2 * i + 1] != live_rows[2 * j + 1] ||
          (live_cols && (live_cols[2 * i] != live_cols[2 * j] || live_cols[2 * i + 1] != live_cols[2 * j + 1])))
        return fail(c, PAOS_EINVAL, "items that share a sum must share their row (and column) window");
      lead[i] = j == i ? 1.0 : 0.0;
    }
    if ((rc = ab.add(lead.data(), lead.size(), &dlead))) return rc;
    if ((rc = ab.add(same_as, nb, &dsame))) return rc;
  }
  if ((rc = ab.commit())) return rc;
  norm2_partial_launch(c, dlead, drows, dcols);
  HIPCHK(c, hipGetLastError());
  return take_power_ticket(c, c->partial, c->nparts, dsame, ticket);
}

int paos_norm2_enqueue_box(paos_ctx* c, const double* live_rows, const double* live_cols, const double* same_as, int* ticket) {
  SETTLE_SCALE(c);
  if (c && live_cols) {
    int rc = check_rows(c, live_cols);
    if (rc) return rc;
  }
  return arena_settled(c, norm2_enqueue_rows_impl(c, live_rows, same_as, ticket, live_cols));
}

int paos_norm2_enqueue_rows(paos_ctx* c, const double* live_rows, int* ticket) {
  SETTLE_SCALE(c);
  return arena_settled(c, norm2_enqueue_rows_impl(c, live_rows, nullptr, ticket));
}

int paos_norm2_enqueue_rows_like(paos_ctx* c, const double* live_rows, const double* same_as, int* ticket) {
  SETTLE_SCALE(c);
  if (!same_as) return fail(c, PAOS_EINVAL, "null argument");
  return arena_settled(c, norm2_enqueue_rows_impl(c, live_rows, same_as, ticket));
}

int paos_norm2(paos_ctx* c, double* host_out) {
  SETTLE_SCALE(c);
  if (c) (void)hipSetDevice(c->device);  // one process may drive several GPUs
  if (!c || !host_out) return fail(c, PAOS_EINVAL, "null argument");
  int rc = norm2_launch(c, nullptr);
  if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(c->norm2_host, c->norm2, (size_t)c->batch * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::memcpy(host_out, c->norm2_host, (size_t)c->batch * sizeof(double));
  return PAOS_OK;
}

int paos_phase_map(paos_ctx* c, int item, const double* host_wfe, double wl) {
  SETTLE_SCALE(c);
  if (c) (void)hipSetDevice(c->device);
  if (!c || !host_wfe || item < 0 || item >= c->batch) return fail(c, PAOS_EINVAL, "bad item or null buffer");
  if (!(wl > 0.0) || !std::isfinite(wl)) return fail(c, PAOS_EINVAL, "wavelength must be positive and finite");
  const size_t count = (size_t)c->n * c->n;
  double wmax = 0.0;
  for (size_t i = 0; i < count; ++i) {  // the device sincos handles any finite argument; reject the rest here
    if (!std::isfinite(host_wfe[i])) return fail(c, PAOS_EINVAL, "the phase map holds a non-finite value (fill masked pixels with 0)");
    wmax = std::max(wmax, std::fabs(host_wfe[i]));
  }
  if (!phase_map_argument_finite(wmax, wl)) return fail(c, PAOS_EINVAL, kPhaseMapOverflow);
  HIPCHK(c, hipMemcpyAsync(c->staging, host_wfe, count * sizeof(double), hipMemcpyHostToDevice, c->stream));
  dispatch_layout(c, [&](auto t, auto br) {
    using T = decltype(t);
    hipLaunchKernelGGL((phase_map_kernel<T, decltype(br)::value, Lay<T>::BC>), dim3(pw_blocks(c)), dim3(kPwThreads), 0, c->stream,
                       (cx<T>*)c->field + (size_t)item * c->item_stride, (const double*)c->staging, c->n, c->pitch, wl);
  });
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the host buffer is only borrowed
  return PAOS_OK;
}

int paos_phase_map_items(paos_ctx* c, const double* host_wfe, unsigned long long key, int n_items, const double* items,
                         const double* wl) {
  SETTLE_SCALE(c);
  if (c) (void)hipSetDevice(c->device);
  if (!c || !items || !wl || n_items < 1 || n_items > c->batch) return fail(c, PAOS_EINVAL, "bad item list or null buffer");
  if (!host_wfe && (key == 0 || key != c->map_key || !c->map_dev)) return fail(c, PAOS_EINVAL, "no host map, and no map kept on the device under this key");
  for (int k = 0; k < n_items; ++k) {
    if (!(items[k] >= 0.0) || items[k] >= (double)c->batch || items[k] != (double)(int)items[k]) return fail(c, PAOS_EINVAL, "bad item index");
    if (!(wl[k] > 0.0) || !std::isfinite(wl[k])) return fail(c, PAOS_EINVAL, "wavelength must be positive and finite");
    // (two slices of one launch would read, modify and write the same field in no order)
    for (int j = 0; j < k; ++j)
      if (items[j] == items[k]) return fail(c, PAOS_EINVAL, "an item is listed twice");
  }
  const size_t count = (size_t)c->n * c->n;
  if (!c->map_dev) HIPCHK(c, hipMalloc(&c->map_dev, count * sizeof(double)));
  if (key == 0 || key != c->map_key) {  // (the same key again: the caller vouches that the map is the one uploaded under it)
    double wmax = 0.0;
    for (size_t i = 0; i < count; ++i) {  // the device sincos handles any finite argument; reject the rest here
      if (!std::isfinite(host_wfe[i])) return fail(c, PAOS_EINVAL, "the phase map holds a non-finite value (fill masked pixels with 0)");
      wmax = std::max(wmax, std::fabs(host_wfe[i]));
    }
    c->map_key = 0;
    HIPCHK(c, hipMemcpyAsync(c->map_dev, host_wfe, count * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the host buffer is only borrowed
    c->map_key = key;
    c->map_max = wmax;
  }
  // (the kept map's largest value decides for every wavelength it is ever applied at, a later call's smaller one included)
  for (int k = 0; k < n_items; ++k)
    if (!phase_map_argument_finite(c->map_max, wl[k])) return fail(c, PAOS_EINVAL, kPhaseMapOverflow);
  const double *ditems = nullptr, *dwl = nullptr;
  int rc;
  ArenaBatch ab(c);
  if ((rc = ab.begin(2 * arena_rounded((size_t)n_items)))) return rc;
  if ((rc = ab.add(items, (size_t)n_items, &ditems)) || (rc = ab.add(wl, (size_t)n_items, &dwl)) || (rc = ab.commit()))
    return arena_settled(c, rc);
  const dim3 grid(pw_blocks(c), n_items), block(kPwThreads);
  dispatch_layout(c, [&](auto t, auto br) {
    using T = decltype(t);
    hipLaunchKernelGGL((phase_map_items_kernel<T, decltype(br)::value, Lay<T>::BC>), grid, block, 0, c->stream, (cx<T>*)c->field,
                       c->item_stride, (const double*)c->map_dev, c->n, c->pitch, ditems, dwl);
  });
  HIPCHK(c, hipGetLastError());
  return PAOS_OK;
}

int paos_psd_screen(paos_ctx* c, const double* host_noise, const double* host_rough, const double* params, unsigned long long key,
                    double* host_out) {
  if (c) (void)hipSetDevice(c->device);
  if (!c || !host_noise || !params || key == 0) return fail(c, PAOS_EINVAL, "null argument (or key 0)");
  if (c->precision != PAOS_F64) return fail(c, PAOS_EUNSUPPORTED, "PSD screens are built on complex128 contexts (build the map on the host for fp32 mode)");
  PsdParams p{params[0], params[1], params[2], params[3], params[4], params[5], params[6], params[7], params[8], params[9], params[10], params[11]};
  for (int k = 0; k < 12; ++k)
    if (std::isnan(params[k])) return fail(c, PAOS_EINVAL, "a PSD parameter is NaN");
  const size_t count = (size_t)c->n * c->n;
  if (!c->map_dev) HIPCHK(c, hipMalloc(&c->map_dev, count * sizeof(double)));
  if (!c->psd_scratch) HIPCHK(c, hipMalloc(&c->psd_scratch, (size_t)c->item_stride * sizeof(cx<double>)));
  if (!c->psd_bad) HIPCHK(c, hipMalloc(&c->psd_bad, sizeof(int)));
  c->map_key = 0;
  double* noise = (double*)c->staging;  // n x n x 16 bytes: the white noise, then the roughness draw
  double* rough = (host_rough && p.SR != 0.0) ? noise + count : nullptr;
  HIPCHK(c, hipMemcpyAsync(noise, host_noise, count * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (rough) HIPCHK(c, hipMemcpyAsync(rough, host_rough, count * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(c->psd_bad, 0, sizeof(int), c->stream));
  // control blocks of the four passes (one item): forward, inverse, scale 1 / n
  std::vector<double> hb((size_t)3 * FP_STRIDE, 0.0);
  hb[0 * FP_STRIDE + FP_ENABLE] = 1.0;
  hb[1 * FP_STRIDE + FP_ENABLE] = 1.0; hb[1 * FP_STRIDE + 1] = 1.0;
  hb[2 * FP_STRIDE + FP_ENABLE] = 1.0; hb[2 * FP_STRIDE + 3] = 1.0 / c->n;
  const double* dblocks = nullptr;
  int rc;
  if ((rc = arena_push(c, hb.data(), hb.size(), &dblocks))) return rc;
  const dim3 grid(pw_blocks(c)), block(kPwThreads);
  hipLaunchKernelGGL((psd_load_kernel<BR, Lay<double>::BC>), grid, block, 0, c->stream, c->psd_scratch, (const double*)noise, c->n, c->pitch);
  PassArgs a{};
  a.field = c->psd_scratch; a.tw = c->tw; a.blocks = dblocks; a.tables = nullptr; a.mask = nullptr; a.batch = 1;
  a.fft1 = 0; a.fft2 = -1; a.pitch = c->pitch; a.item_stride = c->item_stride;
  for (int axis = 0; axis < 2; ++axis)  // spectrum = fft2(noise)
    if ((rc = generic_pass(c, axis, a, 0))) return rc;
  hipLaunchKernelGGL((psd_filter_kernel<BR, Lay<double>::BC>), grid, block, 0, c->stream, c->psd_scratch, c->n, c->pitch, p);
  a.fft1 = 1; a.n_mid = 1; a.mid[0] = {PAOS_PW_SCALE, 0, 2};
  for (int axis = 0; axis < 2; ++axis)  // ifft2: each axis carries its 1 / n
    if ((rc = generic_pass(c, axis, a, 0))) return rc;
  hipLaunchKernelGGL((psd_finish_kernel<BR, Lay<double>::BC>), grid, block, 0, c->stream, c->map_dev, (const cx<double>*)c->psd_scratch,
                     (const double*)rough, c->n, c->pitch, p, c->psd_bad);
  HIPCHK(c, hipGetLastError());
  int bad = 0;
  HIPCHK(c, hipMemcpyAsync(&bad, c->psd_bad, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // (the host buffers were only borrowed)
  if (bad) return fail(c, PAOS_EINVAL, "the PSD screen holds a non-finite value");
  {  // the largest value of the map, for the wavelengths paos_phase_map_items will apply it at
    std::vector<double> own;
    double* host = host_out;
    if (!host) { own.resize(count); host = own.data(); }
    rc = copy_to_host(c, host, c->map_dev, count * sizeof(double));
    if (rc) return rc;
    double wmax = 0.0;
    for (size_t i = 0; i < count; ++i) wmax = std::max(wmax, std::fabs(host[i]));
    c->map_max = wmax;
  }
  c->map_key = key;
  return PAOS_OK;
}

int paos_copy_yardstick(paos_ctx* c, int reps, double* ms_per_launch, double* bytes_per_launch) {
  SETTLE_SCALE(c);
  if (c) (void)hipSetDevice(c->device);
  if (!c || !ms_per_launch || !bytes_per_launch || reps < 1) return fail(c, PAOS_EINVAL, "bad yardstick request");
  const size_t total = (size_t)c->item_stride * c->batch;
  const int blocks = (int)((total + kPwThreads - 1) / kPwThreads < 65536 * 4 ? (total + kPwThreads - 1) / kPwThreads : 65536 * 4);
  hipEvent_t e0, e1;
  HIPCHK(c, hipEventCreate(&e0));
  HIPCHK(c, hipEventCreate(&e1));
  auto launch = [&] {
    dispatch_layout(c, [&](auto t, auto) {
      using T = decltype(t);
      hipLaunchKernelGGL(rmw_copy_kernel<T>, dim3(blocks), dim3(kPwThreads), 0, c->stream, (cx<T>*)c->field, total);
    });
  };
  launch();  // warm
  HIPCHK(c, hipEventRecord(e0, c->stream));
  for (int r = 0; r < reps; ++r) launch();
  HIPCHK(c, hipEventRecord(e1, c->stream));
  HIPCHK(c, hipEventSynchronize(e1));
  float ms = 0.f;
  HIPCHK(c, hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *ms_per_launch = (double)ms / reps;
  *bytes_per_launch = 2.0 * (double)total * (double)elem_bytes(c);  // pitch padding included: it is moved too
  return PAOS_OK;
}

static int zernike_check(paos_ctx* c, int nmax, int kdim, const double* table, const double* params, int param_stride) {
  if (!c || !table || !params) return fail(c, PAOS_EINVAL, "null argument");
  if (nmax < 0 || kdim < nmax / 2 + 1 || param_stride < ZP_HEAD + 2 * (nmax + 1) * kdim)
    return fail(c, PAOS_EINVAL, "inconsistent Zernike table dimensions");
  // NaN is the kernel's "outside the disk" marker in the wfe map: a record that would make NaN inside the disk (a
  // non-finite coefficient, offset or sampling, a radius <= 0) must not come back looking masked
  for (int i = 0; i < c->batch; ++i) {
    const double* q = params + (size_t)i * param_stride;
    if (q[ZP_ENABLE] == 0.0) continue;
    if (!(q[ZP_RADIUS] > 0.0)) return fail(c, PAOS_EINVAL, "Zernike radius must be > 0");
    for (int k = ZP_DX; k < param_stride; ++k)
      if (!std::isfinite(q[k])) return fail(c, PAOS_EINVAL, "non-finite Zernike parameter");
  }
  return PAOS_OK;
}

static int zernike_apply(paos_ctx* c, int nmax, int kdim, const double* table, const double* params,
                         int param_stride, double* host_wfe, bool use_pupil, const double* same_as = nullptr) {
  int rc = zernike_check(c, nmax, kdim, table, params, param_stride);
  if (rc) return rc;
  if (use_pupil && !c->mask) return fail(c, PAOS_EINVAL, "no pupil defined (paos_pupil_aperture / paos_pupil_upload)");
  const double *dt = nullptr, *dp = nullptr;
  // groups of items with one wfe map: records equal in everything but the wavelength (and no per-item pupil)
  const ItemGroups g = map_groups(c->batch, params, param_stride, ZP_ENABLE, ZP_INV_WL, share_wfe_maps() && !use_pupil);
  const double *dgoff = nullptr, *dglen = nullptr, *dmembers = nullptr, *dtwins = nullptr;
  const size_t nt = (size_t)(nmax + 1) * kdim * 3, np = (size_t)c->batch * param_stride;
  ArenaBatch ab(c);
  if ((rc = ab.begin(arena_rounded(nt) + arena_rounded(np) + arena_rounded(g.goff.size()) + arena_rounded(g.glen.size()) +
                     arena_rounded(g.members.size()) + arena_rounded((size_t)c->batch))))
    return rc;
  if ((rc = ab.add(table, nt, &dt))) return rc;
  if ((rc = ab.add(params, np, &dp))) return rc;
  if ((rc = ab.add(g.goff.data(), g.goff.size(), &dgoff))) return rc;
  if ((rc = ab.add(g.glen.data(), g.glen.size(), &dglen))) return rc;
  if ((rc = ab.add(g.members.data(), g.members.size(), &dmembers))) return rc;
  if (same_as) {  // a group whose members all hold copies of one field reads the leader's (paos_zernike_like)
    if (!same_as_valid(same_as, c->batch, false)) return fail(c, PAOS_EINVAL, "same_as must hold item indices");
    std::vector<double> twins(c->batch, 0.0);
    bool any = false;
    for (int i = 0; i < c->batch; ++i) {
      if (g.glen[i] < 2.0) continue;
      bool all = true;
      for (int k = 0; k < (int)g.glen[i]; ++k) all = all && same_as[(int)g.members[(size_t)g.goff[i] + k]] == same_as[i];
      twins[i] = all ? 1.0 : 0.0;
      any = any || all;
    }
    if (any && (rc = ab.add(twins.data(), twins.size(), &dtwins))) return rc;
  }
  if ((rc = ab.commit())) return rc;
  const dim3 grid(pw_blocks(c), c->batch), block(kPwThreads);
  double* wfe = host_wfe ? (double*)c->staging : nullptr;
  const double* pupil = use_pupil ? c->mask : nullptr;
  // The kernel changes pixels with rho <= 1 only: |row - n/2| dy <= radius.  Bound the rows of the union of the
  // items' disks (two pixels of margin, whole block rows) and walk only that part of memory -- unless the caller
  // wants the wfe map, which is written (NaN) outside the disk too.
  unsigned m_first = 0, m_end = c->item_stride;
  if (!host_wfe) {
    double half = -1.0;
    bool known = true;
    for (int i = 0; i < c->batch; ++i) {
      const double* q = params + (size_t)i * param_stride;
      if (q[ZP_ENABLE] == 0.0) continue;
      const double h = q[ZP_RADIUS] / q[ZP_DY];
      if (!(h >= 0.0) || !std::isfinite(h)) { known = false; break; }
      if (h > half) half = h;
    }
    if (known && half >= 0.0 && half < (double)c->n) {
      int lo = (int)std::floor((double)(c->n / 2) - half) - 2, hi = (int)std::ceil((double)(c->n / 2) + half) + 3;
      lo = lo < 0 ? 0 : (lo / c->br) * c->br;
      hi = hi > c->n ? c->n : ((hi + c->br - 1) / c->br) * c->br;
      if (hi > c->n) hi = c->n;
      m_first = (unsigned)(lo / c->br) * c->pitch;
      m_end = (unsigned)(hi / c->br) * c->pitch;
    }
  }
  // orders up to 8 (45 polynomials) run on the unrolled build
  dispatch_layout(c, [&](auto t, auto br) {
    using T = decltype(t);
    dispatch_either<8, 0>(nmax <= 8, [&](auto nc) {
      hipLaunchKernelGGL((zernike_kernel<T, decltype(br)::value, Lay<T>::BC, decltype(nc)::value>), grid, block, 0, c->stream, (cx<T>*)c->field,
                         dt, dp, param_stride, c->n, c->pitch, c->item_stride, nmax, kdim, wfe, pupil, m_first, m_end, dgoff, dglen, dmembers,
                         dtwins);
    });
  });
  HIPCHK(c, hipGetLastError());
  if (host_wfe) return copy_to_host(c, host_wfe, c->staging, (size_t)c->n * c->n * 8);
  return PAOS_OK;
}

int paos_zernike(paos_ctx* c, int nmax, int kdim, const double* table, const double* params,
                 int param_stride, double* host_wfe) {
  SETTLE_SCALE(c);
  if (c) (void)hipSetDevice(c->device);  // one process may drive several GPUs
  return arena_settled(c, zernike_apply(c, nmax, kdim, table, params, param_stride, host_wfe, false));
}

int paos_zernike_like(paos_ctx* c, int nmax, int kdim, const double* table, const double* params,
                      int param_stride, const double* same_as, double* host_wfe) {
  SETTLE_SCALE(c);
  if (c) (void)hipSetDevice(c->device);
  return arena_settled(c, zernike_apply(c, nmax, kdim, table, params, param_stride, host_wfe, false, same_as));
}

int paos_zernike_pupil(paos_ctx* c, int nmax, int kdim, const double* table, const double* params,
                       int param_stride, double* host_wfe) {
  SETTLE_SCALE(c);
  if (c) (void)hipSetDevice(c->device);
  return arena_settled(c, zernike_apply(c, nmax, kdim, table, params, param_stride, host_wfe, true));
}

static int ensure_pupil(paos_ctx* c) {
  if (!c->mask) HIPCHK(c, hipMalloc(&c->mask, (size_t)c->batch * c->item_stride * sizeof(double)));
  return PAOS_OK;
}

int paos_pupil_aperture(paos_ctx* c, int shape, const double* params) {
  if (c) (void)hipSetDevice(c->device);
  if (!c || !params) return fail(c, PAOS_EINVAL, "null argument");
  if (shape != PAOS_SHAPE_ELLIPSE && shape != PAOS_SHAPE_RECT) return fail(c, PAOS_EINVAL, "unknown aperture shape");
  int rc = ensure_pupil(c);
  if (rc) return rc;
  const double* dp = nullptr;
  rc = arena_push(c, params, (size_t)c->batch * AP_STRIDE, &dp);
  if (rc) return rc;
  const dim3 grid(pw_blocks(c), c->batch), block(kPwThreads);
  // the mask values of the aperture OBJECT, whatever its obscuration flag says (run.py:136-141)
  // (the element type is irrelevant without a field; the block height is the context's)
  dispatch_block_rows(c, [&](auto br) {
    dispatch_either<0, 1>(shape == PAOS_SHAPE_ELLIPSE, [&](auto s) {
      hipLaunchKernelGGL((aperture_kernel<double, decltype(br)::value, Lay<double>::BC, decltype(s)::value>), grid, block, 0, c->stream,
                         (cx<double>*)nullptr, dp, (const double*)nullptr, AP_STRIDE, c->n, c->pitch, c->item_stride, c->mask, 2);
    });
  });
  HIPCHK(c, hipGetLastError());
  return PAOS_OK;
}

int paos_pupil_upload(paos_ctx* c, int item, const double* host_weights) {
  if (c) (void)hipSetDevice(c->device);
  if (!c || !host_weights) return fail(c, PAOS_EINVAL, "null argument");
  if (item < 0 || item >= c->batch) return fail(c, PAOS_EINVAL, "item out of range");
  int rc = ensure_pupil(c);
  if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(c->staging, host_weights, (size_t)c->n * c->n * 8, hipMemcpyHostToDevice, c->stream));
  dispatch_block_rows(c, [&](auto br) {
    hipLaunchKernelGGL((import_weights_kernel<decltype(br)::value, Lay<double>::BC>), dim3(pw_blocks(c)), dim3(kPwThreads), 0, c->stream,
                       (const double*)c->staging, c->mask + (size_t)item * c->item_stride, c->n, c->pitch, c->item_stride);
  });
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));  // host_weights is borrowed
  return PAOS_OK;
}

int paos_zernike_gram(paos_ctx* c, int nmax, int kdim, const double* table, const double* params,
                      int param_stride, int K, const double* poly, int use_pupil, double* host_out) {
  SETTLE_SCALE(c);
  if (c) (void)hipSetDevice(c->device);
  if (!c || !table || !params || !poly || !host_out) return fail(c, PAOS_EINVAL, "null argument");
  if (nmax < 0 || kdim < nmax / 2 + 1 || param_stride < ZP_HEAD)
    return fail(c, PAOS_EINVAL, "inconsistent Zernike table dimensions");
  if (K < 1 || K > kGramMaxK) return fail(c, PAOS_EUNSUPPORTED, "1 <= K <= 64 polynomials");
  if (use_pupil && !c->mask) return fail(c, PAOS_EINVAL, "no pupil defined (paos_pupil_aperture / paos_pupil_upload)");
  for (int i = 0; i < c->batch; ++i) {  // (the header only: the coefficient planes are not read)
    const double* q = params + (size_t)i * param_stride;
    if (q[ZP_ENABLE] == 0.0) continue;
    if (!(q[ZP_RADIUS] > 0.0)) return fail(c, PAOS_EINVAL, "Zernike radius must be > 0");
    for (int k = ZP_DX; k < ZP_HEAD; ++k)
      if (!std::isfinite(q[k])) return fail(c, PAOS_EINVAL, "non-finite Zernike parameter");
  }
  // poly[j] = {|m|, k, is_sin, factor}  ->  slot table + factors
  const size_t ncoef = (size_t)(nmax + 1) * kdim;
  std::vector<double> slots(2 * ncoef, -1.0), fac(K);
  for (int j = 0; j < K; ++j) {
    const int am = (int)poly[4 * j], k = (int)poly[4 * j + 1], is_sin = poly[4 * j + 2] != 0.0;
    if (am < 0 || am > nmax || k < 0 || k >= kdim || am + 2 * k > nmax)
      return fail(c, PAOS_EINVAL, "polynomial outside the recurrence table");
    double& slot = slots[2 * ((size_t)am * kdim + k) + (is_sin ? 1 : 0)];
    if (slot >= 0.0) return fail(c, PAOS_EINVAL, "polynomial listed twice");
    slot = (double)j;
    fac[j] = poly[4 * j + 3];
  }
  const double *dt = nullptr, *dp = nullptr, *dslots = nullptr, *dfac = nullptr;
  int rc;
  ArenaBatch ab(c);
  if ((rc = ab.begin(arena_rounded(ncoef * 3) + arena_rounded((size_t)c->batch * param_stride) + arena_rounded(slots.size()) + arena_rounded(fac.size()))))
    return rc;
  if ((rc = ab.add(table, ncoef * 3, &dt)) || (rc = ab.add(params, (size_t)c->batch * param_stride, &dp)) ||
      (rc = ab.add(slots.data(), slots.size(), &dslots)) || (rc = ab.add(fac.data(), fac.size(), &dfac)) || (rc = ab.commit()))
    return arena_settled(c, rc);
  const int nvals = K * (K + 1) / 2 + 1;
  const size_t chunks = ((size_t)c->item_stride + kGramPix - 1) / kGramPix;
  const int nblocks = (int)(chunks < 512 ? chunks : 512);
  double *partial = nullptr, *sums = nullptr;
  HIPCHK(c, hipMalloc(&partial, (size_t)c->batch * nblocks * nvals * sizeof(double)));
  if (hipMalloc(&sums, (size_t)c->batch * nvals * sizeof(double)) != hipSuccess) {
    (void)hipFree(partial);
    return fail(c, PAOS_EHIP, "hipMalloc(gram sums)");
  }
  const size_t lds = (size_t)K * kGramRow * sizeof(double);
  auto kern = dispatch_block_rows(c, [](auto br) { return zernike_gram_kernel<decltype(br)::value, Lay<double>::BC>; });
  hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(kern, dim3(nblocks, c->batch), dim3(kGramThreads), lds, c->stream, dt, dp, param_stride, c->n,
                       c->pitch, c->item_stride, nmax, kdim, K, dslots, dfac,
                       use_pupil ? (const double*)c->mask : (const double*)nullptr, partial);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(zernike_gram_final_kernel, dim3((nvals + 255) / 256, c->batch), dim3(256), 0, c->stream,
                       (const double*)partial, sums, nblocks, nvals);
    e = hipGetLastError();
  }
  if (e == hipSuccess)
    e = hipMemcpyAsync(host_out, sums, (size_t)c->batch * nvals * sizeof(double), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(partial);
  (void)hipFree(sums);
  if (e != hipSuccess) return fail(c, PAOS_EHIP, std::string("zernike gram: ") + hipGetErrorString(e));
  return PAOS_OK;
}

}  // extern "C"
