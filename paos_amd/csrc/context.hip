// context.hip -- contexts and what every entry point leans on: the per-call parameter arena (pinned ring -> device),
// device -> host copies, error texts, the launch timer, the per-device LDS opt-in.  No kernels.
#include "host.h"

#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <set>
#include <utility>

namespace {

// the text of the last failure of a call without a context, per thread: this is the only copy in the library
thread_local std::string g_err;

}  // namespace

int fail(paos_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  g_err = msg;
  return code;
}

namespace {

// PAOS_DUMP_PASSES=1 (passes.hip: the build of every launch) also says, on stderr, when the arena goes to its next slab or grows
bool dump_arena() {
  static const bool dump = env_is("PAOS_DUMP_PASSES", '1');
  return dump;
}

// copy what has been added and not copied yet, [sent, head) of the slab being filled, in ONE transfer
int arena_commit(paos_ctx* c) {
  Arena& a = c->arena;
  size_t first = 0, count = 0;
  if (!a.lay.take(&first, &count)) return PAOS_OK;
  const size_t at = (size_t)a.cur * a.lay.cap + first;
  HIPCHK(c, hipMemcpyAsync(a.dev + at, a.host + at, count * sizeof(double), hipMemcpyHostToDevice, c->stream));
  return PAOS_OK;
}

// next slab: record the fence of the slab left one switch ago, wait for the readers of the slab about to be refilled
// (blocks still pending in the slab being left are copied first)
int arena_switch(paos_ctx* c) {
  Arena& a = c->arena;
  if (int rc = arena_commit(c)) return rc;
  if (a.left >= 0) {
    HIPCHK(c, hipEventRecord(a.fence[a.left], c->stream));
    a.fenced[a.left] = true;
  }
  a.left = a.cur;
  const int next = (a.cur + 1) % kArenaSlabs;
  if (a.used[next]) {
    if (a.fenced[next]) HIPCHK(c, hipEventSynchronize(a.fence[next]));  // (recorded two switches ago: normally long done)
    else HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  a.fenced[next] = false;
  a.used[next] = true;
  a.cur = next;
  a.lay.rewind();
  if (dump_arena()) std::fprintf(stderr, "arena switch to slab %d\n", next);
  return PAOS_OK;
}

}  // namespace

int launch_failed(paos_ctx* c, const char* call, hipError_t e, const char* file, int line) {  // HIPCHK's text
  return fail(c, PAOS_EHIP, std::string(call) + ": " + hipGetErrorString(e) + " (" + file + ":" + std::to_string(line) + ")");
}

// Make room for `total` doubles of pushes that must ALL stay live until the work enqueued with
// them has run (a pass program: its block table plus one record set per pass).  A ring wrap in the
// middle of such a sequence would overwrite parameters that later launches still read, so the
// wrap (one stream synchronisation) or a growth of the arena happens here, before the first push.
int arena_reserve(paos_ctx* c, size_t total) {
  Arena& a = c->arena;
  switch (a.lay.room(total)) {  // (kArenaSlack on top: the rounding of the individual pushes)
    case ARENA_FITS: return PAOS_OK;
    case ARENA_SWITCH: return arena_switch(c);
    case ARENA_GROW: break;
  }
  // grow every slab: one synchronisation, once (behind the copy of what is still pending: its readers may follow)
  if (int rc = arena_commit(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const size_t cap = a.lay.grown(total);
  double *h = nullptr, *d = nullptr;
  HIPCHK(c, hipHostMalloc(&h, kArenaSlabs * cap * sizeof(double)));
  if (hipMalloc(&d, kArenaSlabs * cap * sizeof(double)) != hipSuccess) {
    (void)hipHostFree(h);
    return fail(c, PAOS_EHIP, "hipMalloc(arena growth)");
  }
  (void)hipHostFree(a.host);
  (void)hipFree(a.dev);
  if (dump_arena()) std::fprintf(stderr, "arena grow to %zu doubles per slab\n", cap);
  a.host = h; a.dev = d; a.lay.cap = cap; a.lay.rewind(); a.cur = 0; a.left = -1;
  for (int k = 0; k < kArenaSlabs; ++k) a.fenced[k] = a.used[k] = false;
  a.used[0] = true;
  return PAOS_OK;
}

int ArenaBatch::begin(size_t total) {
  if (st_.closed || st_.reserved) return fail(c_, PAOS_EINVAL, "a parameter batch is begun once, before its first block");
  const int rc = arena_reserve(c_, total);
  if (rc == PAOS_OK) st_.reserved = true;
  return rc;
}

// write `count` doubles into the pinned slab at the head; *dev: where the commit will put them on the device
int ArenaBatch::add(const double* src, size_t count, const double** dev) {
  Arena& a = c_->arena;
  if (!st_.may_add()) return fail(c_, PAOS_EINVAL, "parameter block added to a batch that has been committed");
  if (count > a.lay.cap) return fail(c_, PAOS_EINVAL, "parameter block larger than the arena");
  if (!a.lay.fits(count)) {
    if (!st_.may_switch()) return fail(c_, PAOS_EINVAL, "a parameter batch outgrew the room it reserved");
    if (int rc = arena_switch(c_)) return rc;
  }
  const size_t at = (size_t)a.cur * a.lay.cap + a.lay.place(count);
  std::memcpy(a.host + at, src, count * sizeof(double));
  *dev = a.dev + at;
  return PAOS_OK;
}

int ArenaBatch::commit() {
  st_.closed = true;
  return arena_commit(c_);
}

// one block, one copy (whatever else is pending goes with it)
int arena_push(paos_ctx* c, const double* src, size_t count, const double** dev) {
  ArenaBatch one(c);
  if (int rc = one.add(src, count, dev)) return rc;
  return one.commit();
}

int arena_settled(paos_ctx* c, int rc) {
  if (!c) return rc;
  const bool pending = c->arena.lay.pending();
  c->arena.lay.drop();
  if (rc == PAOS_OK && pending)
    return fail(c, PAOS_EHIP, "parameter blocks were added but never copied to the device: the call's launches read stale parameters");
  return rc;
}

// Device -> caller's (pageable) host buffer.  hipMemcpy into pageable memory pins the target pages
// on the fly: 65-85 ms for a 4 MiB array every time the allocator hands out fresh pages.  Instead
// arrays of up to 4 MiB (grids up to 512^2) cross PCIe into a pinned buffer and are copied out by the CPU (measured:
// run() at 512^2 3.5-4.7 ms every time instead of 4 / 85 ms alternating); larger ones keep the
// runtime's path, which is faster per byte (4096^2 PSFs: 26 vs 20 wavefronts/s).  Synchronises.
constexpr size_t kBounceBytes = size_t(4) << 20;
int copy_to_host(paos_ctx* c, void* host, const void* dev, size_t bytes) {
  if (bytes > kBounceBytes) {  // large arrays: the runtime's own pageable path moves them faster
    HIPCHK(c, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PAOS_OK;
  }
  for (int i = 0; i < 2; ++i)
    if (!c->bounce[i]) {
      HIPCHK(c, hipHostMalloc(&c->bounce[i], kBounceBytes));
      HIPCHK(c, hipEventCreateWithFlags(&c->bounce_ev[i], hipEventDisableTiming));
    }
  const size_t chunks = (bytes + kBounceBytes - 1) / kBounceBytes;
  auto len = [&](size_t k) { return k + 1 < chunks ? kBounceBytes : bytes - k * kBounceBytes; };
  for (size_t k = 0; k <= chunks; ++k) {
    if (k < chunks) {
      HIPCHK(c, hipMemcpyAsync(c->bounce[k & 1], (const char*)dev + k * kBounceBytes, len(k), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipEventRecord(c->bounce_ev[k & 1], c->stream));
    }
    if (k > 0) {
      HIPCHK(c, hipEventSynchronize(c->bounce_ev[(k - 1) & 1]));
      std::memcpy((char*)host + (k - 1) * kBounceBytes, c->bounce[(k - 1) & 1], len(k - 1));
    }
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PAOS_OK;
}

// The launch timer (paos_profile_begin): every timed launch site brackets its launch with this pair, so that event
// pair i and tag i always belong to the same launch -- the tag is stored where (and only where) the closing event is.
bool timed_launch_begin(paos_ctx* c, int kind) {
  const bool timed = (c->prof_kind == kind || c->prof_kind == PAOS_KERNEL_PASS_ANY) && (c->prof_used + 2 <= c->prof_events.size());
  // (a failure to record the opening event switches the timing of this launch off; the launch itself goes ahead)
  return timed && hipEventRecord(c->prof_events[c->prof_used], c->stream) == hipSuccess;
}
hipError_t timed_launch_end(paos_ctx* c, int tag) {
  const hipError_t e = hipEventRecord(c->prof_events[c->prof_used + 1], c->stream);
  if (e != hipSuccess) return e;
  c->prof_tags.resize(c->prof_used / 2, 0);  // pair i <-> tag i, whatever happened before
  c->prof_tags.push_back(tag);
  c->prof_bytes.resize(c->prof_tags.size() - 1, 0.0);
  c->prof_bytes.push_back(c->prof_next_bytes);
  c->prof_lines.resize(c->prof_tags.size() - 1, 0.0);
  c->prof_lines.push_back(c->prof_next_lines);
  c->prof_used += 2;
  return hipSuccess;
}

// The power tickets are handed out round the ring, but a caller may keep a ticket for long (a result it reads at the
// end): the next free slot is looked for instead of declaring the ring full at the first busy one.
int next_norm_slot(paos_ctx* c) {
  for (int k = 0; k < kNormSlots; ++k) {
    const int slot = (c->norm_slot + k) % kNormSlots;
    if (!c->norm_busy[slot]) { c->norm_slot = slot; return slot; }
  }
  return c->norm_slot;  // every slot is outstanding: the caller's check of norm_busy[] reports it
}

int opt_in_lds(paos_ctx* c, const void* kern, size_t lds) {
  static std::mutex mu;
  static std::set<std::pair<int, const void*>> configured;
  std::lock_guard<std::mutex> lock(mu);
  const std::pair<int, const void*> key(c->device, kern);
  if (configured.count(key)) return PAOS_OK;
  HIPCHK(c, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  configured.insert(key);
  return PAOS_OK;
}

// after a synchronisation: did an aperture's partial run overflow its line records?
int check_mask_overflow(paos_ctx* c) {
  if (!c->mask_overflow) return PAOS_OK;
  int n = 0;
  HIPCHK(c, hipMemcpy(&n, c->mask_overflow, sizeof(int), hipMemcpyDeviceToHost));
  if (n != 0) {
    (void)hipMemset(c->mask_overflow, 0, sizeof(int));
    for (auto& ms : c->mask_sets) ms.key.clear();
    return fail(c, PAOS_EUNSUPPORTED, "aperture line records overflowed (partial run longer than kMaskW): results are invalid");
  }
  return PAOS_OK;
}

int check_rows(paos_ctx* c, const double* rows) {
  for (int i = 0; i < c->batch; ++i)
    if (!(rows[2 * i] >= 0.0) || !(rows[2 * i + 1] <= (double)c->n) || !(rows[2 * i] <= rows[2 * i + 1]))
      return fail(c, PAOS_EINVAL, "row range must satisfy 0 <= lo <= hi <= n");
  return PAOS_OK;
}

// Column windows as every consumer uses them: rounded outward to whole multiples of the block height c->br -- the
// granularity at which plan_pruning lets a pass load positions -- so that what paos_start_box writes, what
// paos_norm2_enqueue_box sums, what paos_zero_outside_box keeps and what the first pass of a program loads are ONE window
// (round 5: written to whole blocks of two columns only, the first pass read up to two stale columns at either edge).
std::vector<double> rounded_cols(const paos_ctx* c, const double* cols) {
  std::vector<double> out((size_t)2 * c->batch);
  for (int i = 0; i < c->batch; ++i) {
    int l = (int)cols[2 * i], h = (int)cols[2 * i + 1];
    l = l < 0 ? 0 : (l / c->br) * c->br;
    h = ((h + c->br - 1) / c->br) * c->br;
    if (h > c->n) h = c->n;
    out[2 * i] = l; out[2 * i + 1] = h;
  }
  return out;
}

namespace {

template <typename T>
std::vector<std::complex<T>> twiddles(int n) {
  std::vector<std::complex<T>> tw(n);
  const long double two_pi = 6.283185307179586476925286766559005768L;
  for (int m = 0; m < n; ++m) {
    // exact octant symmetry keeps the table correctly rounded and conj-symmetric
    const long double a = two_pi * (long double)m / (long double)n;
    tw[m] = std::complex<T>((T)cosl(a), (T)-sinl(a));
  }
  return tw;
}


int profile_end(paos_ctx* c, int* launches, double* total_ms, int* pruned_launches, double* pruned_ms) {
  if (c) (void)hipSetDevice(c->device);  // one process may drive several GPUs
  if (!c || !launches || !total_ms) return fail(c, PAOS_EINVAL, "null argument");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  double sum = 0.0, psum = 0.0;
  int pcount = 0;
  for (size_t i = 0; i + 1 < c->prof_used; i += 2) {
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->prof_events[i], c->prof_events[i + 1]));
    sum += ms;
    if (i / 2 < c->prof_tags.size() && c->prof_tags[i / 2]) { psum += ms; ++pcount; }
  }
  *launches = (int)(c->prof_used / 2);
  *total_ms = sum;
  if (pruned_launches) *pruned_launches = pcount;
  if (pruned_ms) *pruned_ms = psum;
  c->prof_kind = -1;
  c->prof_used = 0;
  return PAOS_OK;
}

}  // namespace

extern "C" {

const char* paos_last_error(const paos_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

const char* paos_build_info(void) {
  static const std::string info = std::string("libpaoship gfx950 layout=") + std::to_string(BR) + "(c64 at N>=2048: " + std::to_string(PAOS_F32_BR) + ")x(" +
                                  std::to_string(Lay<double>::BC) + "|" + std::to_string(Lay<float>::BC) +
                                  ") pad_blocks=" + std::to_string(PAOS_PAD_BLOCKS);
  return info.c_str();
}

void* paos_stream(paos_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int paos_ctx_create(int device, int n, int batch, int precision, paos_ctx** out) {
  if (!out) return fail(nullptr, PAOS_EINVAL, "out is null");
  *out = nullptr;
  if (n < 64 || n > 4096 || (n & (n - 1))) return fail(nullptr, PAOS_EUNSUPPORTED, "grid size must be a power of two in 64..4096");
  if (batch < 1) return fail(nullptr, PAOS_EINVAL, "batch must be >= 1");
  if (precision != PAOS_F64 && precision != PAOS_F32) return fail(nullptr, PAOS_EINVAL, "precision must be PAOS_F64 or PAOS_F32");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(nullptr, PAOS_EHIP, "no HIP device available: libpaoship has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(nullptr, PAOS_EINVAL, "device index out of range");
  paos_ctx* c = new paos_ctx();
  c->device = device; c->n = n; c->batch = batch; c->precision = precision;
  const int bc = precision == PAOS_F64 ? Lay<double>::BC : Lay<float>::BC;
  c->br = (precision == PAOS_F32 && n >= 2048) ? PAOS_F32_BR : PAOS_BR;  // block_rows<T, N>()
  c->pitch = (unsigned)n * c->br + (unsigned)PAOS_PAD_BLOCKS * c->br * bc;
  c->item_stride = c->pitch * (unsigned)(n / c->br);
  const size_t eb = elem_bytes(c);
  auto bail = [&](hipError_t e, const char* what) {
    std::string msg = std::string(what) + ": " + hipGetErrorString(e);
    paos_ctx_destroy(c);
    return fail(nullptr, PAOS_EHIP, msg);
  };
  hipError_t e;
  if ((e = hipSetDevice(device)) != hipSuccess) return bail(e, "hipSetDevice");
  if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) return bail(e, "hipStreamCreate");
  if (const char* pad = getenv("PAOS_LDS_PAD")) c->lds_pad = (size_t)std::max(0, std::atoi(pad));
  if (env_is("PAOS_CENTRAL_HALF", '0')) c->central_half = false;
  if (env_is("PAOS_CENTRAL_HALF", '1')) c->central_half = true;
  if (env_is("PAOS_NARROW_WINDOWS", '0')) c->narrow_windows = false;
  if (env_is("PAOS_NARROW_WINDOWS", '1')) c->narrow_windows = true;
  if ((e = hipMalloc(&c->dyn_scale, (size_t)batch * sizeof(double))) != hipSuccess) return bail(e, "hipMalloc(dyn_scale)");
  {
    std::vector<double> ones((size_t)batch, 1.0);
    if ((e = hipMemcpy(c->dyn_scale, ones.data(), ones.size() * sizeof(double), hipMemcpyHostToDevice)) != hipSuccess) return bail(e, "hipMemcpy(dyn_scale)");
  }
  if ((e = hipMalloc(&c->field, (size_t)c->item_stride * batch * eb)) != hipSuccess) return bail(e, "hipMalloc(field)");
  if ((e = hipMemsetAsync(c->field, 0, (size_t)c->item_stride * batch * eb, c->stream)) != hipSuccess) return bail(e, "hipMemset(field)");
  if ((e = hipMalloc(&c->tw, (size_t)n * eb)) != hipSuccess) return bail(e, "hipMalloc(tw)");
  if ((e = hipMalloc(&c->staging, (size_t)n * n * 16)) != hipSuccess) return bail(e, "hipMalloc(staging)");
  c->nparts = 1024;
  if ((e = hipMalloc(&c->partial, (size_t)batch * c->nparts * sizeof(double))) != hipSuccess) return bail(e, "hipMalloc(partial)");
  if ((e = hipMalloc(&c->norm2, (size_t)batch * sizeof(double))) != hipSuccess) return bail(e, "hipMalloc(norm2)");
  if ((e = hipHostMalloc(&c->norm2_host, (size_t)kNormSlots * batch * sizeof(double))) != hipSuccess) return bail(e, "hipHostMalloc(norm2)");
  c->arena.lay.cap = (size_t)1 << 18;  // four slabs of 2 MiB of doubles; a large batch starts with room for one of its programs per slab
  if (c->arena.lay.cap < (size_t)batch * 2048) c->arena.lay.cap = (size_t)batch * 2048;
  // PAOS_ARENA_DOUBLES: another slab size to start with (whole blocks, at least one); a batch that reserves more grows the
  // slabs, a single block pushed on its own has to fit
  if (const char* cap = getenv("PAOS_ARENA_DOUBLES")) c->arena.lay.cap = arena_rounded((size_t)std::max(1LL, std::atoll(cap)));
  if ((e = hipHostMalloc(&c->arena.host, kArenaSlabs * c->arena.lay.cap * sizeof(double))) != hipSuccess) return bail(e, "hipHostMalloc(arena)");
  if ((e = hipMalloc(&c->arena.dev, kArenaSlabs * c->arena.lay.cap * sizeof(double))) != hipSuccess) return bail(e, "hipMalloc(arena)");
  for (int k = 0; k < kArenaSlabs; ++k)
    if ((e = hipEventCreateWithFlags(&c->arena.fence[k], hipEventDisableTiming)) != hipSuccess) return bail(e, "hipEventCreate(arena fence)");
  c->arena.used[0] = true;
  e = dispatch_layout(c, [&](auto t, auto) {
    auto tw = twiddles<decltype(t)>(n);
    return hipMemcpy(c->tw, tw.data(), (size_t)n * eb, hipMemcpyHostToDevice);
  });
  if (e != hipSuccess) return bail(e, "hipMemcpy(tw)");
  *out = c;
  return PAOS_OK;
}

int paos_profile_begin(paos_ctx* c, int kernel_kind, int max_launches) {
  if (c) (void)hipSetDevice(c->device);  // one process may drive several GPUs
  if (!c || max_launches < 0) return fail(c, PAOS_EINVAL, "bad profile request");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  while (c->prof_events.size() < (size_t)2 * max_launches) {
    hipEvent_t e;
    HIPCHK(c, hipEventCreate(&e));
    c->prof_events.push_back(e);
  }
  c->prof_kind = kernel_kind;
  c->prof_used = 0;
  c->prof_tags.clear();
  c->prof_bytes.clear();
  c->prof_lines.clear();
  return PAOS_OK;
}

int paos_profile_end_launches(paos_ctx* c, int capacity, double* ms_out, int* tag_out, int* count) {
  if (c) (void)hipSetDevice(c->device);
  if (!c || !ms_out || !tag_out || !count || capacity < 0) return fail(c, PAOS_EINVAL, "null argument");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int n = (int)(c->prof_used / 2);
  if (n > capacity) return fail(c, PAOS_EINVAL, "more launches were timed than the caller's arrays hold");
  for (int i = 0; i < n; ++i) {
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->prof_events[2 * i], c->prof_events[2 * i + 1]));
    ms_out[i] = ms;
    tag_out[i] = (size_t)i < c->prof_tags.size() ? c->prof_tags[i] : 0;
  }
  *count = n;
  c->prof_kind = -1;
  c->prof_used = 0;
  return PAOS_OK;
}

// bytes the pruning plan had each timed launch so far load + store (call BEFORE paos_profile_end_launches, which resets)
int paos_profile_planned_bytes(paos_ctx* c, int capacity, double* bytes_out, int* count) {
  if (!c || !bytes_out || !count || capacity < 0) return fail(c, PAOS_EINVAL, "null argument");
  const int n = (int)(c->prof_used / 2);
  if (n > capacity) return fail(c, PAOS_EINVAL, "more launches were timed than the caller's array holds");
  for (int i = 0; i < n; ++i) bytes_out[i] = (size_t)i < c->prof_bytes.size() ? c->prof_bytes[i] : 0.0;
  *count = n;
  return PAOS_OK;
}

// 1-D line transforms each timed launch so far ran (call BEFORE paos_profile_end_launches, which resets)
int paos_profile_line_transforms(paos_ctx* c, int capacity, double* lines_out, int* count) {
  if (!c || !lines_out || !count || capacity < 0) return fail(c, PAOS_EINVAL, "bad profile request");
  const int n = (int)(c->prof_used / 2);
  if (n > capacity) return fail(c, PAOS_EINVAL, "profile buffer too small");
  for (int i = 0; i < n; ++i) lines_out[i] = (size_t)i < c->prof_lines.size() ? c->prof_lines[i] : 0.0;
  *count = n;
  return PAOS_OK;
}

int paos_profile_end(paos_ctx* c, int* launches, double* total_ms) {
  return profile_end(c, launches, total_ms, nullptr, nullptr);
}

int paos_profile_end_split(paos_ctx* c, int* launches, double* total_ms, int* pruned_launches, double* pruned_ms) {
  if (!pruned_launches || !pruned_ms) return fail(c, PAOS_EINVAL, "null argument");
  return profile_end(c, launches, total_ms, pruned_launches, pruned_ms);
}

int paos_ctx_destroy(paos_ctx* c) {
  if (!c) return PAOS_OK;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (hipEvent_t e : c->prof_events) (void)hipEventDestroy(e);
  if (c->field) (void)hipFree(c->field);
  if (c->tw) (void)hipFree(c->tw);
  if (c->staging) (void)hipFree(c->staging);
  if (c->tables) (void)hipFree(c->tables);
  if (c->mask) (void)hipFree(c->mask);
  if (c->metric_partial) (void)hipFree(c->metric_partial);
  if (c->metric_out) (void)hipFree(c->metric_out);
  if (c->metric_host) (void)hipHostFree(c->metric_host);
  for (auto& ms : c->mask_sets) {
    if (ms.lines) (void)hipFree(ms.lines);
    if (ms.vals) (void)hipFree(ms.vals);
  }
  if (c->mask_overflow) (void)hipFree(c->mask_overflow);
  if (c->block_stats) (void)hipFree(c->block_stats);
  if (c->partial) (void)hipFree(c->partial);
  if (c->norm2) (void)hipFree(c->norm2);
  if (c->norm2_host) (void)hipHostFree(c->norm2_host);
  if (c->psf) (void)hipFree(c->psf);
  if (c->focus_spec) (void)hipFree(c->focus_spec);
  if (c->otf_spec) (void)hipFree(c->otf_spec);
  if (c->otf_cuts) (void)hipFree(c->otf_cuts);
  if (c->zoom_t) (void)hipFree(c->zoom_t);
  if (c->zoom_psf) (void)hipFree(c->zoom_psf);
  if (c->zoom_field) (void)hipFree(c->zoom_field);
  if (c->zoom_tabs) (void)hipFree(c->zoom_tabs);
  if (c->map_dev) (void)hipFree(c->map_dev);
  if (c->psd_scratch) (void)hipFree(c->psd_scratch);
  if (c->start_norm2) (void)hipFree(c->start_norm2);
  if (c->start_partial) (void)hipFree(c->start_partial);
  if (c->psd_bad) (void)hipFree(c->psd_bad);
  if (c->pow_partial) (void)hipFree(c->pow_partial);
  if (c->dyn_scale) (void)hipFree(c->dyn_scale);
  if (c->ptab) (void)hipFree(c->ptab);
  if (c->psf_partial) (void)hipFree(c->psf_partial);
  if (c->det_img) (void)hipFree(c->det_img);
  if (c->det_rows) (void)hipFree(c->det_rows);
  if (c->det_out) (void)hipFree(c->det_out);
  if (c->ee_buf) (void)hipFree(c->ee_buf);
  if (c->wf_buf) (void)hipFree(c->wf_buf);
  if (c->series_par) (void)hipFree(c->series_par);
  if (c->series_flux) (void)hipFree(c->series_flux);
  if (c->series_frames) (void)hipFree(c->series_frames);
  if (c->series_host) (void)hipHostFree(c->series_host);
  if (c->series_ev) (void)hipEventDestroy(c->series_ev);
  if (c->sum_acc) (void)hipFree(c->sum_acc);
  if (c->sum_par) (void)hipFree(c->sum_par);
  if (c->sum_flux) (void)hipFree(c->sum_flux);
  if (c->sum_host) (void)hipHostFree(c->sum_host);
  if (c->sum_ev) (void)hipEventDestroy(c->sum_ev);
  for (int i = 0; i < 2; ++i) {
    if (c->bounce[i]) (void)hipHostFree(c->bounce[i]);
    if (c->bounce_ev[i]) (void)hipEventDestroy(c->bounce_ev[i]);
  }
  if (c->arena.host) (void)hipHostFree(c->arena.host);
  if (c->arena.dev) (void)hipFree(c->arena.dev);
  for (int k = 0; k < kArenaSlabs; ++k)
    if (c->arena.fence[k]) (void)hipEventDestroy(c->arena.fence[k]);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return PAOS_OK;
}

int paos_sync(paos_ctx* c) {
  if (c) (void)hipSetDevice(c->device);  // one process may drive several GPUs
  if (!c) return fail(c, PAOS_EINVAL, "null context");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return check_mask_overflow(c);
}

int paos_host_alloc(unsigned long long bytes, void** out) {
  if (!out || bytes == 0) return fail(nullptr, PAOS_EINVAL, "null argument");
  *out = nullptr;
  const hipError_t e = hipHostMalloc(out, (size_t)bytes);
  if (e != hipSuccess) {
    *out = nullptr;
    return fail(nullptr, PAOS_EHIP, std::string("hipHostMalloc: ") + hipGetErrorString(e));
  }
  return PAOS_OK;
}

int paos_host_free(void* p) {
  if (!p) return PAOS_OK;
  const hipError_t e = hipHostFree(p);
  if (e != hipSuccess) return fail(nullptr, PAOS_EHIP, std::string("hipHostFree: ") + hipGetErrorString(e));
  return PAOS_OK;
}

int paos_norm2_fetch(paos_ctx* c, int ticket, double* host_out) {
  if (c) (void)hipSetDevice(c->device);  // one process may drive several GPUs
  if (!c || !host_out || ticket < 0 || ticket >= kNormSlots) return fail(c, PAOS_EINVAL, "bad ticket");
  if (!c->norm_busy[ticket]) return fail(c, PAOS_EINVAL, "ticket is not outstanding (already fetched, or never issued)");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->norm_busy[ticket] = false;
  std::memcpy(host_out, c->norm2_host + (size_t)ticket * c->batch, (size_t)c->batch * sizeof(double));
  return check_mask_overflow(c);
}

int paos_norm2_release(paos_ctx* c, int ticket) {
  if (!c || ticket < 0 || ticket >= kNormSlots) return fail(c, PAOS_EINVAL, "bad ticket");
  c->norm_busy[ticket] = false;  // the caller does not want the value; the slot may be handed out again
  return PAOS_OK;
}

int paos_record_set_stats(paos_ctx* c, unsigned long long* found, unsigned long long* rendered) {
  if (!c || !found || !rendered) return fail(c, PAOS_EINVAL, "bad record-set request");
  *found = c->mask_hits;
  *rendered = c->mask_rendered;
  return PAOS_OK;
}

int paos_central_half_stats(paos_ctx* c, unsigned long long* central, unsigned long long* plain) {
  if (!c || !central || !plain) return fail(c, PAOS_EINVAL, "bad central-half request");
  *central = c->central_launches;
  *plain = c->plain_launches;
  return PAOS_OK;
}

int paos_narrow_window_stats(paos_ctx* c, unsigned long long* narrow, unsigned long long* other) {
  if (!c || !narrow || !other) return fail(c, PAOS_EINVAL, "bad narrow-window request");
  *narrow = c->narrow_launches;
  *other = c->other_launches;
  return PAOS_OK;
}

int paos_record_block_stats(paos_ctx* c, unsigned long long* out) {
  if (!c || !out) return fail(c, PAOS_EINVAL, "bad record-block request");
  out[0] = out[1] = out[2] = 0ull;
  if (!c->block_stats) return PAOS_OK;  // nothing was rendered yet
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out, c->block_stats, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return PAOS_OK;
}

int paos_deferred_stop_stats(paos_ctx* c, unsigned long long* rode, unsigned long long* settled) {
  if (!c || !rode || !settled) return fail(c, PAOS_EINVAL, "bad deferred-stop request");
  *rode = c->deferred_rode;
  *settled = c->deferred_settled;
  return PAOS_OK;
}

int paos_ctx_set_pruning(paos_ctx* c, int on) {
  if (!c) return fail(c, PAOS_EINVAL, "null context");
  c->prune = on != 0;
  return PAOS_OK;
}

}  // extern "C"
