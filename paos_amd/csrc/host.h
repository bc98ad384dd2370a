// host.h -- what the translation units of libpaoship share (internal; the C ABI is include/paos_hip.h).
//
// The host side of the library is split by what it launches: context.hip (contexts, the parameter arena, errors,
// the launch timer), passes.hip (pass programs; what a program launches is planned in plain C++: pass_program.h on the
// records of pass_records.h), generic_pass.hip and frugal_<family>.hip (the pass kernels), paos_hip.hip (the pointwise entry points: every kernel of pointwise.h) and the products: focus_otf.hip, zoom.hip,
// detector.hip, energy.hip, wavefront.hip, series.hip.  Here: the build-time layout, the context, the error and launch helpers, the dispatchers that turn what a
// context is at run time into template arguments (dispatch_n: the grid size; dispatch_layout / dispatch_block_rows: element
// type and block height; with pass_records.h's dispatch_family: the families of the frugal pass kernel -- every launch is
// written once, inside a generic lambda), and the declarations of the functions
// that cross unit boundaries.  Whatever is not declared here lives in an anonymous namespace of its unit.  Which items of a
// batch share what is plain C++ in item_groups.h, where the blocks of the parameter arena go in arena_layout.h.
#pragma once
#include "../../include/paos_hip.h"

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <string>
#include <type_traits>
#include <vector>

#include "arena_layout.h"
#include "frugal_pass.h"
#include "pass_records.h"

using namespace paos;

// ---- build-time layout choice -------------------------------------------------------
// A field is stored as blocks of 4 rows x 2 columns (128 B of complex128, 64 B of complex64),
// blocks row-major, so whole or half cache lines are the unit of work for the row pass (2 or 4
// rows per workgroup) and for the column pass (2 columns per workgroup) alike (DESIGN.md
// section 2).  PAD_BLOCKS extra blocks per block row de-tune the power-of-two stride of
// the column pass (measured: 3.5 -> 4.8 TB/s at 4096^2, profiles/r01_fftbench_v2_pitchpad.txt).
#ifndef PAOS_BR
#define PAOS_BR 4
#endif
#ifndef PAOS_PAD_BLOCKS
#define PAOS_PAD_BLOCKS 3
#endif
inline constexpr int BR = PAOS_BR;  // complex128 and the base case of complex64
// complex64 at N >= 2048 (where the frugal kernels serve it): blocks of 8 rows x 2 columns = 128 B like a complex128
// block, so that column tiles own whole lines (round 3; profiles/r02_fftbench_c64_8row_blocks_experiment.txt).  Below
// 2048 the generic kernels keep 4 x 2 (a column tile needs N / 16 >= block height threads per line).
#ifndef PAOS_F32_BR
#define PAOS_F32_BR 8
#endif
template <typename T, int N>
constexpr int block_rows() { return (sizeof(T) == 4 && N >= 2048) ? PAOS_F32_BR : PAOS_BR; }
inline constexpr int kNormSlots = PAOS_NORM_SLOTS;  // outstanding paos_norm2_enqueue results
template <typename T>
struct Lay {
  // 2 columns for both types: a block is 128 B of complex128 or 64 B of complex64.  (4 columns
  // of complex64 would fill the line but make the column tile 4 lines = 1024 threads, which
  // spills; measured 126 wavefronts/s vs the 2-column shape below.)
  static constexpr int BC = 2;
};

// Parameter arena: kArenaSlabs slabs of `cap` doubles each (pinned host mirror + device), filled one after the other.
// Round 5: a slab is reused only after the work that read it has run -- told by an EVENT recorded one slab switch after it
// was left (by then every launch that reads it has been enqueued: a call's pushes and its launches never span more than
// two slabs) -- instead of by a hipStreamSynchronize at every wrap of one ring: at 512 wavefronts per step the ring
// wrapped every second step, and each wrap made the host wait for the GPU to drain (1024^2: 33 ms per step where the GPU
// needs 25 and the host 18).  With four slabs the host may run two to three steps ahead and no further.
// Round 17: a block is written to the pinned slab when it is added and copied to the device when its batch is committed --
// one hipMemcpyAsync for every block a call adds in front of its first launch (ArenaBatch below), instead of one per block
// (22 copy kernels of ~4.7 us per SYN20 step, each a dispatch of its own in front of the kernel that reads it).
// PAOS_ARENA_DOUBLES: the slab size a context starts with (tests: a small one, so that a short sweep goes round the slabs).
constexpr int kArenaSlabs = 4;
struct Arena {
  double* host = nullptr;  // pinned, kArenaSlabs * lay.cap doubles
  double* dev = nullptr;
  ArenaLayout lay;           // doubles per slab, fill of the current slab, what of it is not copied yet (arena_layout.h)
  int cur = 0;               // slab being filled
  int left = -1;             // the slab left at the last switch: its fence is recorded at the NEXT switch
  hipEvent_t fence[kArenaSlabs] = {};
  bool fenced[kArenaSlabs] = {};  // fence[k] has been recorded since slab k was last filled
  bool used[kArenaSlabs] = {};
};

struct paos_ctx {
  int device = 0, n = 0, batch = 0, precision = 0;
  int br = PAOS_BR;  // block height of this context's layout (block_rows<T, N>())
  unsigned pitch = 0, item_stride = 0;
  hipStream_t stream = nullptr;
  double* psf = nullptr;  // batch x item_stride intensities kept on the device, blocked like the field (paos_psf_keep)
  // a through-focus stack (paos_focus_begin .. paos_focus_end): the forward 2-D spectrum of every item's field, complex<T>
  // of the context's precision in the field's own layout; allocated by the first paos_focus_begin
  void* focus_spec = nullptr;
  bool focus_open = false;
  // transfer functions (paos_otf_compute): the spectra of the kept PSFs, complex<T> of the context's precision in the
  // field's own layout (columns 0 .. N/2 hold the spectrum, otf_pass.h); allocated by the first paos_otf_compute.
  // otf_valid: the buffer was computed from what the PSF buffer holds NOW -- cleared by everything that stores a PSF
  void* otf_spec = nullptr;
  bool otf_computed = false, otf_valid = false;
  double* otf_cuts = nullptr;  // [batch][2][N/2 + 1], allocated by the first paos_otf_cuts
  // blurred PSFs (paos_blur_apply): the host copy of every item's two tables, [batch][2][N/2 + 1], and the (d, sigma, pixel)
  // each was evaluated for, [batch][2][3] -- a table is a pure function of those, and its long-double evaluation costs
  // more host time than the launches take on the device (the planes of a focus stack, the batches of a Monte-Carlo study
  // and the steps of a benchmark ask for the same tables again)
  std::vector<double> blur_tabs, blur_key;
  // zoomed windows (paos_zoom_compute): the column-contracted field T [batch][N][M] complex128, the windows [batch][M][M]
  // (intensities; the complex field when asked for) and the phase tables of the fractional centres seen so far -- slot k
  // of zoom_tabs holds the [s][N] table of zoom_fracs[k], zoom_carry[k] its carries (all for oversampling zoom_s)
  cx<double>* zoom_t = nullptr;
  double* zoom_psf = nullptr;
  cx<double>* zoom_field = nullptr;
  int zoom_m = 0;  // the window size the three buffers were allocated for
  bool zoom_done = false, zoom_has_field = false;
  double* zoom_tabs = nullptr;
  int zoom_s = 0, zoom_cap = 0;
  std::vector<double> zoom_fracs;
  std::vector<std::vector<int>> zoom_carry;
  double* map_dev = nullptr;      // one n x n phase map kept on the device (paos_phase_map_items) and the key it was uploaded under
  unsigned long long map_key = 0;
  double map_max = 0.0;  // max |w| of the kept map: fl(fl(2 pi max) / wl) must stay finite for every wavelength it is applied at
  // (round 5) the power sums of the last start, kept with everything they depend on (shape, constant, aperture records,
  // stop flags): the entrance pupil of a wavelength sweep or a Monte-Carlo study is the same step after step, and the sums
  // are a pure function of those -- the next start with the same key copies them instead of evaluating the exact pixel
  // overlaps again (start_power_kernel + norm2_final_kernel: 0.08 ms of a 14.6 ms SYN20 step).  PAOS_START_POWER_MEMO=0: never.
  std::vector<double> start_key;
  double* start_norm2 = nullptr;  // [batch]
  // (round 17) ... and the per-workgroup sums of the power of the start FIELD inside its box (start_norm2_partial_kernel:
  // the saved first surface of a lean sweep, whose field is never stored on its own), [batch][nparts]: a pure function of
  // the start key, the row windows, the rounded column windows and which items lead / share a sum.  The final reduction
  // runs every time, so the power is the same bits.  Both keys are set only once the launches that fill the sums are
  // enqueued, and a failed start clears both.
  std::vector<double> start_partial_key;
  double* start_partial = nullptr;
  cx<double>* psd_scratch = nullptr;  // one item in the field's layout: the spectrum of a PSD screen (paos_psd_screen)
  int* psd_bad = nullptr;
  double* psf_partial = nullptr;  // per-workgroup sums of a pass that stores the PSF (paos_run_program: final_intensity)
  int psf_nparts = 0;
  double* pow_partial = nullptr;  // per-workgroup sums of |u|^2 of a pass that stores the FIELD (final_intensity = 2)
  int pow_nparts = 0;
  // [batch] factors every frugal pass multiplies into the scale of its middle slot (FrugalArgs::dyn_scale): ones, except
  // between paos_stop_defer_last_power and the pass (or settle_scale) that applies the stop's 1 / sqrt(power)
  cx<double>* ptab = nullptr;  // [ptab_slots][batch][n] phase factors by position: a table per operator slot of the launches of the
  int ptab_slots = 0;          // program about to run (FrugalSlot::table; stage_groups)
  double* dyn_scale = nullptr;
  bool dyn_pending = false;
  // a pending factor went into a program's first pass / was applied by the sweep or dropped (paos_deferred_stop_stats)
  unsigned long long deferred_rode = 0, deferred_settled = 0;
  // c->norm2 holds sum |u|^2 of the field exactly as it is stored: set by a pass program whose last pass summed it on the
  // way out (paos_run_program, final_intensity = 2), cleared by every entry point that reads or rewrites the field or
  // reduces into c->norm2 (SETTLE_SCALE / DROP_SCALE sit at the top of all of them).  paos_stop_scale_last_power and
  // paos_stop_defer_last_power trust c->norm2 only while it is set and run paos_make_stop otherwise.
  bool norm2_of_field = false;
  // What the PSF buffer (and psf_partial) is known to hold after a pass stored it: for item i the lines along
  // psf_zero_axis outside [psf_zero_lo[i], psf_zero_hi[i]) are zero (their per-workgroup sums too).  The next
  // PSF-storing pass with the same live lines need not write those zeros again; -1 = nothing known.
  int psf_zero_axis = -1;
  std::vector<double> psf_zero_lo, psf_zero_hi;
  // detector pixel grid of paos_detector_begin (plain types: the struct is the same in every translation unit)
  bool det_set = false;
  int det_nx = 0, det_ny = 0;
  double det_geom[4] = {};         // pitch_x, pitch_y, xc, yc
  double* det_img = nullptr;       // [ny][nx] fp64 accumulator
  double* det_rows = nullptr;      // row-contraction scratch of one chunk of items (allocated on first use, grown)
  size_t det_rows_bytes = 0;
  double* det_out = nullptr;       // per-item images of one chunk (paos_detector_images)
  size_t det_out_bytes = 0;
  // energy profiles (paos_ee_compute): one buffer -- summary [batch][9] | curves [batch][ee_curves][ee_bins] | the partial
  // sums of the launches -- allocated on first use and again when a request needs more.  ee_valid: the curves were
  // computed from what the PSF buffer holds NOW -- cleared by everything that stores a PSF, paos_blur_apply included
  double* ee_buf = nullptr;
  size_t ee_bytes = 0;
  int ee_bins = 0, ee_curves = 0;
  bool ee_computed = false, ee_valid = false;
  // wavefront fits (paos_wavefront_fit): one buffer -- summary [batch][10] | sums [batch][wf_pairs] | the reference phasors
  // | the partial sums of the launches -- allocated on first use and again when a request needs more
  double* wf_buf = nullptr;
  size_t wf_bytes = 0;
  int wf_pairs = 0;
  bool wf_fitted = false;
  // pointing series (paos_series_compute): the parameters of the last call (per-item records | offsets | boxes | response;
  // staged in series_host, pinned, which series_ev guards until the copy has run), the fluxes [batch][frames][nboxes]
  // and the frames of one chunk -- each allocated on first use and again when a request needs more
  double* series_par = nullptr;
  size_t series_par_bytes = 0;
  double* series_host = nullptr;
  size_t series_host_bytes = 0;
  hipEvent_t series_ev = nullptr;
  double* series_flux = nullptr;
  size_t series_flux_bytes = 0;
  double* series_frames = nullptr;
  size_t series_frames_bytes = 0;
  int series_nframes = 0, series_nboxes = 0;
  bool series_done = false;
  // broadband series sum (paos_series_sum_*): the accumulator S[frames][ny][nx] of the open sum with its geometry, the
  // parameters of the last add or flux call (staged in sum_host, pinned, which sum_ev guards until the copy has run) and
  // the fluxes [frames][nboxes] -- its own buffers: nothing of the per-item series above is shared
  double* sum_acc = nullptr;
  size_t sum_acc_bytes = 0;
  int sum_nx = 0, sum_ny = 0, sum_frames = 0;
  double sum_geom[4] = {0, 0, 0, 0};  // pitch_x, pitch_y, xc, yc
  bool sum_open = false;
  double* sum_par = nullptr;
  size_t sum_par_bytes = 0;
  double* sum_host = nullptr;
  size_t sum_host_bytes = 0;
  hipEvent_t sum_ev = nullptr;
  double* sum_flux = nullptr;
  size_t sum_flux_bytes = 0;
  void* bounce[2] = {nullptr, nullptr};  // pinned host buffers for device -> pageable host copies
  hipEvent_t bounce_ev[2] = {nullptr, nullptr};
  void* field = nullptr;
  void* tw = nullptr;
  void* staging = nullptr;  // n*n*16 bytes, row-major
  cx<double>* tables = nullptr;  // kMaxTables x batch x 2n separable phase factors
  double* mask = nullptr;        // batch x item_stride aperture weights (allocated on first use)
  double* metric_partial = nullptr;  // psf metrics scratch
  double* metric_out = nullptr;
  double* metric_host = nullptr;     // pinned
  // Line records of apertures riding on frugal passes: a few rendered sets are kept, keyed by everything the
  // renderer reads (the aperture's two parameter block sets, the pass axis, which items share records), so that a
  // chain whose relays repeat one aperture -- and the next wavefront batch through the same optics (a Monte-Carlo
  // study, a benchmark step) -- find their records instead of rendering them again (round 3: 6 renderings of
  // 0.3 ms per SYN20 step -> 0 in steady state).
  struct MaskSet {
    MaskLine* lines = nullptr;  // batch x n
    double* vals = nullptr;     // batch x n x 2 kMaskW partial weights
    std::vector<double> key;    // empty: holds nothing valid
    unsigned long long used = 0;
    int line_lo = 0, line_hi = 0;  // the lines whose records were rendered (the others hold whatever was there before)
  };
  static constexpr int kMaskSets = 8;  // (SYN20: five relay apertures whose pixel radii differ in the last digits + the field stop)
  MaskSet mask_sets[kMaskSets];
  unsigned long long mask_clock = 0;
  unsigned long long mask_hits = 0, mask_rendered = 0;  // paos_record_set_stats
  // experiment (tools/two_streams.py): extra dynamic LDS per pass workgroup of THIS context (PAOS_LDS_PAD when the
  // context is created): 6 KiB make two of its workgroups too big for one CU but leave room for one of another
  // context's -- two contexts then share every CU one workgroup each (measured: -14 %, profiles/r04_membench6_mixed_kinds.txt)
  size_t lds_pad = 0;
  // Round 11: launches whose first pass loads positions of the central half [n / 4, 3 n / 4) only take the central-half build
  // of their shape (frugal_pass.h: CH).  PAOS_CENTRAL_HALF=0 when the context is created switches it off -- read per
  // context, so that a test can hold an "on" and an "off" context in one process.  (On by default: profiles/r11_central_half.md.)
  bool central_half = true;
  unsigned long long central_launches = 0, plain_launches = 0;  // frugal pass launches on CH / ordinary builds (paos_central_half_stats)
  // Round 23: of the central-half launches, those whose first pass loads and whose last pass stores positions of
  // [5 n / 16, 11 n / 16) only take the narrow-window variant of the build (frugal_pass.h: CH = 2; pass_program.h: pick_narrow).
  // PAOS_NARROW_WINDOWS=0 / 1 when the context is created switches it off / on, like PAOS_CENTRAL_HALF.  (profiles/r23_narrow_windows.md)
  bool narrow_windows = true;
  unsigned long long narrow_launches = 0, other_launches = 0;  // frugal pass launches on the CH = 2 kernels / on any other (paos_narrow_window_stats)
  std::vector<int> pass_builds;  // the FrugalBuild of every frugal launch of the most recent pass program, nine ints each (paos_pass_builds)
  int* mask_overflow = nullptr;    // device counter: partial runs that did not fit (must stay 0)
  unsigned long long* block_stats = nullptr;  // device, three counters of the block renderer of ellipse records (paos_record_block_stats)
  double* partial = nullptr;
  double* norm2 = nullptr;
  double* norm2_host = nullptr;  // pinned, kNormSlots x batch
  bool prune = true;  // skip tiles / loads of lines an aperture has zeroed (paos_ctx_set_pruning)
  int norm_slot = 0;
  bool norm_busy[64] = {};       // ticket handed out and not fetched yet (kNormSlots entries)
  int nparts = 0;
  Arena arena;
  std::string err;
  // optional per-kernel-class timing with HIP events on the context's stream
  int prof_kind = -1;
  std::vector<hipEvent_t> prof_events;  // start/stop pairs
  std::vector<int> prof_tags;           // per pair: 1 = the launch skipped dead tiles / loads (pruned)
  int prof_next_tag = 0;
  double prof_next_bytes = 0.0;         // bytes the planner has the next timed launch load + store (its algorithmic bytes)
  std::vector<double> prof_bytes;       // per pair, like prof_tags
  double prof_next_lines = 0.0;         // 1-D line transforms the next timed launch runs (live lines x transforms that are on, over the batch)
  std::vector<double> prof_lines;       // per pair, like prof_tags
  size_t prof_used = 0;
};

// Everything declared from here on is internal to the library: none of it is exported.
#pragma GCC visibility push(hidden)

// ---- errors (context.hip): the text goes to the context and, for a call without one, to the calling thread -------
int fail(paos_ctx* c, int code, const std::string& msg);

#define HIPCHK(c, call)                                                                     \
  do {                                                                                      \
    hipError_t e_ = (call);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return fail((c), PAOS_EHIP,                                                           \
                  std::string(#call) + ": " + hipGetErrorString(e_) + " (" __FILE__ ":" +   \
                      std::to_string(__LINE__) + ")");                                      \
  } while (0)

inline size_t elem_bytes(const paos_ctx* c) { return c->precision == PAOS_F64 ? 16 : 8; }

// A switch of the environment: is the first character of `name` `ch`?  Flags that are read once keep the answer in a
// static of the one function that asks; the flags that tests switch (mask_render_mode, mask_rect_blocks,
// PAOS_FUSE_PAIRS, PAOS_STAGE_PROGRAM) ask at every call.
inline bool env_is(const char* name, char ch) {
  const char* e = getenv(name);
  return e && e[0] == ch;
}

// ---- FFT launch geometry per grid size ----------------------------------------------
// Row pass: LINES = BR rows per tile; column pass: LINES = BC columns per tile.
// E elements per thread; TILES tiles per workgroup keep small grids at >= 128 threads.
template <typename T, int N>
struct FftCfg {
  static constexpr int BC = Lay<T>::BC;
  static constexpr int BR = block_rows<T, N>();
  // 16 points per thread.  (32 points of complex64 fill the same 64 data VGPRs, but the
  // radix-32 butterflies spill: 256 VGPRs + 60-70 AGPRs measured, so E stays 16 for both types.)
  static constexpr int E = 16;
  // rows of a block row handled by one row tile: all four, except at N = 4096 where four
  // lines of 4096 points do not fit the register file of a spill-free workgroup
  static constexpr int ROW_LINES = (N >= 2048) ? PAOS_BR / 2 : PAOS_BR;  // 256-thread tiles at 2048 measured +29 %
  // the frugal kernels' row tile: half a block row -- 2 rows of complex128, 4 rows of complex64 at N >= 2048 (1024
  // threads at <= 64 VGPRs at 4096: two workgroups per CU either way)
  static constexpr int FR_ROW_LINES = (N >= 2048) ? BR / 2 : BR;
  static constexpr int COL_LINES = BC;
  static constexpr int ROW_THREADS = ROW_LINES * N / E, COL_THREADS = COL_LINES * N / E;
  static constexpr int ROW_TILES = (ROW_THREADS >= 128) ? 1 : 128 / ROW_THREADS;
  static constexpr int COL_TILES = (COL_THREADS >= 128) ? 1 : 128 / COL_THREADS;
  // Exchange whole complex numbers through LDS (two barriers per exchange) whenever the
  // tile fits; otherwise real and imaginary parts take turns in half the space.  Register
  // pressure (~230 VGPRs) already limits these kernels to 8 waves per CU, so using up to
  // 144 KiB of the 160 KiB LDS costs no occupancy (measured +3..7 %, profiles/r01_fftbench_v4).
  static constexpr bool ROW_SPLIT = (size_t)ROW_LINES * ROW_TILES * line_lds_bytes<T, N, false>() > 144 * 1024;
  static constexpr bool COL_SPLIT = (size_t)COL_LINES * COL_TILES * line_lds_bytes<T, N, false>() > 144 * 1024;
  static constexpr int MINW = 1;
};
// lines per workgroup of the frugal kernels' ordinary tiles along `axis` for the context's grid: FftCfg's FR_ROW_LINES /
// COL_LINES at run time (what the per-workgroup sums of a PSF- or power-storing pass are laid out by)
inline int frugal_tile_lines(const paos_ctx* c, int axis) { return axis == 0 ? (c->n >= 2048 ? c->br / 2 : c->br) : 2; }

// ---- context.hip ---------------------------------------------------------------------------------------------
// the parameter arena: make room for `total` doubles that must all stay live / copy `count` doubles, *dev: where they are
int arena_reserve(paos_ctx* c, size_t total);
int arena_push(paos_ctx* c, const double* src, size_t count, const double** dev);  // one block: add + commit
// Several blocks, one copy: begin(total) makes room for all of them in ONE slab (arena_reserve: grow, or switch, before the
// first block), add() writes a block to the pinned slab and says at once where it will be on the device, commit() copies
// everything added and not copied yet -- [first block, head) -- in one transfer.  The device pointers may go to kernels
// launched BEHIND commit() only: a launch in front of it reads whatever the slab held four switches ago.  So a batch is
// closed by its commit (a later add is refused), and an entry point that ends well with blocks still pending fails
// (arena_settled).  Without begin() a block that does not fit the slab commits what is pending and switches, like arena_push.
class ArenaBatch {
 public:
  explicit ArenaBatch(paos_ctx* c) : c_(c) {}
  int begin(size_t total);
  int add(const double* src, size_t count, const double** dev);
  int commit();

 private:
  paos_ctx* c_;
  ArenaBatchState st_;
};
// the last thing an entry point that adds blocks does with its result: an error drops what is still pending (never copied;
// the head stays advanced), PAOS_OK with blocks pending becomes a failure
int arena_settled(paos_ctx* c, int rc);
int copy_to_host(paos_ctx* c, void* host, const void* dev, size_t bytes);  // device -> pageable host; synchronises
int next_norm_slot(paos_ctx* c);                                           // the next free slot of the power-ticket ring
int check_mask_overflow(paos_ctx* c);  // after a synchronisation: did an aperture's partial run overflow its line records?
int check_rows(paos_ctx* c, const double* rows);                           // [batch][2] windows: 0 <= lo <= hi <= n
std::vector<double> rounded_cols(const paos_ctx* c, const double* cols);   // column windows in whole block heights
int opt_in_lds(paos_ctx* c, const void* kern, size_t lds);  // more than 64 KiB of dynamic LDS: once per device and kernel
bool timed_launch_begin(paos_ctx* c, int kind);             // the launch timer (paos_profile_begin)
hipError_t timed_launch_end(paos_ctx* c, int tag);

// Opt in to `lds_opt_in` bytes of dynamic LDS (0: the kernel needs no opt-in), arm the launch timer, launch, check, stop
// the timer under `tag`.  The caller has set c->prof_next_bytes / prof_next_lines.  TIMED_LAUNCH(c, kern, ...): a failed
// launch is reported with the launcher's file and line, like every HIPCHK.
int launch_failed(paos_ctx* c, const char* call, hipError_t e, const char* file, int line);
#define TIMED_LAUNCH(c, ...) timed_launch(__FILE__, __LINE__, (c), __VA_ARGS__)
template <typename Kern, typename... Args>
int timed_launch(const char* file, int line, paos_ctx* c, Kern kern, dim3 grid, dim3 block, size_t lds, size_t lds_opt_in, int kind,
                 int tag, Args... args) {
  if (lds_opt_in) {
    int rc = opt_in_lds(c, (const void*)kern, lds_opt_in);
    if (rc) return rc;
  }
  const bool timed = timed_launch_begin(c, kind);
  hipLaunchKernelGGL(kern, grid, block, lds, c->stream, args...);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return launch_failed(c, "hipGetLastError()", e, file, line);
  if (timed && (e = timed_launch_end(c, tag)) != hipSuccess) return launch_failed(c, "timed_launch_end(c, tag)", e, file, line);
  return PAOS_OK;
}
// the pass kernels on the generic tile shapes (FftCfg) opt in above the 48 KiB every kernel may use
inline size_t generic_lds_opt_in(size_t lds) { return lds > 48 * 1024 ? lds : 0; }

// f(std::integral_constant<int, N>) for the context's grid size N: the one place that knows the sizes of FftCfg
template <typename F>
int dispatch_n(paos_ctx* c, F&& f) {
  switch (c->n) {
#define PAOS_N_CASE(N) case N: return f(std::integral_constant<int, N>{})
    PAOS_N_CASE(64);
    PAOS_N_CASE(128);
    PAOS_N_CASE(256);
    PAOS_N_CASE(512);
    PAOS_N_CASE(1024);
    PAOS_N_CASE(2048);
    PAOS_N_CASE(4096);
#undef PAOS_N_CASE
  }
  return fail(c, PAOS_EUNSUPPORTED, "grid size must be a power of two in 64..4096");
}

// f(std::integral_constant<int, BRV>) for the context's block height BRV (PAOS_F32_BR or PAOS_BR): the launches whose
// element type does not matter (pupil weights, Gram sums)
template <typename F>
auto dispatch_block_rows(const paos_ctx* c, F&& f) {
  if (c->br == PAOS_F32_BR) return f(std::integral_constant<int, PAOS_F32_BR>{});
  return f(std::integral_constant<int, PAOS_BR>{});
}
// f(T{}, std::integral_constant<int, BRV>) for the context's element type and block height: the one place that knows the
// layouts -- (double, PAOS_BR), (float, PAOS_F32_BR) and (float, PAOS_BR), no other pair is ever instantiated.  Returns what
// f returns; a HIPCHK inside f returns from f, so a caller that uses one hands the value on.
template <typename F>
auto dispatch_layout(const paos_ctx* c, F&& f) {
  if (c->precision == PAOS_F64) return f(double{}, std::integral_constant<int, PAOS_BR>{});
  return dispatch_block_rows(c, [&](auto br) { return f(float{}, br); });
}
// f(std::integral_constant<int, A>) if `first`, else f(std::integral_constant<int, B>): a two-way template argument
// (aperture shape 0 / 1, the unrolled Zernike build 8 / 0)
template <int A, int B, typename F>
auto dispatch_either(bool first, F&& f) {
  if (first) return f(std::integral_constant<int, A>{});
  return f(std::integral_constant<int, B>{});
}

// ---- passes.hip ----------------------------------------------------------------------------------------------------
// final_mode (with final_ticket): 1 = the PSF instead of the field, 2 = the field as usual plus the ticket of its power
int run_passes(paos_ctx* c, const paos_pass* passes, int n_passes, const double* blocks, int n_blocks,
               const double* entry_rows = nullptr, bool entry_stale = false, int* final_ticket = nullptr, int final_mode = 1,
               const double* entry_cols = nullptr);
int mask_render_mode();    // how ellipse / rectangle line records are rendered (read per call: tests switch them)
bool mask_rect_blocks();

// ---- generic_pass.hip: one pass on the generic kernel (fft_kernels.h), any grid size; feat != 0: the build with the
// optional operators (phase tables, aperture weight maps) ----
int generic_pass(paos_ctx* c, int axis, const PassArgs& a, int feat);

// ---- frugal_<family>.hip: the pass-kernel builds of one (type, N) family behind one ordinary function each ----
// (the record that names a build, FrugalBuild, and the list of the families, dispatch_family: pass_records.h)
// narrow: a central-half build launches its narrow-window variant (pass_program.h: Launch::narrow)
template <typename T, int N>
int frugal_family(paos_ctx* c, const FrugalBuild& b, const FrugalArgs& a, bool narrow);

// ---- paos_hip.hip: the one unit that includes pointwise.h (its non-template kernels can be compiled once only), so
// whatever another unit needs of that header's kernels is launched through these ----
// the deferred stop scale (paos_stop_defer_last_power): apply it to the field now (unless that is about to be
// overwritten) / the first pass of a program has taken it along: ones again
int settle_scale(paos_ctx* c, bool field_is_overwritten = false);
int dyn_scale_reset(paos_ctx* c);
int zero_outside_rows(paos_ctx* c, const double* live_rows);
int zero_outside_box(paos_ctx* c, const double* live_rows, const double* live_cols);
// the ring of power tickets: refuse while its next slot is still out (before anything is launched) / partial sums -> c->norm2
// (item i: the sums of item source[i], if given) -> the pinned slot of a new ticket
int power_ring_full(paos_ctx* c);
int take_power_ticket(paos_ctx* c, const double* partial, int nparts, const double* source, int* ticket);
int psf_keep_power_impl(paos_ctx* c, int* ticket);
// aperture line records (pointwise.h: MaskJob): render the lines [line0, line_end) along `axis` of the aperture whose two
// parameter block sets start at `params` into record set `set`; at most kMaskRenders of them, in one launch per shape
struct MaskRender {
  const double *params, *shared;
  int set, axis, line0, line_end, shapes;
};
constexpr int kMaskRenders = 8;
int render_mask_records(paos_ctx* c, const MaskRender* jobs, int count);
// the operators of a pass on the generic kernels: the weight map of its aperture into c->mask / a transform-free pass
int render_mask_weights(paos_ctx* c, const double* ap);
int pointwise_pass(paos_ctx* c, const PassArgs& a);

#define SETTLE_SCALE(c) do { if (c) { (c)->norm2_of_field = false; if ((c)->dyn_pending) { int rc_ = settle_scale(c); if (rc_) return rc_; } } } while (0)
#define DROP_SCALE(c) do { if (c) { (c)->norm2_of_field = false; if ((c)->dyn_pending) { int rc_ = settle_scale(c, true); if (rc_) return rc_; } } } while (0)

#pragma GCC visibility pop
