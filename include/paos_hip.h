/* paos_hip.h -- C ABI of libpaoship.so, the MI355X (gfx950) wavefront-propagation core.
 *
 * The reference (arielmission-space/PAOS v1.2.12) is pure Python and has no FFI;
 * the boundary this library replaces is the field arithmetic inside the methods of
 * paos.classes.wfo.WFO (paos/classes/wfo.py) as driven by paos.core.run.run
 * (paos/core/run.py:30-228).  Each entry point below names the reference lines it
 * stands in for.  The scalar "pilot Gaussian beam" bookkeeping of those methods
 * stays on the host (paos_amd/planner.py); only N x N field work crosses this ABI.
 *
 * Conventions
 *   - every function returns 0 on success, a PAOS_E* code otherwise;
 *     paos_last_error(ctx) gives the message (ctx may be NULL for create errors);
 *   - a context owns `batch` fields of n x n complex numbers (double or float) in
 *     HBM, one HIP stream, and all scratch; calls are enqueued on that stream and
 *     return without waiting unless they hand data to the host;
 *   - per-item parameter blocks are plain `double` arrays, `batch` blocks long,
 *     borrowed for the duration of the call; block[0] is an enable flag (0 = leave
 *     that batch item untouched) so that one launch serves wavelengths / Monte-Carlo
 *     draws whose planners disagree on whether a step runs;
 *   - host field buffers are row-major [y][x] complex128, like WFO._wfo;
 *   - contexts are not thread-safe; different contexts are independent.
 */
#ifndef PAOS_HIP_H
#define PAOS_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct paos_ctx paos_ctx;

enum { PAOS_OK = 0, PAOS_EINVAL = 1, PAOS_EHIP = 2, PAOS_EUNSUPPORTED = 3 };
enum { PAOS_F64 = 0, PAOS_F32 = 1 };
enum { PAOS_SHAPE_ELLIPSE = 0, PAOS_SHAPE_RECT = 1 };
enum { PAOS_KERNEL_PASS_ROWS = 0, PAOS_KERNEL_PASS_COLS = 1, PAOS_KERNEL_PASS_ANY = 2 };
/* pointwise operators that ride on an FFT pass (paos_run_passes) */
enum { PAOS_PW_SIGN = 1, PAOS_PW_QPHASE_CENTRED = 2, PAOS_PW_QPHASE_NATURAL = 3, PAOS_PW_SCALE = 4,
       PAOS_PW_MASK = 5 };
enum { PAOS_PWF_MUL2PI = 1,
       /* PAOS_PW_SIGN only (round 4, the separable pass programs): (-1)^column, resp. (-1)^row, instead of the
          checkerboard (-1)^(row + column) -- the two factors the checkerboard of wfo.py:491-545 splits into */
       PAOS_PWF_X_ONLY = 2, PAOS_PWF_Y_ONLY = 4 };
enum { PAOS_MAX_PW = 6 };
enum { PAOS_NORM_SLOTS = 64 };  /* outstanding paos_norm2_enqueue tickets */
enum { PAOS_WHAT_FIELD = 0, PAOS_WHAT_AMPLITUDE = 1, PAOS_WHAT_PHASE = 2, PAOS_WHAT_INTENSITY = 3 };

/* parameter-block layouts (doubles per batch item) */
enum { PAOS_PHASE_STRIDE = 5 };    /* enable, sx, sy, coef, sgn                         */
enum { PAOS_APERTURE_STRIDE = 8 }; /* enable, xc, yc, a|w, b|h, theta, obscuration, subpixels */
enum { PAOS_ZERNIKE_HEAD = 8 };    /* enable, dx, dy, radius, origin_is_y, cos_off, sin_off, 1/wl;
                                      then coefC[(nmax+1)*kdim], coefS[(nmax+1)*kdim]           */

/* One HBM pass over every field of the batch:
 *   load -> pre operators -> [1-D FFTs along `axis`] -> mid operators -> [1-D FFTs] -> post -> store.
 * `block` / `fft1` / `fft2` index parameter block sets of PAOS_PHASE_STRIDE doubles per batch
 * item: operators read [enable, sx, sy, coef, sgn] (SIGN uses enable only, SCALE multiplies by
 * coef); a transform control block reads [enable, inverse].  MASK (WFO.aperture, wfo.py:236-276,
 * riding on a pass) reads two consecutive block sets: `block` = [enable, xc, yc, a|w, b|h] and
 * `block`+1 = [theta, obscuration, subpixels, shape, 0]; at most one MASK per pass.  axis = -1: no transform, the operators of `pre` are applied in a stand-alone pass. */
typedef struct { int kind, flags, block; } paos_pw_op;
typedef struct {
  int axis;                    /* 0 = along rows, 1 = along columns, -1 = no transform */
  int fft1, fft2;              /* control block index, or -1 for "no transform here"  */
  int n_pre, n_mid, n_post;
  paos_pw_op pre[PAOS_MAX_PW], mid[PAOS_MAX_PW], post[PAOS_MAX_PW];
} paos_pass;

/* Options of paos_run_program (round 3); a NULL pointer or all zeros = paos_run_passes.
 *   live_rows      [batch][2] or NULL: on entry the rows of item i outside [lo, hi) are zero (see
 *                  paos_run_passes_live) ...
 *   rows_stale     != 0: ... or rather, they hold old data that STANDS for zeros (what paos_start_rows leaves):
 *                  no pass reads them; the program consumes them (a pass along columns rewrites the whole field) or,
 *                  where it cannot, writes the zeros itself before it ends.
 *   final_intensity  != 0: the caller wants |u|^2 (the PSF, plot.py:125-130) and its sum of the field the program
 *                  ends with, not the field: the last pass stores |u|^2 into the context's PSF buffer (as
 *                  paos_psf_keep_power would afterwards) and *power_ticket receives a ticket for paos_norm2_fetch.
 *                  The field content is UNDEFINED after the call.  (Saves writing the last field and reading it
 *                  back: 32 B/px.)
 *                  == 2 (round 4): the field is stored as usual AND *power_ticket receives the ticket of its
 *                  sum |u|^2 -- the power a caller reports next to a saved surface (push_results, run.py:12-27,
 *                  218-223) -- summed by the last pass while it stores its tiles instead of by a separate sweep
 *                  that reads the field back (16 B/px). */
typedef struct {
  const double* live_rows;
  int rows_stale;
  int final_intensity;
  int* power_ticket;
  /* round 5: [batch][2] or NULL -- with rows_stale, columns outside [lo, hi) of the live rows hold old data that stands
   * for zeros as well (what paos_start_box leaves: the first field is written inside the aperture's box only). */
  const double* live_cols;
} paos_program_opts;

/* ---- lifetime -------------------------------------------------------------------- */
/* WFO.__init__ (wfo.py:99-120): allocates `batch` n x n fields (n = 2^k, 64..4096).
 * The field content is undefined until paos_fill / paos_import. */
int paos_ctx_create(int device, int n, int batch, int precision, paos_ctx** out);
int paos_ctx_destroy(paos_ctx* ctx);
const char* paos_last_error(const paos_ctx* ctx);
int paos_sync(paos_ctx* ctx);
/* describe the build: gfx arch, layout block, pitch padding (for logs) */
const char* paos_build_info(void);
/* round 5: the first 32 hex digits of sha256 over the library's sources as they were when it was built (__graft_entry__.source_hash():
 * every source and header of the library, sorted by name) -- __graft_entry__.build() compares it with the tree and rebuilds on a mismatch, so a prebuilt library that
 * travelled with a tree it was not built from is noticed */
const char* paos_source_hash(void);
/* the HIP stream handle (hipStream_t) of the context, for event timing */
void* paos_stream(paos_ctx* ctx);

/* Measurement aid (no reference counterpart): time every launch of one kernel class with
 * HIP events on the context's stream between begin and end; end synchronises and returns
 * the launch count and the summed durations.  Used by bench.py for the roofline figure. */
int paos_profile_begin(paos_ctx* ctx, int kernel_kind, int max_launches);
int paos_profile_end(paos_ctx* ctx, int* launches, double* total_ms);
/* the same, also telling apart the launches that skipped dead tiles or loads (pruned passes move fewer
 * bytes, so a bandwidth figure must be taken over the others) */
int paos_profile_end_split(paos_ctx* ctx, int* launches, double* total_ms, int* pruned_launches, double* pruned_ms);
/* the same launch by launch, in launch order: ms_out[i], tag_out[i] (bit 0: the launch skipped whole tiles of dead
 * lines, bit 1: loads of dead positions, bit 2: stores nobody reads, bit 3: it stored the PSF instead of the
 * field, bits 4 / 5 (round 4): the launch ran two / three consecutive passes of the program; 0 = a full pass); *count
 * launches, at most `capacity` */
int paos_profile_end_launches(paos_ctx* ctx, int capacity, double* ms_out, int* tag_out, int* count);
/* round 4: the bytes the pruning plan had each launch timed so far load + store (live lines x (loaded + stored positions)
 * x element size, summed over the batch items): the launch's algorithmic bytes.  Call before paos_profile_end_*. */
int paos_profile_planned_bytes(paos_ctx* ctx, int capacity, double* bytes_out, int* count);
/* round 5: the 1-D line transforms each launch timed so far ran (live lines x the transforms switched on for the item,
 * over every pass the launch carries and every batch item): x 5 N log2 N = the launch's nominal flops, what bench.py
 * prices the fused launches with -- they move a sixteenth of the grid and are bound by fp64 issue, not by bytes.
 * Call before paos_profile_end_*. */
int paos_profile_line_transforms(paos_ctx* ctx, int capacity, double* lines_out, int* count);

/* ---- field I/O ---------------------------------------------------------------------- */
/* u[:] = re + i im for every batch item -- np.ones(..., complex128), wfo.py:118 */
int paos_fill(paos_ctx* ctx, double re, double im);
/* The first surface in one go: u = re + i im (wfo.py:118), u *= aperture weight (wfo.py:236-276),
 * and, for items with stop[i] != 0, u /= sqrt(sum |u|^2) (wfo.py:195-201) -- what paos_fill,
 * paos_aperture and paos_make_stop do one after the other, with the same roundings, but the power
 * is summed from the weights alone and the field is written once (16 B/px instead of ~72).
 * aperture: [batch][PAOS_APERTURE_STRIDE] (enable = 0: no aperture on that item); stop may be NULL. */
int paos_start(paos_ctx* ctx, double re, double im, int shape, const double* aperture, const double* stop);
/* paos_start that writes only the rows [write_rows[2 i], write_rows[2 i + 1]) of item i (rounded outward to
 * whole blocks of rows; they must contain every row the aperture leaves non-zero).  The other rows keep whatever
 * they held and merely STAND for the zeros wfo.py:273-276 would have put there: until a pass program has
 * consumed them (paos_run_program with rows_stale) only paos_zernike, paos_norm2_enqueue_rows and
 * paos_zero_outside_rows may touch the field.  Saves three quarters of the first field write at zoom 4. */
int paos_start_rows(paos_ctx* ctx, double re, double im, int shape, const double* aperture, const double* stop,
                    const double* write_rows);
/* make such rows real zeros (whole blocks of rows outside [lo, hi) of every item are cleared) */
int paos_zero_outside_rows(paos_ctx* ctx, const double* live_rows);
/* Round 5: paos_start_rows that also leaves the COLUMNS outside [write_cols[2 i], write_cols[2 i + 1]) (rounded outward to
 * whole blocks) of the written rows alone -- the field is stored inside the aperture's bounding box only, a sixteenth of the
 * grid at zoom 4 instead of a quarter (wfo.py:118 -> :236-276 -> :195-201).  Until a pass program has consumed the box
 * (paos_run_program with rows_stale and live_cols) only paos_zernike, paos_norm2_enqueue_box and paos_zero_outside_box may
 * touch the field. */
int paos_start_box(paos_ctx* ctx, double re, double im, int shape, const double* aperture, const double* stop,
                   const double* write_rows, const double* write_cols);
/* paos_start_box and the Zernike surface right behind it (paos_zernike's nmax, kdim, table, params, param_stride) in ONE write
 * of the field: what the two calls leave inside the box, bit for bit -- the weight is evaluated once per group of items with
 * one start field, the polynomials once per group of items with one wfe map inside it -- without storing the start field and
 * reading it back.  For callers that let nothing read the field between the two surfaces.  power_ticket (may be NULL): the
 * power of the start field itself, summed from the weights exactly as paos_norm2_enqueue_box(write_rows, write_cols, same_as
 * = items with one start field) would sum it from memory -- a saved first surface reports it. */
int paos_start_zernike_box(paos_ctx* ctx, double re, double im, int shape, const double* aperture, const double* stop,
                           const double* write_rows, const double* write_cols, int nmax, int kdim, const double* table,
                           const double* params, int param_stride, int* power_ticket);
/* make everything outside the box rows x cols of every item real zeros (live_cols may be NULL: whole rows) */
int paos_zero_outside_box(paos_ctx* ctx, const double* live_rows, const double* live_cols);
/* host row-major complex128 -> batch item (WFO._wfo assignment in notebooks/tests) */
int paos_import(paos_ctx* ctx, int item, const void* host_c128);
/* batch item -> host.  what = FIELD: complex128 copy (wfo.py:162-164); AMPLITUDE: |u|
 * (wfo.py:166-168); PHASE: angle(u) (wfo.py:170-172); INTENSITY: |u|^2 = the PSF
 * definition of paos/core/plot.py:125-130.  Synchronises. */
int paos_export(paos_ctx* ctx, int item, int what, void* host_out);

/* PSF = |u|^2 (plot.py:125-130) of EVERY batch item written to a device buffer and kept there
 * (doubles, laid out like the field; paos_psf_fetch hands out row-major arrays): the final intensity write of a propagation whose results are consumed on
 * the GPU or fetched later.  paos_psf_fetch copies one item's PSF to the host (synchronises). */
int paos_psf_keep(paos_ctx* ctx);
/* paos_psf_keep and paos_norm2_enqueue of the same field in one sweep (the saved last surface of a chain:
 * |u|^2 is written and summed while the field is read once); *ticket as paos_norm2_enqueue, the sum is
 * bit-identical to it. */
int paos_psf_keep_power(paos_ctx* ctx, int* ticket);
int paos_psf_fetch(paos_ctx* ctx, int item, double* host_out);
/* Page-locked host memory for results (no reference counterpart).  paos_export into pageable
 * memory is bounded by first-touch page faults and on-the-fly pinning (~3 GB/s); into a buffer from
 * paos_host_alloc it is one DMA.  paos_export_pinned requires such a buffer. */
int paos_host_alloc(unsigned long long bytes, void** out);
int paos_host_free(void* p);
int paos_export_pinned(paos_ctx* ctx, int item, int what, void* pinned_out);

/* ---- operators ------------------------------------------------------------------------ */
/* WFO.aperture (wfo.py:203-278): multiply by the exact ellipse mask
 * (EllipticalAperture.to_mask("exact")) or the 32x32 sub-pixel rectangle mask
 * (RectangularAperture.to_mask("subpixel", subpixels=32)); obscuration uses 1 - mask. */
int paos_aperture(paos_ctx* ctx, int shape, const double* params);
/* the mask alone, row-major doubles, for the aperture object's
 * .to_mask(...).to_image(shape) used at run.py:136-141, plot.py:164-184 */
int paos_aperture_render(paos_ctx* ctx, int shape, const double* params1, double* host_mask);
/* WFO.make_stop (wfo.py:195-201): u /= sqrt(sum |u|^2), per enabled item.
 * enable may be NULL (= all). */
int paos_make_stop(paos_ctx* ctx, const double* enable);
/* make_stop (wfo.py:195-201) for a field whose power the context has JUST reduced: the pass program that stored the
 * field ended with final_intensity = 2 (paos_run_program) and nothing has run on the context since.  Only the scaling
 * sweep u *= 1/sqrt(power) is launched -- the reduction that would read the field back has already been done by the
 * pass that stored it.  Round 5: the context checks the precondition itself -- a flag set by such a program and cleared by
 * every entry point that reads or rewrites the field or reduces a power (including this one and the next: behind a stop
 * the reduced power no longer is the field's); when it is clear, both functions run paos_make_stop (same result, one
 * reduction more). */
int paos_stop_scale_last_power(paos_ctx* ctx, const double* enable);
/* The same stop, with even the scaling sweep left out: 1 / sqrt(power) is kept per item on the device and the NEXT pass
 * program's first pass multiplies it into its middle slot (one more factor in a multiplication it performs anyway), so
 * the stop costs neither a read nor a write of the field.  Anything else that touches the field first -- a download, a
 * reduction, an aperture, another stop, a pass program whose first pass cannot take it (generic kernel, an item that
 * sits it out) -- applies it then, by the sweep paos_stop_scale_last_power would have run: same factor, same products,
 * bit-identical.  Same precondition as above. */
int paos_stop_defer_last_power(paos_ctx* ctx, const double* enable);
/* sum |u|^2 per item to the host (np.sum(np.abs(u)**2), wfo.py:200).  Synchronises. */
int paos_norm2(paos_ctx* ctx, double* host_out);
/* The same without stalling the host: enqueue the reduction and its copy to pinned memory,
 * get a ticket, fetch later (the fetch synchronises).  At most PAOS_NORM_SLOTS tickets may be
 * outstanding: one more paos_norm2_enqueue fails with PAOS_EINVAL until a ticket is fetched, and
 * a ticket can be fetched once. */
int paos_norm2_enqueue(paos_ctx* ctx, int* ticket);
/* paos_norm2_enqueue that reads only the rows [lo, hi) of each item: the caller knows the others to be zero
 * (or to stand for zeros, paos_start_rows).  Bit-identical to the full sum of the zero-filled field. */
int paos_norm2_enqueue_rows(paos_ctx* ctx, const double* live_rows, int* ticket);
/* ... and that sums only once what the caller knows to be copies: same_as[i] (a double holding an index) names the
 * item whose field equals item i's (itself for the first of a group; items of a group share their row window) --
 * the wavelengths of a sweep right behind paos_start_rows, whose aperture records agree (wfo.py:195-201 at the
 * entrance pupil does not depend on the wavelength).  Every item gets its leader's sum. */
int paos_norm2_enqueue_rows_like(paos_ctx* ctx, const double* live_rows, const double* same_as, int* ticket);
/* round 5: the same sum over the box rows x cols (live_cols: [batch][2]; same_as may be NULL) -- elements outside are zero
 * or stand for zeros and are not read; bit-identical to the full sum of the zero-filled field. */
int paos_norm2_enqueue_box(paos_ctx* ctx, const double* live_rows, const double* live_cols, const double* same_as, int* ticket);
int paos_norm2_fetch(paos_ctx* ctx, int ticket, double* host_out);
/* give a ticket back without reading it (no synchronisation) */
int paos_norm2_release(paos_ctx* ctx, int ticket);
/* PSF metrics on the GPU for Monte-Carlo studies (the encircled-energy workflow of
 * docs/source/user/montecarlo/index.rst:26-66; PSF = |u|^2, plot.py:125-130).  Per item:
 * [sum I, sum I*col, sum I*row, max I, then nr values: sum of I over pixels whose centre lies
 * within radii_px[k] of (cx_px, cy_px)], nr <= 16.  host_out: [batch][4 + nr].  Radii finite and >= 0, centre
 * finite -- otherwise PAOS_EINVAL.  Synchronises. */
int paos_psf_metrics(paos_ctx* ctx, int nr, const double* radii_px, double cx_px, double cy_px,
                     double* host_out);
/* quadratic phase u *= exp(i sgn [2 pi] coef ((x sx)^2 + (y sy)^2)), x, y centred pixel
 * indices: the field part of WFO.lens (wfo.py:359-366) with mul2pi = 1, sgn = -1,
 * coef = 0.5 lens_phase / wl. */
int paos_phase(paos_ctx* ctx, const double* params, int mul2pi);
/* Tabulated phase screen, the field part of WFO.grid_sag (wfo.py:869-871) and WFO.psd
 * (wfo.py:945-949): u[item] *= exp(2 pi i wfe / wl) with wfe a host map in metres (row-major
 * n x n doubles, finite: masked pixels filled with 0 as the reference does).  The resampling of a
 * sag map and the random draw of a PSD screen stay on the host (paos_amd/wfo.py).  Synchronises.
 * PAOS_EINVAL, the field untouched, also for a finite map whose argument is not: the kernel forms fl(fl(2 pi w) / wl), and
 * the map's largest |w| must leave that finite (|w| near 1e308, or any w over a tiny wl, would put NaN into the field). */
int paos_phase_map(paos_ctx* ctx, int item, const double* host_wfe, double wl);
/* Round 5: the same for `n_items` items that share ONE map (a measured surface map is the same for every wavelength of a
 * sweep and every draw of a Monte-Carlo study): items[k] (indices, as doubles) get u *= exp(2 pi i wfe / wl[k]).  The map
 * crosses PCIe once and stays on the device; `key` != 0 names its content: a later call with the same key skips the
 * validation and the upload (the caller vouches that the host buffer still holds what was uploaded under that key;
 * 0 = always upload).  `host_wfe` may be NULL when a map is kept under `key` (paos_psd_screen).  Does not synchronise when
 * the key matches.  PAOS_EINVAL, the field untouched: an item listed twice (two slices of the launch would update one field
 * in no order), and a wavelength at which fl(fl(2 pi max|wfe|) / wl) is not finite -- max|wfe| is kept with the map, so a
 * later call under the same key with a smaller wavelength is held to it as well. */
int paos_phase_map_items(paos_ctx* ctx, const double* host_wfe, unsigned long long key, int n_items, const double* items,
                         const double* wl);
/* Round 5: the random screen of WFO.psd built ON THE DEVICE (wfo.py:908-943 calling psd.py:100-160): the host draws the
 * white noise -- `host_noise`, then `host_rough` (n x n doubles each; NumPy's generator is the reference's, so a seeded run
 * stays comparable) -- and the library runs  fft2(noise) * sqrt(A / (B + (rho / fknee)^C) / (2 pi rho) * cell) * gain,
 * zero outside [fmin, fmax]  ->  ifft2  ->  (Re + SR * rough) * 2 * unit  on its own passes, in the reference's order of
 * operations.  params[12] = {1 / (n dx), 1 / (n dy), A, B, C, fknee, fmin, fmax, cell, gain = sqrt(n0 n1), SR, unit}.
 * The map stays on the device under `key` (!= 0): paos_phase_map_items(ctx, NULL, key, ...) applies it; `host_out`
 * (n x n doubles or NULL) receives a copy (the `wfe` entry the reference returns).  complex128 contexts only.
 * Synchronises.  Host restatement, and the bit-exact reference for the fixtures: paos_amd/phase_maps.py psd_map. */
int paos_psd_screen(paos_ctx* ctx, const double* host_noise, const double* host_rough, const double* params,
                    unsigned long long key, double* host_out);
/* WFO.ptp (wfo.py:462-472): ifft2(exp(-i coef (fx^2+fy^2)) fft2(u)), ortho norms, shifts
 * cancelled; sx, sy = 1/(n dx), 1/(n dy) (np.fft.fftfreq spacing), coef = pi wl dz. */
int paos_ptp(paos_ctx* ctx, const double* params);
/* WFO.stw (wfo.py:491-509): fftshift(exp(+i coef f^2) FFT(ifftshift u)); inverse != 0
 * selects ifft2 (dz < 0).  sx, sy, coef as for ptp. */
int paos_stw(paos_ctx* ctx, const double* params, int inverse);
/* WFO.wts (wfo.py:528-545): fftshift(FFT(ifftshift(exp(i coef (x^2+y^2)) u))); sx, sy =
 * dx, dy; coef = pi / (dz wl). */
int paos_wts(paos_ctx* ctx, const double* params, int inverse);
/* ---- through-focus stacks (README.md, "Through-focus stacks") --------------------------------------------------------- */
/* WFO.ptp (wfo.py:445-472) from ONE field to MANY defocus planes: u(dz) = ifft2(exp(-i coef (fx^2 + fy^2)) fft2(u)),
 * ortho norms, shifts cancelled (wfo.py:462-472), with the forward transform done once and kept.  The reference's own
 * precondition holds -- the wavefront is planar, C == 0 (wfo.py:458-460) -- and is the caller's to check
 * (paos_amd/run.py), like the scalars of every other operator.
 *
 * paos_focus_begin: allocates, on first use, one more batch-sized complex buffer (the context's precision, the field's
 * layout; freed by paos_focus_end and paos_ctx_destroy) and writes fft2 of every item's field into it: a pass along rows
 * that reads the field and writes the buffer, then a pass along columns in place on the buffer.  The field is read, not
 * modified (a pending deferred stop factor, paos_stop_defer_last_power, is applied first, as by every other reader of the
 * field); it must be the complete field: rows and columns that merely stand for zeros (paos_start_rows / paos_start_box)
 * have to be consumed by a pass program or made zeros (paos_zero_outside_box) before.  Enqueues only.
 * PAOS_EINVAL when a stack is already open. */
int paos_focus_begin(paos_ctx* ctx);
/* The context's field <- u(dz) of every item, built from the kept spectrum: a pass along columns that reads the spectrum,
 * applies the transfer function and the inverse transform and writes the field, then the inverse pass along rows in place
 * on the field -- half the line transforms of paos_ptp, and no copy to restore the field.  params:
 * [batch][PAOS_PHASE_STRIDE] = enable, sx, sy, coef, sgn as for paos_ptp (sx, sy = 1/(n dx), 1/(n dy), coef = pi wl dz,
 * sgn = -1); enable = 0: no transfer function on that item (it receives its field back, up to the rounding of the two
 * transforms).  Afterwards every entry point that reads the field works on the plane (paos_psf_keep[_power],
 * paos_psf_metrics, paos_export*, paos_norm2*, paos_detector_* through the kept PSF); what the context knew about the
 * field before (a power reduced on the way out of a pass program, a deferred stop) is dropped.  Any number of calls
 * after one paos_focus_begin, in any order of dz: a plane does not depend on the planes computed before it.  Enqueues
 * only.  PAOS_EINVAL without an open stack or for a parameter that is not finite (the context stays usable). */
int paos_focus_plane(paos_ctx* ctx, const double* params);
/* Releases the spectrum (waits for the planes enqueued so far).  The field keeps the last plane.  PAOS_EINVAL without
 * an open stack. */
int paos_focus_end(paos_ctx* ctx);
/* ---- transfer functions: OTF / MTF of the kept PSFs (README.md, "Transfer functions") ---------------------------------- */
/* No reference counterpart: the reference hands out PSFs and leaves their transforms to the user.  With P_i[k][j] the kept
 * PSF of item i (paos_psf_keep, paos_psf_keep_power or a pass program with final_intensity; rows k along y, grid centre at
 * pixel N/2):
 *   S_i[ky][kx]   = sum_k sum_j P_i[k][j] exp(-2 pi i ((j - N/2)(kx - N/2) + (k - N/2)(ky - N/2)) / N)
 *   OTF_i[ky][kx] = S_i[ky][kx] / S_i[N/2][N/2],   MTF_i = |OTF_i|
 * = fftshift(fft2(ifftshift(P_i))) over its zero-frequency value, zero frequency at pixel [N/2][N/2]; pixel [ky][kx] is the
 * spatial frequency ((kx - N/2) / (N dx_i), (ky - N/2) / (N dy_i)) in cycles per metre.  The PSF is real, so two of its rows
 * are packed into one complex line and only the columns 0 .. N/2 of the spectrum are transformed a second time: about N line
 * transforms per item where a complex 2-D transform runs 2 N (csrc/otf_pass.h).  The other half is handed out as the exact
 * conjugate mirror: the arrays are Hermitian, and the MTF point-symmetric, bit for bit.  OTF[N/2][N/2] is exactly 1 + 0 i;
 * an item whose PSF sums to zero gets zeros (scale = DC != 0 ? 1 / DC : 0), not NaN.  The transforms run in the context's
 * precision (fp32 contexts read the double PSFs and transform in float); normalisation, modulus and results are doubles. */
enum { PAOS_OTF_MTF = 0, PAOS_OTF_COMPLEX = 1 };
/* The spectra of every item's kept PSF into a batch-sized complex buffer of the context's precision (the field's layout;
 * allocated on first use, freed by paos_ctx_destroy): a pass along rows that reads the PSFs and writes the buffer, a pass
 * along columns in place on the buffer.  The PSF buffer and the field are only read.  Enqueues only (no synchronisation).
 * PAOS_EINVAL before any PSF was kept.  Whatever stores PSFs afterwards (paos_psf_keep, paos_psf_keep_power, a pass
 * program with final_intensity) makes the result stale: paos_otf_fetch / paos_otf_cuts then fail with PAOS_EINVAL until
 * the next paos_otf_compute, rather than serve the transform of an older PSF. */
int paos_otf_compute(paos_ctx* ctx);
/* One item to the host, row-major [ky][kx]: what = PAOS_OTF_MTF: N x N doubles; PAOS_OTF_COMPLEX: N x N complex128.
 * Synchronises.  PAOS_EINVAL for a bad item or `what`, a null buffer, before paos_otf_compute or when its result is
 * stale (the context stays usable). */
int paos_otf_fetch(paos_ctx* ctx, int item, int what, void* host_out);
/* MTF cuts of EVERY item in one launch and one copy: host_out[batch][2][N/2 + 1] = |OTF| along fy = 0, fx >= 0 (pixels
 * [N/2][N/2 + m]) and along fx = 0, fy >= 0 (pixels [N/2 + m][N/2]), m = 0 (zero frequency) .. N/2 (Nyquist, pixel 0 of
 * the fetched array by the mirror symmetry) -- bit for bit the values paos_otf_fetch hands out.  Synchronises.
 * PAOS_EINVAL as for paos_otf_fetch. */
int paos_otf_cuts(paos_ctx* ctx, double* host_out);
/* ---- blurred PSFs: jitter, charge diffusion and pixel aperture on the kept spectrum (README.md, "Blurred PSFs") --------- */
/* No reference counterpart.  What an instrument records is the optical PSF convolved with the line-of-sight jitter of the
 * exposure, the charge diffusion of the detector and, for a sampled "effective PSF", the pixel aperture: each a real, even
 * transfer function on the PSF's spectrum.  Per axis one table of N/2 + 1 doubles, entry m = 0 .. N/2:
 *   f_m = m / (N d)  (cycles per metre; d = dx or dy),   t[m] = exp(-2 pi^2 sigma^2 f_m^2) sinc(p f_m),
 *   sinc(x) = sin(pi x) / (pi x), sinc(0) = 1
 * with sigma the Gaussian 1-sigma blur along that axis in metres at the image plane (jitter and diffusion add in
 * quadrature: pass their root sum of squares) and p the pixel width along that axis in metres (0: no pixel factor).
 * The blurred PSF is
 *   P' = ifft2(T fft2(P)),   T[ky][kx] = ty[min(ky, N - ky)] tx[min(kx, N - kx)]   (unshifted indices)
 * T is real and even, so P' is real; the convolution is circular; sum P' = sum P to rounding; nothing is clamped (with
 * p > 0 the band-limited box rings and negative values are genuine; with sigma alone values below zero are rounding and
 * the truncation at Nyquist).  A rotated jitter ellipse (a cross term fx fy) is not separable and not offered.
 *
 * paos_blur_table: the table of one axis, host only and context-free like paos_zoom_weights, evaluated in long double and
 * rounded to double once; t[n/2 + 1], t[0] == 1.0 exactly.  PAOS_EINVAL for n odd or outside 2 .. 2^20, a d that is not
 * finite and positive, a sigma or pixel that is not finite or is negative, and a null pointer. */
int paos_blur_table(int n, double d, double sigma, double pixel, double* t);
enum { PAOS_BLUR_ITEM = 6 };   /* dx, dy, sigma_x, sigma_y, pixel_x, pixel_y */
/* per_item[batch][PAOS_BLUR_ITEM].  Builds and uploads every item's two tables and turns the spectra paos_otf_compute
 * left into blurred PSFs by a packed real-output inverse 2-D transform (csrc/blur_pass.h; about N line transforms per
 * item): a pass along the columns 0 .. N/2 of the spectrum buffer that multiplies element [ky][kx] by
 * g = fl64(tx[.] ty[.]) (in an fp32 context g is then rounded to float; real and imaginary part times g once each; zero
 * frequency has g = 1 and is unchanged), stores the product back and writes the row-pair-packed half-transformed image
 * into the PSF buffer, then a pass along the N/2 packed lines in place on the PSF buffer that applies the 1 / N^2 of the
 * inverse once (an exact power of two).  fp32 contexts transform in float and store doubles, as paos_otf_compute does.
 * Enqueues only (no synchronisation).  Afterwards the PSF buffer holds P' -- paos_psf_fetch and every paos_detector_*
 * call read it -- and the transfer functions stay valid: paos_otf_fetch / paos_otf_cuts hand out those of P', the SYSTEM
 * OTF / MTF, Hermitian bit for bit and exactly 1 at zero frequency as before.  A second call compounds: it multiplies
 * T2 onto the spectrum that already carries T1, and the PSF buffer then holds the image blurred by T2 T1.  The field is
 * neither read nor written.  PAOS_EINVAL, the context left usable and both buffers untouched: before paos_otf_compute or
 * when its result is stale (the test of paos_otf_fetch), a parameter paos_blur_table refuses, a null pointer. */
int paos_blur_apply(paos_ctx* ctx, const double* per_item);
/* ---- energy profiles: encircled / ensquared energy of the kept PSFs about their own centres (README.md, "Encircled energy") - */
/* The reference's Monte-Carlo workflow reduces every draw to an encircled-energy radius on the host
 * (docs/source/user/montecarlo/index.rst); here the curves are made on the device from the kept PSF P[k][j] (N x N doubles, rows
 * k along y, as paos_psf_fetch returns it; in fp32 contexts too, so everything below is fp64 in both).  Per item a ring
 * width D in units of dx and an aspect a = dy / dx.
 *   Sums over the whole grid: S = sum P, Sx = sum P j, Sy = sum P k; peak = the largest value, (peak_col, peak_row) its
 *   first occurrence in row-major order.
 *   Centre (cx, cy), column and row in pixels: PAOS_EE_GIVEN as passed; PAOS_EE_PEAK (peak_col, peak_row);
 *   PAOS_EE_CENTROID cx = Sx / S, cy = Sy / S, one division each, on the device -- and if S > 0 is false or a centroid
 *   coordinate is not inside [0, N), (N/2, N/2) with fallback = 1 (the flag concerns the centroid; it is 0 otherwise).
 *   Membership, every operation rounded once (no contraction): x = (double)j - cx, y = ((double)k - cy) a,
 *   d2 = x x + y y, r_b = (double)(b + 1) D, t_b = r_b r_b; pixel (k, j) is inside circle b iff d2 <= t_b (the
 *   pixel-centre rule of paos_psf_metrics) and inside square b iff fmax(|x|, |y|) <= r_b.  No wrap: pixels outside the
 *   grid do not exist.
 *   Curves: ee[b] = sum of P over the pixels inside circle b, ensq[b] likewise for square b: powers, not fractions; with
 *   negative values in a blurred PSF they need not be monotone.
 * No float atomics and a fixed summation order: a repeated call gives the same bits, and an item's results do not depend
 * on the batch size or on its place in the batch. */
enum { PAOS_EE_GIVEN = 0, PAOS_EE_CENTROID = 1, PAOS_EE_PEAK = 2 };
enum { PAOS_EE_ITEM = 4 };     /* delta, aspect, cx, cy (cx, cy read for PAOS_EE_GIVEN only) */
enum { PAOS_EE_SUMMARY = 9 };  /* S, Sx, Sy, peak, peak_col, peak_row, cx, cy, fallback */
/* per_item[batch][PAOS_EE_ITEM]; bins in 1 .. 1024; square != 0: the ensquared curve too.  Enqueues only: the centre is
 * formed on the device between the sweep that sums and the launch that bins.  Scratch is allocated on first use and again
 * when a request needs more; its size follows batch x bins x bands of 16 rows, never N^2.  PAOS_EINVAL, nothing touched
 * and the context left usable: before any PSF is kept, a null pointer, bins outside 1 .. 1024, an unknown centre_mode, a
 * delta or aspect that is not finite and positive, bins delta > N/2 or bins delta / aspect > N/2 (the largest circle
 * would be wider or taller than the grid), a given centre that is not finite or not inside [0, N).  PAOS_EHIP for a failed
 * scratch allocation. */
int paos_ee_compute(paos_ctx* ctx, int bins, int square, int centre_mode, const double* per_item);
/* summary[batch][PAOS_EE_SUMMARY] and curves[batch][1 + square][bins] (ee, then ensq) of the last paos_ee_compute.  Either
 * pointer may be NULL, not both.  Synchronises.  PAOS_EINVAL before a compute, with both pointers null, and for `curves`
 * of a compute whose PSFs were stored anew since (paos_psf_keep, paos_psf_keep_power, a PSF-storing pass program,
 * paos_blur_apply): compute again. */
int paos_ee_fetch(paos_ctx* ctx, double* summary, double* curves);
/* ---- zoomed PSF windows: the field interpolated exactly onto a finer grid (README.md, "Zoomed PSFs") ------------------- */
/* No reference counterpart.  With u[k][j] the N x N field of item i (rows k along y), its band-limited interpolant with the
 * Nyquist term split evenly is u(y, x) = sum_k sum_j u[k][j] d(y - k) d(x - j), d(t) = sin(pi t) / (N tan(pi t / N)),
 * d = 1 for t = 0 (mod N), period N.  A window has M fine samples per side at 1 / s of the grid pitch about a centre
 * (cx_i, cy_i) in pixel-index units (pixel N/2 is the grid centre): fine column q lies at x_q = cx + (q - M/2) / s, row p
 * likewise along y, and psf_zoom[p][q] = |u(y_p, x_q)|^2 -- samples of the same intensity as the PSF, not divided by s^2.
 * The interpolant is periodic: a window that runs over the grid edge wraps.  The window is Wy u Wx^T with REAL weights,
 * two dense contractions on the fp64 matrix instruction (csrc/zoom_pass.h), in fp64 for either kind of context (an fp32
 * context's complex64 field is widened on load); the results are doubles.
 *
 * paos_zoom_weights: the weights of one axis for the fractional part `frac` in [0, 1) of a centre, host only, evaluated in
 * long double and rounded to double once.  Per axis c = ci + frac with ci = floor(c); q - M/2 = s a + b with 0 <= b < s
 * (floor division); the phase offset is phi_b = frac + b / s, minus 1 with carry[b] = 1 when it reaches 1 (the carry goes
 * into a); the sample's weight on grid pixel j is w[b][m mod n] with m = ci + a + carry[b] - j wrapped to [-n/2, n/2):
 *   w[b][m] = [m == 0] when phi_b == 0, else (-1)^m sin(pi phi_b) / (n tan(pi (m + phi_b) / n)).
 * So column 0 of a row is m = 0 and columns n/2 .. n-1 are m = -n/2 .. -1, and a fine sample that falls on a grid pixel
 * has a unit-vector row: it is a copy of the field's sample, bit for bit.  w[s][n], carry[s].  PAOS_EINVAL for n odd or
 * outside 2 .. 2^20, s outside 1 .. 64, frac outside [0, 1) and null pointers. */
int paos_zoom_weights(int n, int s, double frac, double* w, int* carry);
enum { PAOS_ZOOM_PSF = 0, PAOS_ZOOM_FIELD = 1 };
/* The m x m windows of EVERY item of the field as it is now, oversampling s, about centres[item][2] = (cx, cy) (NULL: the
 * grid centre N/2, N/2 for every item): |u|^2 into a buffer [batch][m][m] of doubles and, with want_field, u itself into a
 * second one of complex128.  Two launches (columns contracted into a scratch of 16 batch m N bytes, then rows), no
 * atomics, a fixed summation order: a repeated call gives the same bits, and an item's window does not depend on the batch
 * size or on its place in the batch.  The scratch and the windows are allocated on first use, again when m changes, and
 * freed by paos_ctx_destroy; one phase table (s x N doubles) per distinct fractional part of a centre is built on the host,
 * uploaded once and reused by later calls with the same s (the context keeps up to 256 tables; when a call's new ones
 * do not fit beside them, the kept ones are dropped first -- never in the middle of a call).  Enqueues only (a call that has to build a table copies it
 * before it returns; one that has to move or drop tables, or to reallocate, waits for the windows enqueued before).  A
 * pending deferred stop factor (paos_stop_defer_last_power) is applied first, as by every reader of the field; the field
 * is only read and must be the complete field, as for paos_focus_begin.  PAOS_EINVAL (the context stays usable): m not a
 * multiple of 16 or outside 16 .. 1024, m > s N, s outside 1 .. 64, a centre that is not finite or outside [0, N), more
 * than 256 distinct fractional parts among the centres of one call.
 * PAOS_EHIP when the scratch cannot be allocated (the context stays usable; no window is available then). */
int paos_zoom_compute(paos_ctx* ctx, int m, int s, const double* centres, int want_field);
/* The launch plan of paos_zoom_compute for a context of `batch` items on an n x n grid and windows of m samples, host only
 * and context-free like paos_zoom_weights: the number of 16-row tiles a wave owns (8, 4, 2 or 1) in the column contraction
 * (*pt_y) and in the row contraction (*pt_x).  It is the rule paos_zoom_compute itself launches by, so a test can tell
 * which builds of the kernel a case reaches; a window's bits do not depend on it.  PAOS_EINVAL for m as for
 * paos_zoom_compute, n not a multiple of 16 in 16 .. 2^20, batch < 1 and null pointers. */
int paos_zoom_tiles(int n, int batch, int m, int* pt_y, int* pt_x);
/* One item's window to the host, row-major [p][q]: PAOS_ZOOM_PSF m x m doubles, PAOS_ZOOM_FIELD m x m complex128.
 * Synchronises.  The buffers are a snapshot of the field at the time of paos_zoom_compute: nothing tracks whether the
 * field has changed since.  PAOS_EINVAL before any paos_zoom_compute, for a bad item or `what`, a null buffer, and for
 * PAOS_ZOOM_FIELD when the last paos_zoom_compute was not asked for it. */
int paos_zoom_fetch(paos_ctx* ctx, int item, int what, void* host_out);
/* A whole stretch of the propagation loop (run.py:193-207 over consecutive surfaces) as a
 * program of passes: lens phases (wfo.py:359-366), the checkerboard signs that replace
 * fftshift/ifftshift, the quadratic phases and ortho scalings of ptp / stw / wts
 * (wfo.py:462-545) ride on the FFT passes, and the last pass of one propagator merges with the
 * first pass of the next because a 2-D FFT may run rows-then-columns or columns-then-rows.
 * `blocks` = n_blocks sets of [batch][PAOS_PHASE_STRIDE] doubles.  paos_ptp / paos_stw /
 * paos_wts / paos_phase above are one-operator programs of the same machinery. */
int paos_run_passes(paos_ctx* ctx, const paos_pass* passes, int n_passes, const double* blocks,
                    int n_blocks);
/* The same with a promise about the field on entry: for item i, the rows outside
 * [live_rows[2 i], live_rows[2 i + 1]) are exactly zero in memory (what WFO.aperture, wfo.py:273-276,
 * leaves outside the bounding box of a clear aperture).  Transforms of zero rows are zero rows, so the
 * first passes skip them -- the results are the same, only the traffic is not.  (Inside a program the
 * library tracks by itself which rows / columns the apertures riding on its passes have zeroed.) */
/* Measurement aid: an in-place copy of the whole batch (every element read and written back unchanged,
 * 16 B per lane, unit stride), `reps` launches timed with HIP events on the context's stream: the
 * yardstick bench.py prints next to the pass kernels' rate.  The field is left as it was. */
int paos_copy_yardstick(paos_ctx* ctx, int reps, double* ms_per_launch, double* bytes_per_launch);
/* Measurement aid: how often, since the context was created, a pass that carries an aperture (WFO.aperture,
 * wfo.py:246-276, riding on a pass as line records) found its records in one of the context's kept sets
 * (*found) and how often it had to render them (*rendered).  bench.py reports both per step of its walked sweep. */
int paos_record_set_stats(paos_ctx* ctx, unsigned long long* found, unsigned long long* rendered);
/* Measurement / test aid: how many frugal pass launches of the context, since it was created, ran on the central-half
 * build of their shape (*central: every item of the launch's first pass loads positions inside [n / 4, 3 n / 4), so
 * the slot and the first butterfly layer in front skip the outer positions, which are exact zeros) and how many on
 * the ordinary build (*plain).  PAOS_CENTRAL_HALF=0 / 1 in the environment when the context is created switches the
 * central-half builds off / on; results are equal as numbers either way. */
int paos_central_half_stats(paos_ctx* ctx, unsigned long long* central, unsigned long long* plain);
/* Likewise: how many frugal pass launches ran on the narrow-window variant of their central-half build (*narrow: besides,
 * every item of the first pass loads and every item of the pass whose stores leave the launch stores positions inside
 * [5 n / 16, 11 n / 16) only, so the kernel neither loads, computes nor tests what lies outside) and how many on any other
 * build (*other).  A narrow launch counts as *central above.  PAOS_NARROW_WINDOWS=0 / 1 in the environment when the context
 * is created switches the variant off / on; results are equal as numbers either way. */
int paos_narrow_window_stats(paos_ctx* ctx, unsigned long long* narrow, unsigned long long* other);
/* Measurement / test aid: what the block renderer of ellipse line records did since the context was created.  out[0]: lines
 * inside an aperture's bounding box whose records a wave rendered as part of a block of 64 lines, out[1]: such lines handed to
 * the per-line renderers (no window fits, or the block's list of undecided pixels was full), out[2]: window pixels whose exact
 * overlap was evaluated (the others were decided by comparisons).  Waits for the context's stream.  PAOS_MASK_BLOCKS=0 in the
 * environment (read at every call) renders four lines per wave instead; the records are equal bit for bit either way. */
int paos_record_block_stats(paos_ctx* ctx, unsigned long long* out);
/* Test aid, host only (no context): is there a build of the frugal pass kernel of this name in the family (precision, n)?
 * `record`: the nine fields of a build's name -- axis, kpre, kmid, nfft, store, tab, fuse, one_line, central.  1 / 0; a field out
 * of its range names no build (0).  The families are complex128 at 1024, 2048 and 4096 and complex64 at 2048 and 4096: any other
 * (precision, n), or a null record, gives -PAOS_EINVAL (negative, since PAOS_EINVAL itself is 1). */
int paos_frugal_built(int precision, int n, const int* record);
/* Test aid: the builds the frugal launches of the context's most recent pass program took (paos_run_passes and its kin, also
 * the programs behind paos_ptp / paos_stw / paos_wts), nine ints per launch in the order above, in launch order -- what each launch
 * handed to its family after the one-line and central-half decisions.  Launches of the generic kernel log nothing; the log is
 * cleared where a program begins.  *count: launches logged; at most `capacity` records are written (capacity 0: count only). */
int paos_pass_builds(paos_ctx* ctx, int* records, int capacity, int* count);
/* Test aid: what became of the factors paos_stop_defer_last_power left pending, since the context was created: *rode
 * counts those the first pass of the next pass program multiplied into its middle slot, *settled those applied by the
 * scaling sweep (or dropped, where the field was about to be overwritten) because something else came first.  A test
 * that means to cover one route can tell that it did. */
int paos_deferred_stop_stats(paos_ctx* ctx, unsigned long long* rode, unsigned long long* settled);
/* Measurement / test aid: on = 0 makes every pass process every tile (no dead-line pruning). */
int paos_ctx_set_pruning(paos_ctx* ctx, int on);
int paos_run_passes_live(paos_ctx* ctx, const paos_pass* passes, int n_passes, const double* blocks,
                         int n_blocks, const double* live_rows);
/* paos_run_passes with options (paos_program_opts above): entry rows that are zero or stand for zeros, and the
 * PSF + power of the final field instead of the field itself (run.py:222-224 -> plot.py:125-130 in one sweep). */
int paos_run_program(paos_ctx* ctx, const paos_pass* passes, int n_passes, const double* blocks, int n_blocks,
                     const paos_program_opts* opts);
/* WFO.zernikes (wfo.py:620-652) with Zernike polynomials (zernike.py:85-109,245-247):
 * u *= exp(2 pi i wfe / wl) inside rho <= 1.  `table` holds the Jacobi recurrence
 * constants [(nmax+1)][kdim][3]; `params` the per-item blocks (PAOS_ZERNIKE_HEAD +
 * 2 (nmax+1) kdim doubles).  If host_wfe != NULL the wfe map of item 0 is returned
 * (row-major doubles, NaN where rho > 1 -- the masked array of wfo.py:654).  PAOS_EINVAL for an enabled item whose
 * radius is not > 0 or whose record holds a non-finite value: NaN inside the disk would read as masked. */
int paos_zernike(paos_ctx* ctx, int nmax, int kdim, const double* table, const double* params,
                 int param_stride, double* host_wfe);
/* Round 5: paos_zernike for a caller who knows that some items hold COPIES of one field -- the surface right behind the
 * start of a wavelength sweep or of a Monte-Carlo batch (wfo.py:118 fills every wavefront with the same constant under the
 * same aperture): same_as[i] = index of an item whose field equals item i's.  Items that share their wfe map (records equal
 * but for the wavelength) AND their field are served by one load per pixel; the values written are those of paos_zernike
 * bit for bit.  NULL = paos_zernike. */
int paos_zernike_like(paos_ctx* ctx, int nmax, int kdim, const double* table, const double* params,
                      int param_stride, const double* same_as, double* host_wfe);


/* ---- PolyOrthoNorm / Zorthonorm ------------------------------------------------ */
/* The pupil the polynomials are orthonormalised on -- run.py:133-141: the pixels where the exact
 * mask of this surface's aperture object is non-zero (whatever its obscuration flag).  One weight
 * map per batch item stays in HBM until the next call.  params as for paos_aperture. */
int paos_pupil_aperture(paos_ctx* ctx, int shape, const double* params);
/* the same from a host array (row-major doubles, 0 = masked): the `mask` argument of
 * WFO.zernikes, wfo.py:583,623-627.  Synchronises. */
int paos_pupil_upload(paos_ctx* ctx, int item, const double* host_weights);
/* Zernike.cov (zernike.py:293-318) without its final division: per item, the sums over the
 * unmasked pixels (rho <= 1, and pupil weight != 0 when use_pupil) of Z_i Z_j for the first K
 * polynomials, i <= j enumerated row by row, followed by the pixel count:
 * host_out[batch][K (K + 1) / 2 + 1].  poly[K][4] = {|m|, k = (n - |m|) / 2, is_sin, factor}
 * with factor = (-1)^k norm; table / params as for paos_zernike (the coefficient planes of
 * params are not read; the header is refused as for paos_zernike).  K <= 64.  Synchronises. */
int paos_zernike_gram(paos_ctx* ctx, int nmax, int kdim, const double* table, const double* params,
                      int param_stride, int K, const double* poly, int use_pupil, double* host_out);
/* paos_zernike restricted to the pupil: pixels outside it keep their value and read NaN in
 * host_wfe (the mask of PolyOrthoNorm's polynomials, zernike.py:396-400). */
int paos_zernike_pupil(paos_ctx* ctx, int nmax, int kdim, const double* table, const double* params,
                       int param_stride, double* host_wfe);

/* ---- wavefront fits: the Zernike content and the OPD statistics of the field at a surface (README.md, "Wavefront fits") -- */
/* The round trip of WFO.zernikes (wfo.py:574-652): no reference counterpart.  Item i holds the field u[k][j] (rows k along
 * y) with samplings dx, dy; its request is the header of its Zernike parameter block (radius, origin, offset), K
 * polynomials, a weighting and a floor min_intensity >= 0.  The disk is about the grid centre.
 *   Support: x = (double)(j - N/2) dx, y = (double)(k - N/2) dy, rr = sqrt(fl(x x) + fl(y y)), rho = rr / radius -- the
 *   arithmetic of paos_zernike_gram, one rounding per operation; I = fl(fl(re re) + fl(im im)) on the components widened to
 *   double.  Pixel (k, j) is in Omega iff rho <= 1 and I > min_intensity (and, with use_pupil, the pupil weight != 0).
 *   Reference phasor: r = sum over Omega of u, complex, fp64, in a fixed order; r = 1 + 0i and fallback = 1 if that sum
 *   is zero or not finite.
 *   Phase: re' = fl(fl(ux rx) + fl(uy ry)), im' = fl(fl(uy rx) - fl(ux ry)), phi = atan2(im', re') in [-pi, pi].  Nothing
 *   is unwrapped: the result is valid while the OPD stays within +- lambda / 2 of the amplitude-weighted mean.
 *   Weights: w = 1 (PAOS_WF_UNIFORM) or w = I (PAOS_WF_INTENSITY).
 *   Sums: A[p][q] = sum over Omega of fl(fl(w c_p) c_q) for the K + 1 columns c = [Z_0 .. Z_{K-1}, phi], p <= q
 *   enumerated row by row as paos_zernike_gram does: G = sum w Z_i Z_j, b = sum w phi Z_j (the last column) and
 *   sum w phi^2 (the last entry).
 *   Summary, per item: count = |Omega|, r (the sum itself, whatever the fallback), sum sqrt(I), sum I, phi_min, phi_max
 *   (both 0 for an empty Omega), fallback, sum w, sum w phi.
 * No float atomics; every sum is added in an order fixed by the item's own request and the grid: a repeated call gives
 * the same bits, and an item's results do not depend on the batch size, its place in the batch or the other items'
 * requests.  Everything is fp64 in both kinds of context; a complex64 field is widened on load.  The fit itself -- the
 * coefficients, the RMS values, the Strehl ratio -- is host algebra on these sums (paos_amd/wavefront.py). */
enum { PAOS_WF_UNIFORM = 0, PAOS_WF_INTENSITY = 1 };
enum { PAOS_WF_SUMMARY = 10 };  /* count, r_re, r_im, sum sqrt(I), sum I, phi_min, phi_max, fallback, sum w, sum w phi */
/* table / params / poly as for paos_zernike_gram (the header of a block is read, its coefficient planes are not; an item
 * with enable == 0 gets zeros and count = 0); min_intensity[batch], or NULL for zeros.  Settles a pending deferred stop
 * factor, then enqueues only (three launches; the host does not wait between them).  Scratch is allocated on first use,
 * again when a request needs more, and freed by paos_ctx_destroy.  PAOS_EINVAL, with nothing touched and the context
 * usable: null pointers, inconsistent table dimensions, a radius not > 0 or a non-finite header value, a polynomial
 * outside the table or listed twice, an unknown weight_mode, a min_intensity that is negative or not finite, use_pupil
 * without a pupil.  PAOS_EUNSUPPORTED for K outside 1 .. 63; PAOS_EHIP for a failed scratch allocation. */
int paos_wavefront_fit(paos_ctx* ctx, int nmax, int kdim, const double* table, const double* params, int param_stride,
                       int K, const double* poly, int weight_mode, int use_pupil, const double* min_intensity);
/* summary[batch][PAOS_WF_SUMMARY] and sums[batch][(K + 1)(K + 2) / 2] of the last paos_wavefront_fit.  Either pointer may
 * be NULL, not both.  Synchronises.  PAOS_EINVAL before a fit and with both pointers null.  The results are a snapshot of
 * the field at fit time: nothing tracks later changes (as paos_zoom_fetch). */
int paos_wavefront_fetch(paos_ctx* ctx, double* summary, double* sums);

/* ---- broadband PSFs on a detector pixel grid (docs/source/user/montecarlo/index.rst, "Multi-wavelength simulations") -- */
/* No reference counterpart: the reference hands out each wavelength's PSF on its own sampling and leaves the rebinning to
 * the user.  Definitions (README.md, "Detector images"):
 *   grid column j of item i spans [(j - N/2 - 1/2) dx_i, (j - N/2 + 1/2) dx_i] (wfo.py:236-237, run.py:443: a pixel centre
 *   at x / dx + N/2); row k likewise with dy_i.  Detector column m spans [xc + (m - nx/2) pitch_x, xc + (m + 1 - nx/2) pitch_x],
 *   row n likewise with yc, pitch_y; images are [ny][nx] doubles, rows along y (as paos_export / paos_psf_fetch).
 *   fx_i(j, m) = |grid column j  ^  detector column m| / dx_i, fy_i(k, n) likewise, and the per-item image
 *   A_i[n][m] = sum_k sum_j PSF_i[k][j] fy_i(k, n) fx_i(j, m): flux-conserving rebinning of a PSF that is constant within
 *   each grid pixel.  Energy outside the detector is dropped; detector area outside the grid receives nothing.
 *   The accumulator is updated once per item, in ascending item order, in fp64: image <- image + w_i A_i (no atomics,
 *   every sum in a fixed order: splitting a sweep into batches differently changes no bit when the PSFs are the same).
 * The PSF read is the context's kept buffer (paos_psf_keep, paos_psf_keep_power or a pass program with final_intensity),
 * doubles in fp32 contexts too; rebinning and accumulator are fp64.  Only the grid rows and columns under each item's
 * detector footprint are read.  Scratch is allocated on first use and freed by paos_ctx_destroy; when the scratch of a whole
 * batch would exceed 512 MiB (PAOS_DETECTOR_SCRATCH_MIB) the items are processed in chunks, in item order. */
enum { PAOS_DETECTOR_GEOM = 6 };  /* nx, ny, pitch_x, pitch_y, xc, yc (metres, image-plane coordinates) */
enum { PAOS_DETECTOR_ITEM = 3 };  /* dx, dy, w: the item's pitch at the last surface and its weight */
enum { PAOS_DETECTOR_SCRATCH_MIB = 512 };
/* Set the detector geometry (geom[PAOS_DETECTOR_GEOM]) and zero the accumulator.  nx, ny: integers in 1..4096; pitches
 * finite and positive; centre finite -- otherwise PAOS_EINVAL.  Does not read the PSF buffer. */
int paos_detector_begin(paos_ctx* ctx, const double* geom);
/* image <- image + w_i A_i for i = 0 .. batch-1 in order, from the kept PSFs; per_item[batch][PAOS_DETECTOR_ITEM].
 * Enqueues only (no synchronisation).  PAOS_EINVAL before paos_psf_keep or paos_detector_begin, or for a dx / dy that is
 * not finite and positive or a weight that is not finite. */
int paos_detector_add(paos_ctx* ctx, const double* per_item);
/* A_i of every item to host_out[batch][ny][nx] (per_item as above, w not read; Monte-Carlo studies).  Synchronises. */
int paos_detector_images(paos_ctx* ctx, const double* per_item, double* host_out);
/* the accumulator to host_out[ny][nx].  Synchronises. */
int paos_detector_fetch(paos_ctx* ctx, double* host_out);
/* Placed items (README.md, "Detector images"): per_item[batch][PAOS_DETECTOR_PLACED_ITEM] = dx, dy, w, x0, y0, where
 * (x0, y0) is the image-plane position in metres of item i's grid centre (pixel N/2): grid column j of item i spans
 * [x0_i + (j - N/2 - 1/2) dx_i, x0_i + (j - N/2 + 1/2) dx_i], row k likewise with y0_i and dy_i; everything else as above.
 * On the device the detector centre seen from the item is xc - x0_i (and yc - y0_i), rounded once and then used as the
 * unplaced calls use xc: zero offsets give paos_detector_add / paos_detector_images bit for bit.  Footprint, chunking,
 * item order and the fp64 accumulator are per item as above; a footprint that misses the detector adds exact zeros.
 * PAOS_EINVAL, besides the cases above, for an x0 / y0 that is not finite (or whose difference to the centre overflows). */
enum { PAOS_DETECTOR_PLACED_ITEM = 5 };  /* dx, dy, w, x0, y0 */
int paos_detector_add_placed(paos_ctx* ctx, const double* per_item);
int paos_detector_images_placed(paos_ctx* ctx, const double* per_item, double* host_out);

/* ---- pointing series: detector frames and box flux of the kept PSFs while the line of sight moves (README.md, "Pointing series") - */
/* No reference counterpart.  The series carries its own detector (geom[PAOS_DETECTOR_GEOM], what paos_detector_begin takes)
 * and neither reads nor writes the context's detector state: the accumulator and the geometry of paos_detector_begin
 * survive a call untouched.  per_item[batch][PAOS_SERIES_ITEM] = dx, dy, x0, y0: the item's samplings and the image-plane
 * position of its grid centre; offsets[frames][2] (per_item_offsets == 0: one list for every item) or
 * offsets[batch][frames][2] = (ox_t, oy_t) in metres.  In frame t item i's grid centre lies at X = fl(x0_i + ox_t),
 * Y = fl(y0_i + oy_t), the detector centre seen from the item at fl(xc - X), fl(yc - Y); everything else is the definition
 * of the detector images above, and pixel (n, m) is formed in the order of its two contractions:
 *   a = 0;  for k ascending over the grid rows under detector row n:  fy = min(k + 1, e1y) - max(k, e0y), skipped unless > 0;
 *     r = 0;  for j ascending over the grid columns under detector column m:  r = r + P[k][j] fx  where fx > 0;   a = a + r fy
 * so that frame t of item i equals paos_detector_images_placed on the same detector with (x0, y0) = (X, Y) bit for bit (zero
 * offsets and origins: paos_detector_images); with a response g[ny][nx] (pixel gains) every value is multiplied by
 * g[n][m], rounded once.  A frame whose footprint misses the grid is exact zeros and reads nothing.
 * boxes[nboxes][4] = m0, m1, n0, n1: half-open boxes of detector pixels (columns m0 .. m1-1, rows n0 .. n1-1), and
 * flux[i][t][a] the sum of the frame over box a in a fixed order: with q counting the box's pixels row-major, lane l of 64
 * adds the pixels q = l, l + 64, ... in ascending order starting from +0.0; the 64 partial sums are combined by the tree
 * p[l] = p[l] + p[l + s] for s = 32, 16, 8, 4, 2, 1; p[0] is the flux.  No atomics: a flux does not depend on the batch size,
 * the item's place in the batch, the chunking or what else is asked for.  Everything is fp64 in fp32 contexts too.
 * The frames go through a device buffer of at most PAOS_DETECTOR_SCRATCH_MIB (the environment's PAOS_SERIES_SCRATCH_BYTES,
 * read at every call, overrides it) in chunks: as many whole frames of every item as fit, at least one -- or, if one frame
 * of every item does not fit, one frame of as many items as do, at least one.  Chunks run in frame order on the context's
 * stream.  With host_frames == NULL the call enqueues only; otherwise every chunk is copied to
 * host_frames[batch][frames][ny][nx] and the call synchronises.  Scratch is kept in the context, regrown when needed, and
 * freed with it.  PAOS_EINVAL, nothing touched and the context left usable: before any PSF is kept; null geom, per_item or
 * offsets; a geometry paos_detector_begin refuses; a dx or dy that is not finite and positive; an x0, y0, offset, x0 + ox
 * or xc - X (y alike) that is not finite; frames outside 1 .. 65536; nboxes outside 0 .. 16; nboxes == 0 with a null
 * host_frames (nothing to compute); nboxes > 0 with null boxes; an empty box or one outside [0, nx) x [0, ny); a response
 * value that is not finite.  PAOS_EHIP for a failed allocation. */
enum { PAOS_SERIES_ITEM = 4 };  /* dx, dy, x0, y0 */
enum { PAOS_SERIES_MAX_FRAMES = 65536, PAOS_SERIES_MAX_BOXES = 16 };
int paos_series_compute(paos_ctx* ctx, const double* geom, const double* per_item, const double* offsets, int frames,
                        int per_item_offsets, const int* boxes, int nboxes, const double* response, double* host_frames);
/* flux[batch][frames][nboxes] of the last paos_series_compute, in one copy.  Synchronises.  The fluxes are a snapshot of
 * the PSF buffer at compute time: nothing tracks later stores (as paos_zoom_fetch).  PAOS_EINVAL before a compute, after a
 * compute with nboxes == 0, and for a null pointer. */
int paos_series_fetch(paos_ctx* ctx, double* flux);

/* ---- broadband series: weighted sums of frames over the items of a sweep, kept on the device (README.md, "Broadband series") */
/* No reference counterpart.  paos_series_sum_begin opens a sum on a detector geom[PAOS_DETECTOR_GEOM] (what
 * paos_detector_begin takes) for `frames` frames: an accumulator S[frames][ny][nx] of doubles in device memory, all +0.0
 * (it replaces an earlier sum of the context).  Enqueues only.  frames * ny * nx may not exceed PAOS_SERIES_SUM_MAX_DOUBLES
 * (1 GiB of accumulator): more is refused before anything is allocated.
 * paos_series_sum_add adds the kept PSFs of the batch: per_item[batch][PAOS_SERIES_ITEM] = dx, dy, x0, y0 and
 * offsets[frames][2] (per_item_offsets == 0) or offsets[batch][frames][2], both as for paos_series_compute; weights[batch]
 * (per_frame_weights == 0: w[i][t] = weights[i] for every t) or weights[batch][frames].  For every (t, n, m):
 *   a = S[t][n][m];  for i = 0 .. batch-1 ascending:  if w[i][t] == 0.0 skip, reading nothing of item i;
 *     a = a + fl(w[i][t] F_i[t][n][m]);   S[t][n][m] = a
 * where F_i[t][n][m] is the frame value of paos_series_compute without a response, formed by the same operations in the
 * same order (one device function serves both kernels); the product is rounded once, then the sum.  So S does not depend
 * on how a sweep is cut into adds as long as the items arrive in the same order; weight-0 padding adds nothing; a weight-0
 * item whose PSF holds NaN leaves S finite; one item with weight 1 on a fresh sum gives frame t of paos_series_compute bit
 * for bit.  Everything is fp64 in fp32 contexts too; no atomics.  Enqueues only: the parameters go up from a pinned buffer
 * of the sum's own, guarded by an event, so a call never overwrites what the copy of the previous one still reads.
 * paos_series_sum_flux: host_flux[frames][nboxes], the sum of S'[t] = fl(S[t] g) (response g[ny][nx]; NULL: S itself) over
 * boxes[nboxes][4] = m0, m1, n0, n1 in the lane-and-tree order of paos_series_compute.  Synchronises.
 * paos_series_sum_fetch: host_frames[frames][ny][nx] = S itself (no response).  Synchronises.
 * The sum owns its buffers: the context's detector state, the accumulator of paos_detector_add and the results of the last
 * paos_series_compute (paos_series_fetch still serves them) are left untouched, and paos_series_compute leaves S untouched.
 * PAOS_EINVAL, nothing touched and the context left usable: a null pointer; a geometry paos_detector_begin refuses; frames
 * outside 1 .. 65536; the size rule; add, flux or fetch before begin; add before a PSF is kept; a dx or dy that is not
 * finite and positive; an x0, y0, offset, x0 + ox or xc - X (y alike) or weight that is not finite; nboxes outside 1 .. 16;
 * an empty box or one outside [0, nx) x [0, ny); a response value that is not finite.  PAOS_EHIP for a failed allocation
 * (the sum is then closed). */
enum { PAOS_SERIES_SUM_MAX_DOUBLES = 1 << 27 };
int paos_series_sum_begin(paos_ctx* ctx, const double* geom, int frames);
int paos_series_sum_add(paos_ctx* ctx, const double* per_item, const double* offsets, int per_item_offsets, const double* weights,
                        int per_frame_weights);
int paos_series_sum_flux(paos_ctx* ctx, const int* boxes, int nboxes, const double* response, double* host_flux);
int paos_series_sum_fetch(paos_ctx* ctx, double* host_frames);

#ifdef __cplusplus
}
#endif
#endif /* PAOS_HIP_H */
