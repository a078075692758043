/* bbx.h -- C ABI of libbbx_hip.so: the MI355X (gfx950) implementation of the
 * per-image reduction hot path of BlackBOX.
 *
 * The reference (pmvreeswijk/BlackBOX v1.5.1) has no FFI: its boundary is the
 * Python call boundary of the stage functions in blackbox.py.  Each entry point
 * below names the reference function (file:line) whose bulk array work it
 * replaces; the Python mirrors of those functions (blackbox_amd/reduce.py) keep
 * the reference's names and argument meaning and call these through ctypes.
 * INTEGRATION.md shows the binding a BlackBOX maintainer would add.
 *
 * Conventions
 *  - plain C: pointers + sizes, no torch / numpy types.  `d_` = device pointer
 *    (hipMalloc'ed by the caller, e.g. a torch tensor's data_ptr()), `h_` = host
 *    pointer.  The caller owns every buffer.
 *  - every call is asynchronous on `stream` (a hipStream_t passed as void*, NULL
 *    = default stream) unless its comment says "synchronises".
 *  - return value: 0 = BBX_OK, negative = error (bbx_strerror).  HIP errors are
 *    reported, never swallowed; there is no CPU fallback.
 *  - images are C-order, row 0 first (numpy layout of the FITS data array).
 *  - one bbx_ctx per worker process / GPU (or per lane of a pipeline); a ctx is not thread-safe, and its calls belong on ONE
 *    stream at a time: the device work lists, counters and scratch of a ctx are shared by its calls.  Exceptions: the host
 *    waits (bbx_wait, bbx_sync: their state belongs to the calling thread), and bbx_fpack_tiles / bbx_fpack_body, whose
 *    per-call state lives in the caller's buffers and in a hint table the library keeps per calling STREAM: the output stage
 *    runs them on a second and -- from a writer thread -- a third stream of a lane's ctx at the same time.
 *
 * Geometry (reference define_sections, blackbox.py:6334-6402): the raw frame is
 * NY x NX = 2 x 8 channels of (dy x dx) pixels; each channel holds a data
 * section (ysize_chan x xsize_chan) at its left, a vertical overscan strip at
 * its right, and horizontal overscan rows between the two channel rows.  The
 * reduced frame is (2*ysize_chan) x (8*xsize_chan).
 */
#ifndef BBX_H
#define BBX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BBX_OK            0
#define BBX_ERR_ARG      -1   /* bad argument / geometry */
#define BBX_ERR_HIP      -2   /* a HIP runtime call failed (see bbx_last_hip_error) */
#define BBX_ERR_NOMEM    -3
#define BBX_ERR_OVERFLOW -4   /* a device work list overflowed its capacity */
#define BBX_ERR_NOTCONV  -5   /* an iterative device loop hit its bound */
#define BBX_ERR_PSFWIN   -6   /* bbx_zogy_frame: the PSFs' matched-filter kernels exceed their row window (BBX_OPT_ZOGY_KWIN_OFF) */

#define BBX_NCHAN 16

/* mask bits: set_zogy.mask_value */
#define BBX_MASK_BAD        1
#define BBX_MASK_COSMIC     2
#define BBX_MASK_SAT        4
#define BBX_MASK_SATCON     8
#define BBX_MASK_SATELLITE 16
#define BBX_MASK_EDGE      32
#define BBX_MASK_XTALK     64

#define BBX_RAW_U16 0         /* raw pixels uint16 (BZERO-scaled FITS BITPIX 16) */
#define BBX_RAW_F32 1         /* raw pixels float32 */

typedef struct bbx_ctx bbx_ctx;

typedef struct {
    int32_t ny_raw, nx_raw;          /* raw frame shape, e.g. 10600 x 12000 */
    int32_t ysize_chan, xsize_chan;  /* channel data section, e.g. 5280 x 1320 */
} bbx_geom;

/* ---- context ------------------------------------------------------------------ */
int  bbx_ctx_create(int device, bbx_ctx **out);          /* synchronises */
void bbx_ctx_destroy(bbx_ctx *ctx);                      /* synchronises */
const char *bbx_strerror(int code);
const char *bbx_last_hip_error(const bbx_ctx *ctx);
int  bbx_version(void);
/* Timing experiments compile parts of kernels out of scratch builds of this library (tools/exp: -DFPV_*, -DZ3_SKIP_FFT,
 * -DBOXK_*, -DSATV, -DZ3_STAMPS ...; such a build computes wrong results by design).  The Makefile defines none of them;
 * bbx_build_flags() returns 0 for a product build and a bit per family compiled in otherwise (1 fpack, 2 ZOGY, 4 box
 * statistics, 8 satellite stage), so a harness can refuse a knocked-out library. */
int  bbx_build_flags(void);
/* hipStreamSynchronize(stream) + check of the ctx's device-side error flags
 * (list overflow, non-convergence).  Call before trusting host copies. */
int  bbx_sync(bbx_ctx *ctx, void *stream);

/* Options of a context.
 * BBX_OPT_LAC_LEVEL_FEED (default 0): how bbx_lacosmic obtains astroscrappy's background_level
 * (the median of the good input pixels; only CR pixels without a single good 5x5 neighbour take
 * it, which real frames rarely contain).  0: nothing is prepared; when a frame needs the level,
 * 256 workgroups select it exactly over the frame together (about 1 ms for 10^8 pixels, that
 * frame only).  1: the dense candidate pass also feeds a bracketed select (reads the mask plane too,
 * +45 % on that kernel, plus the sample / bracket kernels) and the level costs microseconds
 * when needed.  Results are identical; a host that sees the level being needed
 * (d_stats[15] != 0) can switch the feed on for a while (pipeline.FramePipeline does). */
#define BBX_OPT_LAC_LEVEL_FEED 1
/* BBX_OPT_DEBUG_LISTCAP (default 0 = off): capacity of the LA-Cosmic work lists as the kernels see
 * it, below the allocated one -- lets a test drive the list-overflow path (BBX_ERR_OVERFLOW ->
 * COSMIC-P = False) with an ordinary frame. */
#define BBX_OPT_DEBUG_LISTCAP 2
/* BBX_OPT_ZOGY_CORE: selected between two 1-D transform cores in round 2; the register-DFT core (bbx_zogy2.hip) is
 * gone, the option is accepted and has no effect. */
#define BBX_OPT_ZOGY_CORE 3
/* BBX_OPT_ZOGY_KWIN_OFF (default 0): bbx_zogy_frame takes the matched-filter kernels k_n, k_r (real space) through
 * their inverse row pass, the squares and the forward row pass on a window of 2 wh >= 4 S + 32 rows around the origin
 * only -- they are as compact as the S x S PSF stamps they are made of; the share of their energy outside the
 * window is summed on the device and must stay below 1e-6 (stamp-truncation ringing sits at 1e-9), else the call's step is flagged (device error bit 4).
 * 1: all L rows (the textbook evaluation; same results to float32 rounding). */
#define BBX_OPT_ZOGY_KWIN_OFF 4
/* BBX_OPT_FPACK_ONE_WG (default 0): bbx_fpack_tiles / bbx_fpack_body compress a row with a bit-stream buffer of half the
 * worst case first (two workgroups per CU) and redo the rows that do not fit with the full buffer; 1: full buffer for
 * every row (one workgroup per CU).  Same bytes either way. */
#define BBX_OPT_FPACK_ONE_WG 5
/* BBX_OPT_FPACK_HIST_ONLY (default 0): the three exact row medians of the quantiser's noise estimate come from a sampled
 * bracket + one counting pass (rows the bracket misses fall back to the radix histograms by themselves); 1: radix
 * histograms over all keys for every row (round 3's path).  Same medians, same bytes either way. */
#define BBX_OPT_FPACK_HIST_ONLY 6
/* BBX_OPT_WAIT_SLEEP_US (default 0): how bbx_sync / bbx_wait wait for the device.  0: the runtime's stream synchronisation
 * (it spins on a core).  n > 0: the host thread polls an event and sleeps n microseconds between polls -- a pipeline with
 * several lane, reader and writer threads per GPU would otherwise burn a core per waiting thread (5.4 cores per GPU measured
 * in round 3); costs up to n us of latency per wait.  The wait's event and the pinned copy of the error words belong to
 * the calling thread: any number of threads may wait on one context. */
#define BBX_OPT_WAIT_SLEEP_US 7
/* BBX_OPT_BKG_FULL_SORT (default 0): bbx_bkg_boxstats takes the clipped statistics of a box from a sorted bracket around its
 * median and the list of its wing pixels, and sorts only the boxes where that does not hold (ties, constant boxes); 1: every
 * box is sorted in full (rounds 2-3).  The medians are the same order statistics either way (tests compare the two). */
#define BBX_OPT_BKG_FULL_SORT 8
/* BBX_OPT_ZOGY_KSMALL_OFF (default 0): where the sub-image side L has a plan for M = L / f and the row window leaves a guard
 * band below M / 2 (L = 1400: f = 5, M = 280), bbx_zogy_frame takes k_n, k_r back to real space on the M x M grid, from every
 * f-th frequency of their spectra: inside the window that is the same function, with whatever lies beyond +-M / 2 folded in.
 * The window check then measures the energy of k_n and of k_r in the rows and columns of the small grid outside the window
 * (same bound, same error bit).  1: the full grid, as for the sides without such a plan (same results to float32 rounding). */
#define BBX_OPT_ZOGY_KSMALL_OFF 9
int  bbx_set_option(bbx_ctx *ctx, int option, int value);
/* Host waits that do not spin.  bbx_wait: everything queued on [stream] so far has finished (no error check: bbx_sync does
 * that); bbx_event_wait: [event] (a hipEvent_t, e.g. of bbx_event_create or a framework's) has completed.  sleep_us > 0:
 * poll + nanosleep; <= 0: for bbx_wait the context's BBX_OPT_WAIT_SLEEP_US, for bbx_event_wait hipEventSynchronize.
 * (what the reference does: nothing -- numpy is synchronous; these replace hipStreamSynchronize / blocking copies.) */
int  bbx_wait(bbx_ctx *ctx, void *stream);
/* Copy [nbytes] between two device-accessible addresses (device memory, or pinned host memory: hipHostMalloc'ed memory is
 * mapped into the device's address space) with a KERNEL on [stream] instead of a copy-engine transfer: the few bytes a stage
 * hands to the host (counts, list heads, scalars) then never queue behind the 100 MB transfers of the output / input stages
 * on the DMA engines.  Meant for small copies (<= a few MB). */
int  bbx_copy_kernel(void *dst, const void *src, size_t nbytes, void *stream);
int  bbx_event_wait(void *event, int sleep_us);

/* Per-step attribution of device-side errors.  Kernels report list overflow / non-convergence by
 * setting bits in a flag word of the context; the calls are asynchronous, so the host cannot see
 * them when a stage function returns.  bbx_step_mark enqueues, on [stream], a move of the flags
 * accumulated so far into *d_slot (device int32, caller-owned; e.g. one slot per stage inside the
 * frame's packed result record) and clears them.  A host that marks after every stage reads, with
 * the frame's scalars, which stage failed (bit 1 = BBX_ERR_OVERFLOW, bit 2 = BBX_ERR_NOTCONV, bit 4 = BBX_ERR_PSFWIN) and
 * applies the reference's convention: `<STEP>-P = False` and carry on (blackbox.py:1866-1878). */
int  bbx_step_mark(bbx_ctx *ctx, int32_t *d_slot, void *stream);

/* Stream plumbing for a host that pipelines frames (the reference runs one frame per worker
 * process, blackbox.py:640-700 pool_func; here one process keeps several frames in flight on
 * HIP streams).  Thin wrappers -- hipEvent without timing, hipStreamWaitEvent,
 * hipMemcpyAsync -- so the per-frame loop does not pay an ML runtime's bookkeeping per call.
 * bbx_event_query: 1 = complete, 0 = not yet, < 0 = BBX_ERR_*.
 * bbx_copy_async kind: 0 host->device, 1 device->host, 2 device->device; host memory should be
 * pinned (hipHostMalloc / hipHostRegister) for the copy to be asynchronous. */
int  bbx_event_create(void **out_event);
void bbx_event_destroy(void *event);
int  bbx_event_record(void *event, void *stream);
int  bbx_event_query(void *event);
int  bbx_stream_wait_event(void *stream, void *event);
int  bbx_copy_async(void *dst, const void *src, size_t nbytes, int kind, void *stream);

/* per-kernel timing: when enabled, the library brackets its main kernels with hipEvents
 * on the launch stream (the reference logs wall time per stage with log_timing_memory,
 * e.g. blackbox.py:4366-4367).  Slots: */
#define BBX_PROF_CALIBRATE 0   /* k_calibrate            (1 launch / frame)  */
#define BBX_PROF_LAC_DENSE 1   /* k_lac_cand             (niter launches)    */
#define BBX_PROF_LAC_SPARSE 2  /* seed+grow+clean        (niter groups)      */
#define BBX_PROF_XTALK 3       /* k_xtalk                                     */
#define BBX_PROF_VOS_STD 4     /* read-noise passes      (1 group / frame)   */
#define BBX_PROF_MASK_FINISH 5 /* mask_init tail + fill  (1 group / frame)   */
#define BBX_PROF_ZOGY 6        /* bbx_zogy_subimages, or (register-DFT core) the kernels of bbx_zogy_frame before its last one */
#define BBX_PROF_ZOGY_FINAL 7  /* k_final_rows of bbx_zogy_frame (1 launch / frame) */
#define BBX_PROF_Z_PSF_COLS 8  /* the other kernels of bbx_zogy_frame (LDS-pass core), one slot each: k_psf_cols (with a prepared
                                  reference PSF on the small-grid path: k_ks_cols, the PSF side's column pass), */
#define BBX_PROF_Z_PSF_ROWS 9  /*   k_psf_rows (small grid: k_ks_cols + k_ks_rows; prepared reference PSF: k_ks_rows alone), */
#define BBX_PROF_Z_IMG_ROWS 10 /*   k_img_rows_one (2 launches / frame; 1 with prepared reference rows), */
#define BBX_PROF_Z_IMG_COLS 11 /*   k_img_cols, */
#define BBX_PROF_Z_VAR_COLS 12 /*   k_var_cols, */
#define BBX_PROF_Z_PSF_DFT 13  /*   k_psf_rowdft (the stamps' row DFTs, in front of k_psf_cols) */
#define BBX_PROF_NSLOTS 14
int  bbx_profile_enable(bbx_ctx *ctx, int on);   /* 1: clear + record; 0: clear + stop; 2: stop, keep the records */
/* synchronises on the recorded events; ms_total/calls have nslots entries; resets */
int  bbx_profile_read(bbx_ctx *ctx, double *ms_total, int32_t *calls, int nslots);

/* ---- a2 + a4 + a5(i): overscan statistics ---------------------------------------
 * replaces: inf/nan scrub blackbox.py:1461-1468, gain_corr 7442-7465 (applied on
 * the fly, raw is not modified), and the strip reductions of os_corr 6480-6490.
 *  d_mean_vos_col [16*dy] f64 : per channel and row, 3-sigma/5-iteration clipped
 *      mean of the gain-corrected vertical overscan (zeros excluded).
 *  d_hos [16*hos_rows*dx] f32 : gain-corrected horizontal-overscan rows
 *      (os_sec_hori) of each channel, BEFORE subtraction of the vertical fit.
 *  d_n_infnan [1] i64 : number of non-finite raw pixels (always 0 for u16).   */
int bbx_overscan_stats(bbx_ctx *ctx, const bbx_geom *g, const void *d_raw,
                       int raw_type, const float *h_gain /*[16]*/,
                       double *d_mean_vos_col, float *d_hos, int64_t *d_n_infnan,
                       void *stream);

/* ---- a5(ii): read noise --------------------------------------------------------
 * replaces os_corr 6572-6573: 3-sigma/5-iteration clipped std (zeros excluded) of
 * each channel's vertical overscan after subtraction of the row fit.
 *  d_vfit [16*dy] f64 : fitted vertical-overscan level per channel row.
 *  h_dlevel [16] f32  : level offset of the horizontal overscan (os_corr 6565-6568);
 *      it was subtracted from the full-width overscan rows, i.e. also from the
 *      corner that the vertical strip shares with them.
 *  d_std_vos [16] f64 (RDN{c});  float64 accumulators (tolerance) */
int bbx_vos_std(bbx_ctx *ctx, const bbx_geom *g, const void *d_raw, int raw_type,
                const float *h_gain, const double *d_vfit, const float *h_dlevel,
                double *d_std_vos, void *stream);

/* ---- a5(iii, BlackGEM): saturated columns near the overscan ----------------------
 * replaces os_corr 6624-6640: per channel and data column, the number of pixels
 * >= h_thr[c] in the [rows1] / [rows2] rows of the data section nearest to the
 * horizontal overscan, after gain and vertical-fit subtraction.
 *  d_counts [2*16*xsize_chan] i32                                               */
int bbx_satcol_counts(bbx_ctx *ctx, const bbx_geom *g, const void *d_raw,
                      int raw_type, const float *h_gain, const double *d_vfit,
                      const float *h_thr /*[16]*/, int rows1, int rows2,
                      int32_t *d_counts, void *stream);

/* ---- a4 + a5(iv) + a6 + a9(first half): fused calibration ------------------------
 * replaces, in one pass over the frame: gain_corr 7460, the per-row and
 * per-column overscan subtractions + crop of os_corr 6553/6844-6847, master-bias
 * subtraction 1679, the non-finite scrub + saturation compare of mask_init
 * 4408-4414/4494-4498/4538, and flat division 1825.
 *  d_oscan [16*xsize_chan] f64 : horizontal-overscan vector per channel.
 *  d_bias, d_flat : reduced-shape f32 masters or NULL.  d_bpm : u8 or NULL.
 *  h_satlevel [16] : saturation thresholds in e- (SATLEV{c}, compared in f32).
 *  d_data [N] f32, d_mask [N] u8 : outputs.  Saturated pixels get bit 4 and are
 *  queued in the ctx for bbx_mask_finish.                                       */
int bbx_calibrate(bbx_ctx *ctx, const bbx_geom *g, const void *d_raw, int raw_type,
                  const float *h_gain, const double *d_vfit, const double *d_oscan,
                  const float *d_bias, const float *d_flat, const uint8_t *d_bpm,
                  const float *h_satlevel, float *d_data, uint8_t *d_mask,
                  void *stream);

/* ---- a14 (+ a8 header statistics): statistics of rectangular segments ---------------
 * replaces the np.nanmedian / np.nanstd / np.ma.median calls of get_flatstats
 * (blackbox.py:3661-3820): the ny x nx area at d_data (row stride [stride] elements; a
 * sub-section of a frame is addressed by offsetting the pointers) is cut into
 * (ny/ysz) x (nx/xsz) <= 64 segments; per segment, over the pixels that are not NaN and
 * (when d_mask is given) have no mask bit other than "cosmic ray":
 *   d_out[seg][8] f64 = { n, median (np.median of float32: float32 mean of the two middle
 *   elements for even n), mean, sigma (ddof 0), n_low = #(x <= median),
 *   sigma_low = sqrt(sum_{x<=median} (x - median)^2 / (n_low - 1)), 0, 0 }
 * The medians are exact order statistics (bracketed select, no sort).                   */
int bbx_rect_stats(bbx_ctx *ctx, int ny, int nx, int stride, const float *d_data,
                   const uint8_t *d_mask, int ysz, int xsz, double *d_out, void *stream);

/* ---- a8 (MBMEAN, MBRDN, MBIASM{c}, MBRDN{c}, MD*): sigma-clipped statistics ------------
 * replaces astropy.stats.sigma_clipped_stats(x, mask_value=0) of master_prep
 * (blackbox.py:5167-5230; sigma 3, maxiters 5, centre = median, spread = std): per segment
 * (same segmentation and validity rules as bbx_rect_stats, plus skip_zero: pixels equal to
 * 0 are masked) [maxiters] rounds of clipping about the exact median, then
 * d_out[seg][8] = { n, median, mean, sigma, ... } of the survivors.  The reference feeds a
 * random 20 % subsample (unseeded); all pixels are used here.                             */
int bbx_rect_clipped_stats(bbx_ctx *ctx, int ny, int nx, int stride, const float *d_data,
                           const uint8_t *d_mask, int ysz, int xsz, double sigma, int maxiters,
                           int skip_zero, double *d_out, void *stream);

/* ---- a16 (Z-SCMED, Z-SCSTD, Z-FPEMED, Z-FPESTD): sigma-clipped statistics of a whole frame -------------------
 * replaces the sigma_clipped_stats calls zogy's optimal_subtraction makes on the Scorr and Fpsferr frames for its
 * header (3 sigma, 5 rounds, centre = median, spread = std, mask_value 0).  zogy feeds a random subset of the
 * pixels; here the sample is the lattice of every [step]-th pixel of both axes of the contiguous [ny][nx] frame.
 * Pixels with mask bits other than the cosmic-ray flag, non-finite values (astropy masks them) and (skip_zero)
 * zeros do not take part.  d_out[8] = { n, median, mean, sigma, 0, 0, 0, 0 } of the survivors of [maxiters] rounds:
 * the first four numbers of bbx_rect_clipped_stats on the lattice as one segment (exact medians; the float64 sums are
 * taken in another order), from one sort instead of a bracketed select per round.                              */
int bbx_frame_clipped_stats(bbx_ctx *ctx, int ny, int nx, const float *d_img, const uint8_t *d_mask, int step,
                            double sigma, int maxiters, int skip_zero, double *d_out, void *stream);

/* ---- a8 (GAINCF): channel scaling of the master flat copy ---------------------------
 * replaces `master_median_corr[data_sec_red[c]] /= med` and `*= ratio` (blackbox.py:5104,
 * 5139-5140): float32 IEEE division / multiplication of a rectangle in place.            */
int bbx_rect_scale(bbx_ctx *ctx, int ny, int nx, int stride, float *d_data, float factor,
                   int divide, void *stream);

/* ---- f3: reference co-add (buildref.py) ----------------------------------------------
 * bbx_coadd_prep replaces the array arithmetic of prep_inputimages (buildref.py:2602-2624,
 * 2709-2733): d_data -= d_bkg (d_bkg may be NULL: image already background-subtracted);
 * d_data[mask == edge_value] = 0; d_weights = 1 / d_bkg_std**2 where d_bkg_std != 0, else 0,
 * and 0 where (mask & discard_bits) != 0 (pass discard_bits = 0 for a single image, as the
 * reference only discards when len(imtable) > 1).  float32 throughout, bit-identical to numpy.
 *
 * bbx_resample_lanczos3 replaces SWarp's resampling step (-RESAMPLING_TYPE LANCZOS3,
 * buildref.py:1748): for each output pixel the input position comes from the bilinear
 * interpolation (float64) of d_grid [gny][gnx][2] = exact (x, y) input coordinates (0-based
 * pixel centres) at output pixels (j*gstep, i*gstep) -- SWarp evaluates the projection on such
 * a lattice too; the grid must extend one node past the last output pixel.  Data: 6x6
 * normalised LANCZOS3 taps times fscale (-FSCALE_KEYWORD); weights travel as variances through
 * the same kernel (x fscale^2); a footprint that leaves the input or holds a zero-weight pixel
 * gives weight 0.
 *
 * bbx_coadd_combine replaces SWarp's -COMBINE_TYPE step (buildref.py:1733, 1815) over n <= 32
 * resampled planes d_cube / d_wcube [n][plane_stride]: pixels with weight > 0 take part;
 * float64 sums in plane order.  CLIPPED (Gruen et al. 2014, -CLIP_SIGMA / -CLIP_AMPFRAC,
 * buildref.py:1780-1788): values further than clip_sigma*sqrt(1/w) + clip_ampfrac*|median|
 * from the median of the valid values are dropped, then WEIGHTED; d_clipmask [n][npix] (1 =
 * dropped), d_nsigma [n][npix] (deviation of the dropped values in sigma, 0 elsewhere) and
 * d_nclip [n] take SWarp's clip log (-CLIP_WRITELOG); all three optional.                    */
#define BBX_COMBINE_WEIGHTED 0
#define BBX_COMBINE_AVERAGE  1
#define BBX_COMBINE_MEDIAN   2
#define BBX_COMBINE_CLIPPED  3
#define BBX_COMBINE_MIN      4
#define BBX_COMBINE_MAX      5
#define BBX_COMBINE_SUM      6
int bbx_coadd_prep(bbx_ctx *ctx, int64_t npix, float *d_data, const float *d_bkg,
                   const float *d_bkg_std, const uint8_t *d_mask, int discard_bits,
                   int edge_value, float *d_weights, void *stream);
int bbx_resample_lanczos3(bbx_ctx *ctx, int in_ny, int in_nx, const float *d_in,
                          const float *d_win, int out_ny, int out_nx, const double *d_grid,
                          int gny, int gnx, int gstep, float fscale, float *d_out,
                          float *d_wout, void *stream);
int bbx_coadd_combine(bbx_ctx *ctx, int n, int64_t npix, const float *d_cube,
                      const float *d_wcube, int64_t plane_stride, int combine_type,
                      float clip_sigma, float clip_ampfrac, float *d_out, float *d_wout,
                      uint8_t *d_clipmask, float *d_nsigma, int64_t *d_nclip, void *stream);
/* bbx_clipped2mask replaces clipped2mask_loop + pass_filters (buildref.py:3686-3873) for one
 * input image: d_clip / d_nsigma = that image's plane of bbx_coadd_combine's clip mask and
 * deviations (the clip log, output frame); every clipped pixel with |nsigma| > min(fsigma) is
 * carried to the input frame through the same lattice d_grid as the resampling (rounding
 * `(x + 0.5).astype(uint16)` on 1-based positions), then the filters run in order: points with
 * |nsigma| > fsigma[k] that are not masked yet add 1 to an fsize x fsize box of a count image
 * (positive and negative deviations apart); where a count reaches fmax, the fsize x fsize box
 * ending at that pixel is masked; fsize == 1 masks the points themselves (the reference uses
 * fsize = [5, 1], fsigma = [nsigma_clip, 4], fmax = [4, 1]).  Masked pixels within
 * sqrt(dist2_limit) = 5 S-FWHM of a pixel with (data_mask & sat_bits) are released; d_weights
 * of the others are set to 0 (the second, WEIGHTED pass then ignores them).  d_mask_im
 * [in_ny][in_nx] receives the mask, d_nmasked the number of zeroed weights.  Integer work:
 * identical to the numpy code. */
int bbx_clipped2mask(bbx_ctx *ctx, int out_ny, int out_nx, const uint8_t *d_clip,
                     const float *d_nsigma, const double *d_grid, int gny, int gnx, int gstep,
                     int in_ny, int in_nx, const uint8_t *d_data_mask, int sat_bits,
                     float dist2_limit, int nfilt, const int *h_fsize, const float *h_fsigma,
                     const int *h_fmax, float *d_weights, uint8_t *d_mask_im,
                     int64_t *d_nmasked, void *stream);

/* ---- f2: FITS tile compression (fpack, blackbox.py:812-857) ------------------------
 * RICE_1, one tile per image row, block size 32; float32 images are quantised like CFITSIO's
 * fits_quantize_float with SUBTRACTIVE_DITHER_1 (noise from the 2nd/3rd/5th order MAD of the
 * row, delta = noise / qlevel) -- byte-identical to CFITSIO for the same ZDITHER0.
 *  bbx_fpack_tiles : d_img [ny][nx] of bitpix -32 (float32) / 8 / 16 / 32, d_rnd = CFITSIO's
 *    10000-value random table (float32) for bitpix -32, dither_seed = ZDITHER0 in 1..10000.
 *    d_scratch: ny * bbx_fpack_tile_stride(nx, bytepix) bytes, receives each row's stream at
 *    its stride; d_tiles [ny] of {u32 nbytes, u32 flag, f64 zscale, f64 zzero} (flag 1: row
 *    not quantisable, 2: non-finite pixel).
 *  bbx_fpack_gather: copies the streams to d_heap at d_offsets[row] (int64).              */
size_t bbx_fpack_tile_stride(int nx, int bytepix);
int bbx_fpack_tiles(bbx_ctx *ctx, int ny, int nx, const void *d_img, int bitpix, float qlevel,
                    int dither_seed, const float *d_rnd, uint8_t *d_scratch, void *d_tiles,
                    void *stream);
int bbx_fpack_gather(bbx_ctx *ctx, int ny, int nx, int bitpix, const uint8_t *d_scratch,
                     const void *d_tiles, const long long *d_offsets, uint8_t *d_heap,
                     void *stream);
/* The same compression in ONE enqueue, down to the bytes of the file: tile streams, their offsets (prefix sum on the
 * device) and the descriptor table of the COMPRESSED_IMAGE extension (big-endian) -- d_body = [ny rows of
 * {int32 len, int32 off [, int32 gzlen = 0, int32 gzoff = 0, float64 ZSCALE, float64 ZZERO]}][heap].  No host round
 * trip between the steps, so a lane can queue it behind the kernels that make the image (reference: fpack of the
 * products that are kept, blackbox.py:812-857, 3933-4035).  d_scratch: ny * bbx_fpack_tile_stride bytes; d_tiles:
 * ny * 24 bytes; d_offsets: ny int64; d_info: (4 + max_list) int64 = [heap bytes, rows listed, 1 = heap larger than
 * cap_body - table (nothing gathered), longest stream, rows the quantiser refused (length 0 in the table: the
 * host stores them gzip-compressed behind the heap, as CFITSIO does)]. */
int bbx_fpack_body(bbx_ctx *ctx, int ny, int nx, const void *d_img, int bitpix, float qlevel, int dither_seed,
                   const float *d_rnd, uint8_t *d_scratch, void *d_tiles, long long *d_offsets, uint8_t *d_body,
                   long long cap_body, long long *d_info, int max_list, void *stream);
/* the same of [scale] x the float image (bitpix -32), the product taken as the pixels are loaded -- float32, the bytes of
 * compressing the multiplied image: `_trans_limmag` = T-NSIGMA x Fpsferr (set_blackbox.py:160-162) is then never made as a
 * frame of its own (a 4N write and a 4N read of HBM per frame less) */
int bbx_fpack_body_scaled(bbx_ctx *ctx, int ny, int nx, const void *d_img, int bitpix, float qlevel, int dither_seed,
                          const float *d_rnd, uint8_t *d_scratch, void *d_tiles, long long *d_offsets, uint8_t *d_body,
                          long long cap_body, long long *d_info, int max_list, float scale, void *stream);


/* ---- a1 / f2: funpack -- reading tile-compressed images (raw frames arrive as .fits.fz;
 * read_hdulist, blackbox.py:1451) -------------------------------------------------------
 * Rice decode of row tiles: d_desc [ny][2] int32 = (length, heap offset) of each row's
 * stream, d_heap = the table heap (+ 16 readable bytes of padding).  out_kind: 0 uint8,
 * 1 uint16 = int16 + 32768 (BZERO), 2 int16, 3 int32, 4 float32 = SUBTRACTIVE_DITHER_1
 * un-quantisation ((q - r + 0.5) * ZSCALE + ZZERO).  Rows with length 0 are left untouched
 * (losslessly stored rows are filled in by the host).                                     */
int bbx_funpack_tiles(bbx_ctx *ctx, int ny, int nx, int bytepix, const int *d_desc,
                      const uint8_t *d_heap, int out_kind, void *d_out, const double *d_zscale,
                      const double *d_zzero, int dither_seed, const float *d_rnd, void *stream);

/* Uncompressed raw frames: FITS stores BITPIX 16 pixels big-endian with BZERO 32768 (read_hdulist, blackbox.py:1451:
 * astropy scales them on the host).  bbx_raw_be16: n pixels as they lie in the file -> uint16 = byteswap(x) ^ 0x8000 in
 * one pass on the device (round 4 did this with four frame-sized tensor passes of the host framework). */
int bbx_raw_be16(const void *d_file_pixels, uint16_t *d_out, size_t n, void *stream);
/* The same for the 32-bit images a process reads before its first frame (master bias and flat: read_hdulist at
 * blackbox.py:1677, 1823; the reference image of the subtraction): n big-endian words as they lie in the file -> host
 * order, in place allowed.  The host uploads the file's bytes untouched instead of swapping 446 MB per image on one core. */
int bbx_be32(const void *d_file_words, void *d_out, size_t n, void *stream);

/* ---- a7: nonlin_corr (blackbox.py:7394-7437; set_bb.correct_nonlin is False upstream) ----
 * per channel: counts = data/gain[c]; frac = spline_c(counts) where counts <= 50000, else 1
 * (sic: uncorrected pixels end up divided by 2, reproduced as written); data /= frac + 1.
 * The splines are scipy UnivariateSpline objects in the reference's pickle; here their
 * (t, c, k) arrays, evaluated like FITPACK splev.
 *  bbx_nonlin_set : degree k (1..5), h_nknots[16], h_t / h_c [16][256] float64 (rows padded to
 *                   256 entries).  h_nknots == NULL switches the correction off again.  While
 *                   set, bbx_calibrate applies it between the overscan and the bias steps
 *                   (its place in blackbox_reduce, 1604-1624).
 *  bbx_nonlin_corr: the function on its own, in place on an overscan-corrected frame.      */
int bbx_nonlin_set(bbx_ctx *ctx, int degree, const int32_t *h_nknots, const double *h_t,
                   const double *h_c);
int bbx_nonlin_corr(bbx_ctx *ctx, const bbx_geom *g, float *d_data, const float *h_gain,
                    void *stream);

/* ---- a9 (second half): mask_init tail + fill_sat_holes ---------------------------
 * replaces mask_init 4504-4562 (crosstalk flags of saturated pixels in the 15
 * other channels, NOBJ-SAT label count, 3x3 dilation -> saturated-connected) and
 * fill_sat_holes 4584-4596 (3x3 closing + hole filling, new pixels where the
 * mask was 0).  Uses the saturated-pixel queue left by bbx_calibrate.
 *  d_nobj_sat [1] i32                                                           */
int bbx_mask_finish(bbx_ctx *ctx, const bbx_geom *g, uint8_t *d_mask,
                    int32_t *d_nobj_sat, void *stream);

/* ---- a10: LA-Cosmic ----------------------------------------------------------------
 * replaces cosmics_corr 4259-4370 = astroscrappy.detect_cosmics(sepmed=False,
 * cleantype='medmask', gain=1, satlevel=inf) + mask update + NCOSMICS label count.
 * In place: d_data becomes the cleaned array, CR pixels get bit 2 in d_mask.
 *  readnoise : RDNOISE in e-; if d_rdn16 != NULL it is instead taken on the device as
 *  float32(nanmean(d_rdn16[0..15])) (the 16 RDN{c} of bbx_vos_std), sparing a host hop.
 *  d_stats [16] i32 : [0..niter-1] pixels flagged per iteration, [6] number of
 *  8-connected CR objects, [7] total CR pixels, [8+2k],[9+2k] (k<4) work-list sizes of
 *  iteration k (pruned candidates, first-growth survivors) for diagnostics.                                  */
int bbx_lacosmic(bbx_ctx *ctx, int ny, int nx, float *d_data, uint8_t *d_mask,
                 float sigclip, float sigfrac, float objlim, int niter,
                 float readnoise, const double *d_rdn16, int32_t *d_stats,
                 void *stream);

/* ---- a11: crosstalk -------------------------------------------------------------------
 * replaces xtalk_corr 7138-7258.  h_coeffs[source*16 + victim], float64.          */
int bbx_xtalk(bbx_ctx *ctx, const bbx_geom *g, float *d_data, const uint8_t *d_mask,
              const double *h_coeffs /*[256]*/, void *stream);

/* ---- a13: mask_header counts + edge fill ---------------------------------------------
 * replaces mask_header 4601-4620 (d_counts[6] i64: bad, edge, saturated,
 * saturated-connected, satellite trail, cosmic ray -- pixels with that bit set)
 * and the edge fill 1959-1974 (edge pixels <- np.median of their channel;
 * d_chan_median [16] f32 also returned).                                        */
int bbx_mask_counts(bbx_ctx *ctx, int64_t npix, const uint8_t *d_mask,
                    int64_t *d_counts, void *stream);
int bbx_edge_fill(bbx_ctx *ctx, const bbx_geom *g, float *d_data,
                  const uint8_t *d_mask, float *d_chan_median, void *stream);

/* ---- a8: master frames ------------------------------------------------------------------
 * replaces master_prep 4906-5073: per-pixel np.median of nframes (<= 32) reduced
 * calibration frames; each frame is first divided by h_norm[i] (flats: MEDSEC of
 * 4929-4941; NULL or 1 for bias/dark; 0 = leave as is); with flat_fix != 0 pixels that
 * are BPM-edge (== 32) or <= 0 become 1 (5071-5073).
 *  h_frames : host array of nframes device pointers, each npix float32.             */
int bbx_median_stack(bbx_ctx *ctx, int64_t npix, int nframes, const float *const *h_frames,
                     const float *h_norm, const uint8_t *d_bpm, int flat_fix,
                     float *d_out, void *stream);

/* ---- a12: satellite trails (sat_detect, blackbox.py:4163-4254) ------------------------------
 * The reference calls acstools.satdet.detsat(buf=40, sigma=3, h_thresh=0.2) + make_mask(sigma=5)
 * [EXT: acstools is not in the image; its probabilistic Hough transform draws random pixels, ASTA
 * is a CNN without weights].  Specified in oracle/sattrail.py: 2x2 sum binning; acstools' front end
 * (percentile (4.5, 93) rescale, skimage Canny sigma 3 with thresholds 0.1 / 0.2 of the maximum,
 * remove_small_objects(60): pinned against scikit-image); full Hough accumulator over ntheta angles
 * with skimage.transform.hough_line's cells (h_cos_sin[2*k], [2*k+1] = cos, sin of theta_k, float64,
 * supplied by the host so that both sides use the same table; acstools' grid is 2 .. 177.5 deg in
 * half-degree steps); strongest line with >= 210 votes whose supporting edge pixels reach within
 * 40 px of both frame borders; perpendicular profile, strip -> bit 16 in d_mask.
 *  h_gauss [gauss_radius + 1] : scipy.ndimage's Gaussian weights for sigma = 3, centre first
 *                               (radius int(4 sigma + 0.5) = 12), float64, from the host like the angles.
 *  d_nsats [1] i32 : 8-connected objects of bit 16 (NSATS).
 *  d_info [8] f32  : largest binned pixel, smallest binned pixel, votes of the best cell, its theta index,
 *                    its rho, strips painted, 1 = a segment went to make_mask, 1 = a trail was masked.  */
int bbx_sat_trails(bbx_ctx *ctx, int ny, int nx, const float *d_data, uint8_t *d_mask,
                   const double *h_cos_sin, int ntheta, const double *h_gauss, int gauss_radius,
                   int32_t *d_nsats, float *d_info, void *stream);

/* bbx_sat_trails_state: the decisions of the last bbx_sat_trails call on this context, for tests.  ny, nx and
 * ntheta are those of that call; nothing else may have run on the context in between (the values sit in a
 * shared workspace).  Waits for the stream and copies; launches nothing.
 *  h_state [BBX_SAT_NSTATE] f64 (host), integers as exact doubles:
 *    0 accept (the line passed the vote, refinement, support and segment tests), 1 seg_ok (a segment went to
 *    make_mask), 2 found (a trail was masked), 3 k (theta index), 4 votes, 5 rho,
 *    6 t0, 7 t1 (where the cell's line enters / leaves the binned frame, position along the line),
 *    8 tmin, 9 tmax (extent of the supporting edge pixels along the line; NaN: none seen),
 *    10 icpt, 11 slope (refined line), 12..15 segment x0, y0, x1, y1 (binned pixels),
 *    16 rot_rows, 17 rot_cols (rotated frame), 18 sx, 19 sy (the segment's first point there),
 *    20 band_r0, 21 band_rows (rows of the rotated frame that were interpolated),
 *    22 nwin (strips painted), 23 row_min, 24 row_max (their row range).
 *  h_rects [4 * max_rects] i32 (host): the first min(nwin, max_rects) strips as r0, r1, c0, c1 (rotated
 *    frame, half-open), in the order of the walk.                                                        */
#define BBX_SAT_NSTATE 25
int bbx_sat_trails_state(bbx_ctx *ctx, int ny, int nx, int ntheta, double *h_state, int32_t *h_rects,
                         int max_rects, void *stream);

/* bbx_canny_edge_map: the front end of bbx_sat_trails on its own (parity tests against scikit-image):
 * np.percentile(img, (4.5, 93)) + skimage.exposure.rescale_intensity + skimage.feature.canny(sigma from
 * h_gauss, low / high = low_frac / high_frac x the rescaled maximum) + remove_small_objects(min_size,
 * connectivity 8) of a float32 image -> d_map [ny*nx] u8 (1 = edge), *d_count = number of edge pixels. */
int bbx_canny_edge_map(bbx_ctx *ctx, int ny, int nx, const float *d_img, const double *h_gauss,
                       int gauss_radius, double low_frac, double high_frac, int min_size,
                       uint8_t *d_map, int32_t *d_count, void *stream);

/* ---- a15: background mesh (zogy.get_back / mini2back; buildref.py:2398-2405, 2480-2495) ----
 * [EXT algorithm: conventions in oracle/zogy_core.py]
 * bbx_bkg_boxstats: per box x box tile (box <= 64, divides ny and nx) the sigma-clipped
 *   (median centre, 3 sigma, <= 5 iterations) median and std of the pixels with mask == 0,
 *   objmask == 0 (optional) and value != 0; boxes with fewer than limfrac*box^2 usable
 *   pixels are NaN.  d_mini_* : (ny/box)*(nx/box) float32.
 * bbx_mini_fill_filter: NaN boxes <- nan-median of the 3x3 neighbourhood (repeated),
 *   then 3x3 median filter (edge replicated), in place.
 * bbx_spline_zoom: evaluates scipy.ndimage.zoom(order=3, mode='nearest') from prefiltered
 *   B-spline coefficients d_coef[cny][cnx] (float64) with per-output-row / -column tap
 *   bases d_fy/d_fx (floor index into coef) and weights d_wy/d_wx ([n][4] float64);
 *   writes the background to d_bkg (if non-NULL) and subtracts it from d_data (if non-NULL).
 * bbx_spline_prefilter: the coefficients themselves, on the device: the mini image d_mini[nby][nbx] (float32) cut into
 *   blocks of cy x cx boxes (cy = nby, cx = nbx: one block; the channel blocks for interp_Xchan = False), every block
 *   padded by [npad] edge samples (scipy.ndimage.zoom pads 'nearest' inputs by 12) and run through
 *   scipy.ndimage.spline_filter(order = 3, mode = 'nearest') -> d_coef[(nby/cy)(cy+2 npad)][(nbx/cx)(cx+2 npad)] float64,
 *   bit for bit scipy's values (gcc builds).  zn_y = pow(z, cy + 2 npad), zn_x = pow(z, cx + 2 npad) with
 *   z = sqrt(3) - 2 correctly rounded (-0.2679491924311227), computed by the caller's libm.               */
int bbx_bkg_boxstats(bbx_ctx *ctx, int ny, int nx, int box, const float *d_data,
                     const uint8_t *d_mask, const uint8_t *d_objmask, float limfrac,
                     float *d_mini_med, float *d_mini_std, void *stream);
int bbx_mini_fill_filter(bbx_ctx *ctx, int nby, int nbx, float *d_mini, void *stream);
int bbx_spline_prefilter(bbx_ctx *ctx, int nby, int nbx, int cy, int cx, int npad, double zn_y, double zn_x,
                         const float *d_mini, double *d_coef, void *stream);
/* bbx_mini_median: np.median of a float32 device array of n values (exact order statistics; an even count gives the
 * float32 mean of the middle pair as numpy does; NaN if the array holds one) -> d_med[0].  S-BKGSTD = the median of the
 * sigma mini image (zogy's header value) without a round trip through the host.
 * bbx_zoom_candidates(ctx, d_med, nsigma): the NEXT bbx_spline_zoom_sub call of this context also lists the pixels of
 * the frame it writes with |value| >= (float)(d_med[0] * nsigma) -- the candidates of the source catalogue (peaks above
 * cat_nsigma x S-BKGSTD) -- and bbx_find_peaks on that frame with that threshold starts from the list instead of a
 * pass of its own over the frame (a threshold that is not that number raises the device's list-overflow flag: a failed
 * search, not a wrong one).  d_med = NULL: off. */
int bbx_mini_median(bbx_ctx *ctx, int n, const float *d_a, float *d_med, void *stream);
int bbx_zoom_candidates(bbx_ctx *ctx, const float *d_med, double nsigma);
int bbx_spline_zoom(bbx_ctx *ctx, int ny, int nx, const double *d_coef, int cny, int cnx,
                    const int32_t *d_fy, const double *d_wy, const int32_t *d_fx,
                    const double *d_wx, float *d_data, float *d_bkg, void *stream);
/* the same with separate input and output: d_out = d_in - background (d_in stays as it is) */
int bbx_spline_zoom_sub(bbx_ctx *ctx, int ny, int nx, const double *d_coef, int cny, int cnx,
                        const int32_t *d_fy, const double *d_wy, const int32_t *d_fx,
                        const double *d_wx, const float *d_in, float *d_out, void *stream);

/* ---- a16: ZOGY sub-image subtraction (zogy.optimal_subtraction -> run_ZOGY; call sites
 * blackbox.py:2350-2354, 2460-2465) with rocFFT.  [EXT algorithm: Zackay, Ofek & Gal-Yam
 * 2016; conventions in oracle/zogy_core.py]
 * bbx_cut_subimages / bbx_stitch_subimages: (ny/size)*(nx/size) tiles of size^2 with a
 *   zero-padded border -> [nsub][L][L], L = size + 2*border, and back (borders dropped).
 * bbx_zogy_subimages: per sub-image new N, ref R (background-subtracted), PSFs Pn, Pr
 *   (unit sum, centred on pixel [0,0]), variance images Vn, Vr; h_scal[nsub][6] =
 *   sigma_n, sigma_r, f_n, f_r, dx, dy.  Outputs D, S, S_corr, F_psf, F_psf_err.
 *   Inputs are used as FFT sources (not modified).                                    */
/* helpers: V = max(data,0) + bkg_std^2 ; PSF stamps [nsub][S][S] -> [nsub][L][L] centred on [0,0] */
int bbx_variance(bbx_ctx *ctx, int64_t n, const float *d_data, const float *d_bkgstd,
                 float *d_var, void *stream);
int bbx_embed_psf(bbx_ctx *ctx, int nsub, int S, int L, const float *d_stamps, float *d_out,
                  void *stream);
int bbx_cut_subimages(bbx_ctx *ctx, int ny, int nx, int size, int border,
                      const float *d_img, float *d_subs, void *stream);
int bbx_stitch_subimages(bbx_ctx *ctx, int ny, int nx, int size, int border,
                         const float *d_subs, float *d_img, void *stream);
int bbx_zogy_subimages(bbx_ctx *ctx, int L, int nsub, float *d_new, float *d_ref,
                       float *d_pn, float *d_pr, float *d_vn, float *d_vr,
                       const float *h_scal, float *d_D, float *d_S, float *d_Scorr,
                       float *d_Fpsf, float *d_Fpsferr, void *stream);

/* bbx_zogy_frame: the same subtraction for a whole frame in one call, with the library's own 2-D
 * FFT (bbx_zogy2.hip: 1-D transforms in LDS, transposition folded into the store patterns, the
 * ZOGY algebra in the registers of the column passes) instead of rocFFT + separate element-wise
 * kernels; the cut into (ny/size)*(nx/size) sub-images of side L = size + 2*border (zero-padded
 * at the frame edge), the variance images V = max(d, 0) + sigma^2 and the stitching of the
 * results are part of its kernels.
 *   d_new, d_ref         : background-subtracted frames [ny][nx] (ref on the new frame's grid)
 *   d_sig_new, d_sig_ref : background sigma images [ny][nx]
 *   d_psf_n, d_psf_r     : unit-sum PSF stamps [nsub][S][S] (centre at S/2)
 *   h_scal [nsub][6]     : sigma_n, sigma_r, f_n, f_r, dx, dy
 *   d_D, d_Scorr, d_Fpsf, d_Fpsferr (and d_S, may be NULL) : full frames [ny][nx]
 * Supported sub-image sides: bbx_zogy_frame_supported(L) != 0 (1400 = the reference's
 * 1320 + 2*40, and 64 / 128 / 140 for tests); other sizes go through bbx_zogy_subimages.
 * S = S_n - S_r is formed in real space (identical in exact arithmetic to the inverse transform
 * of S^ that bbx_zogy_subimages takes). */
int bbx_zogy_frame_supported(int L);
/* bbx_zogy_candidates(ctx, thr): thr > 0: the following bbx_zogy_frame calls of this context also list the pixels with
 * |Scorr| >= thr as they write them ([EXT] zogy's get_trans thresholds |Scorr| at transient_nsigma of its settings file,
 * 6 in the deployment: Settings/set_qc.py:387); bbx_find_peaks on that very Scorr frame with the same threshold then starts from the list
 * instead of a pass of its own over the frame (same regions, same peaks).  0 switches the listing off. */
int bbx_zogy_candidates(bbx_ctx *ctx, float thr);
int bbx_zogy_frame(bbx_ctx *ctx, int ny, int nx, int size, int border, const float *d_new,
                   const float *d_ref, const float *d_sig_new, const float *d_sig_ref,
                   const float *d_psf_n, const float *d_psf_r, int S, const float *h_scal,
                   float *d_D, float *d_S, float *d_Scorr, float *d_Fpsf, float *d_Fpsferr,
                   void *stream);

/* bbx_zogy_frame_mini: bbx_zogy_frame with the two sigma images given as their mini images instead of frames.  zogy makes
 * the full-frame sigma image of each side with mini2back(data_bkg_std_mini, ...) [EXT; call sites buildref.py:2480-2495] only
 * to form the variance images: here the kernel that cuts the sub-images reads sigma off the B-spline coefficients of the
 * mini image (bbx_spline_prefilter's output; one patch per channel for the new frame: interp_Xchan False), so the two
 * frames are never written to HBM nor read back (2 x 4N bytes written, 2 x 4N x (L / size)^2 read per frame of N pixels).
 * Per pixel the spline is evaluated as a float32 cubic of the float64-folded coefficients: within 3e-7 (relative) of
 * what bbx_spline_zoom writes (csrc/bbx_spline.h).  Needs frames whose groups of four pixels are aligned (size, border,
 * nx, channel width multiples of 4; 16-byte aligned pointers), BBX_ERR_ARG otherwise: callers then zoom the mini images
 * (bbx_spline_zoom) and use bbx_zogy_frame. */
typedef struct {
    const double *d_coef;      /* bbx_spline_prefilter output: [(nby / cy) * (cy + 2 npad)][(nbx / cx) * (cx + 2 npad)] */
    int32_t nby, nbx;          /* mini image shape in boxes; the frame is nby * box by nbx * box pixels */
    int32_t cy, cx;            /* boxes per patch: (nby, nbx) = one patch, (boxes per channel) = one patch per channel */
    int32_t box, npad;         /* box size [pix]; padding of every patch in boxes (12 = scipy.ndimage.zoom's) */
} bbx_spline_image;
int bbx_zogy_frame_mini(bbx_ctx *ctx, int ny, int nx, int size, int border, const float *d_new,
                        const float *d_ref, const bbx_spline_image *sig_new, const bbx_spline_image *sig_ref,
                        const float *d_psf_n, const float *d_psf_r, int S, const float *h_scal,
                        float *d_D, float *d_S, float *d_Scorr, float *d_Fpsf, float *d_Fpsferr,
                        void *stream);

/* Prepared reference (the names keep "rows": the buffer held the row transforms at first; it now holds the finished
 * spectra).  The row pass of bbx_zogy_frame transforms each side on its own: the new frame and its variance
 * image in one launch, the reference and its variance image in another (the two-for-one transforms pair neighbouring rows
 * of one image).  The reference's half depends on d_ref, its sigma map and the geometry alone; a caller whose
 * reference stays the same from frame to frame (one --ref per image list) makes it once, into a buffer of its own, and
 * tells the contexts that run its frames.  So does the forward column pass of the two: the buffer holds the 2-D half spectra
 * R^ (first half) and Vr^ (second half), each [sub][column group][entry] in the order the column kernels walk their lines,
 * and the frame call's column kernels read their entries straight into registers instead of transforming the reference again.  The library keeps no copy and cannot see whether the reference's pixels changed:
 * the buffer, and the promise that it still belongs to d_ref, are the caller's.
 *   bbx_zogy_refrows_bytes      : size of the buffer for this geometry (2 half spectra per sub-image, 1.01 GB for 64
 *                                 sub-images of 1400^2); 0 where the geometry has no aligned row path (size, border, nx
 *                                 multiples of 4, a supported sub-image side)
 *   bbx_zogy_refrows_fill[_mini]: the reference's row pass (into the context's work arrays) and column pass (into d_rows,
 *                                 16-byte aligned) on the stream, with the sigma map as a frame or as its mini image -- the
 *                                 same transforms on the same data as an unprepared bbx_zogy_frame[_mini] call runs, so
 *                                 the results with and without are equal bit for bit
 *   bbx_zogy_refrows            : sticky, per context (like bbx_zogy_candidates): the following bbx_zogy_frame[_mini] calls
 *                                 of this context skip the reference's row and column pass and read d_rows instead.  ref_sigma is the
 *                                 reference sigma's identity: d_sig_ref, or sig_ref->d_coef of the mini form.  A frame call
 *                                 with another d_ref, reference sigma, ny, nx, size or border returns BBX_ERR_ARG rather than
 *                                 use rows of another reference.  d_rows = NULL clears the setting (the other arguments are
 *                                 then ignored).  One buffer may serve several contexts once its fill has completed. */
size_t bbx_zogy_refrows_bytes(int ny, int nx, int size, int border);
int bbx_zogy_refrows_fill(bbx_ctx *ctx, int ny, int nx, int size, int border, const float *d_ref,
                          const float *d_sig_ref, void *d_rows, void *stream);
int bbx_zogy_refrows_fill_mini(bbx_ctx *ctx, int ny, int nx, int size, int border, const float *d_ref,
                               const bbx_spline_image *sig_ref, void *d_rows, void *stream);
int bbx_zogy_refrows(bbx_ctx *ctx, const void *d_rows, int ny, int nx, int size, int border,
                     const float *d_ref, const void *ref_sigma);

/* Prepared reference PSF.  The spectrum Pr^ of the reference's PSF stamps depends on the stamps d_psf_r [nsub][S][S] and
 * the geometry alone; a caller whose reference PSF stays the same over many frames makes it once, into a buffer of its
 * own, beside the prepared rows.  (The new frame's PSF changes from frame to frame and stays per-frame work.)
 *   bbx_zogy_refpsf_bytes : size of the buffer: nsub half spectra of G column groups x NL lines x L points of 8 bytes
 *                           (505 MB for 64 sub-images of 1400^2); 0 wherever bbx_zogy_refrows_bytes is 0
 *   bbx_zogy_refpsf_fill  : the row DFTs of the stamps (into the context's work array) and their pruned column transform
 *                           (into d_out, 16-byte aligned) on the stream -- the transform an unprepared frame call runs on
 *                           the same data, so the results with and without are equal bit for bit
 *   bbx_zogy_refpsf       : sticky, per context: the following bbx_zogy_frame[_mini] calls transform the new stamps only
 *                           and read Pr^ from d_spec.  Identity is by pointer, as for the reference frame: the library keeps
 *                           no copy and cannot see whether the stamps' values changed.  A frame call with another d_psf_r
 *                           pointer, S, ny, nx, size or border returns BBX_ERR_ARG, and so does one while no prepared rows
 *                           are set (bbx_zogy_refrows); nothing is written then.  d_spec = NULL clears the setting (the
 *                           other arguments are then ignored).  One buffer may serve several contexts once its fill has
 *                           completed. */
size_t bbx_zogy_refpsf_bytes(int ny, int nx, int size, int border);
int bbx_zogy_refpsf_fill(bbx_ctx *ctx, int ny, int nx, int size, int border, const float *d_psf_r, int S,
                         void *d_out, void *stream);
int bbx_zogy_refpsf(bbx_ctx *ctx, const void *d_spec, int ny, int nx, int size, int border,
                    const float *d_psf_r, int S);

/* ---- a17: PSFEx model evaluation [EXT: zogy.get_psf / psfex poly] ----------------------
 * stamp[s][p] = sum_k terms[s][k] * basis[k][p]: terms [nsrc][ncoef] f32 = the polynomial
 * terms x'^i y'^j (i + j <= poldeg, PSFEx order) of each source position, basis
 * [ncoef][npix] f32 = the PSF_MASK cube of the .psf file, out [nsrc][npix] f32.  f32 MFMA
 * (v_mfma_f32_32x32x2_f32): k-ordered float32 fma chain.                                  */
int bbx_psf_model(bbx_ctx *ctx, int nsrc, int ncoef, int npix, const float *d_terms,
                  const float *d_basis, float *d_out, void *stream);

/* ---- a17: PSF-weighted optimal flux (zogy.get_psfoptflux) at integer positions:
 * flux = sum(P D / V) / sum(P^2 / V), err = 1 / sqrt(sum(P^2 / V)) over an S x S stamp of
 * the unit-sum PSF model d_psfs[nsrc][S][S] centred on (d_ys, d_xs); pixels off the frame
 * or with V <= 0 are skipped.                                                          */
int bbx_psf_optflux(bbx_ctx *ctx, int ny, int nx, const float *d_D, const float *d_V,
                    const float *d_psfs, int S, int nsrc, const int32_t *d_ys,
                    const int32_t *d_xs, float *d_flux, float *d_err, void *stream);
/* the same on a background-subtracted frame d_D with its sigma image: V = max(D, 0) + sigma^2 is formed
 * per stamp pixel (float32, as bbx_variance would) instead of being written out for the whole frame */
int bbx_psf_optflux_sigma(bbx_ctx *ctx, int ny, int nx, const float *d_D, const float *d_sigma,
                          const float *d_psfs, int S, int nsrc, const int32_t *d_ys,
                          const int32_t *d_xs, float *d_flux, float *d_err, void *stream);
/* the same with sigma read off its mini image at the stamp pixels (bbx_zogy_frame_mini's companion: no sigma frame exists) */
int bbx_psf_optflux_mini(bbx_ctx *ctx, int ny, int nx, const float *d_D, const bbx_spline_image *sigma,
                         const float *d_psfs, int S, int nsrc, const int32_t *d_ys,
                         const int32_t *d_xs, float *d_flux, float *d_err, void *stream);

/* ---- a17: transient candidates: 8-connected regions of |img| >= thr (|S_corr| >= T-NSIGMA,
 * set_qc.py:387); per region the pixel of largest |value| (first in C order on ties).
 * d_yx[max_out][2] (y, x), d_val[max_out], *d_count = number of regions (may exceed max_out,
 * only the first max_out in arbitrary order are stored).                                  */
int bbx_find_peaks(bbx_ctx *ctx, int ny, int nx, const float *d_img, float thr, int max_out,
                   int32_t *d_yx, float *d_val, int32_t *d_count, void *stream);

/* ---- generic: number of 8-connected objects of (mask & bit) --------------------------
 * replaces ndimage.label(..., structure=ones(3,3)) counts (NOBJ-SAT 4545,
 * NCOSMICS 4355, NSATS 4230).                                                     */
int bbx_count_objects(bbx_ctx *ctx, int ny, int nx, const uint8_t *d_mask,
                      int bit, int32_t *d_count, void *stream);

/* ---- object mask of a background-subtracted frame (zogy's `_objmask` product, whose SExtractor rules
 * are [EXT]: the rules here are THIS PROJECT'S OWN).  d_img[ny][nx] f32: the frame minus its first-pass background;
 * d_sig_mini[ny/box][nx/box] f32: that pass's sigma mini image (box divides ny and nx).
 *   detection image: filter != 0: the 3x3 pyramid (1 2 1 / 2 4 2 / 1 2 1) / 16 with the frame's edge replicated, in float32 as
 *     (((nw+ne)+(sw+se)) + 2((n+s)+(w+e)) + 4c) * 0.0625; filter == 0: the pixel itself
 *   a pixel is listed iff thr = (float)nsigma * sigma[y/box][x/box] > 0 and thr <= filt < inf (a NaN or non-positive sigma lists
 *     nothing in its box, a NaN or an infinity under the 3x3 nothing there); no mask is consulted
 *   8-connected components of the listed pixels with fewer than minarea pixels are dropped
 *   d_objmask[ny][nx] u8 = 1 within dy^2 + dx^2 <= grow^2 (0 <= grow <= 8) of a pixel of a component that stays, 0 elsewhere
 * d_counts[3] i32: pixels listed, components kept, pixels set.  The pixel list holds max_pixels entries (<= 0: max(npix / 8,
 * min(npix, 65536))); more listed pixels raise the device's list-overflow flag (bbx_sync: BBX_ERR_OVERFLOW) and the mask
 * is then that of the pixels that fit: not to be used. */
int bbx_object_mask(bbx_ctx *ctx, int ny, int nx, const float *d_img, const float *d_sig_mini, int box,
                    double nsigma, int minarea, int grow, int filter, int64_t max_pixels,
                    uint8_t *d_objmask, int32_t *d_counts, void *stream);

/* ---- a17: transient thumbnails (THUMBNAIL_RED / _REF / _D / _SCORR of the transient catalogue, qc.py:480-485;
 * [EXT] zogy.get_trans cuts them) and FLAGS_MASK.  d_img: HOST array of the four device frames [ny][nx] f32 in the
 * order RED (background-subtracted new frame), REF (background-subtracted reference on the new frame's grid), D,
 * SCORR; d_ys / d_xs: n integer peak positions (0-based).  d_out[n][4][size][size] f32: cut-out k covers rows
 * y - size/2 ... y - size/2 + size - 1 and the columns likewise, so the peak is pixel [size/2][size/2].
 * d_flags[n] u8 (NULL: not wanted): OR of d_new_mask, and of d_ref_mask when not NULL, over the flag_win x flag_win
 * window centred on the peak.
 * zogy's own footprint of the flags and its padding at the frame edge are [EXT] without a source in the reference
 * tree.  The two conventions here are THIS PROJECT'S OWN: pixels off the frame are 0 in the cut-outs and contribute
 * nothing to the flags; the flag window is a square of flag_win (settings.trans_flags_window) pixels.            */
int bbx_thumbnails(bbx_ctx *ctx, int ny, int nx, const float *const *d_img, int n, const int32_t *d_ys,
                   const int32_t *d_xs, int size, const uint8_t *d_new_mask, const uint8_t *d_ref_mask,
                   int flag_win, float *d_out, uint8_t *d_flags, void *stream);

/* ---- the 8-bit display planes of the thumbnail PNG files: per stamp what save_thumbs_row does
 * (blackbox.py:2786-2808): np.flipud, astropy ZScaleInterval().get_limits (1000 strided samples of the finite
 * values in C order, sorted; iterative line fit with 0/1 weights, krej 2.5, max_reject 0.5, min_npixels 5, at most 5
 * iterations, rejections grown by max(1, int(npix * 0.01)) with numpy.convolve's 'same' alignment; contrast 0.25;
 * sample minimum / maximum when too few samples survive) in float64, the weighted least-squares line in closed
 * form; then scale_data (blackbox.py:2814-2826) in float32 as numpy does it: x - f32(vmin), / f32(vmax - vmin)
 * (difference formed in float64), * 255, three separately rounded operations, clipped to [0, 255], truncated.
 * d_stamps[n_stamps][size][size] f32 -> d_out_u8[n_stamps][size][size] (row 0 = top row of the PNG; 4-byte aligned),
 * d_limits[n_stamps][2] f64 = (vmin, vmax) (NULL: not wanted).  A stamp with vmax == vmin or without a finite value
 * gives zeros (limits (0, 0) in the second case) -- our convention: the reference divides by zero there; NaN
 * pixels give 0.  One workgroup per stamp, the stamp in LDS: BBX_ERR_ARG when size * size * 4 bytes plus the
 * kernel's 5.4 KB of sample buffers exceed the 64 KB of a workgroup (size <= 122).                                */
int bbx_thumb_png8(bbx_ctx *ctx, int n_stamps, int size, const float *d_stamps, uint8_t *d_out_u8,
                   double *d_limits, void *stream);

/* ---- flux ratio and astrometric scatter of a frame against its reference from matched stars (the fratio, dx, dy that
 * bbx_zogy_frame takes per sub-image; header keys Z-DX / Z-DY / Z-DXSTD / Z-DYSTD / Z-FNR / Z-FNRSTD / Z-FNRERR,
 * set_qc.py:370-375, 425).  The shape of the computation is buildref.py:2782-3014 (get_fratio, "simplified version of
 * zogy.get_fratio_dxdy"): matches within dist_max = 2 arcsec, fratio = flux_new / flux_ref over pairs with both fluxes
 * non-zero (2965-2966), its error fratio * sqrt((e_n / f_n)^2 + (e_r / f_r)^2) (2969-2971), a minimum of 15 matches
 * (2992), sigma-clipped statistics.  [EXT] zogy.get_fratio_dxdy, get_matches and get_mean_fratio themselves are not in
 * the reference tree: where the statements above are silent the rules below are THIS PROJECT'S OWN.
 * All three entries are deterministic: no float atomics, every sum in a fixed order, same input -> same bits.         */
#define BBX_MATCH_CAP 8192      /* pairs of one segment that enter its statistics (one 32 KB LDS buffer) */

/* Iterated Gaussian-windowed centroid (the SExtractor XWIN recurrence) of nsrc sources of the frame d_img[ny][nx] at the
 * integer peaks (d_ys, d_xs): starting at the peak, w_i = exp(-r_i^2 / (2 sigma_w^2)) * I_i over the (2 radius + 1)^2
 * pixels around the INTEGER peak (radius <= 10; pixels off the frame contribute nothing), c <- c + 2 sum w_i (p_i - c) /
 * sum w_i, niter times, in float32.  sigma_w = d_sigw[tile] of the sub-image tile (size x size pixels, nsy x nsx
 * tiles, indices clamped) the integer peak lies in.  d_off[nsrc][2] = (dy, dx) RELATIVE TO THE INTEGER PEAK (an absolute
 * float32 coordinate near 10560 has an ulp of 1e-3 px).  Own conventions: the offset is (NaN, NaN) -- and the source then
 * matches nothing -- when sigma_w is not positive and finite, when in any iteration sum w_i is not positive or a sum
 * is not finite, or when the centroid moves further than radius / 2 from the integer peak in y or in x (it has then
 * left the part of the window that still holds the source).  One wave per source, the window in registers, no LDS. */
int bbx_win_centroid(bbx_ctx *ctx, int ny, int nx, const float *d_img, int nsrc, const int32_t *d_ys,
                     const int32_t *d_xs, const float *d_sigw, int size, int nsy, int nsx, int radius, int niter,
                     float *d_off, void *stream);

/* One-to-one match of two source lists A (new) and B (reference), each given as integer peaks + float32 offsets
 * [n][2] = (dy, dx) and SORTED BY (y, x) OF THE INTEGER PEAK ([EXT] get_matches; own rules).  distance^2 is formed in
 * float32 as (dy_int + d off_y)^2 + (dx_int + d off_x)^2.  For each a: the nearest b with distance <= dist_max
 * (inclusive; ties: the lower index) among the b whose integer peak is within ceil(dist_max + 1) rows and columns of
 * a's (offsets are sub-pixel: what lies beyond that band is never a match); the same for each b; d_match[n_a] = that b
 * where the choice is mutual, else -1.  A source with a NaN offset matches nothing.  d_best_b[n_b]: scratch of the
 * caller (nearest a of every b).  n_a == 0: nothing is done.                                                      */
int bbx_match_mutual(bbx_ctx *ctx, int n_a, const int32_t *d_a_ys, const int32_t *d_a_xs, const float *d_a_off,
                     int n_b, const int32_t *d_b_ys, const int32_t *d_b_xs, const float *d_b_off, float dist_max,
                     int32_t *d_best_b, int32_t *d_match, void *stream);

/* Clipped statistics of the matched pairs per segment: the nsy x nsx sub-image tiles (size x size pixels, no border)
 * and, last, the whole frame.  A pair (a, b = d_match[a]) qualifies for a segment when it is matched, both fluxes are
 * > 0 (buildref.py:2965 asks != 0; a negative flux has no ratio), flux / err >= snr_min on both sides (own rule), and
 * a's integer peak lies in the tile.  More than BBX_MATCH_CAP qualifying pairs: every s-th in list order, s = ceil(n /
 * BBX_MATCH_CAP) (own rule: a deterministic sample over the whole segment).  Quantities, float32: fr = f_a / f_b,
 * dx = x_a - x_b, dy = y_a - y_b (integer difference + offset difference).  Each is clipped like astropy's
 * sigma_clipped_stats defaults (oracle/zogy_core.box_stats: 3 sigma about the exact median, population std, at most 5
 * rounds, stop when nothing is clipped); an even count's median is the midpoint of the two float32 values formed in
 * float64; sums are float64.  d_out[nsy * nsx + 1][16] float64 = {n_qualifying, n_fr, med_fr, mean_fr, std_fr, wmean_fr,
 * werr_fr, n_dx, med_dx, mean_dx, std_dx, n_dy, med_dy, mean_dy, std_dy, stride s}; wmean_fr, werr_fr: the inverse-
 * variance weighted mean of the clipped fr sample and 1 / sqrt(sum 1 / sigma_i^2), sigma_i = buildref.py:2969-2971
 * ([EXT] get_mean_fratio(weighted=True)).  An empty segment: the four counts 0, s = 1, NaN elsewhere.
 * n_a == 0: nothing is done (d_out is not written).  One workgroup of 1024 threads per segment, 33 KB of LDS.      */
int bbx_match_stats(bbx_ctx *ctx, int n_a, const int32_t *d_a_ys, const int32_t *d_a_xs, const float *d_a_off,
                    const float *d_a_flux, const float *d_a_err, int n_b, const int32_t *d_b_ys,
                    const int32_t *d_b_xs, const float *d_b_off, const float *d_b_flux, const float *d_b_err,
                    const int32_t *d_match, int size, int nsy, int nsx, float snr_min, double *d_out, void *stream);

/* ---- source shapes of the full-source catalogue and the frame's seeing / elongation statistics: the header keys S-NOBJ,
 * S-FWHM, S-FWSTD, S-SEEING, S-SEESTD, S-ELONG, S-ELOSTD (blackbox.py:3051-3057), which set_qc range-checks (S-SEEING
 * min_max, S-ELONG sigma (1.1, 0.2): set_qc.py:256-266).  In zogy these numbers come from SExtractor ([EXT]: neither is in
 * the reference tree); here they are the published adaptive second moments (Bernstein & Jarvis 2002, AJ 123, 583;
 * Hirata & Seljak 2003, MNRAS 343, 459): parity with the reference's values is UNPINNED, the rules below are THIS
 * PROJECT'S OWN.  Both entries are deterministic: every sum in a fixed order, same input -> same bits.
 *
 * bbx_src_shapes: per source, over the (2 radius + 1)^2 pixels around the INTEGER peak (d_ys, d_xs) (1 <= radius <= 10;
 * pixels off the frame contribute 0), all in float32: c = offset from the peak, starting at d_off[src] (bbx_win_centroid);
 * W = window covariance, starting at sigma_w^2 I, sigma_w = d_sigw[tile of the integer peak].  Each of niter >= 1 rounds:
 * w_k = exp(-1/2 d^T W^-1 d) I_k with d = p_k - c; s0 = sum w, m = sum w d / s0, M = sum w d d^T / s0 - m m^T;
 * c <- c + 2 m; T^-1 = M^-1 - W^-1; W <- T.  (For a Gaussian source of covariance C seen through a Gaussian window W
 * the weighted moments are M^-1 = C^-1 + W^-1, so T = C; the fixed point W = T is the matched window.)
 * The source fails, and its whole row is NaN, when d_off is not finite, sigma_w is not positive and finite, s0 <= 0,
 * det M <= 0 or Myy <= 0, |c_y| or |c_x| > radius / 2, T^-1 is not positive definite (det <= 0 or (T^-1)yy <= 0),
 * Tyy + Txx > 2 (radius / 2)^2, or anything is not finite.
 * d_out[nsrc][8] = {c_y, c_x, Tyy, Txx, Txy, FWHM = 2 sqrt(ln 2 (Tyy + Txx)), ELONGATION = sqrt(A^2 / B^2) with A^2, B^2 =
 * ((Tyy + Txx) +- sqrt((Txx - Tyy)^2 + 4 Txy^2)) / 2, THETA = 1/2 atan2(2 Txy, Txx - Tyy) in degrees from +x}.
 * d_flags[nsrc] u8 = OR of d_mask over the window pixels on the frame (d_mask NULL: 0), written for failed sources too.
 * nsrc == 0: nothing is done.  One wave per source, the window in registers, no LDS.                                  */
int bbx_src_shapes(bbx_ctx *ctx, int ny, int nx, const float *d_img, const uint8_t *d_mask, int nsrc,
                   const int32_t *d_ys, const int32_t *d_xs, const float *d_off, const float *d_sigw, int size, int nsy,
                   int nsx, int radius, int niter, float *d_out, uint8_t *d_flags, void *stream);

/* Clipped statistics of FWHM and ELONGATION (columns 5, 6 of d_shapes[nsrc][8]) per segment: the nsy x nsx sub-image tiles
 * and, last, the whole frame.  The list is SORTED BY (y, x) of the integer peak.  A source qualifies when its FWHM and
 * ELONGATION are finite, d_flags is 0, err > 0, flux / err >= snr_min and its integer peak lies in the tile.  Selection
 * (every s-th in list order above BBX_MATCH_CAP), sort and clipping are bbx_match_stats's, by the same device code.
 * d_out[nsy * nsx + 1][8] float64 = {n_qualifying, stride s, n_fwhm, med_fwhm, std_fwhm, n_elong, med_elong, std_elong};
 * an empty segment: counts 0, s = 1, NaN elsewhere.  nsrc == 0: nothing is done (d_out is not written).                */
int bbx_shape_stats(bbx_ctx *ctx, int nsrc, const int32_t *d_ys, const int32_t *d_xs, const float *d_shapes,
                    const uint8_t *d_flags, const float *d_flux, const float *d_err, int size, int nsy, int nsx,
                    float snr_min, double *d_out, void *stream);

/* ---- a PSF model from the frame's own stars (the _psf.fits product and the PSF-* header keys: blackbox.py:3085-3110,
 * set_qc.py:293-296, 408-409; bbx_psfbuild.hip).  In zogy the model comes from PSFEx ([EXT]: it is not in the reference
 * tree): parity with its numbers is UNPINNED, the rules below are THIS PROJECT'S OWN; only the form of the result -- a
 * polynomial in the normalised frame position over a cube of basis images, what bbx_psf_model evaluates -- is PSFEx's.
 * All four entries are deterministic: no float atomics, every sum in a fixed order, same input -> same bits.
 *
 * bbx_psf_select: the PSF stars of a source list SORTED BY (y, x) of the integer peak (d_ys, d_xs), with peak values d_pk,
 * the rows d_shapes[n][8] and flags d_flags[n] of bbx_src_shapes.  A source is a star when, in this order (d_reason[n] u8 =
 * 0, or the number of the first rule it fails): 1 its shape row is finite and its flags are 0; 2 pk / sigma_bkg >= snr_min;
 * 3 |FWHM / fwhm_med - 1| <= fwhm_tol and ELONGATION <= elong_max (fwhm_med: the float argument, or, where d_fwhm_med is
 * given, that device double as float -- the frame row of bbx_shape_stats without a host wait); 4 the integer peak is at
 * least V / 2 + 3 pixels from every frame edge; 5 no other source of the list with pk > iso_frac * its own pk has its
 * integer peak within Chebyshev distance V / 2 (band search over the sorted list, as bbx_match_mutual).  All in float32.
 * d_nstar[2] = {n qualifying, stride s}, s = ceil(n qualifying / cap) (1 where they fit); d_star[cap] = the indices of every
 * s-th star in list order (ceil(n qualifying / s) entries; the rest is not written), by a prefix count, not by atomics.
 * V odd, <= 49; 1 <= cap <= BBX_MATCH_CAP.  n == 0: d_nstar = {0, 1}.
 *
 * bbx_psf_stamps: one V x V vignette per star s < nstar, of source src = d_star[s] (d_star NULL: src = s) of the list
 * (d_ys, d_xs, d_shapes, d_sig: per source), centred on its CENTROID (c_y, c_x) = d_shapes[src][0..1]: pixel (r, c) is the
 * LANCZOS3 interpolation of the frame at (y + c_y + r - V/2, x + c_x + c - V/2), separable, six taps per axis about the
 * floor, each axis' taps normalised to unit sum (float64, then float32; the co-add's kernel), a row pass then a column
 * pass, float32 products added in float32 in tap order.  norm = sum of the vignette pixels with (r - V/2)^2 + (c - V/2)^2
 * <= (V/2)^2 in float64; I = vignette / norm (float64 division, then float32); w = 1 / var (float32) with var = q (max(
 * vignette, 0) + sigma^2) / norm^2 + (acc I)^2 in float64, sigma = d_sig[src], q = (sum wy^2)(sum wx^2) the variance
 * factor of the resampling (covariances neglected).  The star fails -- d_ok[s] = 0, d_norm[s] = 0, its I and w all 0 --
 * when its centroid or sigma is not finite, any of the (V + 5)^2 pixels under the vignette and its taps is off the frame
 * or not finite, d_mask (may be NULL) is set under the V x V pixels about the floor of the centroid, or norm is not
 * positive and finite.  d_nstar (may be NULL): the device pair of bbx_psf_select; stars s >= ceil(n / stride) fail
 * likewise, so nstar can be the capacity.  One workgroup per star, the window in LDS.
 *
 * bbx_psf_fit: per vignette pixel p the weighted least squares min sum_s w_sp (I_sp - sum_k a_kp t_sk)^2 over the stars
 * with d_ok[s] != 0 and, where d_chi2 is given, d_chi2[s] <= clip * d_chi2_med[0] (float32; a NaN never passes).
 * d_terms[nstar][ncoef] float32 (the PSFEx polynomial terms), ncoef = 1, 3, 6 or 10.  Normal matrix and right-hand side in
 * float64, stars in list order within each of the workgroup's 8 shares, the shares added in order; Cholesky in float64.
 * A pixel whose matrix is not positive definite (a pivot <= 1e-13 of its diagonal element) gets 0 in every plane and
 * raises the device error word (BBX_ERR_NOTCONV at the next bbx_sync).  d_basis[ncoef][V][V] float32.
 *
 * bbx_psf_chi2: d_chi2[s] = sum_p w_sp (I_sp - model_sp)^2 / V^2 as float32, model_sp = the float32 fma chain over k of
 * t_sk basis_kp (bbx_psf_model's arithmetic), difference, square and sum in float64 in a fixed order; NaN where d_ok[s]
 * is 0.  One workgroup per star.                                                                                      */
int bbx_psf_select(bbx_ctx *ctx, int n, const int32_t *d_ys, const int32_t *d_xs, const float *d_pk,
                   const float *d_shapes, const uint8_t *d_flags, float sigma_bkg, float snr_min, float fwhm_med,
                   const double *d_fwhm_med, float fwhm_tol, float elong_max, float iso_frac, int V, int ny, int nx,
                   int cap, uint8_t *d_reason, int32_t *d_star, int32_t *d_nstar, void *stream);
int bbx_psf_stamps(bbx_ctx *ctx, int ny, int nx, const float *d_img, const uint8_t *d_mask, int nsrc,
                   const int32_t *d_ys, const int32_t *d_xs, const float *d_shapes, const float *d_sig, int nstar,
                   const int32_t *d_star, const int32_t *d_nstar, int V, float acc, float *d_I, float *d_w,
                   double *d_norm, uint8_t *d_ok, void *stream);
int bbx_psf_fit(bbx_ctx *ctx, int nstar, int V, int ncoef, const float *d_I, const float *d_w, const float *d_terms,
                const uint8_t *d_ok, const float *d_chi2, const float *d_chi2_med, float clip, float *d_basis,
                void *stream);
int bbx_psf_chi2(bbx_ctx *ctx, int nstar, int V, int ncoef, const float *d_I, const float *d_w, const float *d_terms,
                 const float *d_basis, const uint8_t *d_ok, float *d_chi2, void *stream);

/* ---- catalogue photometry with the PSF on the source's CENTROID (bbx_psfphot.hip): bbx_psf_optflux_sigma /
 * _mini with the stamp formed, shifted and normalised inside the kernel -- zogy.get_psfoptflux shifts the PSF image to the
 * source position ([EXT]: not in the reference tree; the rules below are THIS PROJECT'S OWN).  Per source s < nsrc at the
 * integer peak (d_ys, d_xs) of the background-subtracted frame d_D[ny][nx], S odd, <= 49:
 *  1 the stamp P[S][S]: with d_terms[nsrc][nplane] (model form, nplane = ncoef <= 64) the float32 fma chain over k of
 *    d_terms[s][k] d_cube[k][p] in k order (bbx_psf_model's arithmetic; the terms are those of the integer peak); with
 *    d_idx[nsrc] (plane form) the plane d_cube[d_idx[s]] of d_cube[nplane][S * S] (an index outside [0, nplane) is clamped).
 *    Exactly one of d_terms, d_idx is given.
 *  2 the shift to (dy, dx) = d_off[s] (bbx_win_centroid: relative to the integer peak), separable, a row pass (along x) then
 *    a column pass: per axis l = floor(-d), frac = -d - l in float32, out[i] = sum_{t = -2..3} w_t(frac) P[i + l + t] with P = 0
 *    outside [0, S), w = the six LANCZOS3 taps normalised to unit sum (float64, then float32: bbx_psf_stamps's, the co-add's
 *    kernel), float32 products added in float32 in tap order.  frac == 0: the taps are (0, 0, 1, 0, 0, 0) and the pass is the
 *    copy out[i] = P[i + l], so a zero offset leaves the stamp bit for bit.  An offset that is not finite or beyond 16 pixels
 *    in either axis is no centroid: the stamp stays unshifted, flag 1.
 *  3 norm = sum of the S x S pixels in float64; P / norm in float64.  A norm that is not positive and finite: flux = err =
 *    0, flag 4.
 *  4 num = sum P D / V, den = sum P^2 / V in float64 with V = max(D, 0) + sigma^2 in float32 (bbx_variance's), sigma from
 *    the frame d_sigma[ny][nx] or read off the mini image sigma_mini at the pixel (bbx_psf_optflux_mini's; within 3e-7
 *    of the frame's value) -- exactly one of the two is given.  Skipped: pixels off the frame; on the frame, in this order,
 *    d_mask != 0 (d_mask may be NULL; flag 2), D not finite, V not positive (a NaN sigma included).  The estimator is
 *    unbiased on any subset of the pixels.
 *  5 d_flux[s] = num / den, d_err[s] = 1 / sqrt(den) as float32, both 0 where den is not positive; d_flags[s] u8 = 1 (no
 *    centroid) | 2 (a masked pixel was skipped) | 4 (the stamp has no sum).
 * Deterministic: no atomics, every sum in a fixed order (per thread over pixels tid, tid + 256, ..., then the wave, then
 * the four waves in order), same input -> same bits.  nsrc == 0: nothing is launched.  One workgroup of 256 per source, the
 * stamp in LDS (19.2 KB): nothing but flux, err and flags is written.                                                   */
int bbx_psf_optflux_shift(bbx_ctx *ctx, int ny, int nx, const float *d_D, const float *d_sigma,
                          const bbx_spline_image *sigma_mini, const uint8_t *d_mask, int S, int nplane,
                          const float *d_cube, const float *d_terms, const int32_t *d_idx, int nsrc,
                          const int32_t *d_ys, const int32_t *d_xs, const float *d_off, float *d_flux, float *d_err,
                          uint8_t *d_flags, void *stream);

/* ---- aperture photometry with a local sky annulus (bbx_aper.hip): the model-independent fluxes of the catalogue,
 * E_FLUX_APER_R<r>xFWHM / E_FLUXERR_APER_R<r>xFWHM of qc.py:489-502 (set_zogy.apphot_radii).  zogy's get_apflux and SExtractor are
 * [EXT], not in the reference tree: only the column names and the radii follow the reference, the rules below are THIS PROJECT'S
 * OWN and parity with zogy's numbers is unpinned.  Any image and any positions: per source s < nsrc at the integer peak (d_ys, d_xs)
 * of d_D[ny][nx], all geometry in float64 and no product contracted into an fma:
 *  1 centre = peak + d_off[s] = (dy, dx) (bbx_win_centroid: relative to the peak; d_off NULL: zeros).  An offset that is not finite,
 *    or beyond 1e6 pixels in either axis, is no centroid: the peak alone, flag 1.
 *  2 f = d_fwhm[tile of the integer peak], tile = min(max(y / size, 0), nsy - 1) * nsx + the same of x (zogy.tile_index's clamp);
 *    r_k = (double) radii[k] * (double) f for the naper <= BBX_APER_NMAX apertures (radii: a HOST array, in FWHM),
 *    r_in, r_out = (double) sky_in * f, (double) sky_out * f.
 *  3 too big, flag 32: f not positive and finite, or the largest r_k or r_out beyond BBX_APER_RMAX pixels.  Every float of the row is
 *    NaN, n = 0, nothing else is measured.  (The bound sizes the kernel: a window of at most 97 x 97 pixels, at most
 *    pi (48 + 0.71)^2 = 7454 pixel centres in the annulus, which fit the 8192 floats of one 32 KB LDS buffer.)
 *  4 a pixel iy, ix lies at dy = (double)(iy - yp) - (double) off_y, dx likewise; d^2 = dy dy + dx dx.  It is USED when it is on the
 *    frame, d_mask == 0 there (d_mask may be NULL), D is finite and sigma is finite; sigma from the frame d_sigma[ny][nx] or read off
 *    the mini image sigma_mini (bbx_psf_optflux_shift's: exactly one of the two), V = max(D, 0) + sigma^2 in float32.
 *  5 the weight of a pixel in aperture k is the exact area of the disc of radius r_k inside the unit pixel: 1 when the farthest corner
 *    is inside, (|dx| + 1/2)^2 + (|dy| + 1/2)^2 <= r^2; 0 when the nearest point is not, max(|dx| - 1/2, 0)^2 + max(|dy| - 1/2, 0)^2
 *    >= r^2; otherwise the clipped chord height integrated over the pixel's x-range [max(|dx| - 1/2, -r), min(|dx| + 1/2, r)], split at
 *    +-sqrt(r^2 - y0^2), +-sqrt(r^2 - y1^2) (y0, y1 = |dy| -+ 1/2; the four clamped into the range and sorted), with
 *    G(x) = (x sqrt(r^2 - x^2) + r^2 asin(x / r)) / 2; on each piece the top is the flat edge y1 (y1 <= h at the midpoint, h = sqrt(r^2
 *    - m^2)) or the arc, the bottom the flat edge y0 (y0 >= -h) or the arc; the sum clamped to [0, 1].  No sub-pixel sampling.
 *  6 S_k = sum w D, A_k = sum w, V_k = sum w V over the used pixels, in float64.  Flag 2: a pixel that the largest aperture touches
 *    (weight > 0: its nearest point inside) is on the frame and not used; flag 4: such a pixel lies off the frame.
 *  7 the sky sample: the used pixels with r_in^2 <= d^2 < r_out^2, whole pixels by their centres; flag 16 when such a pixel is not used
 *    or off the frame.  Sorted and clipped by bbx_match_stats's rule (3 sigma about the exact median -- an even count: the float64
 *    midpoint --, population std, at most 5 rounds, stop when nothing is clipped) -> sky, sd, n.  n < sky_nmin (>= 1): flag 8, the
 *    sky outputs are (NaN, NaN, n) and nothing is subtracted.
 *  8 F_k = S_k - sky A_k when sub_sky is set and flag 8 is not, else S_k; E_k = sqrt(V_k + [sky subtracted] A_k^2 (pi / 2) sd^2 / n);
 *    A_k == 0: both NaN.  d_flux[s][k], d_err[s][k], d_sky[s] = (sky, sd, n) as float32, rounded once; d_flags[s] u8.
 * Deterministic: the sample's order of arrival in LDS does not reach the result (it is sorted), every sum is taken in a fixed order
 * (per thread over its pixels, then the crossed pixels its wave noted, the wave, the four waves in order): same input -> same bits.
 * nsrc == 0: nothing is launched, the outputs may be NULL.  One workgroup of 256 per source.                                  */
#define BBX_APER_RMAX 48        /* [pix] largest aperture or annulus radius */
#define BBX_APER_NMAX 8         /* apertures of one call */
int bbx_aper_phot(bbx_ctx *ctx, int ny, int nx, const float *d_D, const float *d_sigma,
                  const bbx_spline_image *sigma_mini, const uint8_t *d_mask, int nsrc, const int32_t *d_ys,
                  const int32_t *d_xs, const float *d_off, const float *d_fwhm, int size, int nsy, int nsx, int naper,
                  const float *radii, float sky_in, float sky_out, int sub_sky, int sky_nmin, float *d_flux, float *d_err,
                  float *d_sky, uint8_t *d_flags, void *stream);

/* ---- limiting-flux image of the reduced frame (bbx_limflux.hip): `_red_limmag.fits` and the keys LIMEFLUX, LIMFNU,
 * LIMMAG of blackbox.py:3151-3153.  The quantity is what bbx_psf_optflux* return as err, taken at every pixel: the error of the
 * PSF-weighted optimal flux of a faint source centred there, on sky noise alone, times nsigma.  zogy.get_psfoptflux(
 * get_limflux_array=True) is [EXT], not in the reference tree: only the file name, the key names and the 5 sigma convention follow
 * the reference, the rules below are THIS PROJECT'S OWN and parity with zogy's numbers is unpinned.
 *  1 the tile of the output pixel (y, x): t = min(max(y / size, 0), nsy - 1) * nsx + the same of x (zogy.tile_index's clamp: a frame
 *    that is no multiple of size gives the rest to the last tile).  d_planes[nsy * nsx][S][S]: unit-sum stamps, S odd, <= 49, the
 *    centre at S / 2.
 *  2 Q_t[j][i] = (P_t[j][i] / norm_t)^2 in float64, norm_t = the float64 sum of the plane; Q rounded to float32 once.  A norm_t
 *    that is not positive and finite: every pixel of the tile is 0, d_win[t] = 0.
 *  3 the window T_t: the smallest odd T <= S for which the float64 sum of Q over the central T x T pixels is at least (1 - frac)
 *    times the float64 sum over all S x S (both sums ring by ring, outwards, each ring row-major; O(S^2) per tile); frac == 0:
 *    T_t = S.  frac in [0, 1), anything else BBX_ERR_ARG.  d_win[t] = T_t (d_win may be NULL).  Q is NOT renormalised to the
 *    window: on a uniform background the limit is high by at most frac / 2 (relative).  The window is made on the device by a small
 *    kernel of the same call, no host wait.
 *  4 W(iy, ix) = min(1.0f / (sigma * sigma), the largest finite float32) in float32 (a sigma below 5e-20, whose square underflows,
 *    gives that largest number, not inf: every W is finite), sigma from the frame d_sigma[ny][nx] or read off the mini image sigma_mini at
 *    the pixel (bbx_psf_optflux_shift's reader: within 3e-7 of the frame's value) -- exactly one of the two, else BBX_ERR_ARG.
 *    W = 0 off the frame, where d_mask != 0 (d_mask may be NULL), and where sigma is not finite or not positive.  Sky noise only:
 *    no max(D, 0) term, this is the limit for a faint source.
 *  5 den(y, x) = sum over j, i in [-k, k], k = T_t / 2, h = S / 2, of Q_t[h + j][h + i] W(y + j, x + i): float32 fma chain, i
 *    outermost, then j, both ascending.  No atomics: same input -> same bits.
 *  6 d_lim[y][x] = nsigma / sqrt(den) as float32, 0 where den is not positive.  The pixel's own mask value plays no part beyond 4:
 *    a masked pixel gets the limit of a source centred on it.
 *  7 ny * nx == 0: nothing is launched.
 * Two kernels: the windows (one workgroup per tile), then blocks of 64 x 32 output pixels laid out per tile, W of block + halo in
 * LDS, Q read as a wave-uniform operand, eight outputs per lane.  2 T^2 ny nx FLOP.                                             */
#define BBX_LIMFLUX_SMAX 49     /* largest stamp side */
int bbx_limflux_image(bbx_ctx *ctx, int ny, int nx, const float *d_sigma, const bbx_spline_image *sigma_mini,
                      const uint8_t *d_mask, int S, const float *d_planes, int size, int nsy, int nsx,
                      float nsigma, double frac, float *d_lim, int32_t *d_win, void *stream);

/* ---- transient vetting: the PSF of D per sub-image and its fit to D per candidate (bbx_transfit.hip).  zogy fits
 * the PSF of the difference image to D at every candidate with free position (E_FLUX_PSF_D, X_PSF_D, Y_PSF_D, CHI2_PSF_D) ([EXT]:
 * zogy is not in the reference tree; the rules below are THIS PROJECT'S OWN, parity is unpinned).
 *
 * bbx_zogy_pd_stamps: d_pd[nsub][S][S] float32, the PSF of D of every sub-image, from the stamps d_pn, d_pr [nsub][S][S] (unit
 * sum, centre at S / 2; S odd, <= 49) and h_scal[nsub][6] = (sn, sr, fn, fr, dx, dy), a HOST array as bbx_zogy_frame takes it:
 *  1 on an M x M grid (M even, 4 S <= M <= 512) both stamps are embedded with their centre on the origin and transformed;
 *  2 PD^ = (fr fn / fD) Pr^ Pn^ / sqrt(sn^2 fr^2 |Pr^|^2 + sr^2 fn^2 |Pn^|^2), fD = fr fn / sqrt(sn^2 fr^2 + sr^2 fn^2); 0 where
 *    the denominator is 0;
 *  3 back to real space, p[M][M]; the S x S pixels around the origin, divided by their sum, are the stamp;
 *  4 d_fold[sub] = (sum |p| over the grid - sum |p| over the stamp) / sum |p| over the grid: what the cut leaves out.
 * Every step in float64 (plain matrix DFTs with twiddles from sincospi: rows over S taps, columns over S rows; only the columns
 * kx <= M / 2 are made, p is real), sums in a fixed order, no atomics; the stamp is rounded to float32 at the end.  A sub-image
 * whose sn, sr, fn or fr is not finite and positive, or whose stamps or p have no positive finite sum: a zero stamp, fold = 1.
 * Workspace (nsub M (M / 2 + 1) complex128 and less) from the context.  nsub == 0: nothing is launched.
 *
 * bbx_trans_psffit: per candidate c < ncand at the integer peak (y0, x0) = (d_ys[c], d_xs[c]), sub-image k = min(y0 / size, nsy - 1)
 * nsx + min(x0 / size, nsx - 1) (nsy = nsub / nsx), window of W x W pixels around the peak (W odd, 3 <= W <= S - 10):
 *  - used pixels: on the frame, d_mask == 0 (d_mask may be NULL; a pixel left out for it: flag 2), D finite, V_D positive and
 *    finite, V_D = (fr^2 Vn + fn^2 Vr) / (fr fn)^2 in float32 with Vn = max(N, 0) + sigma_n^2, Vr = max(R, 0) + sigma_r^2
 *    (bbx_variance's: fmaxf, so a NaN in N or R counts 0): N = d_N, R = d_R the background-subtracted new and reference frames
 *    on the new grid, the two sigma maps as
 *    frames (d_sig_n, d_sig_r) or as mini images (mini_n, mini_r; read as bbx_psf_optflux_mini reads them) -- one form for both;
 *    fr, fn from h_scal[k] (HOST array [nsub][6], as above).  On background alone V_D = 1 / fD^2, the variance ZOGY gives D;
 *    elsewhere it is the unsmoothed approximation;
 *  - theta = (dy, dx) float32 starts at (0, 0).  niter times (1 <= niter <= 64, never fewer on the data's account):
 *      Ps = d_pd[k] shifted by theta with steps 2 and 3 of bbx_psf_optflux_shift (the same device function: row pass, column pass,
 *      float32 taps; norm in float64, Ps / norm in float64); Gx[j][i] = (Ps[j][i + 1] - Ps[j][i - 1]) / 2, Gy likewise;
 *      the weighted least squares D ~ F Ps - a Gx - b Gy over the used pixels, weights 1 / V_D: the nine sums in float64 (fixed
 *      order), the 3 x 3 system by cofactors in float64; Delta = (b / F, a / F), each component clamped to +-0.5,
 *      theta = float32(clamp(theta + Delta, +-maxshift)), 0 < maxshift <= 16.
 *      det == 0 or not finite, F == 0 or not finite, Delta not finite: the stepping stops, theta stays (flag 8);
 *  - the final pass at theta: F = sum Ps D / V / sum Ps^2 / V, err = 1 / sqrt(sum Ps^2 / V), chi2 = sum (D - F Ps)^2 / V /
 *    (n_used - 3); d_flux, d_err, d_dy, d_dx, d_chi2 float32.
 * d_flags[c] u8 = 1 (|theta| at maxshift in an axis) | 2 (a masked pixel was left out) | 4 (no fit: the peak off the frame,
 * n_used < 4, a P_D stamp without a positive sum, sum Ps^2 / V not positive; all five outputs 0) | 8 (the last unclamped
 * max(|Delta_y|, |Delta_x|) > 0.01 pixel, or the stepping stopped).  A negative candidate fits a negative F.
 * Deterministic as bbx_psf_optflux_shift: no atomics, per thread over pixels tid, tid + 256, ..., then the wave, then the four
 * waves in order.  One workgroup of 256 per candidate; the stamp, the row pass's output and the window's D and V_D in LDS
 * (31.5 KB).  ncand == 0: nothing is launched.                                                                              */
int bbx_zogy_pd_stamps(bbx_ctx *ctx, int nsub, int S, int M, const float *d_pn, const float *d_pr, const float *scal,
                       float *d_pd, float *d_fold, void *stream);
int bbx_trans_psffit(bbx_ctx *ctx, int ny, int nx, const float *d_D, const float *d_N, const float *d_R,
                     const float *d_sig_n, const float *d_sig_r, const bbx_spline_image *mini_n,
                     const bbx_spline_image *mini_r, const uint8_t *d_mask, int S, int nsub, const float *d_pd, int size,
                     int nsx, const float *scal, int ncand, const int32_t *d_ys, const int32_t *d_xs, int W, int niter,
                     float maxshift, float *d_flux, float *d_err, float *d_dy, float *d_dx, float *d_chi2,
                     uint8_t *d_flags, void *stream);

/* ---- transient vetting: an elliptical Gaussian and an elliptical Moffat fitted to D per candidate (bbx_transfit.hip, DESIGN.md
 * 4k).  zogy fits both to D at every candidate (X/Y_GAUSS_D, FWHM_GAUSS_D, ELONG_GAUSS_D, CHI2_GAUSS_D and the same of _MOFFAT_D)
 * ([EXT]: zogy is not in the reference tree; the rules below are THIS PROJECT'S OWN, parity is unpinned).
 *
 * bbx_trans_shapefit: per candidate c < ncand the window of bbx_trans_psffit, by the same device function: the same sub-image
 * k, used pixels, V_D in float32, sigma forms, mask rule and flag 2; W odd, 5 <= W <= 39 (no stamp is involved).
 *  - model m = B + A g(q), q = cyy dy^2 + 2 cxy dy dx + cxx dx^2, dy = y - y0, dx = x - x0 relative to the integer peak;
 *    g = exp(-q / 2) (Gauss) or (1 + q)^-beta (Moffat, beta > 1 given by the caller); seven parameters (A, B, y0, x0, cyy, cxy, cxx);
 *  - start: A = D at the peak pixel, or at the used pixel of largest |D| (the first in row-major order) if the peak is not used;
 *    B = y0 = x0 = 0; cyy = cxx = 4 kk / f0^2, cxy = 0 with f0 = d_fwhm0[k] (DEVICE array [nsub]) clamped to [fwhm_lo, fwhm_hi]
 *    and kk = 2 ln 2 (Gauss), 2^(1 / beta) - 1 (Moffat);
 *  - Levenberg-Marquardt, niter times (1 .. 128, never fewer on the data's account), all in float64 on the float32 D and V_D of
 *    the window: H = sum J J^T / V, g = sum J r / V, chi2 = sum r^2 / V (analytic J; 28 + 7 + 1 sums in a fixed order, no atomics);
 *    (H + lambda diag H) delta = g by Cholesky, a pivot that is not positive and finite refuses the step; trial = p + delta, y0 and
 *    x0 clamped to +-maxshift; refused for its shape (flag 16 if it is the last) if p + delta is not finite, the form is not
 *    positive definite or an axis FWHM = 2 sqrt(kk / l) (l: eigenvalue of the form) lies outside [fwhm_lo, fwhm_hi]; else accepted
 *    if chi2(trial) is finite and <= chi2.  Accepted: lambda = max(lambda / 10, 1e-9); refused: min(10 lambda, 1e9); lambda_0 = 1e-3;
 *  - d_out[model][7][ncand] float32, model 0 Gauss, 1 Moffat: y0, x0, their errors (sqrt of the diagonal of the undamped H^-1 at the
 *    final parameters), FWHM (geometric mean of the two axes), ELONG = sqrt(l1 / l2), chi2 / (n_used - 7).
 * d_flags[model][ncand] u8 = 1 (|y0| or |x0| at maxshift) | 2 (a masked pixel was left out) | 4 (no fit: the peak off the frame,
 * n_used < 8, d_fwhm0[k] not positive and finite, the final H not invertible, a result not finite, or the model not asked for in
 * `models` (1 Gauss | 2 Moffat); all seven outputs 0) | 8 (no step was ever accepted, or a parameter of the last accepted step moved
 * by more than 0.01 of its own error, errors from the undamped H at the point the step left) | 16 (the last trial was refused for
 * its shape).  A negative candidate fits a negative A.  One wave per candidate, four candidates per workgroup, the windows in LDS
 * (48.7 KB); sums per lane over pixels lane, lane + 64, ..., then the wave: same input, same bits.  ncand == 0 or models == 0:
 * nothing is launched.  h_scal: HOST array [nsub][6] as above, staged in a workspace slot of its own.                       */
int bbx_trans_shapefit(bbx_ctx *ctx, int ny, int nx, const float *d_D, const float *d_N, const float *d_R,
                       const float *d_sig_n, const float *d_sig_r, const bbx_spline_image *mini_n,
                       const bbx_spline_image *mini_r, const uint8_t *d_mask, int nsub, int size, int nsx, const float *scal,
                       const float *d_fwhm0, int ncand, const int32_t *d_ys, const int32_t *d_xs, int W, int niter,
                       float maxshift, int models, float beta, float fwhm_lo, float fwhm_hi, float *d_out, uint8_t *d_flags,
                       void *stream);

/* ---- registration of the reference on the new frame from the two star lists (bbx_align.hip).  zogy registers
 * with SWarp and two astrometric solutions ([EXT]); the method here and every rule below are THIS PROJECT'S OWN, stated in float64
 * numpy by tests/test_align_host.py (vote_ref, fit_ref, apply_ref, grid_of, remap_mask_ref).  A list is integer peaks + float32
 * offsets [n][2] = (dy, dx) + fluxes [+ errors]; A is the new frame's, B the reference's ON ITS OWN GRID.  T maps new-frame to
 * reference pixels: per axis a polynomial in u = (x - nx / 2) / (nx / 2), v likewise, terms 1, u, v, u^2, uv, v^2;
 * coef[12] = the six of x, then the six of y (degree 1: the last three of each are 0).  All entries are deterministic: integer
 * atomics only, every float64 sum in a fixed order.  Every array crosses with its extent.                                  */
#define BBX_ALIGN_NBRIGHT_MAX 2048   /* bbx_align_vote: sources of a list that vote (one 16 KB LDS sort) */
#define BBX_ALIGN_CAP_MAX     8192   /* bbx_align_vote: pairs of the winning block that are written (one 32 KB LDS sort) */

/* The vote for the coarse offset.  Of each list the nbright (<= BBX_ALIGN_NBRIGHT_MAX) brightest eligible sources (flux > 0 and
 * finite, both offsets finite; ties to the lower index), in that order: their ranks.  Every pair's d = p_A - p_B, float32 as
 * bbx_match_mutual forms it ((float)(integer difference) + (offset difference)), with |dy|, |dx| <= (float)max_shift counts into
 * bin floor((d + max_shift) / bin) (float32) of an nb x nb histogram, nb = floor(2 max_shift / bin) + 1 (< 1024).  3 x 3 block
 * sums; winner: the largest, the lowest (y, x) cell on ties; runner-up: the largest outside the winner's 5 x 5; far: the largest
 * outside +- far cells.  The winning block's pairs in row-major order of (rank in A, rank in B), the first cap (<=
 * BBX_ALIGN_CAP_MAX) of them: d_pairs[cap][2] = (index into A, index into B), (-1, -1) past those written; d_coarse[2] = medians of
 * their dy, dx (even count: the midpoint of the two float32 values in float64; none: NaN).  d_info[8] = {winner's sum, runner-up's
 * sum, winner's cell y, x, pairs written, failed, pairs found, far sum}; failed = 1 when the winner has fewer than nmin votes, is
 * not above the runner-up, or is not above the far sum f by more than 3 sqrt(f).  d_work: scratch of work_bytes >=
 * bbx_align_vote_bytes(nbright, max_shift, bin, cap) bytes (0: arguments out of range), 256-byte aligned.                       */
size_t bbx_align_vote_bytes(int nbright, double max_shift, double bin, int cap);
int bbx_align_vote(bbx_ctx *ctx, int n_a, const int32_t *d_a_ys, const int32_t *d_a_xs, const float *d_a_off,
                   const float *d_a_flux, int n_b, const int32_t *d_b_ys, const int32_t *d_b_xs, const float *d_b_off,
                   const float *d_b_flux, int nbright, double max_shift, double bin, int nmin, int far, int cap,
                   void *d_work, size_t work_bytes, int32_t *d_info, double *d_coarse, int32_t *d_pairs, void *stream);

/* The clipped least-squares fit of T (poldeg 1 or 2) to the pairs d_items[n_items][2] = (index into A, index into B); an index
 * that is negative or not below its list's length: no pair.  A pair qualifies with both fluxes > 0, flux / err >= snr_min
 * (float32) on both sides and finite offsets.  Normal equations in float64 on the basis above at the new frame's position
 * (integer + (double)offset), Cholesky (a pivot not above 1e-12 of its diagonal element: not positive definite); first all
 * qualifying pairs, then three passes that drop the pairs with r^2 > clip^2 (sx + sy) / n of those kept so far and fit again.
 * d_coef[12] (NaN before the first solve), d_stats[4] = {n_used, rms_x, rms_y, flags}, d_kept[n_items] u8: the pairs of the last
 * solve attempted.  flags: 2 fewer than max(nmin, number of terms) pairs at a solve (or an empty list), 4 not positive definite,
 * 8 determinant of the linear part in pixels outside [0.5, 2].  One workgroup; sums: per thread over items t, t + 512, ..., the
 * wave by DPP, the waves in order.                                                                                        */
int bbx_align_fit(bbx_ctx *ctx, int n_a, const int32_t *d_a_ys, const int32_t *d_a_xs, const float *d_a_off,
                  const float *d_a_flux, const float *d_a_err, int n_b, const int32_t *d_b_ys, const int32_t *d_b_xs,
                  const float *d_b_off, const float *d_b_flux, const float *d_b_err, int n_items, const int32_t *d_items,
                  int ny, int nx, int poldeg, float snr_min, double clip, int nmin, double *d_coef, double *d_stats,
                  uint8_t *d_kept, void *stream);

/* A list of the reference through the inverse of T (d_coef[12] on the device; ny, nx: the NEW frame's shape): the closed-form
 * inverse of the linear part, two Newton steps for poldeg 2, float64 operation by operation as apply_ref.  Where |x|, |y| < 1e9:
 * integer = floor(. + 0.5), offset = (float)(. - integer); else the integers of the input and a (NaN, NaN) offset.  Not sorted. */
int bbx_align_apply(bbx_ctx *ctx, int n, const int32_t *d_ys, const int32_t *d_xs, const float *d_off, const double *d_coef,
                    int ny, int nx, int poldeg, int32_t *d_oys, int32_t *d_oxs, float *d_ooff, void *stream);

/* The lattice of bbx_resample_lanczos3 from T: d_grid[gny][gnx][2] = (x, y) of T at the new frame's pixels (j step, i step).
 * The lattice must hold the node after the last pixel in both directions: BBX_ERR_ARG otherwise.                            */
int bbx_align_grid(bbx_ctx *ctx, const double *d_coef, int ny, int nx, int step, int gny, int gnx, double *d_grid,
                   void *stream);

/* The mask d_mask[in_ny][in_nx] (NULL: none) on the output grid: per output pixel the input position by the resampler's own
 * lattice interpolation (float64, its operations), the OR of the mask over the up-to-four pixels a bilinear interpolation would
 * touch (the pixel at + 1 only where the position has a fractional part on that axis: the identity lattice gives the mask back),
 * and edge_bit where the 6 x 6 LANCZOS3 footprint leaves the input (where bbx_resample_lanczos3 writes weight 0) or the position
 * is not finite (nothing is read then).  d_out[out_ny][out_nx] u8, 4-byte aligned; d_nedge[1]: pixels that got the edge bit.
 * The lattice must hold the node after the last output pixel in both directions: BBX_ERR_ARG otherwise.                     */
int bbx_remap_mask(bbx_ctx *ctx, int in_ny, int in_nx, const uint8_t *d_mask, int out_ny, int out_nx, const double *d_grid,
                   int gny, int gnx, int step, int edge_bit, uint8_t *d_out, int64_t *d_nedge, void *stream);

/* ---- fake stars (bbx_fake.hip): stars of an asked S/N added to the background-subtracted new frame IN PLACE before
 * it is cut into sub-images, and read back from Scorr / Fpsf / Fpsferr.  zogy's fake-star code is [EXT], not in the reference tree:
 * only the key names T-NFAKE, T-FAKESN follow the reference, the rules below are THIS PROJECT'S OWN and parity is unpinned.
 * Per star s < nstar at the integer pixel (d_ys, d_xs) of d_frame[ny][nx], S odd, <= 49; the first rule of 1-2 that holds is the
 * star's flag (one bit), and a flagged star adds nothing and gets 0 in its three floats:
 *  1 the stamp P[S][S] as steps 1-3 of bbx_psf_optflux_shift form it (d_terms or d_idx: exactly one; the same device functions),
 *    shifted by (dy, dx) = d_off[s], divided by its float64 sum.  FAKE_NO_PSF 8: the sum is not positive and finite, or an offset
 *    is not within [-0.5, 0.5].
 *  2 FAKE_OFF_FRAME 4: the S x S stamp about the pixel leaves the frame.  Then, in the (2 clear_half + 1)^2 window about the pixel
 *    (0 <= clear_half <= S / 2: the window lies inside the star's own stamp; clipped to the frame): FAKE_MASKED 1: d_mask_new or
 *    d_mask_ref (either may be NULL) is not 0 at a pixel; FAKE_ON_SOURCE 2: the frame's value, or d_ref's (d_ref may be NULL: the
 *    reference's background-subtracted frame on the same grid), is not finite or |value| > clear_nsigma * sigma in float32, sigma
 *    the new frame's at that pixel, from the frame d_sigma[ny][nx] or read off sigma_mini (bbx_psf_optflux_shift's reader: exactly
 *    one of the two).  FAKE_NO_FLUX 16: d_s2n[s] is not positive and finite, a sigma of the stamp's pixels is not positive and
 *    finite (or its float32 square is 0), or A, q or F below leave the range of finite numbers (F: of float32).
 *  3 the flux F: S/N(F) = F sqrt(sum_i P_i^2 / (v_i + F max(P_i, 0))) = d_s2n[s], v_i = sigma_i sigma_i in float32, everything else
 *    float64 (the variance model of bbx_psf_optflux_shift's step 4 for a source on an empty sky).  S/N^2 is convex and increasing
 *    in F: Newton's iteration from F_hi, kept inside [F_lo, F_hi] by bisection, until the step is below 1e-15 F; F_lo = s / sqrt(A),
 *    F_hi = (s^2 q + sqrt(s^4 q^2 + 4 A s^2)) / (2 A), A = sum P_i^2 / v_i, q = max_i max(P_i, 0) / v_i.  F is rounded to float32,
 *    and that float32 is the flux of everything below.
 *  4 frame_i = (float)((double) frame_i + F P_i + [noise] sqrt(F max(P_i, 0)) g_i): float64, one rounding per pixel.  g_i is the
 *    standard normal of (seed, s, i), i = row * S + column of the stamp, stateless:
 *      Philox4x32-10 (Salmon et al. 2011; multipliers 0xD2511F53 on word 0, 0xCD9E8D57 on word 2, key increments 0x9E3779B9,
 *      0xBB67AE85 after every round) on the counter (i, s, 0, 0) with the key (seed & 0xffffffff, seed >> 32) -> words r0..r3;
 *      u1 = (r0 + 0.5) / 2^32, u2 = (r1 + 0.5) / 2^32, g = sqrt(-2 ln u1) cos(2 pi u2), in float64 (r2, r3 are not used).
 *  5 d_flux[s] = F; d_real[s] = the float64 sum of everything step 4 added (before the rounding of the frame), as float32;
 *    d_snr_sky[s] = F sqrt(A) as float32; d_flags[s] u8.
 * The CALLER guarantees that the stamps of two stars do not overlap (Chebyshev distance of their pixels >= S): every frame pixel is
 * then read and written by one thread of one workgroup, which is what makes the in-place add free of races without atomics.
 * Deterministic: no atomics, no state, every sum in a fixed order (bbx_psf_optflux_shift's): same arguments -> same bits.
 * nstar == 0: nothing is launched.  One workgroup of 256 per star, no host wait.                                             */
#define BBX_FAKE_MASKED    1
#define BBX_FAKE_ON_SOURCE 2
#define BBX_FAKE_OFF_FRAME 4
#define BBX_FAKE_NO_PSF    8
#define BBX_FAKE_NO_FLUX   16
int bbx_fake_inject(bbx_ctx *ctx, int ny, int nx, float *d_frame, const float *d_ref, const float *d_sigma,
                    const bbx_spline_image *sigma_mini, const uint8_t *d_mask_new, const uint8_t *d_mask_ref, int S,
                    int nplane, const float *d_cube, const float *d_terms, const int32_t *d_idx, int nstar,
                    const int32_t *d_ys, const int32_t *d_xs, const float *d_off, const float *d_s2n, int clear_half,
                    float clear_nsigma, int noise, uint64_t seed, float *d_flux, float *d_real, float *d_snr_sky,
                    uint8_t *d_flags, void *stream);

/* The stars read back: per star the largest finite value of d_scorr[ny][nx] in the (2 radius + 1)^2 window about (d_ys, d_xs)
 * clipped to the frame, radius <= 4; equal values: the lowest row, then the lowest column.  d_out[nstar][6] float32 = (dy, dx of
 * that pixel relative to the star's, Scorr, Fpsf, Fpsferr there, Fpsf at the star's own pixel -- 0 where that is off the frame).  A
 * window without a finite value: dy = dx = NaN, the four values 0.  One wave per star, nstar == 0: nothing is launched.  */
int bbx_fake_recover(bbx_ctx *ctx, int ny, int nx, const float *d_scorr, const float *d_fpsf, const float *d_fpsferr,
                     int nstar, const int32_t *d_ys, const int32_t *d_xs, int radius, float *d_out, void *stream);

/* ---- astrometric solution from a star catalogue (bbx_wcs.hip).  zogy solves with astrometry.net ([EXT]); only the
 * key names A-* follow the reference, the method and every rule below are THIS PROJECT'S OWN, stated in float64 numpy by
 * tests/astrometry_ref.py, and parity is unpinned.  The solve itself is the chain of bbx_align_* with A = the frame's star list and
 * B = the catalogue on a virtual pixel grid of the frame's shape; these three entries are the sphere.  Everything is float64.
 *
 * Rule 1, standard coordinates about the pointing (ra0, dec0), all angles in degrees at the interface (d2r = pi / 180):
 *   D = sin dec0 sin dec + cos dec0 cos dec cos(ra - ra0), xi = cos dec sin(ra - ra0) / D,
 *   eta = (cos dec0 sin dec - sin dec0 cos dec cos(ra - ra0)) / D, both times 180 / pi.  D <= 0 or a non-finite xi, eta: the row is
 *   not in the field.  Inverse, with xi, eta in radians: den = cos dec0 - eta sin dec0, ra = ra0 + atan2(xi, den) brought into
 *   [0, 360) (a - 360 floor(a / 360); 360 itself: 0), dec = atan2(sin dec0 + eta cos dec0, hypot(xi, den)).
 * Rule 2, the virtual grid: (xi, eta) = CD0 (x - xc, y - yc), xc = (nx - 1) / 2, yc = (ny - 1) / 2, cd[4] = CD0 row-major in
 *   deg / pix (HOST array; the caller forms it: (s / 3600) [[-p cos r, -sin r], [-p sin r, cos r]]).  The kernel inverts it in closed
 *   form: x = xc + (cd[3] xi - cd[1] eta) / det, y = yc + (cd[0] eta - cd[2] xi) / det.
 * Rule 3, list B: a row is eligible when it is in the field, its magnitude is finite, -margin <= x <= nx - 1 + margin and the same
 *   in y, and its flux = (float) 10^(-0.4 ((double) mag - mag_zp)) is positive and finite.  Eligible: integer = floor(v + 0.5), offset
 *   = (float)(v - integer) as (dy, dx), err = flux / 1000 (float32).  Else integers 0, offsets NaN, flux = err = 0: the row neither
 *   votes in bbx_align_vote nor matches in bbx_match_mutual.  d_count[1] = the eligible rows (integer adds).
 * d_sky[n][2] = (ra, dec) float64, d_mag[n] float32.  n == 0: d_count is cleared, nothing is launched.                        */
int bbx_wcs_cat_list(bbx_ctx *ctx, int n, const double *d_sky, const float *d_mag, double ra0, double dec0, int ny, int nx,
                     const double *cd, double margin, double mag_zp, int32_t *d_ys, int32_t *d_xs, float *d_off, float *d_flux,
                     float *d_err, int32_t *d_count, void *stream);

/* Rule 5, pixel to sky: the position (x, y), 0-based, of row i is d_pos[i] = (x, y) float64 where d_pos is given, else
 * d_xs[i] + (double) d_off[i][1], d_ys[i] + (double) d_off[i][0] (d_off NULL: the integers).  (X, Y) = T(x, y) by bbx_align_grid's
 * operations on d_coef[12] (DEVICE, bbx_align_fit's basis with the frame's ny, nx), (xi, eta) = CD0 (X - xc, Y - yc), then the
 * inverse of rule 1 -> d_sky[n][2] = (ra, dec).  A position that is not finite gives NaN.  n == 0: nothing is launched.        */
int bbx_wcs_pix2sky(bbx_ctx *ctx, int n, const double *d_pos, const int32_t *d_ys, const int32_t *d_xs, const float *d_off,
                    const double *d_coef, int ny, int nx, const double *cd, double ra0, double dec0, double *d_sky, void *stream);

/* Rule 6, residuals: over the items i of bbx_align_fit's d_items[n_items][2] with d_kept[i] set and both indices inside their
 * lists: (ra, dec) of A's position by rule 5 against d_cat_sky[ib]: dra = (ra - ra_cat, brought into [-180, 180)) cos dec_cat,
 * ddec = dec - dec_cat, both times 3600.  d_out[8] = {count, mean dra, std dra, mean ddec, std ddec, 0, 0, 0}, std =
 * sqrt(sum (d - mean)^2 / count) (no pair: count 0, NaN).  One workgroup of 256: per thread over the items t, t + 256, ... in that
 * order, the 256 partial sums added in thread order; the means first, then the deviations.  n_items == 0: nothing is launched and
 * d_out is left as it is.                                                                                                    */
int bbx_wcs_pair_stats(bbx_ctx *ctx, int n_items, const int32_t *d_items, const uint8_t *d_kept, int n_a, const int32_t *d_a_ys,
                       const int32_t *d_a_xs, const float *d_a_off, int n_b, const double *d_cat_sky, const double *d_coef, int ny,
                       int nx, const double *cd, double ra0, double dec0, double *d_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BBX_H */
