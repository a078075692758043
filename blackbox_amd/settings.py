"""Reduction parameters for the hot path, under the reference's own names.

Mirror of the rows of ``Settings/set_blackbox.py`` that the per-image reduction
reads (file:line given per entry) plus the ``set_zogy`` values the reference
takes from the (external) ZOGY settings module.  Values that are dictionaries
are keyed by telescope ('ML1', 'BG2', ...) or by telescope family ('BG') and
are resolved with :func:`get_par`, like the reference's ``get_par(par, tel)``.
"""

# ---- reduction switches (set_blackbox.py:36-52) --------------------------------
subtract_mbias = {'ML1': False, 'BG': True}
detect_sats = True
correct_nonlin = False
voscan_poldeg = 3
ncal_max = {'bias': 20, 'dark': 20, 'flat': 15}
# master frames (set_blackbox.py:47, 331): days either side of the evening date searched for
# reduced calibration frames; flats taken in the evening (or just after midnight UT) left out
cal_window = {'bias': 3, 'dark': 3, 'flat': 7}
flat_reject_eve = {'ML': False, 'BG': True}

# ---- LA-Cosmic (set_blackbox.py:211-218) ---------------------------------------
sigclip = {'ML1': 15, 'BG': 20}
sigfrac = 0.01
objlim = 3
niter = 3
sepmed = False

# ---- satellite trails (set_blackbox.py:222-228) --------------------------------
use_asta = False          # ASTA's Keras model cannot be shipped; classical path
sat_bin = 2               # binning of the classical (acstools-like) path, blackbox.py:4163

# ---- CCD (set_blackbox.py:241-337) ----------------------------------------------
gain = {
    'ML1': [2.112, 2.125, 2.130, 2.137, 2.156, 2.158, 2.163, 2.164,
            2.109, 2.124, 2.126, 2.132, 2.136, 2.154, 2.155, 2.157],
    'BG2': [2.694, 2.685, 2.691, 2.661, 2.655, 2.673, 2.695, 2.659,
            2.654, 2.748, 2.712, 2.717, 2.714, 2.702, 2.673, 2.743],
    'BG3': [2.614, 2.609, 2.634, 2.647, 2.600, 2.616, 2.683, 2.649,
            2.680, 2.679, 2.644, 2.604, 2.615, 2.633, 2.615, 2.714],
    'BG4': [2.415, 2.393, 2.365, 2.333, 2.340, 2.320, 2.348, 2.389,
            2.395, 2.403, 2.381, 2.350, 2.362, 2.369, 2.391, 2.430],
}
satlevel = {
    'ML1': [5.89e4, 5.94e4, 5.82e4, 5.59e4, 5.60e4, 5.63e4, 5.60e4, 5.75e4,
            5.88e4, 5.81e4, 5.71e4, 5.65e4, 5.59e4, 5.60e4, 5.59e4, 5.65e4],
    'BG2': [3.84e4, 3.77e4, 3.75e4, 3.79e4, 3.79e4, 3.80e4, 3.75e4, 3.93e4,
            4.50e4, 4.08e4, 4.08e4, 4.09e4, 4.07e4, 3.95e4, 4.15e4, 4.37e4],
    'BG3': [3.96e4, 3.83e4, 3.79e4, 3.77e4, 3.81e4, 3.83e4, 3.74e4, 3.94e4,
            4.00e4, 3.98e4, 4.13e4, 4.29e4, 4.29e4, 4.22e4, 4.13e4, 4.38e4],
    'BG4': [4.11e4, 4.09e4, 4.16e4, 4.29e4, 4.32e4, 4.29e4, 4.23e4, 4.41e4,
            4.66e4, 4.60e4, 4.53e4, 4.67e4, 4.66e4, 4.65e4, 4.64e4, 4.66e4],
}
flat_norm_sec = {'ML1': (slice(6600, 9240), slice(5280, 7920)),
                 'BG2': (slice(500, 2000), slice(1320, 6600)),
                 'BG3': (slice(300, 1200), slice(5280, 10000)),
                 'BG4': (slice(2640, 5280), slice(3960, 7920))}
ny, nx = 2, 8
ysize_chan, xsize_chan = 5280, 1320

# rows of the data section searched for saturated columns by os_corr
# (blackbox.py:6625)
os_ypix_lim = {'BG2': (2640, 5280), 'BG3': (1320, 2640), 'BG4': (1320, 2640)}

# ---- set_zogy values used by the reduction (external module upstream) -----------
mask_value = {'bad': 1, 'cosmic ray': 2, 'saturated': 4,
              'saturated-connected': 8, 'satellite trail': 16, 'edge': 32,
              'crosstalk': 64}
bkg_boxsize = 60
bkg_filtersize = 3
subimage_size = 1320
subimage_border = 40
transient_nsigma = 6

# ---- transient thumbnails (set_blackbox.py:62-66, 90; size_thumbnails: set_zogy, qc.py:484-485) ----
# The reference's default for save_thumbnails_pngs is True; here both switches are off by default so
# that existing product sets do not change.
save_thumbnails = False        # THUMBNAIL_RED/_REF/_D/_SCORR + FLAGS_MASK columns in `_trans.fits`
save_thumbnails_pngs = False   # {NUMBER}_{RED,REF,D,SCORR}.png per transient (blackbox.py:2674-2826)
size_thumbnails = 100          # [pix] side of the square cut-outs
thumbnails_dir = None          # PNGs go to {thumbnails_dir}/{image base name}/; None: `thumbnails/` next to the products
trans_flags_window = 5         # [pix] side of the window around the peak whose mask values make FLAGS_MASK (this project's own)

# ---- transient vetting: the PSF of D fitted to D at every candidate with free position (bbx_zogy_pd_stamps, bbx_trans_psffit,
# DESIGN.md 4j; zogy's E_FLUX_PSF_D / X_PSF_D / Y_PSF_D / CHI2_PSF_D, [EXT]: the rules are this project's own) ----
# Off by default: `_trans.fits` keeps its columns, `_trans_hdr.fits` its keys.
trans_psffit = False           # X_PSF_D Y_PSF_D E_FLUX_PSF_D E_FLUXERR_PSF_D CHI2_PSF_D FLAGS_PSF_D columns, T-PSFD T-FITSZ T-NFIT T-PDFOLD T-CHI2MD keys
trans_fit_size = 11            # [pix] side of the (square, odd) window of the fit, 3 .. PSF stamp side - 10
trans_fit_niter = 8            # linearised steps of the position, always all of them
trans_fit_maxshift = 2.0       # [pix] the position stays within this of the integer peak in either axis
trans_pd_grid = 256            # side of the grid P_D is formed on, >= 4 x the PSF stamp side, even, <= 512
trans_chi2_max = None          # rows without a fit or with CHI2_PSF_D above this are dropped (T-NVET); None: no row is dropped

# ---- transient vetting: an elliptical Gaussian and an elliptical Moffat fitted to D at every candidate (bbx_trans_shapefit, DESIGN.md
# 4k; zogy's X/Y_GAUSS_D FWHM_GAUSS_D ELONG_GAUSS_D CHI2_GAUSS_D and the same of _MOFFAT_D, [EXT]: the rules are this project's own) ----
# Off by default: `_trans.fits` keeps its columns, `_trans_hdr.fits` its keys.  Works with and without trans_psffit.
trans_shapefit = False         # the sixteen catalogs.TRANSSHAPE_COLUMNS, T-SHAPE T-SHPSZ T-MBETA T-NGAUS T-NMOFF T-FWGMD T-ELGMD keys
trans_shape_size = 11          # [pix] side of the (square, odd) window of the two fits, 5 .. 39
trans_shape_niter = 32         # Levenberg-Marquardt iterations, always all of them
trans_shape_maxshift = 2.0     # [pix] the centre stays within this of the integer peak in either axis
trans_moffat_beta = 2.5        # the Moffat's beta, fixed (a free beta does not converge in this many iterations: DESIGN.md 4k)
trans_shape_fwhm_lo = 0.5      # [pix] an axis FWHM below this refuses the step
trans_shape_fwhm_hi = None     # [pix] ... and one above this; None: twice the window's side
trans_fwhm_gauss_min = None    # rows without a Gauss fit or with FWHM_GAUSS_D below this are dropped (T-NVET); None: no bound
trans_fwhm_gauss_max = None    # ... above this
trans_elong_gauss_max = None   # ... or with ELONG_GAUSS_D above this

# ---- flux ratio and dx, dy from matched stars (buildref.py:2782-3014 get_fratio; [EXT] zogy.get_fratio_dxdy) ----
# Off by default: the subtraction then takes the caller's fratio, dx, dy (--fratio --zogy_dx --zogy_dy) as before.
zogy_match = False             # measure fratio, dx, dy per sub-image from the stars matched between new frame and reference
match_dist_pix = 3.5           # [pix] largest distance of a match: dist_max = 2 arcsec (buildref.py:2816) at 0.564 arcsec/px
match_nmin = 15                # fewer pairs than this: no measurement (nmatch_min, buildref.py:2992)
match_snr_min = 20.0           # flux / fluxerr a star needs on both sides to enter the statistics (this project's own)
centroid_radius = 6            # [pix] the windowed centroid reads (2 * radius + 1)^2 pixels around the integer peak
centroid_niter = 8             # iterations of the windowed centroid

# ---- registration of the reference on the new frame from the two star lists (bbx_align.hip; [EXT] SWarp and two
# astrometric solutions in zogy: the method is this project's own) ----
# Off by default: --ref is taken to lie on the new frame's pixel grid (or the caller gives ref_grid), as before.
ref_align = False              # register --ref (any shape) on the new frame from the stars of both; the A-* keys, T-NOFFR
align_poldeg = 1               # degree of the transform's polynomial, 1 or 2
align_max_shift = 256.0        # [pix] largest offset new - ref the vote looks for, in either axis
align_bin = 4.0                # [pix] bin of the vote's histogram of pair differences
align_nbright = 2048           # sources of each list that vote (at most 2048)
align_rounds = 3               # rounds of (reference list through T^-1, match, fit) behind the vote

# ---- astrometric solution from a star catalogue (bbx_wcs.hip + the chain of bbx_align.hip; [EXT] astrometry.net in
# zogy: only the A-* key names follow the reference, blackbox.py:3067-3084, 3144-3145; the method is this project's own) ----
# Off by default: no kernel of bbx_wcs.hip is launched, no WCS or A-* key and no RA / DEC column is added.
astrometry = False             # --ast_cat on the new frame's star list: the TAN[-SIP] WCS and the A-* keys in _red.fits, RA DEC columns
ast_cat = None                 # the catalogue: a FITS binary table with positions in degrees (ICRS) and a magnitude
ast_cat_cols = ('RA', 'DEC', 'MAG')    # its column names
ast_cat_max = 2000000          # more rows than this: an error at load
ast_rot = 0.0                  # [deg] nominal rotation (FITS CROTA2 convention); the scale is pixscale below
ast_parity = 1                 # +1: north up, east left at rotation 0; -1: mirrored
ast_max_shift = 256.0          # [pix] largest pointing error the vote looks for, in either axis (2.4 arcmin at 0.564 arcsec/px)
ast_bin = 4.0                  # [pix] bin of the vote's histogram
ast_poldeg = 2                 # degree of T, 1 (TAN) or 2 (TAN-SIP)
ast_rounds = 3                 # rounds of (catalogue through T^-1, match, fit) behind the vote
ast_dist = None                # [pix] largest distance of a match; None: match_dist_pix
ast_mag_zp = 25.0              # flux of a catalogue row = 10^(-0.4 (mag - ast_mag_zp)): only the brightness ranking rests on it

# ---- source shapes of `_cat.fits` and the frame's seeing statistics (header keys S-NOBJ S-FWHM S-FWSTD S-SEEING S-SEESTD
# S-ELONG S-ELOSTD, blackbox.py:3051-3057; [EXT] SExtractor in zogy: adaptive second moments here) ----
# Off by default: `_cat.fits` keeps its seven columns and the header gets none of the keys.
cat_shapes = False             # FWHM, ELONGATION, A, B, THETA, X2, Y2, XY, FLAGS_MASK columns, sub-pixel X_POS / Y_POS, the S-* keys
shape_snr_min = 20.0           # flux / fluxerr a source needs to enter the frame's statistics (this project's own)
shape_nmin = 15                # fewer unflagged stars than this in the frame: the six statistics are 'None' (this project's own)
pixscale = 0.564               # [arcsec/pix] S-SEEING = S-FWHM x pixscale (finding_chart.py:502)
# the window radius and the number of iterations are the centroid's: centroid_radius, centroid_niter

# ---- catalogue photometry with the PSF placed on the windowed centroid instead of the integer peak (bbx_psf_optflux_shift,
# DESIGN.md 4h; what zogy.get_psfoptflux does, [EXT]) ----
# Off by default: the fluxes keep their bits, `_cat.fits` its columns.
phot_centroid = False          # E_FLUX_OPT / E_FLUXERR_OPT / SNR_OPT with the shifted PSF, masked pixels left out, FLAGS_OPT, sub-pixel X_POS / Y_POS, PHOT-CEN

# ---- aperture photometry of `_cat.fits` with a local sky annulus (bbx_aper_phot; the E_FLUX_APER_R<r>xFWHM columns of
# qc.py:489-502 with set_zogy.apphot_radii; [EXT] zogy.get_apflux / SExtractor: the rules of include/bbx.h here, this project's own) ----
# Off by default: `_cat.fits` keeps its columns and the header gets none of the AP-* keys.
cat_apphot = False             # E_FLUX_APER_R*xFWHM, E_FLUXERR_APER_R*xFWHM, BKG_APER, BKGSTD_APER, NSKY_APER, FWHM_APER, FLAGS_APER; the AP-* keys
apphot_radii = (0.66, 1.5, 5.0)    # [FWHM] aperture radii (set_zogy.apphot_radii), at most 8
apphot_sky_inout = (5.0, 7.0)  # [FWHM] inner and outer radius of the sky annulus
apphot_local_sky = True        # subtract the annulus' clipped median from the aperture fluxes
apphot_sky_nmin = 20           # fewer annulus pixels than this after clipping: no local sky (FLAGS_APER 8), nothing subtracted

# ---- limiting-flux image of the reduced frame (`_red_limmag.fits`, set_blackbox.py:157-159; LIMEFLUX, LIMFNU, LIMMAG:
# blackbox.py:3151-3153; bbx_limflux_image; [EXT] zogy.get_psfoptflux(get_limflux_array=True): the rules of
# include/bbx.h here, this project's own) ----
# Off by default: no kernel of bbx_limflux.hip is launched, no LIM* key is added, no file is written.
limmag = False                 # _red_limmag.fits; LIMMAG-P LIMNSIG LIMEFLUX LIMMAG LIMFNU LIMPFRAC LIMWIN LIMNPIX
limmag_nsigma = 5.0            # [sigma] significance of the limit (finding_chart.py:232)
limmag_psf_frac = 1e-4         # share of sum PSF^2 the window may leave out (0: the whole stamp)

# ---- fake stars: injection at a set S/N into the background-subtracted new frame, recovery from Scorr / Fpsf and the candidate
# list (T-NFAKE, T-FAKESN: blackbox.py:3192-3193; bbx_fake_inject, bbx_fake_recover; [EXT] zogy's fake stars: the
# rules of include/bbx.h here, this project's own) ----
# Off by default: no kernel of bbx_fake.hip is launched, no T-FK* key or FAKE_STAR column is added, no file is written.
nfakestars = 0                 # stars per sub-image; _trans_fakestars.fits, FAKE_STAR in _trans.fits, T-NFAKE T-FAKESN T-FK*
fakestar_s2n = 10.0            # asked S/N, source noise included: one number or up to 8, taken in turn
fakestar_seed = 0              # of the positions and of the source noise
fakestar_noise = True          # add the stars' own Poisson noise (a normal deviate of variance F P per pixel)
fakestar_radius = 2            # [pix] recovery window about the injected pixel (<= 4)
fake_clear_half = 3            # [pix] half side of the window that must be free of mask bits and sources
fake_clear_nsigma = 5.0        # [sigma] |new| or |ref| above this in that window: the star is not planted (FLAGS_IN 2)

# ---- PSF model from the frame's own stars (`_psf.fits`, header keys PSF-*: blackbox.py:3085-3110, set_qc.py:293-296;
# [EXT] PSFEx in zogy: the rules of include/bbx.h here; this project's own unless a PSFEx parameter is named) ----
# Off by default: a frame without --psf_new is processed without a PSF as before.
psf_build = False              # build the model where no PSF file is given (zogy.build_psf)
psf_size = 49                  # [pix] side of the (square, odd) vignettes and of the model, at most 49
psf_poldeg = 2                 # degree of the polynomial in the frame position (zogy's psf_poldeg, [EXT])
psf_seed_fwhm = 4.0            # [pix] FWHM of the window the centroids and adaptive moments start from
psf_snr_min = 20.0             # peak / S-BKGSTD a PSF star needs (PSFEx SAMPLE_MINSN)
psf_fwhm_tol = 0.2             # |FWHM / median - 1| a PSF star may have (PSFEx SAMPLE_VARIABILITY)
psf_elong_max = 1.3            # largest ELONGATION of a PSF star
psf_iso_frac = 0.05            # a neighbour inside the vignette with a peak above this fraction of the star's excludes it
psf_stars_nmax = 2048          # at most this many stars enter the fit (every s-th in list order above it)
psf_nstars_min = 15            # fewer stars than this in the final fit: no model (PSF-P False)
psf_accuracy = 0.01            # relative error of the model added to the pixel variances (PSFEx PSF_ACCURACY)
psf_chi2_clip = 3.0            # stars with a chi^2 above this many times the median leave the fit
psf_nclip = 2                  # rounds of that

# ---- object mask and a second, object-free background pass (`_objmask.fits`, set_blackbox.py:157; SURVEY 3.5: run_sextractor
# (2 passes, object mask) -> get_back; [EXT] SExtractor in zogy: the rules of DESIGN.md 4i here, this project's own) ----
# Off by default: the background mesh is measured once, with sigma clipping alone, as before.
objmask = False                # detect on the first pass's frame, mask the objects, measure the mesh again; OBJM-* S-BKG1 S-BKGSD1
objmask_nsigma = 1.5           # a pixel is listed at this many of its box's sigma (SExtractor DETECT_THRESH)
objmask_minarea = 5            # [pix] components with fewer listed pixels are dropped (DETECT_MINAREA)
objmask_grow = 3               # [pix] radius of the disk every pixel of a kept component masks (0 ... 8)
objmask_filter = True          # detection on the 3x3 pyramid-smoothed frame (SExtractor's default.conv)
objmask_max_frac = 0.5         # a mask that covers more of the frame than this is not used: the frame keeps its first pass

# calibration files of a reduction (explicit paths; the date-based master selection
# of master_prep, blackbox.py:4625-4905, is blackbox_amd.masters, run by --master_date)
bad_pixel_mask = None      # path containing 'bpm' -> 'bpm_{filt}' (blackbox.py:4386)
crosstalk_file = None
master_flat = None
master_bias = None


def get_par(par, tel):
    """value of [par] for telescope [tel]: exact key, then the alphabetic
    prefix ('BG2' -> 'BG'), else the parameter itself (zogy.get_par)."""
    if isinstance(par, dict):
        if tel in par:
            return par[tel]
        base = ''.join(c for c in str(tel) if c.isalpha())
        if base in par:
            return par[base]
    return par
