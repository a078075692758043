"""Numerical core of zogy.optimal_subtraction on the GPU: background mesh, sub-image ZOGY
(rocFFT), PSF photometry.  Call sites in the reference: blackbox.py:2350-2354 / 2460-2465;
helper signatures seen in buildref.py:2398-2405, 2480-2495, 3357-3366.

[EXT] zogy itself is not part of /root/reference: the conventions are those of
oracle/zogy_core.py (parity unpinned).  Astrometry, PSFEx,
SExtractor and the real-bogus CNN stay out of scope: PSF images and a WCS-aligned
reference frame are inputs.
"""
import ctypes as C                                    # noqa: F401  (zogy.C)
import inspect
import logging
import os

import numpy as np
import torch
from scipy import ndimage                             # noqa: F401  (zogy.ndimage)

from . import settings
from ._lib import lib, check, fetch, push, ptr as _p, BBXError as _lib_BBXError, Readback, SplineImage as _SplineImage         # noqa: F401
from ._lib import BBX_OPT_ZOGY_KSMALL_OFF          # noqa: F401  (k_n, k_r through the full grid: tests and timings compare the paths)
from .catalogs import format_cat, transient_table         # noqa: F401  (zogy.format_cat)
# The stages, one module each, in import order: a module imports only from those above it.  This module is the facade:
# callers and tests reach every stage function as zogy.<name>, and _optimal_subtraction's own stages, which live below it in
# this file, find them in this module's globals at call time (a test that counts calls assigns zogy.<name>).  The lists are
# the index of the package.
from .zoom import (NPAD, SPLINE_POLE, MiniImage, _axis_map, _bspline_weights, _device_taps, _tap_tables,         # noqa: F401
                   device_zoom_coefficients, mini2back, remap_mini, zoom_coefficients, zoom_plan)
from .background import (_objmask_counts, _objmask_stage, frame_clipped_stats, frame_clipped_stats_enqueue, get_back,         # noqa: F401
                         object_mask, object_mask_enqueue, variance)
from .peaks import find_peaks_arrays, find_peaks_collect, find_peaks_enqueue, find_transients, win_centroid, window_sigma         # noqa: F401
from .shapes import (SHAPE_COLS, SHAPE_STAT_COLS, _SC, _SHAPE_HDR, empty_shape_table, shape_columns, shape_header,         # noqa: F401
                     shape_stats, src_shapes)
from .psfphot import (PHOT_MASKED, PHOT_NO_CENTROID, PHOT_NO_SUM, _source_sigma, embed_psfs, psf_model_stamps, psf_optflux,         # noqa: F401
                      psf_optflux_centroid, psf_poly_terms, resample_psf_basis, source_psfs, subimage_psfs, tile_index)
from .transients import (PD_FOLD_WARN, SHAPE_GAUSS, SHAPE_MOFFAT, SHAPE_OUT, TRANS_AT_BOUND, TRANS_MASKED, TRANS_NO_FIT,         # noqa: F401
                         TRANS_NOT_CONVERGED, TRANS_SHAPE_REFUSED, pd_stamps, shape_start_fwhm, thumbnail_stamps, trans_fit_header,
                         trans_psffit, trans_shape_header, trans_shapefit, vet_transients)
from .subtract import (RefPsf, RefRows, StreamGate, _NoGate, cut_subimages, frame_path_supported, mini_path_supported,         # noqa: F401
                       run_zogy, run_zogy_frame, stitch_subimages, zogy_frame_outputs)
from .starmatch import (MATCH_COLS, _MATCH_HDR, _MC, RefCatalog, empty_match_table, match_enqueue, match_mutual,         # noqa: F401
                        match_scalars, match_stats)
from .psfbuild import (BBX_ERR_NOTCONV, PSF_REASONS, _PSF_HDR, build_psf, psf_chi2, psf_chi2_median, psf_fit, psf_header,         # noqa: F401
                       psf_ncoef, psf_select, psf_stamps)
from .aperphot import (APER_FEW_SKY, APER_MASKED, APER_NO_CENTROID, APER_OFF_FRAME, APER_SKY_CUT, APER_TOO_BIG, _radii as _aper_radii,         # noqa: F401
                       aper_column_names, aper_columns, aper_fwhm, aper_header, aper_phot)
from .limflux import check_parameters as _limflux_parameters, limflux_header, limflux_image, limit_magnitudes         # noqa: F401
from .align import (ALIGN_CLIP, ALIGN_DET, ALIGN_FAR, ALIGN_FEW_PAIRS, ALIGN_NMIN, ALIGN_NOT_PD, ALIGN_PAIR_CAP,         # noqa: F401
                    ALIGN_VOTE_FAILED, RefStars, _expect_list, align_apply, align_fit, align_grid, align_grid_host, align_grid_shape,
                    align_header, align_reference, align_sort, align_vote, remap_mask)
from . import astrometry as _ast                                     # (_optimal_subtraction's switch bears the module's name)
from . import transients as _tr                                      # (the candidate table's host functions: _transient_rows)
from .astrometry import AstCatalog, ast_header, frame_pointing, wcs_header, wcs_pix2sky         # noqa: F401
from .fakestars import (FAKE_COLS, FAKE_MASKED, FAKE_NO_FLUX, FAKE_NO_PSF, FAKE_OFF_FRAME, FAKE_ON_SOURCE, FOUND_KEPT, FOUND_PEAK,         # noqa: F401
                        FOUND_ROW, check_apart, fake_header, fake_inject, fake_launch, fake_layout, fake_match, fake_prepare, fake_recover,
                        fake_s2n_list, fake_table)

BBX_ERR_OVERFLOW, BBX_ERR_PSFWIN = -4, -6          # include/bbx.h
BBX_OPT_ZOGY_KWIN_OFF = 4
_trans_psffit = trans_psffit                                         # (_optimal_subtraction's switch bears the name)
_trans_shapefit = trans_shapefit                                     # (_optimal_subtraction's switch bears the name)
_aper_phot = aper_phot                                               # (_optimal_subtraction's switch bears the name)
_limflux_image = limflux_image                                       # (the stage calls it by this name)
_fake_launch, _fake_recover = fake_launch, fake_recover              # (the stage calls them by these names)


def optimal_subtraction(ctx, *args, **kw):
    try:
        return _optimal_subtraction(ctx, *args, **kw)
    finally:
        # the candidate-list handoffs (zoom -> catalogue search, final ZOGY kernel -> transient search) are keyed on the
        # frames' addresses inside the context: whatever way this call ends, none of that may outlive it (the caching
        # allocator hands the same address to the next frame)
        lib.bbx_zoom_candidates(ctx.h, None, 0.0)
        lib.bbx_zogy_candidates(ctx.h, 0.0)


def _optimal_subtraction(ctx, new, ref, new_mask, ref_mask, psf_new, psf_ref, fratio=1.0, dx=0.0, dy=0.0,
                         subimage_size=None, subimage_border=None, bkg_boxsize=None, nsigma=None,
                         ref_is_bkgsub=False, ref_bkg_std_mini=None, ref_grid=None, ref_grid_step=32,
                         cat_extract=False, cat_nsigma=5.0, trans_extract=True, frame_stats=True, max_sources=200000,
                         zogy_gate=None, ref_bkg_std=None, sigma_frames=False, thumbnails=False, thumbnail_size=None,
                         thumbnail_pngs=False, ref_rows=None, ref_psf=None, match=False, ref_catalog=None, match_dist=None, match_nmin=None,
                         match_snr_min=None, shapes=False, shape_snr_min=None, psf_build=False, psf_size=None, psf_poldeg=None,
                         phot_centroid=False, objmask=False, objmask_nsigma=None, objmask_minarea=None, objmask_grow=None,
                         objmask_max_frac=None, trans_psffit=False, trans_fit_size=None, trans_chi2_max=None,
                         trans_shapefit=False, trans_shape_size=None, trans_fwhm_gauss_min=None, trans_fwhm_gauss_max=None,
                         trans_elong_gauss_max=None, ref_align=False, align_poldeg=None, align_max_shift=None, align_bin=None,
                         align_nbright=None, align_rounds=None, ref_stars=None, aper_phot=False, apphot_radii=None, apphot_sky_inout=None,
                         apphot_local_sky=None, limmag=False, limmag_nsigma=None, limmag_psf_frac=None, fake_stars=0, fake_s2n=None,
                         fake_seed=None, fake_noise=None, fake_radius=None, fake_clear_nsigma=None, astrometry=False, ast_catalog=None,
                         ast_pointing=None, ast_poldeg=None, ast_max_shift=None, ast_bin=None, ast_rounds=None, ast_dist=None, ast_rot=None,
                         ast_parity=None, ast_pixscale=None, ast_mag_zp=None):
    """The numerical core of zogy.optimal_subtraction(new_fits, ref_fits, ...) (call sites
    blackbox.py:2350-2354 new-only, 2460-2465 new + ref) on device tensors: background mesh +
    subtraction, variance images, [remapping of the reference to the new frame's grid],
    sub-image ZOGY, stitching, transient candidates with PSF fluxes, [full-source catalogue by
    PSF-weighted optimal photometry].
      new, new_mask : reduced frame (float32, e-) and its mask
      fratio, dx, dy: flux ratio new / ref and the astrometric scatter, one number or one per sub-image
      ref, ref_mask : reference frame or None (new-only mode, trans_extract False or no ref:
                      the 2350-2354 branch): then only the background products and the catalogue
      ref_is_bkgsub : the reference is a background-subtracted co-add (buildref product);
                      ref_bkg_std_mini: its `_bkg_std_mini` image (else measured here);
                      ref_bkg_std: what an earlier call made from it (res['bkg_std_ref']: a MiniImage, or the
                      full-frame sigma image), when the caller keeps it for many frames of the same field
      ref_rows      : a RefRows made of the reference and of ref_bkg_std by the caller that keeps both for many frames: the
                      subtraction skips the reference's row transforms (used only where it was made of this call's very
                      reference, sigma map and geometry; same result bit for bit)
      ref_psf       : a RefPsf made of this call's very psf_ref object by the caller that keeps it for many frames: its stamp
                      tensor serves as the reference's PSFs and, where ref_rows is used, the subtraction skips the
                      reference PSF's transforms (same result bit for bit)
      sigma_frames  : True: the two sigma images are made as full frames (rounds 1-4; bbx_zogy_frame) instead of
                      being read off their mini images inside the kernels (bbx_zogy_frame_mini)
      ref_grid      : projection lattice (coadd.projection_grid) when the reference lives on
                      another pixel grid: it is remapped with the LANCZOS3 kernel (zogy runs SWarp)
      psf_new/ref   : PSF stamps [nsub, S, S] / [S, S] (unit sum) or a PSFEx model dict
                      (subimage_psfs) -- running PSFEx itself is out of scope
      thumbnails    : True: res['thumbnails'], device float32 [n, 4, S, S]: the cut-outs RED / REF / D / SCORR of every
                      transient candidate (qc.py:480-485), S = thumbnail_size (settings.size_thumbnails)
      thumbnail_pngs: True: res['thumbnail_png8'], device uint8 [n, 4, S, S]: their display planes (blackbox.py:2786-2826)
                      either switch adds 'flags' (FLAGS_MASK: the masks under the peak) to each transient; both off: no
                      kernel of bbx_thumb.hip is launched and the result has none of these keys
      match         : True (with a reference and both PSFs): fratio, dx, dy of every sub-image are measured from the stars matched
                      between the new frame and the reference (bbx_win_centroid, bbx_match_mutual, bbx_match_stats; match_scalars)
                      and go into the subtraction in place of the caller's, which stay the fallback where the frame has fewer
                      than match_nmin pairs; res['match'] = dict(success, n_new, n_ref, n_pairs, table, fratio_sub, dx_sub,
                      dy_sub), res['ref_catalog'], and header_trans gets Z-DXSTD, Z-DYSTD, Z-FNRSTD, Z-FNRERR.  False: no kernel
                      of bbx_match.hip is launched, no such keys.  match_dist [pix], match_nmin, match_snr_min: settings
      shapes        : True (with cat_extract and psf_new): every catalogue source gets its adaptive second moments (bbx_src_shapes,
                      started at the windowed centroids, which the star match shares when it is on too) and the frame its
                      clipped FWHM / elongation statistics (bbx_shape_stats), both riding the photometry's copy back:
                      res['catalog'] gains FWHM, ELONGATION, A, B, THETA, X2, Y2, XY, FLAGS_MASK and sub-pixel X_POS / Y_POS,
                      res['shapes'] = dict(table, n_good), header_new gets S-NOBJ, S-FWHM, S-FWSTD, S-SEEING, S-SEESTD,
                      S-ELONG, S-ELOSTD (shape_header).  False: no kernel of bbx_shapes.hip is launched, no such keys or columns.
                      shape_snr_min: settings
      psf_build     : True with psf_new None: the new frame's PSF model is built from its own stars (build_psf) between the
                      catalogue's peak search and the photometry and used as psf_new from there on (catalogue, shapes, star
                      match, sub-image PSFs, subtraction); res['psf'] = dict(model, header, stars), header_new gets PSF-P,
                      PSF-NOBJ, PSF-CHI2, PSF-FWHM, PSF-SEE, PSF-SIZE, PSF-CFGS, PSF-SAMP, PSF-PLDG, PSF-FIX.  A build that fails
                      (PSF-P False): the frame goes on as one without a PSF (background products only).  With psf_new given, or
                      False: no kernel of bbx_psfbuild.hip is launched, no such keys.  psf_size, psf_poldeg: settings
      phot_centroid : True: the catalogue photometry (cat_extract, and the star match's two lists) places every source's PSF on
                      its windowed centroid instead of its integer peak (bbx_psf_optflux_shift in place of source_psfs +
                      psf_optflux; the centroids are taken first and shared with shapes and match) and leaves the masked pixels
                      of new_mask out of the sums: res['catalog'] gains FLAGS_OPT (PHOT_NO_CENTROID | PHOT_MASKED | PHOT_NO_SUM)
                      and sub-pixel X_POS / Y_POS (peak + 1 + offset; the integer peak where there is no centroid), header_new
                      gets PHOT-CEN.  False: no kernel of bbx_psfphot.hip is launched, no such key or column
      objmask       : True: the new frame's background mesh is measured twice: the first pass's background-subtracted frame
                      gives the object mask (object_mask; objmask_nsigma, objmask_minarea, objmask_grow: settings), the second pass
                      leaves the masked pixels out, and everything from there on (S-BKG, S-BKGSTD, the sigma image, the catalogue,
                      the PSF build, the match, the subtraction) rests on the second pass.  res['objmask'] (device uint8),
                      res['bkg_mini_pass1'], res['bkg_std_mini_pass1']; header_new gets OBJM-P, OBJM-THR, OBJM-MIN, OBJM-GRW,
                      OBJM-NPX, OBJM-NOB, OBJM-FRC, S-BKG1, S-BKGSD1.  One more host wait.  A pixel list that overflows, an
                      exception in the stage or a mask over more than objmask_max_frac (settings) of the frame: the frame goes
                      on with its first pass, OBJM-P False, no res['objmask'].  False: no kernel of bbx_objmask.hip is
                      launched, no such keys
      ref_catalog   : a RefCatalog made of the reference and of ref_bkg_std by the caller that keeps both for many frames (used
                      only where it was made of this call's very reference, sigma map and geometry; same result bit for bit)
      trans_psffit  : True (with candidates and PSF stamps of one side): the PSF of D of every sub-image (pd_stamps) is fitted to D at
                      every candidate with free position (bbx_trans_psffit; trans_fit_size: settings), queued behind the peak
                      search with the Fpsf gather and read in the same copy back: every transient gains x_psf_d, y_psf_d (0-based,
                      peak + offset), flux_psf_d, fluxerr_psf_d, chi2_psf_d, flags_psf_d; header_trans gets T-PSFD, T-FITSZ, T-NFIT,
                      T-PDFOLD, T-CHI2MD (trans_fit_header).  trans_chi2_max: rows without a fit or with a chi2 above it are
                      dropped, with their thumbnails; T-NVET = the rows kept, T-NTRANS stays.  An exception in the stage:
                      today's table, T-PSFD False.  False: no kernel of bbx_transfit.hip is launched, no such keys
      trans_shapefit: True (same conditions, with or without trans_psffit): an elliptical Gaussian and an elliptical Moffat are fitted
                      to D at every candidate (bbx_trans_shapefit; trans_shape_size: settings), queued behind the fit of P_D or
                      the peak search and read in the same copy back: every transient gains x_, xerr_, y_, yerr_, fwhm_, elong_,
                      chi2_, flags_gauss_d and the same eight of _moffat_d; header_trans gets T-SHAPE, T-SHPSZ, T-MBETA, T-NGAUS,
                      T-NMOFF, T-FWGMD, T-ELGMD (trans_shape_header).  trans_fwhm_gauss_min / _max, trans_elong_gauss_max: rows
                      without a Gauss fit or outside a bound are dropped, with their thumbnails (T-NVET).  An exception in the
                      stage: today's table, T-SHAPE False.  False: bbx_trans_shapefit is not launched, no such keys
      ref_align     : True (with a reference of any shape and both PSFs; a caller's ref_grid with it is a ValueError): the reference
                      is registered on the new frame from the stars of both (align_reference): the new frame's
                      photometry and centroids first, then the reference's list on its own grid (RefStars: ref_stars where the
                      caller keeps one of this very reference, else made here and returned as res['ref_stars']), the transform, its
                      lattice -- which takes the place of ref_grid -- and the reference's mask on the new frame's grid, which
                      takes the place of ref_mask (res['ref_mask_remapped']).  One more host wait.  Transient candidates whose peak
                      has no reference under it (the mask's edge bit) are dropped with their thumbnails: T-NOFFR; T-NTRANS stays.
                      res['align'] = align_reference's dict; header_trans gets A-P, A-PLDG, A-NVOTE, A-NRUN, A-NFAR, A-NPAIR, A-RMSX,
                      A-RMSY, A-DX, A-DY, A-ROT, A-SCALE, A-FLAGS, A-NEDGE.  A registration that fails (flag word not 0, or an exception
                      in the stage): the frame goes on as one without a reference, A-P False -- it is never subtracted unregistered.
                      align_poldeg, align_max_shift, align_bin, align_nbright, align_rounds: settings.  False: no kernel of
                      bbx_align.hip is launched, no such keys
      aper_phot     : True (with cat_extract and psf_new): every catalogue source gets its aperture fluxes and errors in circles of
                      apphot_radii x FWHM with the exact circle-pixel overlap as weight, its local sky from the annulus
                      apphot_sky_inout x FWHM (subtracted unless apphot_local_sky is False) and a flag byte (bbx_aper_phot, DESIGN.md
                      4m), about the windowed centroids that phot_centroid, shapes or the registration made, else taken here; queued
                      behind the photometry and read in the same copy back, with the frame's FWHM (aper_fwhm: one number per
                      frame): res['catalog'] gains E_FLUX_APER_R<r>xFWHM, E_FLUXERR_APER_R<r>xFWHM per radius, BKG_APER, BKGSTD_APER,
                      NSKY_APER, FWHM_APER, FLAGS_APER (APER_NO_CENTROID | APER_MASKED | APER_OFF_FRAME | APER_FEW_SKY | APER_SKY_CUT |
                      APER_TOO_BIG), res['aper'] = dict(fwhm, radii, n_good), header_new gets AP-P, AP-FWHM, AP-NAPER, AP-R1..n,
                      AP-SKYIN, AP-SKYOU, AP-LSKY, AP-NSTAR, AP-OPT1..n (aper_header).  An exception in the stage: today's catalogue,
                      AP-P False.  False: no kernel of bbx_aper.hip is launched, no such keys or columns.  apphot_radii,
                      apphot_sky_inout, apphot_local_sky: settings
      limmag        : True (with psf_new, or a model that psf_build made): the limiting flux of the frame at every pixel, limmag_nsigma x
                      the error of the PSF-weighted optimal flux of a faint source centred there on sky noise alone (bbx_limflux_image,
                      DESIGN.md 4n), from the second-pass sigma map, new_mask and the tiles' PSF stamps over the window that holds
                      1 - limmag_psf_frac of sum PSF^2; queued behind the catalogue photometry, its clipped frame statistic (3 sigma,
                      5 rounds, zeros skipped) and the tiles' windows ride the same copy back: res['limflux'] = the device image,
                      res['limflux_info'] = dict(stat, win, nsigma, frac), header_new gets LIMMAG-P, LIMNSIG, LIMEFLUX, LIMMAG,
                      LIMFNU, LIMPFRAC, LIMWIN, LIMNPIX (limflux_header; exposure time and zeropoint are the caller's: LIMEFLUX, LIMMAG
                      and LIMFNU are 'None' here).  Without a PSF, or on an exception in the stage: the frame goes on, LIMMAG-P
                      False, the other keys 'None', no res['limflux'].  False: no kernel of bbx_limflux.hip is launched, no such keys.
                      A limmag_nsigma that is not positive or a limmag_psf_frac outside [0, 1): ValueError before anything is queued
      fake_stars    : N > 0 (with a reference and PSF stamps of the new frame): N stars per sub-image of the S/N values fake_s2n (taken
                      in turn) are added to the background-subtracted new frame IN PLACE (fake_layout, bbx_fake_inject)
                      behind the catalogue, the PSF build, the star match and the registration -- none of which sees a fake star --
                      and immediately before the frame is cut into sub-images; they ride the one subtraction and are read back from
                      Scorr / Fpsf / Fpsferr (bbx_fake_recover, within fake_radius pixels) in the copy back that follows it.  After
                      the call res['data_bkgsub'], D, Scorr, Fpsf, Fpsferr and the thumbnails CARRY THE STARS, by design, as in zogy;
                      `new` is untouched.  res['fakestars'] = dict(table (FAKE_COLS), layout); every row of res['transients'] gains
                      fake_star (the 1-based star, 0: a real candidate; the rows stay, T-NTRANS counts them); header_trans gets T-FKP,
                      T-NFAKE, T-FAKESN, T-FKNASK, T-FKNREJ, T-FKSEED, T-FKNOIS, T-FKRAD, T-NFKTR, per asked S/N T-FKSNk T-FKNk T-FKEFk
                      T-FKVTk, and T-FKFRAT T-FKFSTD T-FKPULL T-FKSCRT (fake_header).  An exception before the kernel is queued
                      (a layout that does not fit the sub-image, ...): the frame goes on untouched, T-FKP False, T-NFAKE 0.  0: no
                      kernel of bbx_fake.hip is launched, no such keys.  fake_s2n, fake_seed, fake_noise, fake_radius,
                      fake_clear_nsigma: settings
      astrometry    : True (with ast_catalog, an astrometry.AstCatalog kept by the caller for the run, and a PSF of the new frame; no
                      reference is needed): the frame is solved against the catalogue (astrometry.solve_enqueue): the
                      list the registration takes (windowed centroids + PSF fluxes of the catalogue's peaks) against the catalogue
                      on a virtual grid about ast_pointing = (RA, DEC) in degrees -- a PER-FRAME argument: the caller reads it off
                      the frame's header (astrometry.frame_pointing) -- through the registration's own chain (align_chain), queued
                      behind the photometry; its six small tensors and the RA / DEC of the catalogue's rows (bbx_wcs_pix2sky at the
                      very positions X_POS / Y_POS state) ride the photometry's copy back, the RA / DEC of the transient rows the
                      transients': NO host wait is added.  res['astrometry'] = astrometry.solve_finish's dict; header_new gets the
                      TAN[-SIP] WCS (CTYPE CRVAL CRPIX CD [A_ B_ terms] RADESYS), A-P A-PSCALE A-PSCALX A-PSCALY A-ROT A-ROTX A-ROTY
                      A-CAT-F A-NAST A-TNAST A-DRA A-DRASTD A-DDEC A-DDESTD RA-CNTR DEC-CNTR A-PLDG A-NVOTE A-MSHFT A-FLAGS;
                      res['catalog'] gains RA, DEC (float64), every transient ra_peak, dec_peak and, with trans_psffit, ra_psf_d,
                      dec_psf_d.  A solve that fails (the chain's flag word, a coefficient that is not finite, no pointing, no PSF,
                      an exception in the stage): A-P False, 'None' for the other keys, no WCS key and no column; the frame goes on
                      exactly as without the switch.  ast_poldeg, ast_max_shift, ast_bin, ast_rounds, ast_dist, ast_rot, ast_parity,
                      ast_pixscale (pixscale), ast_mag_zp: settings.  False: no kernel of bbx_wcs.hip is launched, no such keys or
                      columns
    -> dict(D, Scorr, Fpsf, Fpsferr, bkg_mini_new, bkg_std_mini_new, ..., transients, catalog,
            header (= header_new additions), header_trans)"""
    c = _setup(dict(locals()))                                       # (the arguments, by name)
    _new_frame_background(c)
    _catalogue(c)
    res = c.res
    if not c.have_ref:
        c.hdr['Z-P'] = (False, 'successfully processed by ZOGY?')
        res['header'], res['header_new'], res['header_trans'], res['transients'] = _HeaderView(c.hdr, c.hdr_t), c.hdr, c.hdr_t, []
        return res
    if c.ref_side is None:
        # the reference frame on the new frame's grid, where neither the star match nor the registration asked for it before
        c.ref_side = _prepare_reference(c)
    fk = _fake_stars(c)
    scal, ms, frame_args = _subtract(c)
    tys, txs, tsc, ntrans = _transient_search(c, frame_args)
    got = _transient_readback(c, scal, fk, tys, txs)
    _transient_rows(c, got, fk, tys, txs, tsc)
    _closing_headers(c, scal, ms, got.get('stats'), ntrans)
    return res


class _Call:
    """The state of one _optimal_subtraction call, which its stage functions share: an attribute bag (a misspelt name raises)"""
    __slots__ = tuple(inspect.signature(_optimal_subtraction).parameters) + (
        # the arguments under their own names (psf_new, ref_grid and phot_centroid are rebound on the way), and their geometry
        'ny', 'nx', 'size', 'border', 'box', 'L', 'nsy', 'nsx', 'nsub', 'bs',
        # settings with their defaults filled in
        'lim_nsigma', 'lim_frac', 'nsig', 'fit_size', 'shape_size',
        # the switches: what the call was asked for and is able to do; a stage that fails clears those that rested on it
        'have_ref', 'have_psf', 'build_here', 'do_match', 'do_shapes', 'do_aper', 'do_align', 'do_lim', 'do_ast', 'want_phot', 'want_cat',
        'use_mini',
        # what one stage makes and a later one reads or replaces
        'mini_std', 'd_sstd', 'work', 'sdn', 'bstd', 'sub_pn', 'sub_pr', 'peaks_off', 'ref_grid_host', 'ref_mask_remapped', 'ref_side', 'own', 'scal_n',
        'mtab', 'ast_pending', 'ast_sol',
        # the result and the two headers
        'res', 'hdr', 'hdr_t')


def _setup(args):
    """the call's state from _optimal_subtraction's arguments (by name), with the refusals that come before anything is queued"""
    c = _Call()
    for k, v in args.items():
        setattr(c, k, v)
    c.size = c.subimage_size or settings.subimage_size
    c.border = settings.subimage_border if c.subimage_border is None else c.subimage_border
    c.box = c.bkg_boxsize or settings.bkg_boxsize
    c.ny, c.nx = c.new.shape
    c.L = c.size + 2 * c.border
    c.res, c.hdr, c.hdr_t = {}, {}, {}
    c.nsy, c.nsx = c.ny // c.size, c.nx // c.size
    c.nsub = c.nsy * c.nsx
    c.bs = c.size // c.box if c.size % c.box == 0 else None
    c.have_ref = c.ref is not None and c.trans_extract
    c.build_here = bool(c.psf_build) and c.psf_new is None         # the PSF of the new frame is made behind the catalogue's peak search
    c.have_psf = c.psf_new is not None or c.build_here
    c.do_match = bool(c.match) and c.have_ref and c.have_psf and c.psf_ref is not None
    c.do_shapes = bool(c.shapes) and bool(c.cat_extract) and c.have_psf
    c.phot_centroid = bool(c.phot_centroid)
    c.do_aper = bool(c.aper_phot) and bool(c.cat_extract) and c.have_psf
    c.do_align = bool(c.ref_align) and c.have_ref
    c.do_lim = bool(c.limmag)
    c.do_ast = bool(c.astrometry)
    c.want_phot = c.cat_extract or c.do_match or c.do_align or c.do_ast
    c.want_cat = (c.want_phot or (c.build_here and c.have_ref)) and c.have_psf
    c.nsig = settings.transient_nsigma if c.nsigma is None else c.nsigma
    c.fit_size = int(settings.trans_fit_size if c.trans_fit_size is None else c.trans_fit_size)
    c.shape_size = int(settings.trans_shape_size if c.trans_shape_size is None else c.trans_shape_size)
    c.d_sstd = c.peaks_off = c.ref_side = c.scal_n = c.mtab = c.ast_pending = c.ast_sol = c.sub_pr = None
    c.own = []
    if c.do_lim:
        c.lim_nsigma, c.lim_frac = _limflux_parameters(c.limmag_nsigma, c.limmag_psf_frac)
    if c.do_align and c.ref_grid is not None:
        raise ValueError('ref_align=True makes the lattice itself: a ref_grid beside it is refused')
    c.ref_mask_remapped = c.ref_grid_host = None                    # set by a registration that succeeded
    return c


def _new_frame_background(c):
    """the new frame: mesh, [object mask and second pass], subtraction, sigma image, the mini images on the host, the BKG keys"""
    ctx, new, new_mask, box, res, hdr = c.ctx, c.new, c.new_mask, c.box, c.res, c.hdr
    ny, nx = c.ny, c.nx
    mini, mini_std = get_back(ctx, new, new_mask, bkg_boxsize=box)
    work = torch.empty_like(new)
    second_pass = False
    if c.objmask:
        # the first pass's frame (no candidate list: it is not the frame the catalogue is searched on), the object mask made of
        # it, and -- when the mask is usable -- the mesh once more without the masked pixels
        mini2back(ctx, mini, (ny, nx), bkg_boxsize=box, interp_Xchan=True, subtract_from=new, subtract_into=work)
        om = _objmask_stage(ctx, new, new_mask, work, mini, mini_std, box, c.objmask_nsigma, c.objmask_minarea, c.objmask_grow,
                            c.objmask_max_frac)
        hdr.update(om['header'])
        if om['objmask'] is not None:
            second_pass = True
            mini, mini_std = om['mini'], om['mini_std']
            res['objmask'], res['bkg_mini_pass1'], res['bkg_std_mini_pass1'] = om['objmask'], om['bkg_mini_pass1'], om['bkg_std_mini_pass1']
    if c.want_cat and (second_pass or not c.objmask):
        # the kernel that writes the background-subtracted frame lists the pixels above cat_nsigma x S-BKGSTD for the
        # catalogue's peak search; S-BKGSTD = median of the sigma mini image, taken on the device for that
        # (a frame that fell back to its first pass has that frame already: bbx_find_peaks makes its own pass)
        # (the call keeps the median: the peak search reads it on the device, to see that its threshold is the list's)
        c.d_sstd = torch.empty(1, dtype=torch.float32, device=ctx.device)
        check(lib.bbx_mini_median(ctx.h, mini_std.numel(), _p(mini_std), _p(c.d_sstd), ctx.stream()), 'bbx_mini_median', ctx.h)
        check(lib.bbx_zoom_candidates(ctx.h, _p(c.d_sstd), float(c.cat_nsigma)), 'bbx_zoom_candidates', ctx.h)
    if second_pass or not c.objmask:
        mini2back(ctx, mini, (ny, nx), bkg_boxsize=box, interp_Xchan=True, subtract_from=new, subtract_into=work)
    # the sigma image of the new frame: read off its mini image by the kernels that need it (catalogue photometry, the cut
    # into sub-images) where the geometry allows, a frame otherwise
    c.use_mini = frame_path_supported(c.L) and not c.sigma_frames and not os.environ.get('BBX_SIGMA_FRAMES')     # (the switch: A/B timing)
    bstd = None
    if c.use_mini:
        try:
            bstd = MiniImage(ctx, mini_std, box, interp_Xchan=False)
            c.use_mini = mini_path_supported((ny, nx), c.size, c.border, box, bstd)
        except ValueError:
            c.use_mini = False
    if not c.use_mini:
        bstd = mini2back(ctx, mini_std, (ny, nx), bkg_boxsize=box, interp_Xchan=False)
    res['bkg_mini_new'], sdn = fetch(ctx, mini, mini_std)
    res['bkg_std_mini_new'] = sdn
    hdr['BKG-SIZE'] = (box, '[pix] background boxsize used')
    hdr['BKG-SUB'] = (False, 'sky background was subtracted?')          # the _red product keeps its sky
    # zogy's per-channel background correction factors (BKG-CF1..16, BKG-FDEG, BKG-FC0: blackbox.py:3061-3066, all None_OK)
    # are [EXT] without a source in the reference tree: not applied here, and the header says so
    hdr['BKG-CORR'] = (False, 'channel background correction applied?')
    hdr['S-BKGSTD'] = (float(np.median(sdn)), '[e-] sigma (STD) background full-frame image')
    res['data_bkgsub'], res['bkg_std'] = work, bstd
    c.mini_std, c.work, c.sdn, c.bstd = mini_std, work, sdn, bstd
    c.sub_pn = subimage_psfs(ctx, c.psf_new, c.nsy, c.nsx, c.size) if c.psf_new is not None else None


def _tile_medians(c, a):
    """median of the mini image over the boxes of each sub-image (or over all of it)"""
    bs, nsy, nsx, nsub = c.bs, c.nsy, c.nsx, c.nsub
    if bs and a.shape == (nsy * bs, nsx * bs):
        return np.median(a.reshape(nsy, bs, nsx, bs).transpose(0, 2, 1, 3).reshape(nsub, bs * bs), axis=1)
    if bs:
        return np.asarray([np.median(a[(k // nsx) * bs:(k // nsx + 1) * bs, (k % nsx) * bs:(k % nsx + 1) * bs]) for k in range(nsub)])
    return np.full(nsub, np.median(a))


def _host_side_meanwhile(c):
    """host work that needs nothing from the device: done while a search runs there"""
    c.hdr['S-BKG'] = (float(np.median(c.res['bkg_mini_new'])), '[e-] median background full-frame image')
    return _tile_medians(c, c.sdn) if c.have_ref else None


def _reference_own_grid(c):
    """the reference as it comes, on its own grid: background-subtracted image + sigma mini image (made once per call: the
    registration measures its stars on it before _prepare_reference brings it to the new frame)"""
    if c.own:
        return c.own[0]
    ctx, ref, box, res = c.ctx, c.ref, c.box, c.res
    rny, rnx = ref.shape
    if c.ref_is_bkgsub:
        rwork = ref
        if c.ref_bkg_std_mini is None:
            _, rstd_mini = get_back(ctx, ref, c.ref_mask, bkg_boxsize=box)
            sdr = fetch(ctx, rstd_mini)
        else:
            sdr = np.asarray(c.ref_bkg_std_mini, np.float32)
    else:
        rmini, rstd_mini = get_back(ctx, ref, c.ref_mask, bkg_boxsize=box)
        rwork = torch.empty_like(ref)
        mini2back(ctx, rmini, (rny, rnx), bkg_boxsize=box, interp_Xchan=True, subtract_from=ref, subtract_into=rwork)
        res['bkg_mini_ref'], sdr_meas = fetch(ctx, rmini, rstd_mini)
        sdr = sdr_meas if c.ref_bkg_std_mini is None else np.asarray(c.ref_bkg_std_mini, np.float32)
    res['bkg_std_mini_ref'] = sdr
    c.own.append((rwork, sdr))
    return c.own[0]


def _prepare_reference(c):
    """the reference frame on the new frame's grid: background-subtracted image + sigma image (before the star match
    where that is asked for, else where the subtraction needs it) -> (image, sigma image, sigma mini image on the host, PSF stamps
    of the sub-images, hand-written path?)"""
    ctx, ref, box, res, size, border = c.ctx, c.ref, c.box, c.res, c.size, c.border
    ny, nx = c.ny, c.nx
    rny, rnx = ref.shape
    rwork, sdr = _reference_own_grid(c)
    if c.ref_grid is not None:
        from . import coadd
        ones = torch.ones_like(rwork)
        rwork, _ = coadd.resample(ctx, rwork, ones, c.ref_grid, (ny, nx), 1.0, c.ref_grid_step)
        # (a registration's lattice lives on the device: the mini image is remapped with its host twin)
        sdr = remap_mini(sdr, c.ref_grid_host if c.ref_grid_host is not None else np.asarray(c.ref_grid), (rny, rnx), box, c.ref_grid_step,
                         shape_out=(ny, nx))
    elif (rny, rnx) != (ny, nx):
        raise ValueError('reference frame of another shape needs ref_grid')
    # co-added reference: no channel structure in its noise -> interpolation across the frame
    # (a RefPsf of this psf_ref: its own stamp tensor, the one its spectra were made of -- the library knows them by pointer)
    rpsf = c.ref_psf if c.ref_psf is not None and c.ref_psf.matches(c.psf_ref, (ny, nx), size, border) else None
    sub_pr = rpsf.stamps if rpsf is not None else subimage_psfs(ctx, c.psf_ref, c.nsy, c.nsx, size)
    frame_path = frame_path_supported(c.L) and c.sub_pn.shape[1] == sub_pr.shape[1]
    ref_bkg_std = c.ref_bkg_std
    if ref_bkg_std is not None and c.ref_grid is None and tuple(ref_bkg_std.shape) == (ny, nx) and isinstance(ref_bkg_std, MiniImage) == c.use_mini:
        rbstd = ref_bkg_std
    elif c.use_mini and frame_path:
        rbstd = MiniImage(ctx, np.asarray(sdr, np.float32), box, interp_Xchan=True)
        if not mini_path_supported((ny, nx), size, border, box, rbstd):
            rbstd = rbstd.frame(ctx)
    else:
        rbstd = mini2back(ctx, sdr, (ny, nx), bkg_boxsize=box, interp_Xchan=True)
    if isinstance(c.bstd, MiniImage) and not (frame_path and isinstance(rbstd, MiniImage)):
        c.bstd = res['bkg_std'] = c.bstd.frame(ctx)                # the other side needs frames: both as frames
        if isinstance(rbstd, MiniImage):
            rbstd = rbstd.frame(ctx)
    res['ref_bkgsub'], res['bkg_std_ref'] = rwork, rbstd
    c.hdr_t['S-BKGSTDR'] = (float(np.median(sdr)), '[e-] sigma (STD) background reference image')
    return rwork, rbstd, sdr, sub_pr, frame_path


def _register_reference(c, new_list):
    """ref_align: the reference's star list on its own grid (the caller's RefStars of this very reference, else made
    here), the registration against the new frame's list (ys, xs, off, flux, err on the device; None: the frame has none)
    and, where it succeeds, the lattice in place of ref_grid and the remapped mask in place of ref_mask.  Where it fails the
    frame goes on as one without a reference"""
    ctx, ref, psf_ref, size, box, res, hdr, hdr_t = c.ctx, c.ref, c.psf_ref, c.size, c.box, c.res, c.hdr, c.hdr_t
    ny, nx = c.ny, c.nx
    al, why = None, None
    try:
        if new_list is None:
            raise ValueError('the new frame has no source list (no PSF, or nothing above the threshold)')
        if psf_ref is None:
            raise ValueError('no PSF of the reference')
        rs = c.ref_stars if c.ref_stars is not None and c.ref_stars.matches(ref) else None
        if rs is None:
            rwork_own, sdr_own = _reference_own_grid(c)
            rny, rnx = ref.shape
            if isinstance(psf_ref, dict) or psf_ref.dim() == 2:
                r_nsy, r_nsx = max(1, rny // size), max(1, rnx // size)
            else:                                                # stamps of the new frame's tiling: the clamped tile's plane
                r_nsy, r_nsx = c.nsy, c.nsx
            stamps = subimage_psfs(ctx, psf_ref, r_nsy, r_nsx, size).contiguous()
            sig_med = float(np.median(sdr_own))
            try:
                sig = mini2back(ctx, sdr_own, (rny, rnx), bkg_boxsize=box, interp_Xchan=True)
            except (ValueError, _lib_BBXError):                  # a reference that is no multiple of the box: one level
                sig = torch.full((rny, rnx), sig_med, dtype=torch.float32, device=ctx.device)
            rs = RefStars(ctx, rwork_own, sig, c.ref_mask, stamps, r_nsy, r_nsx, size, c.cat_nsigma, sigma_median=sig_med,
                          max_sources=c.max_sources, made_of=ref)
        res['ref_stars'] = rs
        al = align_reference(ctx, new_list, rs, (ny, nx), tuple(ref.shape), c.ref_mask, poldeg=c.align_poldeg, max_shift=c.align_max_shift,
                             bin=c.align_bin, dist=c.match_dist, snr_min=c.match_snr_min, step=c.ref_grid_step, rounds=c.align_rounds,
                             nbright=c.align_nbright)
        if al['flags'] != 0:
            why = 'flag word %d (vote %s)' % (al['flags'], np.asarray(al['fit']['info']).tolist())
    except Exception as e:                                       # the frame goes on without its reference
        al, why = None, str(e)
    res['align'] = al
    if why is None:
        c.ref_grid, c.ref_grid_host, c.ref_mask_remapped = al['grid'], align_grid_host(al['coef'], (ny, nx), c.ref_grid_step), al['mask']
        res['ref_mask_remapped'] = al['mask']
        hdr_t.update(al['header'])
        return True
    logging.getLogger(__name__).warning('registration of the reference failed (%s): processing the new image only', why)
    hdr_t.update(al['header'] if al is not None else align_header(None))
    hdr_t['T-NOFFR'] = ('None', 'candidates dropped: no reference there')
    hdr.update({k: v for k, v in hdr_t.items() if k.startswith('A-')})         # (no _trans products will carry them: the frame's own header does)
    c.have_ref = c.do_match = False
    return False


def _limflux_enqueue(c):
    """the limiting-flux image and its frame statistic, queued on the frame's stream -> [statistic [8] float64, windows [nsub]
    int32] on the device; None (and a warning) where the stage fails"""
    try:
        lim, win = _limflux_image(c.ctx, c.bstd, c.new_mask, c.sub_pn.contiguous(), c.size, c.nsy, c.nsx, nsigma=c.lim_nsigma, frac=c.lim_frac)
        d_lst = frame_clipped_stats_enqueue(c.ctx, lim, c.new_mask)
        c.res['limflux'] = lim
        return [d_lst, win]
    except Exception as ex:                                      # the frame goes on without the image
        logging.getLogger(__name__).warning('limiting-flux image of the reduced frame failed: %s', ex)
        c.res.pop('limflux', None)
        return None


def _limflux_finish(c, got):
    """got: the host copies of _limflux_enqueue's pair, or None"""
    c.res['limflux_info'] = dict(stat=got[0] if got else None, win=got[1] if got else None, nsigma=c.lim_nsigma, frac=c.lim_frac)
    c.hdr.update(limflux_header(got is not None, *(got or (None, None)), nsigma=c.lim_nsigma, frac=c.lim_frac))


def _astrometry_enqueue(c, new_list):
    """astrometry: the solve of the frame's list (ys, xs, off, flux, err on the device) against the catalogue, queued -> what
    astrometry.solve_finish wants; None (and a warning) where the stage fails before it is queued"""
    try:
        if c.ast_catalog is None:
            raise ValueError('no catalogue (ast_catalog)')
        return _ast.solve_enqueue(c.ctx, new_list, c.ast_catalog, c.ast_pointing, (c.ny, c.nx), pixscale=c.ast_pixscale, rot=c.ast_rot,
                                  parity=c.ast_parity, max_shift=c.ast_max_shift, bin=c.ast_bin, poldeg=c.ast_poldeg, rounds=c.ast_rounds,
                                  dist=c.ast_dist, snr_min=c.match_snr_min, mag_zp=c.ast_mag_zp)
    except Exception as ex:                                      # the frame goes on without a solution
        logging.getLogger(__name__).warning('astrometric solve failed: %s', ex)
        return None


def _astrometry_sky(c, **where):
    """the sky positions of device positions by the frame's solution -> device float64 [n, 2]; None where that fails"""
    p = c.ast_pending
    try:
        return _ast.pix2sky(c.ctx, p['coef'], p['shape'], p['cd'], p['pointing'], **where)
    except Exception as ex:
        logging.getLogger(__name__).warning('sky positions by the astrometric solution failed: %s', ex)
        return None


def _catalogue(c):
    """full-source catalogue (a17): peaks of the background-subtracted frame above cat_nsigma x S-BKGSTD, PSF-weighted optimal
    flux at each (zogy.get_psfoptflux), what is queued behind the photometry and read in its copy back, and the ends of the
    frames on which no list was formed"""
    res, hdr = c.res, c.hdr
    res['catalog'] = None
    if c.want_cat:
        ys, xs, pk = _catalogue_peaks(c)
    if c.want_phot and c.sub_pn is not None:
        _catalogue_photometry(c, ys, xs, pk)
    if c.do_ast and 'astrometry' not in res:
        # no list was formed (no PSF of the new frame, nothing above the threshold) or the stage failed before it was queued
        res['astrometry'] = None
        hdr.update(ast_header(None))
    if c.do_lim and 'limflux_info' not in res:
        # no photometry was read back (no catalogue asked for, no PSF, or nothing above the threshold): a copy back of its own
        rb = Readback()
        d_lim = _limflux_enqueue(c) if c.sub_pn is not None else None
        if d_lim is not None:
            rb.add('lim', *d_lim)
        _limflux_finish(c, rb.fetch(c.ctx).get('lim'))
    if 'S-BKG' not in hdr:
        c.scal_n = _host_side_meanwhile(c)
    if c.do_align and c.have_ref and 'align' not in res:
        _register_reference(c, None)                                 # (no photometry ran: no PSF of the new frame)


def _catalogue_peaks(c):
    """the peak search of the catalogue, with the host's work and the match-only preparation of the reference behind its launch,
    and the PSF build from these very peaks -> ys, xs, pk on the host"""
    ctx, res, hdr = c.ctx, c.res, c.hdr
    thr = float(c.cat_nsigma) * hdr['S-BKGSTD'][0]
    if np.isfinite(thr) and thr > 0:
        pending = find_peaks_enqueue(ctx, c.work, thr, max_out=c.max_sources)
        if c.do_match and not c.build_here and not c.do_align:       # (a reference to be registered is prepared behind the photometry)
            c.ref_side = _prepare_reference(c)                       # (behind the search: its zoom would drop the candidate list)
        c.scal_n = _host_side_meanwhile(c)
        ys, xs, pk = find_peaks_collect(ctx, pending)
    else:                                                            # no usable noise level: nothing is significant
        lib.bbx_zoom_candidates(ctx.h, None, 0.0)
        if c.do_match and not c.build_here and not c.do_align:
            c.ref_side = _prepare_reference(c)
        c.scal_n = _host_side_meanwhile(c)
        ys = xs = np.zeros(0, np.int32); pk = np.zeros(0, np.float32)
    keep = pk > 0
    ys, xs, pk = ys[keep], xs[keep], pk[keep]
    if c.build_here:
        # the model from this very list of peaks; from here on the frame is one whose PSF was given
        res['psf'] = build_psf(ctx, c.work, c.mini_std, c.new_mask, c.size, c.nsy, c.nsx, c.cat_nsigma, sigma_median=hdr['S-BKGSTD'][0],
                               peaks=(ys, xs, pk), psf_size=c.psf_size, poldeg=c.psf_poldeg, max_sources=c.max_sources)
        hdr.update(res['psf']['header'])
        c.psf_new = res['psf']['model']
        if c.psf_new is not None:
            c.sub_pn = subimage_psfs(ctx, c.psf_new, c.nsy, c.nsx, c.size)
            if c.do_match and not c.do_align:
                c.ref_side = _prepare_reference(c)
        else:                                                        # no model: the frame of today without --psf_new
            c.want_phot = c.do_match = c.do_shapes = c.do_aper = c.have_ref = False
    return ys, xs, pk


def _centroids(c, d_y32, d_x32, sigw):
    """the windowed centroids of the catalogue's peaks, taken on first use and once: for the photometry (phot_centroid), the shapes,
    the apertures, the registration, the astrometric solve and the star match"""
    if c.peaks_off is None:
        c.peaks_off = (d_y32, d_x32, win_centroid(c.ctx, c.work, d_y32, d_x32, sigw, c.size, c.nsy, c.nsx))
    return c.peaks_off[2]


def _catalogue_photometry(c, ys, xs, pk):
    """the photometry of the peaks with everything that rides its copy back, and the catalogue's columns and header keys"""
    if ys.size:
        rb, rc = _catalogue_enqueue(c, ys, xs)
        m = _catalogue_measured(c, rb.fetch(c.ctx), rc)
        ok = m['ok']
        ys, xs, pk = ys[ok], xs[ok], pk[ok]
    else:
        m = _catalogue_of_no_peaks(c)
    _catalogue_table(c, ys, xs, pk, m)


def _catalogue_enqueue(c, ys, xs):
    """queued on the frame's stream: the photometry at the peaks and, behind it, the registration, the astrometric solve, the
    shapes, the star match, the apertures, the limiting-flux image -> the copy back of all of them, the reference's catalogue"""
    ctx, new_mask, size, nsy, nsx = c.ctx, c.new_mask, c.size, c.nsy, c.nsx
    # peaks on masked pixels are dropped; their mask values come back with the fluxes (one host wait: the photometry
    # of the few masked ones is made and thrown away)
    d_ys, d_xs = push(ctx, ys.astype(np.int64), xs.astype(np.int64))
    d_mk = new_mask[d_ys, d_xs]
    if c.phot_centroid or c.do_shapes or c.do_align or c.do_aper or c.do_ast:
        # what _centroids wants: the peaks as int32 and the window
        d_y32, d_x32 = push(ctx, ys.astype(np.int32), xs.astype(np.int32))
        sigw = window_sigma(c.sub_pn)
    if c.phot_centroid:
        f, e, d_pfl = psf_optflux_centroid(ctx, c.work, c.bstd, c.psf_new, c.sub_pn, ys, xs, _centroids(c, d_y32, d_x32, sigw), new_mask, nsx,
                                           size, d_peaks=(d_y32, d_x32))
    else:
        stamps = source_psfs(ctx, c.psf_new, c.sub_pn, ys, xs, nsx, size)
        f, e = psf_optflux(ctx, c.work, c.bstd, stamps, ys, xs, v_is_sigma=True)        # (bstd: frame or MiniImage)
    if c.do_align or c.do_ast:
        # the new frame's list as the star match sees it (a peak on a masked pixel: no offset, no flux)
        off = _centroids(c, d_y32, d_x32, sigw)
        bad = d_mk != 0
        a_off = torch.where(bad[:, None], torch.full_like(off, float('nan')), off).contiguous()
        new_list = (d_y32, d_x32, a_off, torch.where(bad, torch.zeros_like(f), f).contiguous(), e)
    if c.do_align:
        # the registration, then the reference on this frame's grid -- before anything below asks for it
        if _register_reference(c, new_list):
            c.ref_side = _prepare_reference(c)
    if c.do_ast:
        c.ast_pending = _astrometry_enqueue(c, new_list)             # queued: read back with the photometry
    rb = Readback()
    rb.add('phot', d_mk, f, e)
    if c.do_shapes:
        # the moments and their statistics are queued behind the photometry and come back with it
        d_shp, d_sfl = src_shapes(ctx, c.work, new_mask, d_y32, d_x32, _centroids(c, d_y32, d_x32, sigw), sigw, size, nsy, nsx)
        d_stab = shape_stats(ctx, d_y32, d_x32, d_shp, d_sfl, f, e, size, nsy, nsx, c.shape_snr_min)
    rc = None
    if c.do_match:
        # the star match rides on the same copy back: centroids, match against the reference's catalogue (the run's,
        # or made here) and the table of clipped statistics are queued behind the photometry
        rwork, rbstd, _, sub_pr, _ = c.ref_side
        rc = c.ref_catalog if c.ref_catalog is not None and c.ref_catalog.matches(rwork, rbstd, size, c.border, c.phot_centroid) else \
            RefCatalog(ctx, rwork, rbstd, c.ref_mask if c.ref_grid is None else c.ref_mask_remapped, c.psf_ref, size, c.border,
                       cat_nsigma=c.cat_nsigma, sigma_median=c.hdr_t['S-BKGSTDR'][0], sub_psfs=sub_pr, max_sources=c.max_sources,
                       phot_centroid=c.phot_centroid)
        rb.add('match', *match_enqueue(ctx, c.work, ys, xs, d_mk, f, e, c.sub_pn, rc, size, nsy, nsx, c.match_dist, c.match_snr_min,
                                       peaks_off=c.peaks_off))
    d_aper = None
    if c.do_aper:
        # the apertures and the annulus are queued behind the photometry and come back with it, the frame's FWHM too
        try:
            off = _centroids(c, d_y32, d_x32, sigw)
            d_afw = aper_fwhm(c.sub_pn)
            d_aper = _aper_phot(ctx, c.work, c.bstd, new_mask, d_y32, d_x32, off, d_afw.expand(c.nsub).contiguous(), size, nsy, nsx,
                                radii=c.apphot_radii, sky_inout=c.apphot_sky_inout, sub_sky=c.apphot_local_sky)
        except Exception as ex:                                  # the frame keeps today's catalogue
            logging.getLogger(__name__).warning('aperture photometry of the catalogue failed: %s', ex)
            d_aper = None
    if c.do_shapes:
        rb.add('shapes', d_shp, d_sfl, d_stab)
    if c.phot_centroid:
        rb.add('centroid', c.peaks_off[2], d_pfl)
    if d_aper is not None:
        rb.add('aper', *d_aper, d_afw)                               # (flux, err, sky, flags, FWHM)
    d_lim = _limflux_enqueue(c) if c.do_lim else None                # behind the photometry, in the same copy back
    if d_lim is not None:
        rb.add('lim', *d_lim)
    if c.ast_pending is not None:
        # the solution's six small tensors, and the sky positions of the catalogue's rows at the float32 positions X_POS /
        # Y_POS will state (formed here as below: shapes', else the photometry's centroids, else the peaks), in the same copy back
        d_csky = None
        if c.cat_extract:
            if c.do_shapes:
                o32 = torch.where(torch.isnan(d_shp[:, :2]), torch.zeros_like(d_shp[:, :2]), d_shp[:, :2])
            elif c.phot_centroid:
                o32 = torch.where(((d_pfl & PHOT_NO_CENTROID) == 0)[:, None], c.peaks_off[2], torch.zeros_like(c.peaks_off[2]))
            else:
                o32 = torch.zeros((int(ys.size), 2), dtype=torch.float32, device=ctx.device)
            p32 = (torch.stack([d_x32, d_y32], dim=1).to(torch.float32) + 1.0) + o32.flip(1)
            d_csky = _astrometry_sky(c, pos=(p32.to(torch.float64) - 1.0).contiguous())
        rb.add('ast', *c.ast_pending['back'])
        if d_csky is not None:
            rb.add('csky', d_csky)
    return rb, rc


def _catalogue_measured(c, got, rc):
    """the host copies of _catalogue_enqueue's copy back -> what _catalogue_table wants, without the peaks on masked pixels ('ok')"""
    res = c.res
    if c.ast_pending is not None:
        c.ast_sol = _ast.solve_finish(c.ast_pending, got['ast'])
    if c.do_lim:
        _limflux_finish(c, got.get('lim'))
    mk, f, e = got['phot']
    if c.do_match:
        c.mtab, npairs = got['match']
        res['ref_catalog'] = rc
        res['match'] = dict(n_new=int((mk == 0).sum()), n_ref=rc.n, n_pairs=int(npairs[0]))
    ok = mk == 0
    m = dict(ok=ok, f=f[ok], e=e[ok], aper=None, csky=got['csky'][0] if 'csky' in got else None)
    if c.phot_centroid:
        m['poff'], m['pfl'] = [a[ok] for a in got['centroid']]
    if c.do_shapes:
        shp, sfl, m['stab'] = got['shapes']
        m['shp'], m['sfl'] = shp[ok], sfl[ok]
    if 'aper' in got:
        m['aper'] = [a[ok] for a in got['aper'][:4]] + [float(got['aper'][4][0])]
    return m


def _catalogue_of_no_peaks(c):
    """what _catalogue_table wants for a frame with nothing above the threshold (the registration fails for want of a list)"""
    if c.do_align:
        _register_reference(c, None)
    m = dict(ok=None, f=np.zeros(0, np.float32), e=np.zeros(0, np.float32), shp=np.zeros((0, 8), np.float32), sfl=np.zeros(0, np.uint8),
             stab=empty_shape_table(c.nsub), poff=np.zeros((0, 2), np.float32), pfl=np.zeros(0, np.uint8), aper=None, csky=None)
    if c.do_aper:
        try:
            na = len(_aper_radii(c.apphot_radii))
            m['aper'] = [np.zeros((0, na), np.float32), np.zeros((0, na), np.float32), np.zeros((0, 3), np.float32), np.zeros(0, np.uint8),
                         float(fetch(c.ctx, aper_fwhm(c.sub_pn))[0])]
        except Exception as ex:
            logging.getLogger(__name__).warning('aperture photometry of the catalogue failed: %s', ex)
    return m


def _catalogue_table(c, ys, xs, pk, m):
    """res['catalog'] and the header keys of the catalogue and of what rode its copy back (m: _catalogue_measured's dict)"""
    res, hdr, f, e, aper = c.res, c.hdr, m['f'], m['e'], m['aper']
    if c.cat_extract:
        res['catalog'] = dict(Y_POS=ys.astype(np.float32) + 1, X_POS=xs.astype(np.float32) + 1,
                              E_FLUX_PEAK=pk.astype(np.float32), E_FLUX_OPT=f, E_FLUXERR_OPT=e,
                              SNR_OPT=np.where(e > 0, f / np.where(e > 0, e, 1), 0).astype(np.float32))
        hdr['NOBJECTS'] = (len(ys), 'number of objects detected')
        if c.phot_centroid:
            # positions as shape_columns forms them: peak + 1 + offset, the integer peak where there is no centroid
            cen = ((m['pfl'] & PHOT_NO_CENTROID) == 0)[:, None]
            o = np.where(cen, m['poff'], np.float32(0)).astype(np.float32)
            res['catalog'].update(Y_POS=(ys.astype(np.float32) + np.float32(1)) + o[:, 0], X_POS=(xs.astype(np.float32) + np.float32(1)) + o[:, 1],
                                  FLAGS_OPT=m['pfl'].astype(np.uint8))
    if c.phot_centroid:
        hdr['PHOT-CEN'] = (True, 'PSF placed on the centroids in the catalogue photometry?')
    if c.do_shapes:
        res['catalog'].update(shape_columns(ys, xs, m['shp'], m['sfl']))
        res['shapes'] = dict(table=m['stab'], n_good=int(m['stab'][c.nsub, _SC['n_fwhm']]))
        hdr.update(shape_header(m['stab'], len(ys), settings.shape_nmin, settings.pixscale))
    if c.do_aper and aper is not None:
        cat = res['catalog']
        acols = aper_columns(*aper, radii=c.apphot_radii)
        hdr.update(aper_header(True, aper[4], c.apphot_radii, c.apphot_sky_inout, c.apphot_local_sky, acols, cat['E_FLUX_OPT'], cat['SNR_OPT']))
        cat.update(acols)
        res['aper'] = dict(fwhm=aper[4], radii=_aper_radii(c.apphot_radii), n_good=hdr['AP-NSTAR'][0])
    elif c.do_aper:
        hdr.update(aper_header(False))
    ast_sol = c.ast_sol
    if ast_sol is not None:
        res['astrometry'] = ast_sol
        hdr.update(ast_sol['header'])
        if ast_sol['ok'] and c.cat_extract and m['csky'] is not None:
            res['catalog'].update(RA=m['csky'][m['ok'], 0].copy(), DEC=m['csky'][m['ok'], 1].copy())
        elif not ast_sol['ok']:
            logging.getLogger(__name__).warning('astrometric solve failed: flag word %d (vote %s)', ast_sol['flags'],
                                                np.asarray(ast_sol['fit']['info']).tolist())


def _fake_stars(c):
    """fake stars: planted in the frame that is about to be cut, behind everything that reads the frame as it was observed ->
    dict(layout, inj, peaks, noise, radius) of the stars that ride the subtraction; None without the switch or where nothing was planted"""
    if not (c.fake_stars and int(c.fake_stars) > 0):
        return None
    ctx, sub_pn, size = c.ctx, c.sub_pn, c.size
    fk_noise = settings.fakestar_noise if c.fake_noise is None else bool(c.fake_noise)
    fk_radius = int(settings.fakestar_radius if c.fake_radius is None else c.fake_radius)
    fk_prep = None
    try:
        # everything that can fail before the frame is touched (fake_prepare): an exception leaves the frame as it is
        if sub_pn is None:
            raise ValueError('no PSF stamps of the new frame')
        if not 0 <= fk_radius <= 4:
            raise ValueError('fake_radius: 0 .. 4 pixels expected')
        lay = fake_layout(c.ny, c.nx, size, c.nsy, c.nsx, int(sub_pn.shape[1]), int(c.fake_stars),
                          settings.fakestar_s2n if c.fake_s2n is None else c.fake_s2n, settings.fakestar_seed if c.fake_seed is None else c.fake_seed)
        fk_prep = fake_prepare(ctx, c.work, c.ref_side[0], c.bstd, c.new_mask, c.ref_mask if c.ref_grid is None else c.ref_mask_remapped,
                               c.psf_new, sub_pn, lay, c.nsx, size, clear_half=settings.fake_clear_half,
                               clear_nsigma=settings.fake_clear_nsigma if c.fake_clear_nsigma is None else c.fake_clear_nsigma,
                               noise=fk_noise, seed=lay['seed'])
    except Exception as ex:
        logging.getLogger(__name__).warning('fake stars were not injected: %s', ex)
        c.hdr_t.update(fake_header(False))
    if fk_prep is None:
        return None
    # the launch itself is not survived: a frame that may carry stars is never subtracted under T-FKP False
    fk_inj, fk_peaks = _fake_launch(ctx, fk_prep)
    return dict(layout=lay, inj=fk_inj, peaks=fk_peaks, noise=fk_noise, radius=fk_radius)


def _subtract(c):
    """the sub-images: their scalars (sigmas, and fratio, dx, dy as given or as the star match measured them), then cut, variance
    images, ZOGY and stitching on the hand-written path or through rocFFT -> scal [nsub, 6], the match's scalars or None, and on
    the hand-written path what _zogy_frame_call wants for a second call"""
    ctx, res, size, border, nsub = c.ctx, c.res, c.size, c.border, c.nsub
    rwork, rbstd, sdr, sub_pr, frame_path = c.ref_side
    scal = np.zeros((nsub, 6), np.float32)
    scal[:, 0], scal[:, 1] = c.scal_n, _tile_medians(c, sdr)
    # fratio, dx, dy: one number for the frame or one per sub-image (zogy measures them per sub-image from the matched stars)
    ms = None
    if c.do_match:
        # measured here (match=True): per sub-image where it has the pairs, the frame's values elsewhere, the caller's as fallback
        if c.mtab is None:
            c.mtab = empty_match_table(nsub)
            res['match'] = dict(n_new=0, n_ref=c.ref_catalog.n if c.ref_catalog is not None else 0, n_pairs=0)
        ms = match_scalars(c.mtab, c.fratio, c.dx, c.dy, settings.match_nmin if c.match_nmin is None else c.match_nmin)
        if not ms['success']:
            logging.getLogger(__name__).warning('star match: %d qualifying pairs in the frame, fewer than the minimum: fratio, dx, dy as given '
                                                'by the caller', int(c.mtab[nsub, 0]))
        res['match'].update(success=ms['success'], table=c.mtab, fratio_sub=ms['fratio_sub'], dx_sub=ms['dx_sub'], dy_sub=ms['dy_sub'])
        fratio_in, dx_in, dy_in = ms['fratio_sub'], ms['dx_sub'], ms['dy_sub']
    else:
        fratio_in, dx_in, dy_in = c.fratio, c.dx, c.dy
    fr = np.broadcast_to(np.asarray(fratio_in, np.float64), (nsub,))
    scal[:, 2], scal[:, 3] = 1.0, np.where(fr != 0, 1.0 / np.where(fr != 0, fr, 1.0), 1.0)
    scal[:, 4], scal[:, 5] = np.broadcast_to(np.asarray(dx_in, np.float64), (nsub,)), np.broadcast_to(np.asarray(dy_in, np.float64), (nsub,))
    c.sub_pr = sub_pr
    if frame_path:
        # hand-written FFT path: cut, variance images, ZOGY and stitching in one library call
        outs = zogy_frame_outputs(c.work)                         # allocated on the caller's stream, filled inside the gate
        c.sub_pn, c.sub_pr = c.sub_pn.contiguous(), sub_pr.contiguous()
        rows = c.ref_rows if c.ref_rows is not None and c.ref_rows.matches(rwork, rbstd, size, border) else None
        # prepared reference PSF spectra: with prepared rows only, and only where sub_pr is the tensor they were made of
        rpsf = c.ref_psf if rows is not None and c.ref_psf is not None and c.sub_pr is c.ref_psf.stamps else None
        frame_args = (scal, outs, rows, rpsf)
        D, _, Scorr, Fpsf, Fpsferr = _zogy_frame_call(c, frame_args)
        res['D'], res['Scorr'], res['Fpsf'], res['Fpsferr'] = D, Scorr, Fpsf, Fpsferr
        return scal, ms, frame_args
    Vn = variance(ctx, c.work, c.bstd)
    Vr = variance(ctx, rwork, rbstd)
    subs = [cut_subimages(ctx, a, size, border) for a in (c.work, rwork, Vn, Vr)]
    Pn, Pr = embed_psfs(ctx, c.sub_pn, c.L), embed_psfs(ctx, sub_pr, c.L)
    D, S, Scorr, Fpsf, Fpsferr = run_zogy(ctx, subs[0], subs[1], Pn, Pr, subs[2], subs[3], scal)
    del subs, Pn, Pr, S, Vr, Vn
    for name, a in (('D', D), ('Scorr', Scorr), ('Fpsf', Fpsf), ('Fpsferr', Fpsferr)):
        res[name] = stitch_subimages(ctx, a, (c.ny, c.nx), size, border)
    return scal, ms, None


def _zogy_frame_call(c, frame_args):
    """bbx_zogy_frame on the call's frames and (scal, outs, rows, rpsf): the very ones of the first call when it is repeated"""
    scal, outs, rows, rpsf = frame_args
    rwork, rbstd = c.ref_side[:2]
    # the kernel that writes Scorr lists the pixels above the transient threshold for the peak search below
    check(lib.bbx_zogy_candidates(c.ctx.h, float(c.nsig)), 'bbx_zogy_candidates', c.ctx.h)
    with (c.zogy_gate or _NoGate()):
        return run_zogy_frame(c.ctx, c.work, rwork, c.bstd, rbstd, c.sub_pn, c.sub_pr, scal, c.size, c.border, outs=outs, ref_rows=rows,
                              ref_psf=rpsf)


def _transient_search(c, frame_args):
    """transient candidates: regions of |Scorr| >= T-NSIGMA -> ys, xs, scorr of the peaks on the host, T-NTRANS"""
    ctx = c.ctx
    for attempt in (0, 1):
        try:
            # (the first host wait behind bbx_zogy_frame: its device-side checks surface here)
            tys, txs, tsc = find_peaks_arrays(ctx, c.res['Scorr'], c.nsig)
            ntrans = int(tys.size)
        except _lib_BBXError as e:
            if e.code == BBX_ERR_PSFWIN and frame_args is not None and attempt == 0:
                # the matched-filter kernels of these PSFs do not fit their row window (include/bbx.h, BBX_OPT_ZOGY_KWIN_OFF):
                # V(S) of this call is off by more than the tolerance.  Once more on all rows -- the frame keeps its subtraction
                check(lib.bbx_set_option(ctx.h, BBX_OPT_ZOGY_KWIN_OFF, 1), 'bbx_set_option', ctx.h)
                try:
                    _zogy_frame_call(c, frame_args)
                finally:
                    check(lib.bbx_set_option(ctx.h, BBX_OPT_ZOGY_KWIN_OFF, 0), 'bbx_set_option', ctx.h)
                c.hdr_t['Z-KWIN'] = (False, 'ZOGY matched-filter kernels on a row window?')
                continue
            if e.code != BBX_ERR_OVERFLOW:
                raise
            # more significant pixels than the candidate list holds (a failed subtraction: wrong
            # reference, gross misalignment): the images stand, the candidate table stays empty
            tys = txs = np.zeros(0, np.int32); tsc = np.zeros(0, np.float32)
            ntrans = 'None'
        break
    return tys, txs, tsc, ntrans


def _transient_readback(c, scal, fk, tys, txs):
    """the fluxes at the candidates, the fits, the thumbnails, the frame statistics of the header, the fake stars and the sky
    positions: queued together, one copy back, one host wait -> {name: [array]} of those that were queued"""
    ctx, res, hdr_t, new_mask, sub_pn, sub_pr = c.ctx, c.res, c.hdr_t, c.new_mask, c.sub_pn, c.sub_pr
    rbstd = c.ref_side[1]
    d_fe = d_st = d_fl = None
    if tys.size:
        d_ys, d_xs = push(ctx, tys.astype(np.int64), txs.astype(np.int64))
        d_fe = torch.stack([res['Fpsf'][d_ys, d_xs], res['Fpsferr'][d_ys, d_xs]])
    d_edge = None
    if tys.size and c.ref_mask_remapped is not None:
        # the registered reference's mask under every candidate: where it carries the edge bit the frame has no reference, D
        # is the new frame there and every star a candidate
        d_edge = (c.ref_mask_remapped[d_ys, d_xs] & settings.mask_value['edge']).to(torch.float32)
    d_tf = None
    if c.trans_psffit:
        hdr_t['T-PSFD'] = trans_fit_header(False)['T-PSFD']          # until the fit has been read back
    if c.trans_psffit and tys.size and sub_pn is not None and sub_pr is not None and tuple(sub_pn.shape) == tuple(sub_pr.shape):
        try:
            d_pd, d_fold = pd_stamps(ctx, sub_pn, sub_pr, scal)
            fit = _trans_psffit(ctx, res['D'], res['data_bkgsub'], res['ref_bkgsub'], c.bstd, rbstd, new_mask, d_pd, tys, txs, scal, c.size, c.nsx,
                                fit_size=c.fit_size)
            d_tf = torch.cat([torch.stack(list(fit[:5]) + [fit[5].to(torch.float32)]).reshape(-1), d_fold])
        except Exception as e:                                       # the frame keeps today's table
            logging.getLogger(__name__).warning('fit of P_D to the transient candidates failed: %s', e)
            d_tf = None
    d_ts = None
    if c.trans_shapefit:
        hdr_t['T-SHAPE'] = trans_shape_header(False)['T-SHAPE']      # until the fits have been read back
    if c.trans_shapefit and tys.size and sub_pn is not None and sub_pr is not None and tuple(sub_pn.shape) == tuple(sub_pr.shape):
        try:
            sh_out, sh_fl = _trans_shapefit(ctx, res['D'], res['data_bkgsub'], res['ref_bkgsub'], c.bstd, rbstd, new_mask,
                                            shape_start_fwhm(sub_pn, sub_pr), tys, txs, scal, c.size, c.nsx, fit_size=c.shape_size)
            d_ts = torch.cat([sh_out.reshape(-1), sh_fl.to(torch.float32).reshape(-1)])
        except Exception as e:                                       # the frame keeps today's table
            logging.getLogger(__name__).warning('Gauss and Moffat fits to the transient candidates failed: %s', e)
            d_ts = None
    if c.thumbnails or c.thumbnail_pngs:
        # the cut-outs of the four frames, which are all still in HBM, and the mask flags under each peak in one pass; the
        # display planes from the cut-outs.  The reference's mask counts only where it shares the new frame's grid
        d_fl = thumbnail_stamps(ctx, res, (res['data_bkgsub'], res['ref_bkgsub'], res['D'], res['Scorr']), tys, txs,
                                int(c.thumbnail_size or settings.size_thumbnails), new_mask,
                                c.ref_mask if c.ref_grid is None else c.ref_mask_remapped, floats=c.thumbnails, pngs=c.thumbnail_pngs)
    if c.frame_stats:
        # statistics over the unmasked pixels (new frame's mask), clipped like zogy's header values
        d_st = torch.stack([frame_clipped_stats_enqueue(ctx, res['Scorr'], new_mask),
                            frame_clipped_stats_enqueue(ctx, res['Fpsferr'], new_mask)])
    if d_fl is not None and not d_fl.numel():
        d_fl = None
    d_fk = None
    if fk is not None:
        # the stars read back, with what the injection wrote per star: one more tensor in the same copy back
        d_rec = _fake_recover(ctx, res['Scorr'], res['Fpsf'], res['Fpsferr'], fk['layout'], fk['radius'], d_peaks=fk['peaks'])
        d_fk = torch.cat([d_rec.reshape(-1)] + [t.to(torch.float32) for t in fk['inj']])
    d_tsky = None
    if tys.size and c.ast_sol is not None and c.ast_sol['ok']:
        # the sky positions of the candidates' peaks and, with the fit of P_D, of the fitted positions as X_PSF_D / Y_PSF_D will state
        # them (float32, formed here as catalogs.transient_table does): one more tensor in the same copy back
        t_y32, t_x32 = d_ys.to(torch.int32), d_xs.to(torch.int32)
        parts = [_astrometry_sky(c, ys=t_y32, xs=t_x32)]
        if d_tf is not None:
            pf = torch.stack([t_x32.to(torch.float32) + fit[3], t_y32.to(torch.float32) + fit[2]], dim=1)
            parts.append(_astrometry_sky(c, pos=((pf.to(torch.float64) + 1.0).to(torch.float32).to(torch.float64) - 1.0).contiguous()))
        d_tsky = torch.cat(parts) if all(p is not None for p in parts) else None
    rb = Readback()
    for name, t in (('fe', d_fe), ('stats', d_st), ('flags', d_fl), ('pd', d_tf), ('shapes', d_ts), ('edge', d_edge), ('fake', d_fk),
                    ('sky', d_tsky)):
        if t is not None:
            rb.add(name, t)
    return {name: a[0] for name, a in rb.fetch(ctx).items()}


def _keep_thumbnails(res, keep):
    """the thumbnails of the rows that stay"""
    for k in ('thumbnails', 'thumbnail_png8'):
        if k in res:
            res[k] = res[k][torch.as_tensor(keep, dtype=torch.int64, device=res[k].device)]


def _transient_rows(c, got, fk, tys, txs, tsc):
    """res['transients'] from the host copies of _transient_readback (the columns: transients.py), the rows that leave with their
    thumbnails, the header keys of the fits and of the fake stars"""
    res, hdr_t = c.res, c.hdr_t
    tf, ts = got.get('pd'), got.get('shapes')
    if fk is not None:
        nfk = int(fk['layout']['ys'].size)
        fkh = got['fake']
        fk_rec, fk_host = fkh[:6 * nfk].reshape(nfk, 6), [fkh[(6 + j) * nfk:(7 + j) * nfk] for j in range(3)] + [fkh[9 * nfk:].astype(np.uint8)]
        fk_first = np.zeros(0, np.int32)
    if tys.size:
        rows = res['transients'] = _tr.candidate_rows(tys, txs, tsc, got['fe'])
        if 'sky' in got:
            _tr.sky_columns(rows, got['sky'])
        if 'flags' in got:
            for d, v in zip(rows, got['flags'].tolist()):
                d['flags'] = v
        if fk is not None:
            # the rows that are fake stars: flagged here, so that every drop below carries the flag along with its row
            fk_first = fake_match(rows, fk['layout'], fk['radius'], flags=fk_host[3])
            for d, v in zip(rows, fk_first.tolist()):
                d['fake_star'] = v
        if tf is not None:
            fold = _tr.pd_columns(rows, tf)
            hdr_t.update(trans_fit_header(True, c.fit_size, rows, fold))
            if len(fold) and float(np.max(fold)) > PD_FOLD_WARN:
                logging.getLogger(__name__).warning('P_D leaves %.3g of its |sum| outside its stamp (T-PDFOLD)', float(np.max(fold)))
        if ts is not None:
            _tr.shapefit_columns(rows, ts)
            hdr_t.update(trans_shape_header(True, c.shape_size, settings.trans_moffat_beta, rows))
        if 'edge' in got:
            # candidates without a reference under their peak leave, with their thumbnails; T-NTRANS stays the count before
            kept, keep = _tr.drop_edge_rows(rows, got['edge'])
            if len(keep) < len(rows):
                res['transients'] = kept
                _keep_thumbnails(res, keep)
            hdr_t['T-NOFFR'] = (int(tys.size) - len(keep), 'candidates dropped: no reference there')
        # the vetting: the chi2 bound needs the fit of P_D, the Gauss bounds the shape fits
        kept, keep = _tr.vet_rows(res['transients'], tf is not None, ts is not None, chi2_max=c.trans_chi2_max, fwhm_gauss_min=c.trans_fwhm_gauss_min,
                                  fwhm_gauss_max=c.trans_fwhm_gauss_max, elong_gauss_max=c.trans_elong_gauss_max)
        if keep is not None:
            res['transients'] = kept
            _keep_thumbnails(res, keep)
            hdr_t['T-NVET'] = (len(keep), 'number of transient candidates that passed the vetting')
    else:
        res['transients'] = []
    if fk is not None:
        tab = fake_table(fk['layout'], fk_host, fk_rec, c.nsig, fk_first, [d['fake_star'] for d in res['transients']])
        res['fakestars'] = dict(table=tab, layout=fk['layout'])
        hdr_t.update(fake_header(True, tab, fk['layout'], fk['noise'], fk['radius'], int((fk_first > 0).sum())))


def _closing_headers(c, scal, ms, st, ntrans):
    """the Z- and T- keys that close the two headers, and the result's own entries for them (st: the frame statistics, or None)"""
    res, hdr, hdr_t = c.res, c.hdr, c.hdr_t
    if c.ref_mask_remapped is not None and 'T-NOFFR' not in hdr_t:
        hdr_t['T-NOFFR'] = (0, 'candidates dropped: no reference there')
    hdr['Z-P'] = (True, 'successfully processed by ZOGY?')
    for h in (hdr, hdr_t):
        h['Z-SIZE'] = (c.size, '[pix] size of (square) ZOGY subimages')
        h['Z-BSIZE'] = (c.border, '[pix] size of ZOGY subimage borders')
    if ms is not None:
        hdr_t.update(ms['header'])
    else:
        hdr_t['Z-DX'] = (float(np.median(c.dx)), '[pix] dx median offset full image')
        hdr_t['Z-DY'] = (float(np.median(c.dy)), '[pix] dy median offset full image')
        hdr_t['Z-FNR'] = (float(np.median(c.fratio)), 'median flux ratio (Fnew/Fref) full image')
    if c.frame_stats:
        hdr_t['Z-SCMED'] = (float(st[0, 1]), 'median Scorr full image')
        hdr_t['Z-SCSTD'] = (float(st[0, 3]), 'sigma (STD) Scorr full image')
        hdr_t['Z-FPEMED'] = (float(st[1, 1]), '[e-] median Fpsferr full image')
        hdr_t['Z-FPESTD'] = (float(st[1, 3]), '[e-] sigma (STD) Fpsferr full image')
    hdr_t['T-NSIGMA'] = (float(c.nsig), '[sigma] transient detection threshold')
    hdr_t['T-NTRANS'] = (ntrans, 'number of transient candidates')
    res['header'] = _HeaderView(hdr, hdr_t)
    res['header_new'], res['header_trans'] = hdr, hdr_t
    res['scal'] = scal


class _HeaderView(dict):
    """header_new additions as {KEY: (value, comment)}; item access also finds header_trans
    keys and returns plain values (what the callers of the tensor-level function read)"""

    def __init__(self, hdr, hdr_t):
        dict.__init__(self, hdr)
        self._t = hdr_t

    def __getitem__(self, k):
        v = dict.__getitem__(self, k) if dict.__contains__(self, k) else self._t[k]
        return v[0] if isinstance(v, tuple) else v
