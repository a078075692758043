"""Catalogue products of the subtraction stage: the binary
tables `_red_cat.fits` / `_red_trans.fits` (set_blackbox.py:160-164) and their empty "dummy"
versions for red-flagged images (qc.py:451-503 -> zogy.format_cat).

[EXT] zogy.format_cat is not part of /root/reference; the column names follow the BlackGEM /
MeerLICHT catalogue conventions for the quantities the hot path produces (pixel positions,
PSF-weighted optimal fluxes, ZOGY significance and PSF flux); everything that needs the photometric
calibration or the real-bogus classifier (MAG_*, CLASS_REAL) is out of scope and absent; sky
positions come with the astrometric solution (below).

Thumbnails (settings.save_thumbnails / save_thumbnails_pngs, both off by default): a transient
table that carries them is written with THUMBNAIL_RED, THUMBNAIL_REF, THUMBNAIL_D, THUMBNAIL_SCORR
(qc.py:480-485; 100 x 100 float32 cells, TDIM '(100,100)') and FLAGS_MASK after the six columns
above; save_png_thumbnails writes the reference's {NUMBER}_{RED,REF,D,SCORR}.png files
(blackbox.py:2674-2826) from the display planes the GPU made (zogy.thumbnail_stamps).

Source shapes (settings.cat_shapes, off by default): a 'new' table that carries them is written with FWHM, ELONGATION, A, B,
THETA, X2, Y2, XY and FLAGS_MASK (SHAPE_COLUMNS) after the seven columns above; the dummy catalogue keeps the seven.

Photometry with the PSF on the centroid (settings.phot_centroid, off by default): a 'new' table that carries it is written with
FLAGS_OPT (PHOT_COLUMNS: 1 no centroid, 2 masked pixels left out, 4 no PSF sum) after those.

Aperture photometry (settings.cat_apphot, off by default): a 'new' table that carries it is written with the columns of
aper_columns(table) after those: E_FLUX_APER_R<r>xFWHM / E_FLUXERR_APER_R<r>xFWHM per radius (qc.py:489-502), BKG_APER, BKGSTD_APER,
NSKY_APER, FWHM_APER, FLAGS_APER; the dummy catalogue keeps the seven.

Astrometric solution (settings.astrometry, off by default): a 'new' table of a frame that was solved is written with RA, DEC (float64,
degrees, ICRS) after those, at the very position its X_POS / Y_POS state; a 'trans' table with RA_PEAK, DEC_PEAK at X_PEAK / Y_PEAK and,
where it carries the fit of P_D, RA_PSF_D, DEC_PSF_D at X_PSF_D / Y_PSF_D.  A frame that was not solved, and the dummy catalogues: none.
"""
import os
import shutil
import struct
import zlib

import numpy as np

from . import fitsio

COLUMNS = {
    'new': (('NUMBER', np.int32, ''), ('X_POS', np.float32, 'pix'), ('Y_POS', np.float32, 'pix'),
            ('E_FLUX_PEAK', np.float32, 'e-'), ('E_FLUX_OPT', np.float32, 'e-'), ('E_FLUXERR_OPT', np.float32, 'e-'),
            ('SNR_OPT', np.float32, '')),
    'trans': (('NUMBER', np.int32, ''), ('X_PEAK', np.int32, 'pix'), ('Y_PEAK', np.int32, 'pix'),
              ('SNR_ZOGY', np.float32, ''), ('E_FLUX_ZOGY', np.float32, 'e-'), ('E_FLUXERR_ZOGY', np.float32, 'e-')),
}
COLUMNS['ref'] = COLUMNS['new']
# source shapes (settings.cat_shapes; zogy.optimal_subtraction(shapes=True)): appended to the 'new' columns of a table that carries them
SHAPE_COLUMNS = (('FWHM', np.float32, 'pix'), ('ELONGATION', np.float32, ''), ('A', np.float32, 'pix'), ('B', np.float32, 'pix'),
                 ('THETA', np.float32, 'deg'), ('X2', np.float32, 'pix2'), ('Y2', np.float32, 'pix2'), ('XY', np.float32, 'pix2'),
                 ('FLAGS_MASK', np.uint8, ''))
# photometry with the PSF on the centroid (settings.phot_centroid; zogy.optimal_subtraction(phot_centroid=True)): likewise
PHOT_COLUMNS = (('FLAGS_OPT', np.uint8, ''),)
# the fit of P_D to D at every transient candidate (settings.trans_psffit; zogy.optimal_subtraction(trans_psffit=True)): appended to the
# 'trans' columns of a table that carries them
TRANSFIT_COLUMNS = (('X_PSF_D', np.float32, 'pix'), ('Y_PSF_D', np.float32, 'pix'), ('E_FLUX_PSF_D', np.float32, 'e-'),
                    ('E_FLUXERR_PSF_D', np.float32, 'e-'), ('CHI2_PSF_D', np.float32, ''), ('FLAGS_PSF_D', np.uint8, ''))
# the Gauss and Moffat fits to D at every transient candidate (settings.trans_shapefit; zogy.optimal_subtraction(trans_shapefit=True)):
# appended after TRANSFIT_COLUMNS to the 'trans' columns of a table that carries them
TRANSSHAPE_COLUMNS = tuple((n + '_' + m + '_D', np.uint8 if n == 'FLAGS' else np.float32, '' if n in ('ELONG', 'CHI2', 'FLAGS') else 'pix')
                           for m in ('GAUSS', 'MOFFAT') for n in ('X', 'XERR', 'Y', 'YERR', 'FWHM', 'ELONG', 'CHI2', 'FLAGS'))
# aperture photometry (settings.cat_apphot; zogy.optimal_subtraction(aper_phot=True)): the fixed columns behind the flux / error pair
# of every radius, whose names carry the radius (aper_columns)
APER_COLUMNS = (('BKG_APER', np.float32, 'e-'), ('BKGSTD_APER', np.float32, 'e-'), ('NSKY_APER', np.int32, ''), ('FWHM_APER', np.float32, 'pix'),
                ('FLAGS_APER', np.uint8, ''))
# fake stars (settings.nfakestars; zogy.optimal_subtraction(fake_stars=N)): the star a candidate row belongs to, 0 for a real candidate;
# appended to the 'trans' columns of a table that carries it
FAKE_COLUMNS = (('FAKE_STAR', np.int16, ''),)
# the table of `_trans_fakestars.fits` (fakestars.fake_table)
FAKESTAR_TABLE = (('NUMBER', np.int32, ''), ('X_IN', np.float32, 'pix'), ('Y_IN', np.float32, 'pix'), ('SNR_IN', np.float32, ''),
                  ('SNR_SKY_IN', np.float32, ''), ('E_FLUX_IN', np.float32, 'e-'), ('E_FLUX_REAL', np.float32, 'e-'), ('FLAGS_IN', np.int16, ''),
                  ('X_PEAK', np.float32, 'pix'), ('Y_PEAK', np.float32, 'pix'), ('SCORR_OUT', np.float32, ''), ('E_FLUX_OUT', np.float32, 'e-'),
                  ('E_FLUXERR_OUT', np.float32, 'e-'), ('E_FLUX_OUT_AT', np.float32, 'e-'), ('FOUND', np.int16, ''), ('NUMBER_TRANS', np.int32, ''))
# astrometric solution (settings.astrometry; zogy.optimal_subtraction(astrometry=True)): the sky position at the table's own X_POS /
# Y_POS ('new'), X_PEAK / Y_PEAK and, with TRANSFIT_COLUMNS, X_PSF_D / Y_PSF_D ('trans'), appended to a table that carries them
AST_COLUMNS = (('RA', np.float64, 'deg'), ('DEC', np.float64, 'deg'))
AST_TRANS_COLUMNS = (('RA_PEAK', np.float64, 'deg'), ('DEC_PEAK', np.float64, 'deg'))
AST_TRANSFIT_COLUMNS = (('RA_PSF_D', np.float64, 'deg'), ('DEC_PSF_D', np.float64, 'deg'))
THUMBNAILS = ('RED', 'REF', 'D', 'SCORR')                    # plane order of zogy.thumbnail_stamps; blackbox.py:2701
THUMBNAIL_COLUMNS = tuple('THUMBNAIL_' + c for c in THUMBNAILS)


def aper_columns(table):
    """the aperture columns a table carries, in the order they are written: every E_FLUX_APER_R<r>xFWHM with its E_FLUXERR_ twin in
    the table's own order, then APER_COLUMNS -> ((name, dtype, unit), ...); () for a table without them"""
    if table is None or APER_COLUMNS[-1][0] not in table:
        return ()
    out = []
    for name in table:
        if name.startswith('E_FLUX_APER_R'):
            out += [(name, np.float32, 'e-'), (name.replace('E_FLUX_', 'E_FLUXERR_', 1), np.float32, 'e-')]
    return tuple(out) + APER_COLUMNS


def format_cat(table, cat_output, cat_type='new', header2add=None):
    """zogy.format_cat(cat_in, cat_out, cat_type=, header2add=): write the catalogue of type
    [cat_type] with its fixed column set; table None -> zero rows (dummy catalogue)"""
    if cat_type not in COLUMNS:
        raise ValueError('cat_type {} not in {}'.format(cat_type, sorted(COLUMNS)))
    n = 0 if table is None else len(next(iter(table.values()))) if table else 0
    cols, units = {}, {}
    for name, dt, unit in COLUMNS[cat_type]:
        if table is not None and name in table:
            cols[name] = np.asarray(table[name]).astype(dt)
        elif name == 'NUMBER':
            cols[name] = np.arange(1, n + 1, dtype=dt)
        else:
            cols[name] = np.zeros(n, dtype=dt)
        units[name] = unit
    if cat_type != 'trans' and table is not None and SHAPE_COLUMNS[0][0] in table:
        for name, dt, unit in SHAPE_COLUMNS:
            cols[name] = np.asarray(table[name]).astype(dt)
            units[name] = unit
    if cat_type != 'trans' and table is not None and PHOT_COLUMNS[0][0] in table:
        for name, dt, unit in PHOT_COLUMNS:
            cols[name] = np.asarray(table[name]).astype(dt)
            units[name] = unit
    if cat_type != 'trans':
        for name, dt, unit in aper_columns(table):
            cols[name] = np.asarray(table[name]).astype(dt)
            units[name] = unit
    if cat_type == 'trans' and table is not None and TRANSFIT_COLUMNS[0][0] in table:
        for name, dt, unit in TRANSFIT_COLUMNS:
            cols[name] = np.asarray(table[name]).astype(dt)
            units[name] = unit
    if cat_type == 'trans' and table is not None and TRANSSHAPE_COLUMNS[0][0] in table:
        for name, dt, unit in TRANSSHAPE_COLUMNS:
            cols[name] = np.asarray(table[name]).astype(dt)
            units[name] = unit
    if cat_type == 'trans' and table is not None and FAKE_COLUMNS[0][0] in table:
        for name, dt, unit in FAKE_COLUMNS:
            cols[name] = np.asarray(table[name]).astype(dt)
            units[name] = unit
    for ctype, group in (('new', AST_COLUMNS), ('trans', AST_TRANS_COLUMNS), ('trans', AST_TRANSFIT_COLUMNS)):
        if cat_type == ctype and table is not None and group[0][0] in table:
            for name, dt, unit in group:
                cols[name] = np.asarray(table[name]).astype(dt)
                units[name] = unit
    if cat_type == 'trans' and table is not None and THUMBNAIL_COLUMNS[0] in table:
        for name in THUMBNAIL_COLUMNS:
            cols[name] = np.asarray(table[name]).astype(np.float32)
            units[name] = 'e-' if name != 'THUMBNAIL_SCORR' else ''
        cols['FLAGS_MASK'] = np.asarray(table['FLAGS_MASK']).astype(np.uint8) if 'FLAGS_MASK' in table else np.zeros(n, np.uint8)
        units['FLAGS_MASK'] = ''
    fitsio.write_table(cat_output, cols, header2add, units=units)
    return cat_output


def transient_table(transients, thumbnails=None, fake_star=False):
    """list of dict(y, x, scorr, fpsf, fpsferr[, flags]) (zogy.optimal_subtraction) -> column dict (FITS
    pixel coordinates, 1-based); thumbnails: float32 [n, 4, S, S] (res['thumbnails'] on the host) -> the four
    THUMBNAIL_* columns and FLAGS_MASK as well; fake_star: the table of a frame with fake stars: FAKE_STAR also where it has no row"""
    t = transients or []
    tab = _transient_columns(t)
    if fake_star and 'FAKE_STAR' not in tab:
        tab['FAKE_STAR'] = np.array([d.get('fake_star', 0) for d in t], np.int16)
    if thumbnails is not None:
        th = np.asarray(thumbnails, np.float32)
        if th.ndim != 4 or th.shape[0] != len(t) or th.shape[1] != 4:
            raise ValueError('thumbnails of shape {} for {} transients'.format(th.shape, len(t)))
        for k, name in enumerate(THUMBNAIL_COLUMNS):
            tab[name] = th[:, k]
        tab['FLAGS_MASK'] = np.array([d.get('flags', 0) for d in t], np.uint8)
    return tab


def _transient_columns(t):
    tab = dict(X_PEAK=np.array([d['x'] + 1 for d in t], np.int32), Y_PEAK=np.array([d['y'] + 1 for d in t], np.int32),
               SNR_ZOGY=np.array([d['scorr'] for d in t], np.float32),
               E_FLUX_ZOGY=np.array([d['fpsf'] for d in t], np.float32),
               E_FLUXERR_ZOGY=np.array([d['fpsferr'] for d in t], np.float32))
    if t and all('chi2_psf_d' in d for d in t):
        # the fit of P_D to D (zogy.trans_psffit): sub-pixel FITS coordinates, 1-based
        tab.update(X_PSF_D=np.array([d['x_psf_d'] + 1.0 for d in t], np.float32), Y_PSF_D=np.array([d['y_psf_d'] + 1.0 for d in t], np.float32),
                   E_FLUX_PSF_D=np.array([d['flux_psf_d'] for d in t], np.float32),
                   E_FLUXERR_PSF_D=np.array([d['fluxerr_psf_d'] for d in t], np.float32),
                   CHI2_PSF_D=np.array([d['chi2_psf_d'] for d in t], np.float32), FLAGS_PSF_D=np.array([d['flags_psf_d'] for d in t], np.uint8))
    if t and all('chi2_gauss_d' in d for d in t):
        # the Gauss and Moffat fits to D (zogy.trans_shapefit): sub-pixel FITS coordinates, 1-based
        for name, dt, _ in TRANSSHAPE_COLUMNS:
            key = name.lower()
            tab[name] = np.array([d[key] + 1.0 if name[:2] in ('X_', 'Y_') else d[key] for d in t], dt)
    if t and all('fake_star' in d for d in t):
        tab['FAKE_STAR'] = np.array([d['fake_star'] for d in t], np.int16)
    for group in (AST_TRANS_COLUMNS, AST_TRANSFIT_COLUMNS):
        # the astrometric solution (zogy.optimal_subtraction(astrometry=True)): degrees, float64
        if t and all(group[0][0].lower() in d for d in t):
            for name, dt, _ in group:
                tab[name] = np.array([d[name.lower()] for d in t], dt)
    return tab


def fakestar_cat(table, cat_output, header2add=None):
    """`_trans_fakestars.fits`: the table of fakestars.fake_table with its fixed column set (FAKESTAR_TABLE)"""
    cols = {name: np.asarray(table[name]).astype(dt) for name, dt, _ in FAKESTAR_TABLE}
    fitsio.write_table(cat_output, cols, header2add, units={name: unit for name, _, unit in FAKESTAR_TABLE})
    return cat_output


def _png_gray8(plane):
    """8-bit grayscale PNG file of a uint8 [h, w] array (row 0 on top), with zlib and struct only"""
    plane = np.ascontiguousarray(plane, np.uint8)
    h, w = plane.shape
    raw = np.empty((h, w + 1), np.uint8)
    raw[:, 0] = 0                                             # filter type 0 (None) in front of every scanline
    raw[:, 1:] = plane

    def chunk(tag, body):
        return struct.pack('>I', len(body)) + tag + body + struct.pack('>I', zlib.crc32(tag + body) & 0xffffffff)
    return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 0, 0, 0, 0)) +
            chunk(b'IDAT', zlib.compress(raw.tobytes(), 6)) + chunk(b'IEND', b''))


def save_png_thumbnails(png8, numbers, dir_dest):
    """blackbox.py:2674-2782 for a local destination: {dir_dest}/{NUMBER}_{RED,REF,D,SCORR}.png, one 8-bit grayscale file per
    plane of png8 (uint8 [n, 4, S, S]: res['thumbnail_png8'] on the host, already flipped and scaled like save_thumbs_row's
    arrays).  An existing dir_dest is emptied first, so that two reductions of an image do not mix (2725-2735); zero rows:
    nothing is made, not even the directory (2775-2777).  -> the files written"""
    png8 = np.asarray(png8)
    numbers = np.asarray(numbers).reshape(-1)
    if png8.shape[0] != numbers.size:
        raise ValueError('{} thumbnail rows for {} catalogue numbers'.format(png8.shape[0], numbers.size))
    if numbers.size == 0:
        return []
    if png8.ndim != 4 or png8.shape[1] != len(THUMBNAILS) or png8.dtype != np.uint8:
        raise ValueError('png8 must be uint8 [n, 4, S, S]')
    if os.path.isdir(dir_dest):
        shutil.rmtree(dir_dest)
    os.makedirs(dir_dest)
    written = []
    for row, number in zip(png8, numbers.tolist()):
        for plane, col in zip(row, THUMBNAILS):
            fn = os.path.join(dir_dest, '{}_{}.png'.format(int(number), col))
            with open(fn, 'wb') as f:
                f.write(_png_gray8(plane))
            written.append(fn)
    return written


def write_small_products(jobs):
    """the small files of a frame in one call (a worker process of the host pool runs it for blackbox.py's list run, so
    that their formatting does not hold the interpreter lock of the process that drives the GPU): jobs = [(kind, args)],
    kind in 'image' (fitsio.write_image), 'header' (fitsio.write_header), 'psf' (fitsio.write_psfex: path, model with a host
    basis, header), 'cat' (format_cat), 'trans' (format_cat of
    transient_table(args[0]); an optional fourth argument dict(thumbnails=float32 [n, 4, S, S] or None, png8=uint8 [n, 4, S, S] or
    None, png_dir=[, fake_star=True]) adds the thumbnail columns and / or writes the PNG files of the rows, NUMBER = 1..n; fake_star: the
    FAKE_STAR column even without a row), 'fakestars' (fakestar_cat:
    table, path, header)"""
    done = []
    for kind, args in jobs:
        if kind == 'image':
            fitsio.write_image(*args)
        elif kind == 'header':
            fitsio.write_header(*args)
        elif kind == 'psf':
            fitsio.write_psfex(*args)
        elif kind == 'cat':
            format_cat(args[0], args[1], cat_type=args[2], header2add=args[3])
        elif kind == 'trans':
            extra = args[3] if len(args) > 3 and args[3] else {}
            format_cat(transient_table(args[0], extra.get('thumbnails'), fake_star=bool(extra.get('fake_star'))), args[1], cat_type='trans',
                       header2add=args[2])
            if extra.get('png8') is not None:
                save_png_thumbnails(extra['png8'], np.arange(1, len(args[0] or []) + 1), extra['png_dir'])
        elif kind == 'fakestars':
            fakestar_cat(args[0], args[1], header2add=args[2])
        else:
            raise ValueError('unknown small product {!r}'.format(kind))
        done.append(args[1] if kind in ('cat', 'trans', 'fakestars') else args[0])
    return done
