#!/usr/bin/env python
"""blackbox.py -- per-file entry point of the MI355X reduction, same command line as the
reference's `python blackbox.py --telescope T --img_reduce True --cat_extract True
--trans_extract True --force_reproc_new True --image FILE` (blackbox.py:8128-8213,
blackbox_slurm_google.py:305-309).

FITS in -> `{tel}_{yyyymmdd}_{hhmmss}_red.fits` (float32, e-), `..._mask.fits` (uint8),
`..._red_hdr.fits`, `..._red.log`; with --cat_extract / --trans_extract the products of
zogy.optimal_subtraction that the hot path covers (set_blackbox.py:157-164): `_red_bkg_mini`,
`_red_bkg_std_mini`, `_red_cat` (+ `_red_cat_hdr`), `_red_D`, `_red_Scorr`, `_red_Fpsf`,
`_red_trans` (+ `_red_trans_hdr`), with --objmask True `_red_objmask`, with --limmag True `_red_limmag`.  The reference image, its mask and the PSFs are explicit
inputs (--ref, --ref_mask, --psf_new, --psf_ref), like the masters (--mflat, --mbias, --bpm):
their selection / creation (reference building, PSFEx, astrometry) is orchestration.
`--master_date D --red_dir R --master_dir M` makes the masters of the evening date D (or of a file
of dates) from the reduced bias / dark / flat frames under R (blackbox.py:617-782, create_masters;
blackbox_amd/masters.py): one line per master, its path or None; the exit status is non-zero when
a master failed.  Given --image / --image_list as well, those are reduced afterwards as usual (the
reference stops after the masters).  Flags of the reference that concern orchestration only
(night mode, dates) are accepted and ignored with a warning.  With WORLD_SIZE > 1 (torch.distributed.run) every
rank takes every world-th file of --image_list on its own GPU; an --image_list of object
frames runs through the frames-in-flight pipeline (blackbox_amd.pipeline.FramePipeline).
"""
import argparse
import logging
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

KEYWORDS_VERSION = '1.2.2'      # header keywords version this product follows (blackbox.py:123)
log = logging.getLogger('blackbox')

# BBX_TIMING=1: where the wall time of a `python blackbox.py --image F` process goes (the reference's Slurm contract is one
# interpreter per file, blackbox_slurm_google.py:305-309): seconds since this module was imported at each mark, printed
# as one `BBX_TIMING {json}` line when main() returns
_T0 = time.time()
_MARKS = []
_PIPE_STATS = {}          # --image_list: mean wall time of a frame per pipeline state (BBX_TIMING)
_FILES_DONE = []          # --image_list: the moment every product of a file was on disk (BBX_TIMING: the list's rate)


def _mark(name):
    _MARKS.append((name, time.time() - _T0))


def _start_sampler(path):
    """BBX_CLI_SAMPLE=<file> (debug): every 5 ms the innermost Python frame of every thread; at exit the most frequent
    (thread, function) pairs go to the file -- where the threads of a list run spend their wall time (a thread inside a
    library call that released the interpreter lock shows the calling line; one waiting for the lock shows wherever it
    stopped)"""
    if not path:
        return None
    import atexit
    import collections
    counts = collections.Counter()
    stop = threading.Event()

    def run():
        me = threading.get_ident()
        while not stop.wait(0.005):
            names = {t.ident: t.name for t in threading.enumerate()}
            for tid, fr in sys._current_frames().items():
                if tid == me:
                    continue
                name = names.get(tid, '?').rstrip('0123456789-_ ')
                chain = []
                f = fr
                while f is not None and len(chain) < 3:
                    chain.append('%s:%s:%d' % (os.path.basename(f.f_code.co_filename), f.f_code.co_name, f.f_lineno))
                    f = f.f_back
                counts[(name, ' < '.join(chain))] += 1
    th = threading.Thread(target=run, daemon=True, name='sampler')
    th.start()

    def dump():
        stop.set()
        per = collections.Counter()
        for (name, _), c in counts.items():
            per[name] += c
        with open(path, 'w') as f:
            for name, tot in per.most_common():
                f.write('== %s: %d samples\n' % (name, tot))
                for (n2, where), c in counts.most_common():
                    if n2 == name and c >= 0.02 * tot:
                        f.write('   %5.1f %%  %s\n' % (100.0 * c / tot, where))
    atexit.register(dump)
    return th


def align_keywords(a, S, tel=None):
    """the keywords --ref_align adds to the subtraction's: the switch, and the align_* settings with the command line over them
    (only degrees 1 and 2)"""
    kw = dict(ref_align=True)
    for key, arg in (('align_poldeg', 'align_poldeg'), ('align_max_shift', 'align_max_shift'), ('align_bin', 'align_bin'),
                     ('align_nbright', None), ('align_rounds', None)):
        v = getattr(a, arg, None) if arg else None
        kw[key] = S.get_par(getattr(S, key), tel) if v is None else v
    if kw['align_poldeg'] not in (1, 2):
        raise ValueError('--align_poldeg: degree 1 or 2, got {}'.format(kw['align_poldeg']))
    return kw


def astrometry_keywords(a, S, tel=None):
    """the keywords --astrometry adds to the subtraction's, without the catalogue itself: the switch, and the ast_* settings with the
    command line over them (only degrees 1 and 2, parity +1 or -1).  The pointing is not among them: it is the frame's"""
    kw = dict(astrometry=True)
    for key, arg, name in (('ast_poldeg', 'ast_poldeg', 'ast_poldeg'), ('ast_max_shift', 'ast_max_shift', 'ast_max_shift'),
                           ('ast_bin', 'ast_bin', 'ast_bin'), ('ast_rounds', 'ast_rounds', 'ast_rounds'), ('ast_dist', 'ast_dist', 'ast_dist'),
                           ('ast_rot', 'ast_rot', 'ast_rot'), ('ast_parity', 'ast_parity', 'ast_parity'), ('ast_pixscale', 'ast_pixscale', 'pixscale'),
                           ('ast_mag_zp', 'ast_mag_zp', 'ast_mag_zp')):
        v = getattr(a, arg, None)
        kw[key] = S.get_par(getattr(S, name), tel) if v is None else v
    if kw['ast_dist'] is None:
        kw['ast_dist'] = S.get_par(S.match_dist_pix, tel)
    if kw['ast_poldeg'] not in (1, 2):
        raise ValueError('--ast_poldeg: degree 1 or 2, got {}'.format(kw['ast_poldeg']))
    if kw['ast_parity'] not in (1, -1):
        raise ValueError('--ast_parity: +1 or -1, got {}'.format(kw['ast_parity']))
    return kw


def name_list(v):
    """'RA,DEC,MAG' -> ('RA', 'DEC', 'MAG')"""
    out = tuple(t.strip() for t in str(v).split(',') if t.strip())
    if len(out) != 3:
        raise argparse.ArgumentTypeError('three comma separated column names expected, got %r' % (v,))
    return out


def float_list(v):
    """'0.66,1.5,5' -> (0.66, 1.5, 5.0)"""
    try:
        out = tuple(float(t) for t in str(v).split(',') if t.strip())
    except ValueError:
        raise argparse.ArgumentTypeError('a comma list of numbers expected, got %r' % (v,))
    if not out:
        raise argparse.ArgumentTypeError('a comma list of numbers expected, got %r' % (v,))
    return out


def str2bool(v):
    """blackbox.py:8115-8123"""
    if isinstance(v, bool):
        return v
    if v.lower() in ('yes', 'true', 't', 'y', '1'):
        return True
    if v.lower() in ('no', 'false', 'f', 'n', '0'):
        return False
    raise argparse.ArgumentTypeError('Boolean value expected.')


class WrapException(Exception):
    """the exception of a worker with its formatted traceback, so that a multiprocessing pool can hand it to
    the parent (what blackbox.py:933-943 is for): raised by try_blackbox_reduce in place of whatever
    blackbox_reduce raised"""

    def __init__(self):
        import traceback
        exc_type, exc_value, exc_tb = sys.exc_info()
        Exception.__init__(self, repr(exc_value))
        self.exception = exc_value
        self.formatted = ''.join(traceback.format_exception(exc_type, exc_value, exc_tb))

    def __reduce__(self):                                          # crosses the pool as text
        return (_rebuild_wrapexception, (self.args, self.formatted))

    def __str__(self):
        return '{}\nOriginal traceback:\n{}'.format(Exception.__str__(self), self.formatted)


def _rebuild_wrapexception(args, formatted):
    e = WrapException.__new__(WrapException)
    Exception.__init__(e, *args)
    e.exception, e.formatted = None, formatted
    return e


# ---- operator-level entry the reference's farm imports (blackbox.py:363-379: `pool_func(try_blackbox_reduce,
# filenames, nproc)`): module-level functions of one argument.  The settings the reference keeps in module globals
# set by run_blackbox (tel, filts, types, proc_mode; blackbox.py:141, 321-323) are the parsed command line here:
# configure() stores it in this process and in the environment, so that spawned pool workers -- which import this
# module afresh and must create their GPU context themselves -- find it.
_ENV_KEY = 'BBX_BLACKBOX_ARGV'
_STATE = {'argv': None, 'reducer': None, 'exit_status': 0}


def configure(argv):
    """set the per-process settings (the command-line flags of main(), as a list of strings) for blackbox_reduce /
    try_blackbox_reduce; inherited by pool workers through the environment.  Makes no GPU call."""
    import json
    _STATE['argv'] = list(argv)
    _STATE['reducer'] = None
    os.environ[_ENV_KEY] = json.dumps(_STATE['argv'])


def _reducer(filename=None):
    """this process's Reducer (GPU context + masters resident in HBM), created at the first frame"""
    if _STATE['reducer'] is None:
        if _STATE['argv'] is None:
            import json
            if _ENV_KEY not in os.environ:
                raise RuntimeError('blackbox.configure(argv) has not been called (and %s is not set)' % _ENV_KEY)
            _STATE['argv'] = json.loads(os.environ[_ENV_KEY])
        args = build_parser().parse_args(_STATE['argv'])
        _STATE['reducer'] = Reducer(telescope_of(args, filename), args)
    return _STATE['reducer']


def blackbox_reduce(filename):
    """blackbox.py:1027-2669 for one file: -> path of the reduced image, or None if it was skipped"""
    return _reducer(filename).blackbox_reduce(filename)


def try_blackbox_reduce(filename):
    """blackbox.py:948-999: blackbox_reduce in a try / except that re-raises as WrapException (formatted traceback
    for the parent of a multiprocessing pool); the per-image log is closed in blackbox_reduce's own finally"""
    try:
        return blackbox_reduce(filename)
    except BaseException:
        raise WrapException()


def pool_func(func, filelist, nproc=1):
    """blackbox.py:363-379 / zogy.pool_func: map [func] over the files with [nproc] worker processes.  Workers
    are SPAWNED (a forked child cannot use a GPU runtime its parent initialised) and each creates its own GPU
    context at its first file; the parent makes no GPU call.  WORLD_SIZE / LOCAL_RANK are not needed: worker k
    takes GPU k modulo the number of visible devices."""
    import multiprocessing as mp
    if nproc <= 1:
        return [func(f) for f in filelist]
    with mp.get_context('spawn').Pool(nproc, initializer=_pool_worker_init, initargs=(os.environ.get(_ENV_KEY),)) as pool:
        return pool.map(func, filelist, chunksize=1)


def _pool_worker_init(argv_json):
    import multiprocessing as mp
    if argv_json is not None:
        os.environ[_ENV_KEY] = argv_json
    ident = mp.current_process()._identity
    import torch
    ndev = max(1, torch.cuda.device_count())                      # counting devices does not initialise the GPU
    os.environ['LOCAL_RANK'] = str(((ident[0] - 1) if ident else 0) % ndev)
    os.environ['RANK'], os.environ['WORLD_SIZE'] = '0', '1'      # the pool hands out the files; no sharding inside a worker


def telescope_of(args, filename=None):
    """telescope from the file name prefix, else --telescope (blackbox.py:145-152)"""
    tel = args.telescope
    if filename:
        base = os.path.basename(filename)
        for t in ('ML1', 'BG2', 'BG3', 'BG4'):
            if base.startswith(t):
                tel = t
    return tel


def outname(header, tel, red_dir):
    """{tel}_{yyyymmdd}_{hhmmss}_red.fits from DATE-OBS (blackbox.py:1004-1022, 1166-1184)"""
    date_obs = str(_hval(header, 'DATE-OBS', time.strftime('%Y-%m-%dT%H:%M:%S')))
    d, t = date_obs.split('T')[0].replace('-', ''), date_obs.split('T')[-1].split('.')[0].replace(':', '')
    return os.path.join(red_dir, '{}_{}_{}_red.fits'.format(tel, d, t))


def _base(p):
    return os.path.basename(p) if p else 'None'


def _stem(p):
    return os.path.basename(p).split('.fits')[0] if p else 'None'


def _frame_header(h):
    """the header of a raw frame as a dict, without the keywords that describe its stored pixels"""
    header = dict(h)
    for k in ('BZERO', 'BSCALE', 'BITPIX', 'NAXIS', 'NAXIS1', 'NAXIS2', 'SIMPLE', 'EXTEND'):
        header.pop(k, None)
    return header


def _hval(header, key, default):
    from blackbox_amd.reduce import hval
    return hval(header, key) if key in header else default


def imgtype_of(header):
    return str(_hval(header, 'IMAGETYP', 'object')).lower()


def exptime_of(header):
    return _hval(header, 'EXPTIME', 1.0)


class _Products:
    """where the products of one frame go.  Direct (staged=None): each is written at once.  Staged (a frame of the list run
    whose images [staged] the output stage is writing, compressed on its lane): such an image only hands its header over;
    the small products (mini image, table, header file) are noted for one catalogs.write_small_products in a worker process"""

    def __init__(self, reducer, staged=None):
        self.reducer, self.staged = reducer, None if staged is None else set(staged)
        self.headers, self.deferred = {}, []          # staged name -> its header (the names the frame keeps); [(kind, args)]

    def stages(self, path):
        return self.staged is not None and (path + '.fz') in self.staged

    def image(self, path, img, header):
        if not self.stages(path):
            return self.reducer.write_image(path, img, header)
        # the output stage is writing this image already: it only waits for the header
        self.headers[path + '.fz'] = dict(header)
        return path + '.fz'

    def small(self, kind, *args):
        if self.staged is not None:
            return self.deferred.append((kind, args))
        from blackbox_amd import catalogs
        catalogs.write_small_products([(kind, args)])


class Reducer:
    """per-process state: GPU context + masters / reference / PSFs resident in HBM"""

    def __init__(self, tel, args):
        _mark('main_start')
        import torch
        _mark('torch_imported')
        from blackbox_amd import fitsio, reduce as R
        _mark('package_imported')
        self.R, self.torch, self.fitsio = R, torch, fitsio
        _, _, local = __import__('blackbox_amd.farm', fromlist=['rank_world']).rank_world()
        if os.environ.get('BBX_ONE_GPU'):                          # rehearsal of a multi-rank run on a one-GPU box: every rank on device 0
            local = 0
        self.ctx = R.Context(local)
        _mark('gpu_context')
        self.tel = tel
        self.args = args

        def load(path, dtype, what):
            """a master that cannot be read is not applied: <X>-P False (blackbox.py:1674-1699, 1820-1846)"""
            if not path:
                return None
            try:
                return R.image_to_device(self.ctx, path, dtype)      # (float32 files: bytes up, swapped on the device)
            except Exception:
                log.exception('exception was raised while reading the %s %s', what, path)
                return None
        self.mflat = load(args.mflat, np.float32, 'master flat')
        self.mbias = load(args.mbias, np.float32, 'master bias')
        self.bpm = load(args.bpm, np.uint8, 'bad pixel mask')
        if self.bpm is not None and bool((self.bpm & 12).any()):
            raise ValueError('bad-pixel mask carries saturated(4)/saturated-connected(8) bits; expected 1 and 32 only')
        self.xtalk = None
        if args.crosstalk:
            try:
                self.xtalk = R.read_crosstalk(args.crosstalk)
            except Exception:
                log.exception('exception was raised while reading the crosstalk file %s', args.crosstalk)
        self.nonlin = None
        if args.nonlin:
            try:
                self.nonlin = R.read_nonlin_splines(args.nonlin)
            except Exception:
                log.exception('exception was raised while reading the non-linearity splines %s', args.nonlin)
        # inputs of the subtraction stage
        self.sub = None
        from blackbox_amd import settings as _S
        if args.cat_extract or args.trans_extract or (_S.get_par(_S.limmag, tel) if args.limmag is None else args.limmag) or \
                (_S.get_par(_S.astrometry, tel) if args.astrometry is None else args.astrometry):
            self.sub = self._load_subtraction_inputs(load)
        _mark('calibration_and_reference_files_in_hbm')

    def _load_psf(self, path):
        """PSF input: a PSFEx .psf table (model evaluated on the GPU) or a FITS image / cube of
        unit-sum stamps ([S, S] or [nsub, S, S])"""
        if not path:
            return None
        torch, fitsio = self.torch, self.fitsio
        try:
            if path.endswith('.psf') or path.endswith('_psf.fits'):
                m = fitsio.read_psfex(path)
                if m['psf_samp'] != 1.0:
                    # the model is tabulated every PSF_SAMP pixels: bring the basis to image pixels (zogy.get_psf_ima)
                    from blackbox_amd import zogy as G
                    if not (0.05 <= m['psf_samp'] <= 20.0):
                        raise ValueError('PSF_SAMP {} out of range'.format(m['psf_samp']))
                    m['basis'] = G.resample_psf_basis(m['basis'], m['psf_samp'])
                    log.info('PSF model resampled from PSF_SAMP %.3f to image pixels: %d x %d', m['psf_samp'], *m['basis'].shape[1:])
                m['basis'] = torch.from_numpy(np.ascontiguousarray(m['basis'])).to(self.ctx.device)
                return m
            st = np.ascontiguousarray(fitsio.read_image(path, dtype=np.float32))
            st = st / st.sum(axis=(-2, -1), keepdims=True)
            return torch.from_numpy(st).to(self.ctx.device)
        except Exception:
            log.exception('exception was raised while reading the PSF %s', path)
            return None

    def _load_subtraction_inputs(self, load):
        a = self.args
        sub = dict(psf_new=self._load_psf(a.psf_new), psf_ref=None, ref=None, ref_mask=None,
                   cat_extract=bool(a.cat_extract), trans_extract=bool(a.trans_extract),
                   fratio=a.fratio, dx=a.zogy_dx, dy=a.zogy_dy, ref_is_bkgsub=bool(a.ref_bkgsub))
        from blackbox_amd import settings as S

        def par(value, name):
            return S.get_par(getattr(S, name), self.tel) if value is None else value
        # the PSF model from the frame's own stars where no PSF file is given; the keywords are only passed when switched on
        psf_build = bool(par(a.psf_build, 'psf_build'))
        if psf_build:
            sub['psf_build'] = True
            if a.psf_size is not None:
                sub['psf_size'] = a.psf_size
            if a.psf_poldeg is not None:
                sub['psf_poldeg'] = a.psf_poldeg
        if a.subimage_size:
            sub['subimage_size'] = a.subimage_size
        if a.subimage_border is not None:
            sub['subimage_border'] = a.subimage_border
        if a.bkg_boxsize:
            sub['bkg_boxsize'] = a.bkg_boxsize
        if a.trans_extract and a.ref:
            sub['ref'] = load(a.ref, np.float32, 'reference image')
            sub['ref_mask'] = load(a.ref_mask, np.uint8, 'reference mask') if a.ref_mask else None
            if sub['ref'] is not None and sub['ref_mask'] is None:
                sub['ref_mask'] = self.torch.zeros(sub['ref'].shape, dtype=self.torch.uint8, device=self.ctx.device)
            sub['psf_ref'] = self._load_psf(a.psf_ref)
            if a.ref_bkg_std_mini:
                sub['ref_bkg_std_mini'] = self.fitsio.read_image(a.ref_bkg_std_mini, dtype=np.float32)
            if psf_build and sub['ref'] is not None and sub['psf_ref'] is None and not a.psf_ref:
                # the reference's model from its own stars, once per run
                sub['psf_ref'] = self._build_ref_psf(sub)
            if sub['ref'] is None or sub['psf_ref'] is None or (sub['psf_new'] is None and not psf_build):
                log.error('reference image or PSFs missing: processing the new image only')
                sub['ref'] = None
        elif a.trans_extract:
            log.info('no reference image given: processing the new image only, without comparison to a reference '
                     '(blackbox.py:2338-2354)')
        # thumbnails of the transient candidates: command line over settings; the keywords are only passed when switched on
        self.thumbnails_dir = par(a.thumbnails_dir, 'thumbnails_dir')
        if sub['cat_extract'] and par(a.cat_shapes, 'cat_shapes'):
            # source shapes of the catalogue and the frame's seeing / elongation keys; the keyword is only passed when switched on
            sub['shapes'] = True
        if sub['cat_extract'] and par(a.cat_apphot, 'cat_apphot'):
            # aperture fluxes with a local sky annulus in the catalogue and the AP-* keys; the keywords are only passed when switched on
            sub['aper_phot'] = True
            if a.apphot_radii is not None:
                sub['apphot_radii'] = a.apphot_radii
            if a.apphot_local_sky is not None:
                sub['apphot_local_sky'] = a.apphot_local_sky
        if par(a.limmag, 'limmag'):
            # the limiting-flux image of the reduced frame and the LIM* keys; the keywords are only passed when switched on
            sub['limmag'] = True
            from blackbox_amd import limflux
            limflux.check_parameters(a.limmag_nsigma, a.limmag_psf_frac)      # (a ValueError here, not a frame without its image later)
            if a.limmag_nsigma is not None:
                sub['limmag_nsigma'] = a.limmag_nsigma
            if a.limmag_psf_frac is not None:
                sub['limmag_psf_frac'] = a.limmag_psf_frac
        if par(a.astrometry, 'astrometry'):
            # the astrometric solution of every frame against one catalogue, read once per run; the keywords are only passed when
            # switched on.  No catalogue, a missing column, too many rows: an error here, before any frame runs
            from blackbox_amd import astrometry
            path = par(a.ast_cat, 'ast_cat')
            if not path:
                raise ValueError('--astrometry True needs --ast_cat (or settings.ast_cat)')
            sub.update(astrometry_keywords(a, S, self.tel))
            sub['ast_catalog'] = astrometry.load_catalog(self.ctx, path, par(a.ast_cat_cols, 'ast_cat_cols'))
            log.info('astrometric catalogue %s: %d rows', path, sub['ast_catalog'].n)
        if par(a.objmask, 'objmask'):
            # object mask + second background pass, whenever the subtraction stage runs; the keywords are only passed when switched on
            sub['objmask'] = True
            for k in ('objmask_nsigma', 'objmask_minarea', 'objmask_grow'):
                if getattr(a, k) is not None:
                    sub[k] = getattr(a, k)
        if sub['ref'] is not None:
            if par(a.save_thumbnails, 'save_thumbnails'):
                sub['thumbnails'] = True
            if par(a.save_thumbnails_pngs, 'save_thumbnails_pngs'):
                sub['thumbnail_pngs'] = True
            # fratio, dx, dy measured from the stars matched with the reference instead of --fratio --zogy_dx --zogy_dy,
            # which stay the fallback of a frame with too few pairs
            if par(a.zogy_match, 'zogy_match'):
                sub['match'] = True
                sub['match_dist'] = par(a.match_dist, 'match_dist_pix')
            # the reference registered on the new frame from the stars of both; the keywords are only passed when switched on
            if par(a.ref_align, 'ref_align'):
                sub.update(align_keywords(a, S, self.tel))
            # the PSF of D fitted to every transient candidate; the keywords are only passed when switched on
            if par(a.trans_psffit, 'trans_psffit'):
                sub['trans_psffit'] = True
                if a.trans_fit_size is not None:
                    sub['trans_fit_size'] = a.trans_fit_size
                chi2_max = par(a.trans_chi2_max, 'trans_chi2_max')
                if chi2_max is not None:
                    sub['trans_chi2_max'] = chi2_max
            # fake stars planted in the frame that is subtracted and read back from Scorr / Fpsf; the keywords are only passed when switched on
            nfake = par(a.fake_stars, 'nfakestars')
            if nfake and int(nfake) > 0:
                from blackbox_amd import fakestars
                sub['fake_stars'] = int(nfake)
                sub['fake_s2n'] = fakestars.fake_s2n_list(par(a.fake_s2n, 'fakestar_s2n'))       # (a ValueError here, not a frame without its stars later)
                for k in ('fake_seed', 'fake_noise', 'fake_radius', 'fake_clear_nsigma'):
                    if getattr(a, k) is not None:
                        sub[k] = getattr(a, k)
            # a Gauss and a Moffat fitted to every transient candidate, with or without the fit of P_D; likewise
            if par(a.trans_shapefit, 'trans_shapefit'):
                sub['trans_shapefit'] = True
                if a.trans_shape_size is not None:
                    sub['trans_shape_size'] = a.trans_shape_size
                for k in ('trans_fwhm_gauss_min', 'trans_fwhm_gauss_max', 'trans_elong_gauss_max'):
                    if par(getattr(a, k), k) is not None:
                        sub[k] = par(getattr(a, k), k)
        if (sub['cat_extract'] or sub.get('match')) and par(a.phot_centroid, 'phot_centroid'):
            # the PSF on the centroids wherever photometry runs (the catalogue, the star match's two lists); the keyword is only
            # passed when switched on
            sub['phot_centroid'] = True
        return sub

    def _build_ref_psf(self, sub):
        """the reference's PSF model from its own stars (zogy.build_psf): the reference is background-subtracted here unless
        --ref_bkgsub, its sigma is --ref_bkg_std_mini or measured; None where the build fails"""
        from blackbox_amd import zogy as G, settings as S
        try:
            ref = sub['ref']
            ny, nx = ref.shape
            size, box = sub.get('subimage_size') or S.subimage_size, sub.get('bkg_boxsize') or S.bkg_boxsize
            mini, mini_std = G.get_back(self.ctx, ref, sub['ref_mask'], bkg_boxsize=box)
            work = ref
            if not sub['ref_is_bkgsub']:
                work = self.torch.empty_like(ref)
                G.mini2back(self.ctx, mini, (ny, nx), bkg_boxsize=box, interp_Xchan=True, subtract_from=ref, subtract_into=work)
            sdr = sub.get('ref_bkg_std_mini')
            sdr = mini_std.cpu().numpy() if sdr is None else np.asarray(sdr, np.float32)
            built = G.build_psf(self.ctx, work, sdr, sub['ref_mask'], size, ny // size, nx // size, sigma_median=float(np.median(sdr)),
                                psf_size=sub.get('psf_size'), poldeg=sub.get('psf_poldeg'))
            log.info('PSF model of the reference: %s', {k: v[0] for k, v in built['header'].items()})
            return built['model']
        except Exception:
            log.exception('exception was raised while building the PSF model of the reference')
            return None

    def _thumbnail_products(self, res, base):
        """what the transient table's writer needs for the thumbnails of a frame, on the host: the float cut-outs only when
        they become columns, the uint8 display planes only when PNG files are made; None when neither is switched on"""
        def host(name):
            t = res.get(name + '_host', res.get(name))           # (the list run has copied them on the frame's lane already)
            if t is None:
                return None
            return t.cpu().numpy() if self.torch.is_tensor(t) else np.asarray(t)
        th, png = host('thumbnails'), host('thumbnail_png8')
        if th is None and png is None:
            return None
        name = os.path.basename(base)
        name = name[:-len('_red')] if name.endswith('_red') else name
        root = self.thumbnails_dir or os.path.join(os.path.dirname(base), 'thumbnails')
        return dict(thumbnails=th, png8=png, png_dir=os.path.join(root, name))

    # ------------------------------------------------------------------------------------
    def try_blackbox_reduce(self, filename):
        """blackbox.py:948-999: the reduced file name or None (skipped); raises WrapException with the formatted
        traceback when blackbox_reduce raised"""
        try:
            return self.blackbox_reduce(filename)
        except BaseException:
            raise WrapException()

    def reduce_logged(self, filename):
        """what the reference's single-process loop amounts to for the caller of main(): a failing file is logged
        with its traceback and reported as None, the run goes on"""
        try:
            return self.try_blackbox_reduce(filename)
        except WrapException as e:
            log.error('exception was raised during [blackbox_reduce] of %s:\n%s', filename, e.formatted)
            return None

    def read_raw(self, filename):
        """-> (raw device tensor, header dict)"""
        torch, fitsio = self.torch, self.fitsio
        if filename.endswith('.fz'):
            # fpacked raw frame (the reference's usual input): the compressed bytes go to the GPU
            # and are decoded there
            from blackbox_amd import fpack as P
            d_raw, hraw = P.funpack_image(self.ctx, filename)
            if d_raw.dtype not in (torch.uint16, torch.float32):
                d_raw = d_raw.to(torch.float32)
        else:
            raw, hraw = fitsio.read_image(filename, get_header=True)
            if raw.dtype not in (np.uint16, np.float32):
                raw = raw.astype(np.float32)
            d_raw = torch.from_numpy(np.ascontiguousarray(raw)).to(self.ctx.device)
        return d_raw, _frame_header(hraw)

    def names(self, header):
        red_dir = self.args.red_dir or '.'
        fits_out = outname(header, self.tel, red_dir)
        return red_dir, fits_out

    def already_done(self, fits_out):
        return os.path.isfile(fits_out) and os.path.isfile(fits_out.replace('_red', '_mask')) \
            and not (self.args.img_reduce and self.args.force_reproc_new)

    def blackbox_reduce(self, filename):
        R = self.R
        t0 = time.time()
        d_raw, header = self.read_raw(filename)
        _mark('raw_read')
        if not self.args.red_dir:
            self.args.red_dir = os.path.dirname(os.path.abspath(filename))
        red_dir, fits_out = self.names(header)
        if self.already_done(fits_out):
            log.info('%s already reduced; skipping', filename)           # blackbox.py:1336-1390
            return fits_out
        os.makedirs(red_dir, exist_ok=True)
        fh = self.open_image_log(fits_out)
        try:
            exptime, imgtype = exptime_of(header), imgtype_of(header)
            data, mask, header, hm = R.reduce_object(
                self.ctx, d_raw, header, self.tel, mflat=self.mflat, mbias=self.mbias, bpm=self.bpm,
                xtalk_coeffs=self.xtalk, exptime=exptime, ysize_chan=self.args.ysize_chan,
                xsize_chan=self.args.xsize_chan, nonlin_splines=self.nonlin, imgtype=imgtype, log=log)
            _mark('reduced')
            if imgtype != 'object':
                return self.finish_calibration_frame(data, mask, header, imgtype, fits_out)
            return self.finish_object(filename, data, mask, header, hm, fits_out, t0, _Products(self))
        finally:
            self.close_image_log(fh)

    # ---- per-image log (blackbox.py:1311-1318: {base}_red.log next to the product) ----------
    def open_image_log(self, fits_out):
        try:
            fh = logging.FileHandler(fits_out.replace('.fits', '.log'), mode='w')
            fh.setFormatter(logging.Formatter('%(asctime)s [%(levelname)s, %(process)s] %(message)s'))
            log.addHandler(fh)
            return fh
        except OSError:
            return None

    def close_image_log(self, fh):
        if fh is not None:
            log.removeHandler(fh)
            fh.close()

    # ---- bias / dark / flat frames -------------------------------------------------------------
    def finish_calibration_frame(self, data, mask, header, imgtype, fits_out):
        """blackbox.py:1627-1637 (bias), 1764-1784 (flat): statistics, QC flags, write the frame
        (no mask product)"""
        R, fitsio = self.R, self.fitsio
        from blackbox_amd import qc
        header['BUNIT'] = ('e-', 'pixel values are in electrons')
        if imgtype == 'flat' and R.hval(header, 'OS-P'):
            from blackbox_amd import flatstats
            flatstats.get_flatstats(self.ctx, data, header, mask, self.tel, statsec=self.args.flat_norm_sec,
                                    ysize_chan=self.args.ysize_chan, xsize_chan=self.args.xsize_chan)
        self.bookkeeping(header, time.time())
        qc.run_qc_check(header, self.tel)
        fits_out = fits_out.replace('_red.fits', '.fits')       # calibration frames keep their plain name
        fitsio.write_image(fits_out, data.cpu().numpy(), header)
        return fits_out

    def bookkeeping(self, header, t0):
        """bookkeeping keywords of the header contract (blackbox.py:1110-1112, 1520, 1607, 1669-1690,
        1817-1855; verify_header 2893-3255)"""
        R = self.R
        from blackbox_amd import __version__ as bbx_version
        a = self.args
        header['BB-V'] = ('amd-' + bbx_version, 'BlackBOX version used')
        header['KW-V'] = (KEYWORDS_VERSION, 'header keywords version used')
        header['BB-START'] = (time.strftime('%Y-%m-%dT%H:%M:%S', time.gmtime(t0)), 'start UTC date of BlackBOX image run')
        header['XTALK-F'] = (_base(a.crosstalk), 'name crosstalk coefficients file')
        header.setdefault('GAIN', (1.0, '[e-/ADU] effective gain all channels'))
        header.setdefault('GAIN-P', (True, 'corrected for gain?'))
        header.setdefault('NONLIN-P', (False, 'corrected for non-linearity?'))
        header['NONLIN-F'] = (_base(a.nonlin) if R.hval(header, 'NONLIN-P') else 'None', 'name non-linearity correction file')
        header['MBIAS-F'] = (_stem(a.mbias) if header.get('MBIAS-P') and R.hval(header, 'MBIAS-P') else 'None',
                             'name of master bias applied')
        header['MFLAT-F'] = (_stem(a.mflat) if header.get('MFLAT-P') and R.hval(header, 'MFLAT-P') else 'None',
                             'name of master flat applied')
        for k, c in (('XTALK-P', 'corrected for crosstalk?'), ('COSMIC-P', 'corrected for cosmic rays?'),
                     ('SAT-P', 'processed for satellite trails?'), ('MBIAS-P', 'corrected for master bias?'),
                     ('MFLAT-P', 'corrected for master flat?'), ('MASK-P', 'mask image created?')):
            header.setdefault(k, (False, c))                                     # steps that did not run
        header.setdefault('NCOSMICS', ('None', '[/s] number of cosmic rays identified'))
        header.setdefault('NSATS', ('None', 'number of satellite trails identified'))
        header['MFRING-P'] = (False, 'corrected for master fringe map?')
        header['MFRING-F'] = ('None', 'name of master fringe map applied')
        header['FRRATIO'] = ('None', 'fringe ratio (science/fringe map) applied')

    # ---- object frames -------------------------------------------------------------------------
    def finish_object(self, filename, data, mask, header, hm, fits_out, t0, products, sub_result=None):
        R, fitsio = self.R, self.fitsio
        from blackbox_amd import qc
        header['BUNIT'] = ('e-', 'pixel values are in electrons')
        self.bookkeeping(header, t0)
        redfile = os.path.basename(fits_out).split('.fits')[0]
        header['REDFILE'] = (redfile, 'BlackBOX reduced image name')
        header['MASKFILE'] = (redfile.replace('_red', '_mask'), 'BlackBOX mask image name')
        # QC flags on the reduction keywords (blackbox.py:2000; qc.py)
        qc_flag = qc.run_qc_check(header, self.tel, check_key_type='full')      # flags go into the image header
        qc.verify_header(header, ['full'], name=fits_out)                     # blackbox.py:2062 (raises on a DB keyword)
        base = fits_out.replace('.fits', '')
        if qc_flag == 'red':
            # red flag: dummy catalogues, no subtraction (blackbox.py:2015-2046)
            log.error('red QC flag in image %s; making dummy catalogs and returning', fits_out)
            written = products.image(fits_out, data, header)
            products.image(fits_out.replace('_red', '_mask'), mask, hm)
            fitsio.write_header(base + '_hdr.fits', header)
            if self.sub is not None:
                qc.run_qc_check(header, self.tel, cat_type='new', cat_dummy=base + '_cat.fits', check_key_type='full')
                htrans = dict(header)
                qc.run_qc_check(htrans, self.tel, cat_type='trans', cat_dummy=base + '_trans.fits', check_key_type='trans')
            return written
        if self.sub is not None:
            self.subtract_and_write(data, mask, header, base, products, sub_result)
        written = products.image(fits_out, data, header)
        products.image(fits_out.replace('_red', '_mask'), mask, hm)
        products.small('header', base + '_hdr.fits', dict(header))              # update_imcathead(create_hdrfile=True), 2011
        log.info('reduced %s -> %s in %.2f s', filename, written, time.time() - t0)
        _mark('products_written')
        return written

    def write_image(self, path, img, header):
        if self.args.fpack and self.torch.is_tensor(img):
            # products leave the GPU tile-compressed (reference: fpack of the files kept,
            # copy_files2keep 4033-4035): only the compressed bytes cross PCIe
            from blackbox_amd import fpack as P
            P.fpack_image(self.ctx, path, img, header)
            return path + '.fz'
        self.fitsio.write_image(path, img.cpu().numpy() if self.torch.is_tensor(img) else img, header)
        return path

    def subtract_and_write(self, data, mask, header, base, products, res=None):
        """zogy.optimal_subtraction + the products it leaves (set_blackbox.py:157-164); a failure
        keeps the reduction products (blackbox.py:2364-2382)"""
        from blackbox_amd import zogy as G, qc
        try:
            if res is None:
                kw = {k: v for k, v in self.sub.items() if k not in ('ref', 'ref_mask', 'psf_new', 'psf_ref')}
                if self.sub.get('astrometry'):
                    # the pointing is the frame's own: its header's RA, DEC, with --ast_ra --ast_dec over them
                    from blackbox_amd import astrometry
                    kw['ast_pointing'] = astrometry.frame_pointing(header, self.args.ast_ra, self.args.ast_dec)
                res = G.optimal_subtraction(self.ctx, data, self.sub['ref'], mask, self.sub['ref_mask'],
                                            self.sub['psf_new'], self.sub['psf_ref'], **kw)
                self.ctx.sync()
                _mark('subtracted')
        except Exception:
            log.exception('exception was raised during [optimal_subtraction]; saving just the image reduction products')
            header['Z-P'] = (False, 'successfully processed by ZOGY?')
            return
        hnew, htrans = res['header_new'], res['header_trans']
        header.update(hnew)
        self.write_red_limmag(base, res, header, products)
        bkg_hdr = {'BKG-SIZE': hnew['BKG-SIZE']}
        products.small('image', base + '_bkg_mini.fits', np.asarray(res['bkg_mini_new']), bkg_hdr)
        products.small('image', base + '_bkg_std_mini.fits', np.asarray(res['bkg_std_mini_new']), bkg_hdr)
        qc_flag = qc.run_qc_check(header, self.tel, check_key_type='full')
        if res.get('objmask') is not None:
            # the object mask the second background pass left out (set_blackbox.py:157), written as `_mask.fits` is
            products.image(base + '_objmask.fits', res['objmask'], {k: v for k, v in hnew.items() if k.startswith(('OBJM-', 'BKG-SIZE'))})
        if res.get('psf') is not None and res['psf']['model'] is not None:
            # the model built from the frame's own stars, in PSFEx's form: --psf_new takes it
            m = res['psf']['model']
            m = dict(m, basis=m['basis'].cpu().numpy() if self.torch.is_tensor(m['basis']) else np.asarray(m['basis']))
            products.small('psf', base + '_psf.fits', m, {k: v for k, v in hnew.items() if k.startswith('PSF-')})
        if res.get('catalog') is not None:
            if qc_flag == 'red':
                qc.run_qc_check(header, self.tel, cat_type='new', cat_dummy=base + '_cat.fits', check_key_type='full')
            else:
                products.small('cat', res['catalog'], base + '_cat.fits', 'new', dict(header))
            products.small('header', base + '_cat_hdr.fits', dict(header))
        if res.get('D') is not None:
            full_t = dict(header)
            full_t.update(htrans)
            tqc = qc.run_qc_check(full_t, self.tel, check_key_type='trans')
            for ext in ('D', 'Scorr', 'Fpsf'):
                products.image('{}_{}.fits'.format(base, ext), res[ext], full_t)
            self.write_limmag(base, res, full_t, products)
            if tqc == 'red' or qc_flag == 'red':
                qc.run_qc_check(full_t, self.tel, cat_type='trans', cat_dummy=base + '_trans.fits', check_key_type='trans')
            else:
                thumbs = self._thumbnail_products(res, base)
                extra = dict(thumbs or {}, fake_star=True) if res.get('fakestars') is not None else thumbs      # (FAKE_STAR even in an empty table)
                products.small('trans', res['transients'], base + '_trans.fits', dict(full_t), *([extra] if extra else []))
                if res.get('fakestars') is not None:
                    # the injected stars and what came back of them (fake_table), by the route of `_trans.fits`
                    products.small('fakestars', res['fakestars']['table'], base + '_trans_fakestars.fits', dict(full_t))
            products.small('header', base + '_trans_hdr.fits', dict(full_t))

    def _limmag_is_flux(self, header):
        """one rule for the unit of `_trans_limmag`, whichever path writes it: a flux limit only when no zeropoint is known --
        neither --zeropoint nor a numeric PC-ZP in the frame's header (then the output stage may queue it on the lane)"""
        if self.args.zeropoint is not None:
            return False
        return not ('PC-ZP' in header and not isinstance(self.R.hval(header, 'PC-ZP'), str))

    def write_limmag(self, base, res, header, products):
        """`_trans_limmag.fits` (set_blackbox.py:160-162): the transient detection limit per pixel,
        T-NSIGMA x Fpsferr -- in magnitudes when a zeropoint is known (--zeropoint, or PC-ZP of the header, with the
        extinction term PC-EXTCO x AIRMASSC when both are there: the photometric calibration itself is outside this
        path), else as a flux in e- (LIMUNIT says which)"""
        if res.get('Fpsferr') is None:
            return
        nsig = float(_hval(header, 'T-NSIGMA', 6.0))
        lim = None
        if not products.stages(base + '_trans_limmag.fits'):
            # (else the output stage has queued the flux limit already: only its header is made here, no image)
            lim = res['Fpsferr'] * nsig
        lim, h = self._limit_product(lim, header)
        h['LIMNSIG'] = (nsig, '[sigma] significance of the limit')
        products.image(base + '_trans_limmag.fits', lim.contiguous() if lim is not None else None, h)

    def _zeropoint(self, header):
        """-> (zp, ext): the zeropoint of the frame (--zeropoint, else a numeric PC-ZP of the header; None: none is known) and the
        extinction term PC-EXTCO x AIRMASSC (0 unless both are there)"""
        R = self.R
        zp = self.args.zeropoint
        if zp is None and 'PC-ZP' in header and not isinstance(R.hval(header, 'PC-ZP'), str):
            zp = float(R.hval(header, 'PC-ZP'))
        ext = 0.0
        if zp is not None and 'PC-EXTCO' in header and 'AIRMASSC' in header:
            try:
                ext = float(R.hval(header, 'PC-EXTCO')) * float(R.hval(header, 'AIRMASSC'))
            except (TypeError, ValueError):
                ext = 0.0
        return zp, ext

    def _limit_product(self, lim, header):
        """the one unit rule of `_trans_limmag` and `_red_limmag`: lim, a flux limit in e- (None: the output stage has queued it, as
        a flux: _limmag_is_flux) -> (the image to write, a copy of the header with LIMUNIT): magnitudes when a zeropoint is known"""
        from blackbox_amd.limflux import limit_magnitudes
        h = dict(header)
        zp, ext = self._zeropoint(header) if lim is not None else (None, 0.0)
        if zp is not None:
            lim = limit_magnitudes(lim, zp, float(exptime_of(header)), ext)
            h['LIMUNIT'] = ('mag', 'unit of the limiting-magnitude image')
        else:
            h['LIMUNIT'] = ('e-', 'limit in flux: no zeropoint was given')
        return lim, h

    def write_red_limmag(self, base, res, header, products):
        """`_red_limmag.fits` (set_blackbox.py:157-159): the detection limit of the reduced frame per pixel (res['limflux'],
        bbx_limflux_image) in the unit of `_trans_limmag`, and the frame keys LIMEFLUX, LIMMAG, LIMFNU in [header]"""
        from blackbox_amd.limflux import limflux_header
        info = res.get('limflux_info')
        if info is None:
            return
        zp, ext = self._zeropoint(header)
        header.update(limflux_header(res.get('limflux') is not None, info.get('stat'), info.get('win'), info.get('nsigma'), info.get('frac'),
                                     exptime=float(exptime_of(header)), zp=zp, ext=ext))
        if res.get('limflux') is None or not self.R.hval(header, 'LIMMAG-P'):
            return
        lim = None if products.stages(base + '_limmag.fits') else res['limflux']
        lim, h = self._limit_product(lim, header)
        products.image(base + '_limmag.fits', lim.contiguous() if lim is not None else None, h)

    # ---- many object frames: frames-in-flight pipeline ------------------------------------------
    def reduce_list(self, files):
        """object frames of one geometry through FramePipeline (several frames in flight on this GPU); anything else goes
        through blackbox_reduce one by one.  Raw frames are read and uploaded as the pipeline takes them (at most its depth
        in HBM at a time).  With --fpack True the image products are compressed on the lane that made them and written by
        the output stage's threads (blackbox_amd/outstage.py).  -> list of output names"""
        from blackbox_amd import pipeline as _pl
        out, todo = self._triage(files)
        first_raw, first_hdr = self._first_readable(todo, out)
        if not todo:
            return [out.get(fn) for fn in files]
        geom = self.R.geometry(first_raw.shape, self.args.ysize_chan, self.args.xsize_chan)
        os.makedirs(self.args.red_dir, exist_ok=True)
        run = _ListRun(self, todo, out, geom, first_raw, first_hdr)
        del first_raw                               # (the run alone holds the first frame, and drops it when the input stage reads the list)
        run.build(*list_run_sizes(_pl.cpu_budget(), len(todo), os.environ))
        try:
            try:
                run.pipe.run(run.source, on_done=run.on_done, on_input_error=run.on_input_error)
            except Exception:
                run.pipeline_gave_up()
            run.wait_for_writers()
        finally:
            run.close()
        for fn, _ in todo:
            if fn not in out:
                out[fn] = self.reduce_logged(fn)
        return [out.get(fn) for fn in files]

    def _triage(self, files):
        """-> out: fn -> result of the files reduced one by one here, done already or unreadable; todo: [(fn, fits_out)]"""
        out, todo = {}, []
        for fn in files:
            try:
                header = self.read_header(fn)
                if not self.args.red_dir:
                    self.args.red_dir = os.path.dirname(os.path.abspath(fn))
                _, fits_out = self.names(header)
                if imgtype_of(header) != 'object' or self.nonlin is not None:
                    out[fn] = self.reduce_logged(fn)
                elif self.already_done(fits_out):
                    out[fn] = fits_out
                else:
                    todo.append((fn, fits_out))
            except Exception:
                log.exception('exception was raised while reading %s', fn)
                out[fn] = None
        return out, todo

    def _first_readable(self, todo, out):
        # the list's geometry from its first readable file (one that is not fails alone, like any other: blackbox.py:948-999)
        while todo:
            try:
                return self.read_raw(todo[0][0])
            except Exception:
                log.exception('exception was raised while reading %s', todo[0][0])
                out[todo.pop(0)[0]] = None
        return None, None

    def read_header(self, filename):
        """the header of a raw frame without its pixels"""
        if filename.endswith('.fz'):
            return _frame_header(self.fitsio.read_hdus(filename, headers_only=True)[1][0])
        return _frame_header(self.fitsio.read_hdus(filename, headers_only=True)[0][0])


# threads and frames in flight from the cores this process may use (cgroup quota / affinity mask), like bench.py's
# files-to-files run: on the 16 cores of a one-GPU box 6 lanes, 16 frames, 12 writers, 4 readers (one process), or 4 lanes,
# 12 frames, 8 writers, 2 readers in each of two (list_processes)
def list_run_sizes(cores, nfiles, environ):
    """-> (lanes, depth, nwriters, nreaders) of a list run of [nfiles] frames on [cores] cores"""
    lanes = max(2, min(6, cores // 2))
    depth = max(2, min(16 if cores >= 12 else (12 if cores >= 8 else 8), nfiles))
    nwriters = max(2, min(12, cores))                     # (they wait in copies and write calls: 4 per 8 cores held the RAM-disk run at 70-75 frames/s, 8 give 90-95)
    nreaders = max(2, min(4, cores // 4))
    # (tuning runs: BBX_LIST_LANES / BBX_LIST_DEPTH / BBX_LIST_WRITERS / BBX_LIST_READERS override the choice above)
    lanes = int(environ.get('BBX_LIST_LANES', lanes))
    depth = max(2, min(int(environ.get('BBX_LIST_DEPTH', depth)), nfiles))
    nwriters = int(environ.get('BBX_LIST_WRITERS', nwriters))
    nreaders = int(environ.get('BBX_LIST_READERS', nreaders))
    return lanes, depth, nwriters, nreaders


class _SerialSource:
    """read + upload a frame when the pipeline asks for the next one (raw frames that are not unsigned 16-bit); a file
    that cannot be read fails alone (instage.InputError in its place)"""

    def __init__(self, run):
        self.run, self.k = run, 0

    def __iter__(self):
        return self

    def __next__(self):
        run, idx = self.run, self.k
        if idx >= len(run.todo):
            raise StopIteration
        self.k += 1
        fn = run.todo[idx][0]
        try:
            d_raw, header = (run.first_raw, run.first_hdr) if idx == 0 else run.r.read_raw(fn)
            if tuple(d_raw.shape) != (run.geom.ny_raw, run.geom.nx_raw):
                raise ValueError('frames of different shapes in one --image_list: {} vs {}'.format(
                    tuple(d_raw.shape), (run.geom.ny_raw, run.geom.nx_raw)))
        except Exception as e:
            from blackbox_amd.instage import InputError
            raise InputError(idx, fn, e)
        return d_raw, header


class _ListRun:
    """one pipelined --image_list run of a Reducer: the state its callbacks share.  Three kinds of thread call them (see
    blackbox_amd/pipeline.py): the orchestrating thread (the one inside pipe.run), the pipeline's finisher thread and the
    output stage's writer threads; each method says which"""

    def __init__(self, reducer, todo, out, geom, first_raw, first_hdr):
        self.r, self.todo, self.out, self.geom = reducer, todo, out, geom      # todo: [(fn, fits_out)]; out: fn -> result
        self.first_raw, self.first_hdr = first_raw, first_hdr
        self.exptime = exptime_of(first_hdr)                       # the one exposure time the pipeline works with
        self.t0 = time.time()
        self.written, self.input_failed = {}, set()                # idx -> error of its files or None; idx that failed on input
        self.all_written = threading.Event()
        self.stage = self.src = self.pipe = None

    def build(self, lanes, depth, nwriters, nreaders):            # output stage (--fpack True), pipeline, input stage
        from blackbox_amd import instage, outstage, pipeline
        r, geom = self.r, self.geom
        kw = {}
        self.source = _SerialSource(self)
        if r.args.fpack:
            # (output slots: the images of two frames per lane, one more image per frame with the object mask)
            nslots = 14 if r.sub is not None and r.sub.get('objmask') else 12
            if r.sub is not None and r.sub.get('limmag'):
                nslots += 2                                      # (and one with the limiting-flux image)
            self.stage = outstage.OutputStage(r.ctx.device, 2 * geom.ysize_chan, 8 * geom.xsize_chan, nwriters=nwriters, nslots=nslots)
            kw = dict(outstage=self.stage, out_base=self.out_base, on_written=self.on_written,
                      header_hook=self.header_hook, stage_limmag=r._limmag_is_flux)
        self.pipe = pipeline.FramePipeline(r.ctx, r.tel, geom, mflat=r.mflat, mbias=r.mbias, bpm=r.bpm, xtalk_coeffs=r.xtalk,
                                           exptime=self.exptime, depth=depth, lanes=min(lanes, depth), do_finish=True, detect_sats=True,
                                           keep_outputs=True, subtract=dict(r.sub) if r.sub is not None else None, log=log,
                                           ast_pointing=(r.args.ast_ra, r.args.ast_dec), **kw)
        # unsigned 16-bit raw frames (plain or fpacked: what the telescopes deliver) come through the input stage: reader
        # threads, one upload per file, the Rice decode on the device, nothing of it on the orchestrating thread
        if self.first_raw.dtype == r.torch.uint16 and len(self.todo) > 1:
            self.first_raw = None                                  # (the stage reads it again: not twice in HBM)
            self.source = self.src = instage.InputStage(r.ctx, [fn for fn, _ in self.todo], (geom.ny_raw, geom.nx_raw),
                                                        nreaders=nreaders, nbuf=self.pipe.depth + 4, ahead=max(2, min(4, nreaders)))

    def out_base(self, idx, header):                               # orchestrating thread
        return self.todo[idx][1].replace('.fits', '')

    def finish(self, f, products):
        """header completion + products of a frame that came out of the pipeline (header_hook's or on_done's thread)"""
        R, r = self.r.R, self.r
        (fn, fits_out), header = self.todo[f.idx], f.header        # (the dict the source handed to the pipeline: the frame's own)
        # the pipeline works with one exposure time; NCOSMICS follows the frame's own
        et = exptime_of(header)
        if et != self.exptime and not isinstance(R.hval(header, 'NCOSMICS'), str):
            header['NCOSMICS'] = (R.hval(header, 'NCOSMICS') * float(self.exptime) / float(et), header['NCOSMICS'][1])
        if 'zogy' in f.failed:
            header['Z-P'] = (False, 'successfully processed by ZOGY?')
        fh = r.open_image_log(fits_out)                       # the per-image log (blackbox.py:1311-1318) of a pipelined frame:
        try:                                                  # what its completion has to say (QC flags, failed steps)
            for step in f.failed:
                log.error('step [%s] failed for %s', step, fn)
            f.written_name = r.finish_object(fn, f.data, f.mask, header, f.hm, fits_out, self.t0, products, sub_result=f.sub)
        finally:
            r.close_image_log(fh)

    def header_hook(self, f, hdrs):
        """finisher thread: the frame's scalars are in: complete the headers (bookkeeping, QC flags, subtraction keywords)
        through the very code of the serial path; its image writes only hand their headers to the stage"""
        products = _Products(self.r, staged=f.out_names.values())
        self.finish(f, products)
        f.staged_wanted = set(products.headers)
        res = {**hdrs, **products.headers}
        if products.deferred:
            # the frame's small files: one task of the host pool (a worker process formats and writes them);
            # they count among the frame's files -- on_written fires when they and the images are on disk
            g = f.out_group
            g.add_task()
            from blackbox_amd import catalogs
            self.pipe.pool.apply_async(catalogs.write_small_products, (products.deferred,), callback=lambda r: g.file_done(None),
                                       error_callback=lambda e: g.file_done(None, e))
        return res

    def on_written(self, f, group):                                # a writer thread: the last file of the frame is on disk
        # products the frame's QC decided against (red flag: no subtraction products) were queued before the flag
        # was known: take them away again
        for p in group.paths:
            if f.staged_wanted is not None and p not in f.staged_wanted:       # (None: the hook did not get that far)
                try:
                    os.unlink(p)
                except OSError:
                    pass
        self.written[f.idx] = group.error
        _FILES_DONE.append(time.time())
        self.check_complete()

    def on_done(self, idx, f):                                     # orchestrating thread
        if self.src is not None:
            self.src.release(f.raw)
        fn = self.todo[idx][0]
        try:
            if self.stage is None:
                self.finish(f, _Products(self.r))
            self.out[fn] = f.written_name
        except Exception:
            log.exception('exception was raised during [blackbox_reduce] of %s', fn)
            self.out[fn] = None
        if self.stage is None:
            _FILES_DONE.append(time.time())

    def on_input_error(self, idx, e):                              # orchestrating thread
        # this file fails (blackbox.py:948-999: exception logged, None for the file), the list goes on
        log.error('exception was raised while reading %s: %r', self.todo[idx][0], e.cause)
        self.out[self.todo[idx][0]] = None
        self.input_failed.add(idx)
        self.check_complete()

    def check_complete(self):                                      # (on_written's, on_input_error's, pipeline_gave_up's thread)
        # every frame of todo has either been written or failed on input: wait_for_writers may go on
        if len(self.written) + len(self.input_failed) >= len(self.todo):
            self.all_written.set()

    def pipeline_gave_up(self):                                    # orchestrating thread, in the handler of pipe.run's exception
        # the pipeline itself gave up (not a file's fault): what it finished stands, the rest goes one by one.  No product
        # of the stage is waited for any more: every frame not written yet counts as failed on input
        log.exception('pipelined run failed; the files without products are reduced one by one')
        self.input_failed.update(idx for idx in range(len(self.todo)) if idx not in self.written)
        self.check_complete()

    def wait_for_writers(self):                                    # orchestrating thread; -> None for the files that were not written
        if self.stage is not None and not self.all_written.wait(600.0):
            log.error('output stage: %d of %d frames written', len(self.written), len(self.todo))
        for idx, err in self.written.items():
            if err is not None:
                log.error('writing the products of %s failed: %r', self.todo[idx][0], err)
                self.out[self.todo[idx][0]] = None

    def close(self):                              # the pipeline's BBX_TIMING figures; then pipeline, output stage (joins the writers), input stage
        pipe = self.pipe
        n = max(1, pipe.t_stats[3])
        _PIPE_STATS.update(frames=pipe.t_stats[3], lanes=len(pipe.lane_thread), depth=pipe.depth,
                           ms_start_to_strip_statistics=round(1e3 * pipe.t_stats[0] / n, 2), ms_overscan_fits=round(1e3 * pipe.t_stats[1] / n, 2),
                           ms_device_stage_and_lane_queue=round(1e3 * pipe.t_stats[2] / n, 2))
        pipe.close()
        if self.stage is not None:
            self.stage.close()
        if self.src is not None:
            self.src.close()
        self.pipe = None                             # (it holds this run's callbacks: no reference cycle left behind, the pool's semaphores go now)


def list_processes(args, nfiles):
    """how many pipelined processes a list run uses on its GPU.  One interpreter drives the GPU through some 300 library
    calls and a dozen file writes per frame from ~25 threads that share its lock: at ~60-75 frames/s that lock, not the
    GPU, is what a 16-core host runs out of.  Two processes with half the list, half the cores and a GPU context each have
    two locks (the GPU time-slices their queues; the masters are in HBM twice)."""
    if not args.image_list or nfiles < 2 or args.nproc > 1:
        return 1
    nlp = args.list_procs or int(os.environ.get('BBX_LIST_PROCS', '0'))     # (the variable: tuning runs)
    if nlp > 0:
        return min(nlp, nfiles)
    from blackbox_amd import pipeline as _pl
    world = int(os.environ.get('LOCAL_WORLD_SIZE', '1') or 1)
    return 2 if (_pl.cpu_budget() // max(1, world) >= 16 and nfiles >= 32) else 1


def reduce_list_in_processes(argv, files, nproc):
    """--image_list over [nproc] child processes `python blackbox.py ... --image_list <share> --list_procs 1` (the file k of
    the list goes to child k mod nproc; each child is told its share of the cores: BBX_CPU_BUDGET).  The parent makes no
    GPU call.  -> the results in the order of [files]; a child that dies reports None for the files it had not finished"""
    import json
    import subprocess
    import tempfile
    from blackbox_amd import pipeline as _pl
    cores = _pl.cpu_budget()
    base = []
    skip = False
    for a in argv:                                               # the parent's flags without the list and the split
        if skip:
            skip = False
            continue
        if a in ('--image_list', '--list_procs', '--image', '--master_date'):      # (the masters are made by the parent)
            skip = True
            continue
        if a.startswith(('--image_list=', '--list_procs=', '--image=', '--master_date=')):
            continue
        base.append(a)
    td = tempfile.mkdtemp(prefix='bbx_list_')
    procs = []
    try:
        for k in range(nproc):
            share = files[k::nproc]
            lst = os.path.join(td, 'share_%d.txt' % k)
            with open(lst, 'w') as f:
                f.write('\n'.join(share) + '\n')
            env = dict(os.environ, BBX_CPU_BUDGET=str(max(2, cores // nproc)), BBX_TIMING='1')
            procs.append((share, subprocess.Popen([sys.executable, os.path.abspath(__file__)] + base + ['--image_list', lst, '--list_procs', '1'],
                                                  env=env, stdout=subprocess.PIPE, text=True)))
        _mark('list_processes_started')
        out = {}
        done, stats = [], []
        for share, p in procs:
            text, _ = p.communicate()
            lines = [ln for ln in text.splitlines() if ln.strip()]
            tm = [ln for ln in lines if ln.startswith('BBX_TIMING ')]
            res = [ln for ln in lines if not ln.startswith('BBX_TIMING ')][-len(share):]
            if p.returncode != 0 or len(res) != len(share):
                log.error('list process for %d files ended with code %s and %d result lines', len(share), p.returncode, len(res))
                res = (res + ['None'] * len(share))[:len(share)] if p.returncode == 0 else ['None'] * len(share)
            for fn, r in zip(share, res):
                out[fn] = None if r == 'None' else r
            if tm:
                t = json.loads(tm[-1][len('BBX_TIMING '):])
                done += t.get('files_done_unix', [])
                stats.append(dict(pipeline=t.get('pipeline'), hbm_peak_GB_tensors=t.get('hbm_peak_GB_tensors'), marks=t.get('marks'), t0=t.get('t_module_import_unix', _T0)))
    finally:
        for _, p in procs:
            if p.poll() is None:
                p.kill()
        import shutil
        shutil.rmtree(td, ignore_errors=True)
    res = [out.get(fn) for fn in files]
    for o in res:
        print(o)
    if os.environ.get('BBX_TIMING'):
        _mark('done')
        # (the moment the last child had its masters in HBM, on this process's clock)
        first = [s_['t0'] + dict(s_['marks']).get('calibration_and_reference_files_in_hbm', 0.0) - _T0 for s_ in stats if s_.get('marks')]
        print('BBX_TIMING ' + json.dumps(dict(marks=_MARKS + [('calibration_and_reference_files_in_hbm', max(first) if first else 0.0)],
                                              t_module_import_unix=_T0, files_done_unix=sorted(done), list_processes=nproc,
                                              pipeline=[s_['pipeline'] for s_ in stats],
                                              hbm_peak_GB_tensors=round(sum(s_.get('hbm_peak_GB_tensors') or 0.0 for s_ in stats), 2))))
    return res


def section(v):
    """'y0:y1,x0:x1' (0-based Python slices of the y and x axes) -> (slice, slice)"""
    try:
        parts = [[int(p) for p in s.split(':')] for s in v.split(',')]
        if len(parts) != 2 or any(len(p) != 2 or p[0] < 0 or p[1] <= p[0] for p in parts):
            raise ValueError(v)
    except ValueError:
        raise argparse.ArgumentTypeError('section y0:y1,x0:x1 expected (0-based, y0 < y1, x0 < x1), got {!r}'.format(v))
    return slice(*parts[0]), slice(*parts[1])


def make_masters(args, argv):
    """--master_date: the masters of the evening date(s) (masters.create_masters, blackbox.py:617-782), one line per
    master printed (its path, or None).  A master that failed sets the exit status; one skipped for a reason the
    reference skips it too (too few frames, all too old) does not.  With --nproc > 1 the masters are spread over
    pool_func's spawned workers, one GPU context each.  -> [path or None]"""
    from blackbox_amd import masters
    kw = dict(tel=args.telescope, imgtypes=args.imgtypes, filters=args.filters, bpm=args.bpm,
              flat_norm_sec=args.flat_norm_sec, ysize_chan=args.ysize_chan, xsize_chan=args.xsize_chan,
              fpack=bool(args.fpack))
    if args.nproc > 1:
        configure(argv)
        res = masters.create_masters(args.master_date, args.red_dir, args.master_dir,
                                     pool=lambda func, items: pool_func(func, items, nproc=args.nproc), **kw)
    else:
        from blackbox_amd import farm, reduce as R
        ctx = R.Context(farm.rank_world()[2])
        try:
            res = masters.create_masters(args.master_date, args.red_dir, args.master_dir, ctx=ctx, **kw)
        finally:
            ctx.close()
    for name, path, err in res:
        print(path)
        if err is not None:
            log.error('master %s failed: %s', name, err)
            _STATE['exit_status'] = 1
    return [path for _, path, _ in res]


def build_parser():
    ap = argparse.ArgumentParser(description='BlackBOX per-image reduction on MI355X')
    ap.add_argument('--telescope', type=str, default='ML1')
    ap.add_argument('--mode', type=str, default='day')
    ap.add_argument('--date', type=str, default=None)
    ap.add_argument('--read_path', type=str, default=None)
    ap.add_argument('--recursive', type=str2bool, default=False)
    ap.add_argument('--imgtypes', type=str, default=None)
    ap.add_argument('--filters', type=str, default=None)
    ap.add_argument('--image', type=str, default=None)
    ap.add_argument('--image_list', type=str, default=None)
    ap.add_argument('--img_reduce', type=str2bool, default=True)
    ap.add_argument('--cat_extract', type=str2bool, default=False)
    ap.add_argument('--trans_extract', type=str2bool, default=False)
    ap.add_argument('--cat_shapes', type=str2bool, default=None,
                    help='with --cat_extract: FWHM, ELONGATION, A, B, THETA, X2, Y2, XY, FLAGS_MASK and sub-pixel X_POS / Y_POS in '
                         '_cat.fits, S-NOBJ S-FWHM S-FWSTD S-SEEING S-SEESTD S-ELONG S-ELOSTD in the header (default: settings.cat_shapes)')
    ap.add_argument('--cat_apphot', type=str2bool, default=None,
                    help='with --cat_extract: aperture fluxes E_FLUX_APER_R<r>xFWHM / E_FLUXERR_APER_R<r>xFWHM, BKG_APER, BKGSTD_APER, NSKY_APER, '
                         'FWHM_APER, FLAGS_APER in _cat.fits, AP-P AP-FWHM AP-NAPER AP-R* AP-SKYIN AP-SKYOU AP-LSKY AP-NSTAR AP-OPT* in the '
                         'header (default: settings.cat_apphot)')
    ap.add_argument('--apphot_radii', type=float_list, default=None,
                    help='[FWHM] aperture radii of --cat_apphot, a comma list of at most 8 (default: settings.apphot_radii)')
    ap.add_argument('--apphot_local_sky', type=str2bool, default=None,
                    help='subtract the sky annulus\' clipped median from the aperture fluxes (default: settings.apphot_local_sky)')
    ap.add_argument('--limmag', type=str2bool, default=None,
                    help='the limiting-flux image of the reduced frame from its sky noise, mask and PSF (--psf_new or --psf_build): '
                         '_red_limmag.fits (magnitudes with --zeropoint or PC-ZP, else e-), LIMMAG-P LIMNSIG LIMEFLUX LIMMAG LIMFNU LIMPFRAC '
                         'LIMWIN LIMNPIX in the header (default: settings.limmag)')
    ap.add_argument('--limmag_nsigma', type=float, default=None,
                    help='[sigma] significance of --limmag\'s limit (default: settings.limmag_nsigma)')
    ap.add_argument('--limmag_psf_frac', type=float, default=None,
                    help='share of the sum of PSF^2 that --limmag\'s window may leave out, in [0, 1); 0: the whole stamp (default: '
                         'settings.limmag_psf_frac)')
    ap.add_argument('--trans_psffit', type=str2bool, default=None,
                    help='fit the PSF of D to D at every transient candidate: X_PSF_D Y_PSF_D E_FLUX_PSF_D E_FLUXERR_PSF_D CHI2_PSF_D '
                         'FLAGS_PSF_D in `_trans.fits`, T-PSFD T-FITSZ T-NFIT T-PDFOLD T-CHI2MD in its header (default: '
                         'settings.trans_psffit)')
    ap.add_argument('--trans_fit_size', type=int, default=None, help='[pix] side of the window of that fit (default: settings.trans_fit_size)')
    ap.add_argument('--trans_chi2_max', type=float, default=None,
                    help='drop the candidates without a fit or with CHI2_PSF_D above this, T-NVET (default: settings.trans_chi2_max)')
    ap.add_argument('--fake_stars', type=int, default=None,
                    help='fake stars per sub-image, added to the background-subtracted new frame before the subtraction and read back from '
                         'Scorr / Fpsf: _trans_fakestars.fits, FAKE_STAR in `_trans.fits`, T-NFAKE T-FAKESN T-FK* in its header; 0: none '
                         '(default: settings.nfakestars)')
    ap.add_argument('--fake_s2n', type=float_list, default=None,
                    help='asked S/N of the fake stars, a comma list of at most 8 taken in turn (default: settings.fakestar_s2n)')
    ap.add_argument('--fake_seed', type=int, default=None, help='seed of their positions and noise (default: settings.fakestar_seed)')
    ap.add_argument('--fake_noise', type=str2bool, default=None, help='add their own Poisson noise (default: settings.fakestar_noise)')
    ap.add_argument('--fake_radius', type=int, default=None, help='[pix] recovery window about the injected pixel, <= 4 (default: settings.fakestar_radius)')
    ap.add_argument('--fake_clear_nsigma', type=float, default=None,
                    help='[sigma] no star where |new| or |ref| exceeds this within 3 pixels (default: settings.fake_clear_nsigma)')
    ap.add_argument('--trans_shapefit', type=str2bool, default=None,
                    help='fit an elliptical Gaussian and an elliptical Moffat to D at every transient candidate: X/Y_GAUSS_D FWHM_GAUSS_D '
                         'ELONG_GAUSS_D CHI2_GAUSS_D FLAGS_GAUSS_D and the same of _MOFFAT_D in `_trans.fits`, T-SHAPE T-SHPSZ T-MBETA T-NGAUS '
                         'T-NMOFF T-FWGMD T-ELGMD in its header (default: settings.trans_shapefit)')
    ap.add_argument('--trans_shape_size', type=int, default=None, help='[pix] side of the window of those fits (default: settings.trans_shape_size)')
    ap.add_argument('--trans_fwhm_gauss_min', type=float, default=None,
                    help='[pix] drop the candidates without a Gauss fit or with FWHM_GAUSS_D below this, T-NVET (default: settings.trans_fwhm_gauss_min)')
    ap.add_argument('--trans_fwhm_gauss_max', type=float, default=None, help='[pix] ... above this (default: settings.trans_fwhm_gauss_max)')
    ap.add_argument('--trans_elong_gauss_max', type=float, default=None,
                    help='... or with ELONG_GAUSS_D above this (default: settings.trans_elong_gauss_max)')
    ap.add_argument('--phot_centroid', type=str2bool, default=None,
                    help='catalogue photometry (--cat_extract, --zogy_match) with the PSF shifted to each source\'s windowed centroid and '
                         'masked pixels left out: FLAGS_OPT and sub-pixel X_POS / Y_POS in _cat.fits, PHOT-CEN in the header (default: '
                         'settings.phot_centroid)')
    ap.add_argument('--objmask', type=str2bool, default=None,
                    help='subtraction stage: object mask from the first background pass, the mesh measured again without the masked '
                         'pixels; _objmask.fits, OBJM-P OBJM-THR OBJM-MIN OBJM-GRW OBJM-NPX OBJM-NOB OBJM-FRC S-BKG1 S-BKGSD1 in the '
                         'header (default: settings.objmask)')
    ap.add_argument('--objmask_nsigma', type=float, default=None, help='[sigma] --objmask: detection threshold (settings.objmask_nsigma)')
    ap.add_argument('--objmask_minarea', type=int, default=None, help='[pix] --objmask: smallest component kept (settings.objmask_minarea)')
    ap.add_argument('--objmask_grow', type=int, default=None, help='[pix] --objmask: growth radius, 0 ... 8 (settings.objmask_grow)')
    ap.add_argument('--force_reproc_new', type=str2bool, default=False)
    ap.add_argument('--master_date', type=str, default=None,
                    help='make the masters of this evening date yyyymmdd, or of the dates in this file (one per line, '
                         'optionally followed by the flat filters), from the frames under --red_dir')
    ap.add_argument('--master_dir', type=str, default=None,
                    help='--master_date: root of the masters (<master_dir>/<yyyy/mm/dd>/<imgtype>/)')
    ap.add_argument('--name_genlog', type=str, default=None)
    ap.add_argument('--keep_tmp', type=str2bool, default=None)
    # explicit calibration inputs (the date-based master selection of master_prep is orchestration)
    ap.add_argument('--mflat', type=str, default=None)
    ap.add_argument('--fpack', type=lambda v: str(v).lower() in ('1', 'true', 'yes'), default=False,
                    help='write tile-compressed .fits.fz products (compressed on the GPU)')
    ap.add_argument('--mbias', type=str, default=None)
    ap.add_argument('--bpm', type=str, default=None)
    ap.add_argument('--crosstalk', type=str, default=None)
    ap.add_argument('--nonlin', type=str, default=None, help='pickle of 16 scipy splines (set_bb.nonlin_corr_file)')
    ap.add_argument('--red_dir', type=str, default=None)
    ap.add_argument('--ysize_chan', type=int, default=None)
    ap.add_argument('--xsize_chan', type=int, default=None)
    # explicit inputs of zogy.optimal_subtraction (reference selection / PSFEx are orchestration)
    ap.add_argument('--ref', type=str, default=None, help='reference image on the new frame\'s pixel grid (_red.fits)')
    ap.add_argument('--ref_mask', type=str, default=None)
    ap.add_argument('--ref_bkg_std_mini', type=str, default=None, help='the reference\'s _bkg_std_mini.fits')
    ap.add_argument('--ref_bkgsub', type=str2bool, default=False, help='reference is background-subtracted (BKG-SUB)')
    ap.add_argument('--psf_new', type=str, default=None, help='PSFEx .psf model or FITS stamp / cube of the new image')
    ap.add_argument('--psf_ref', type=str, default=None)
    ap.add_argument('--psf_build', type=str2bool, default=None,
                    help='without --psf_new (--psf_ref): build the PSF model from the frame\'s (the reference\'s) own stars, write it as '
                         '_psf.fits and put PSF-P PSF-NOBJ PSF-CHI2 PSF-FWHM PSF-SEE PSF-SIZE PSF-CFGS PSF-SAMP PSF-PLDG PSF-FIX into the '
                         'header (default: settings.psf_build)')
    ap.add_argument('--psf_size', type=int, default=None, help='[pix] --psf_build: side of the model, odd, at most 49 (settings.psf_size)')
    ap.add_argument('--psf_poldeg', type=int, default=None, help='--psf_build: degree of the polynomial in the position (settings.psf_poldeg)')
    ap.add_argument('--fratio', type=float, default=1.0, help='flux ratio new / ref (Z-FNR)')
    ap.add_argument('--zogy_dx', type=float, default=0.0, help='[pix] astrometric scatter in x (Z-DXSTD)')
    ap.add_argument('--zogy_dy', type=float, default=0.0)
    ap.add_argument('--zogy_match', type=str2bool, default=None,
                    help='measure the flux ratio and dx, dy per sub-image from the stars matched with the reference (Z-FNR, '
                         'Z-DX, Z-DY and Z-DXSTD, Z-DYSTD, Z-FNRSTD, Z-FNRERR); --fratio --zogy_dx --zogy_dy are the fallback '
                         '(default: settings.zogy_match)')
    ap.add_argument('--match_dist', type=float, default=None, help='[pix] largest distance of a star match (settings.match_dist_pix)')
    ap.add_argument('--ref_align', type=str2bool, default=None,
                    help='register --ref (any shape) on the new frame from the stars of both instead of taking it to lie on the new '
                         'frame\'s pixel grid: A-P A-PLDG A-NVOTE A-NRUN A-NFAR A-NPAIR A-RMSX A-RMSY A-DX A-DY A-ROT A-SCALE A-FLAGS A-NEDGE '
                         'T-NOFFR in the header of _trans; a registration that fails leaves the new-only products (default: settings.ref_align)')
    ap.add_argument('--align_poldeg', type=int, choices=(1, 2), default=None,
                    help='--ref_align: degree of the transform\'s polynomial, 1 or 2 (settings.align_poldeg)')
    ap.add_argument('--align_max_shift', type=float, default=None,
                    help='[pix] --ref_align: largest offset new - ref the vote looks for (settings.align_max_shift)')
    ap.add_argument('--align_bin', type=float, default=None, help='[pix] --ref_align: bin of the vote\'s histogram (settings.align_bin)')
    ap.add_argument('--astrometry', type=str2bool, default=None,
                    help='solve the new frame against --ast_cat from its own star list (needs --psf_new or --psf_build): the TAN[-SIP] WCS, '
                         'A-P A-PSCALE A-PSCALX A-PSCALY A-ROT A-ROTX A-ROTY A-CAT-F A-NAST A-TNAST A-DRA A-DRASTD A-DDEC A-DDESTD RA-CNTR '
                         'DEC-CNTR A-PLDG A-NVOTE A-MSHFT A-FLAGS in the header of _red, RA DEC in _red_cat, RA_PEAK DEC_PEAK [RA_PSF_D '
                         'DEC_PSF_D] in _red_trans; a solve that fails leaves A-P False and today\'s products (default: settings.astrometry)')
    ap.add_argument('--ast_cat', type=str, default=None,
                    help='--astrometry: the star catalogue, a FITS binary table with positions in degrees (ICRS) and a magnitude (settings.ast_cat)')
    ap.add_argument('--ast_cat_cols', type=name_list, default=None,
                    help='--astrometry: its three column names, comma separated (settings.ast_cat_cols: RA,DEC,MAG)')
    ap.add_argument('--ast_ra', type=float, default=None, help='[deg] --astrometry: the pointing of every frame, over the header\'s RA')
    ap.add_argument('--ast_dec', type=float, default=None, help='[deg] --astrometry: the pointing of every frame, over the header\'s DEC')
    ap.add_argument('--ast_pixscale', type=float, default=None, help='[arcsec/pix] --astrometry: nominal pixel scale (settings.pixscale)')
    ap.add_argument('--ast_rot', type=float, default=None, help='[deg] --astrometry: nominal rotation, FITS CROTA2 convention (settings.ast_rot)')
    ap.add_argument('--ast_parity', type=int, choices=(-1, 1), default=None,
                    help='--astrometry: +1 north up, east left at rotation 0; -1 mirrored (settings.ast_parity)')
    ap.add_argument('--ast_max_shift', type=float, default=None,
                    help='[pix] --astrometry: largest pointing error the vote looks for (settings.ast_max_shift)')
    ap.add_argument('--ast_bin', type=float, default=None, help='[pix] --astrometry: bin of the vote\'s histogram (settings.ast_bin)')
    ap.add_argument('--ast_poldeg', type=int, choices=(1, 2), default=None,
                    help='--astrometry: degree of the solution, 1 (TAN) or 2 (TAN-SIP) (settings.ast_poldeg)')
    ap.add_argument('--ast_rounds', type=int, default=None, help='--astrometry: rounds of match and fit behind the vote (settings.ast_rounds)')
    ap.add_argument('--ast_dist', type=float, default=None, help='[pix] --astrometry: largest distance of a match (settings.ast_dist, else match_dist_pix)')
    ap.add_argument('--ast_mag_zp', type=float, default=None, help='--astrometry: zeropoint of the catalogue fluxes (settings.ast_mag_zp)')
    ap.add_argument('--subimage_size', type=int, default=None)
    ap.add_argument('--flat_norm_sec', type=section, default=None,
                    help='y0:y1,x0:x1: flat normalisation / statistics section (default set_bb.flat_norm_sec of the telescope)')
    ap.add_argument('--subimage_border', type=int, default=None)
    ap.add_argument('--bkg_boxsize', type=int, default=None)
    # transient thumbnails (set_blackbox.py:62-66, 90): unset = blackbox_amd.settings (both switches off there)
    ap.add_argument('--save_thumbnails', type=str2bool, default=None,
                    help='THUMBNAIL_RED/_REF/_D/_SCORR and FLAGS_MASK columns in _trans.fits')
    ap.add_argument('--save_thumbnails_pngs', type=str2bool, default=None,
                    help='{NUMBER}_{RED,REF,D,SCORR}.png of every transient under --thumbnails_dir')
    ap.add_argument('--thumbnails_dir', type=str, default=None,
                    help='root of the PNG thumbnails: <thumbnails_dir>/<image base name>/ (default: thumbnails/ next to the products)')
    ap.add_argument('--zeropoint', type=float, default=None,
                    help='[mag] photometric zeropoint for 1 e-/s (else header PC-ZP): _trans_limmag in magnitudes')
    ap.add_argument('--nproc', type=int, default=1, help='worker processes for --image_list (one GPU context each)')
    ap.add_argument('--list_procs', type=int, default=0,
                    help='--image_list: this many pipelined processes share the GPU, each with a share of the list and of the cores '
                         '(0 = by the cores this process may use; 1 = one process)')
    return ap


def main(argv=None):
    ap = build_parser()
    argv = list(sys.argv[1:] if argv is None else argv)
    args = ap.parse_args(argv)
    logging.basicConfig(level='INFO', format='%(asctime)s [%(levelname)s, %(process)s] %(message)s')
    _STATE['exit_status'] = 0
    for flag in ('date', 'read_path', 'name_genlog') + (() if args.master_date else ('imgtypes', 'filters')):
        if getattr(args, flag):
            log.warning('--%s concerns orchestration and is ignored by the hot-path build', flag)
    if args.mode != 'day':
        log.warning('night mode (watchdog) is out of scope; running the given files once')
    if args.master_date:
        if not (args.red_dir and args.master_dir):
            ap.error('--master_date needs --red_dir (the reduced calibration frames) and --master_dir')
        from blackbox_amd import masters
        try:
            masters.master_dates(args.master_date)
        except ValueError as e:
            ap.error(str(e))
    files = []
    if args.image:
        files.append(args.image)
    if args.image_list:
        with open(args.image_list) as f:
            files += [ln.strip() for ln in f if ln.strip()]
    if args.master_date:
        made = make_masters(args, argv)
        if not files:
            return made
    if not files:
        ap.error('--image or --image_list required')
    tel = telescope_of(args, files[0])
    from blackbox_amd import farm
    mine = farm.shard(files)
    if args.nproc > 1 and len(mine) > 1:
        # the reference's farm (blackbox.py:375-379): a pool of workers over the file list, one GPU context each
        configure(argv)
        _mark('pool_start')
        try:
            out = pool_func(try_blackbox_reduce, mine, nproc=args.nproc)
        except WrapException as e:
            log.error('a worker raised during [blackbox_reduce]:\n%s', e.formatted)
            raise
        for o in out:
            print(o)
        if os.environ.get('BBX_TIMING'):
            import json
            _mark('done')
            print('BBX_TIMING ' + json.dumps(dict(marks=_MARKS, t_module_import_unix=_T0)))
        return out
    nlp = list_processes(args, len(mine))
    if nlp > 1:
        return reduce_list_in_processes(argv, mine, nlp)
    red = Reducer(tel, args)
    sampler = _start_sampler(os.environ.get('BBX_CLI_SAMPLE'))
    if args.image_list and len(mine) > 1:
        out = red.reduce_list(mine)
    else:
        out = [red.reduce_logged(f) for f in mine]
    for o in out:
        print(o)
    if os.environ.get('BBX_TIMING'):
        import json
        _mark('done')
        import torch
        print('BBX_TIMING ' + json.dumps(dict(marks=_MARKS, t_module_import_unix=_T0, files_done_unix=sorted(_FILES_DONE), pipeline=_PIPE_STATS,
                                              hbm_peak_GB_tensors=round(torch.cuda.max_memory_allocated() / 1e9, 2))))
    return out


if __name__ == '__main__':
    main()
    # Every product is on disk and every line printed: leave without the interpreter's teardown (module destructors, the
    # GPU runtime's unload, the worker pools' joins: 0.3-0.6 s of a 2 s per-file process -- the reference's Slurm contract
    # is one process per file).  An exception never gets here: it ends the process the ordinary way, with its traceback.
    logging.shutdown()
    sys.stdout.flush()
    sys.stderr.flush()
    if os.environ.get('BBX_FAST_EXIT', '1') != '0':
        os._exit(_STATE['exit_status'])
    sys.exit(_STATE['exit_status'])
