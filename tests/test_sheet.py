"""Sample sheets on the host: the threshold table, the colour map, ``sheet.render_host`` on hand-written clips and against the
pixel-by-pixel model of tests/sheet_model.py over the whole case table (byte for byte), the checker against mutants of the model,
the PNG writer through a reader written here, ``SheetWriter``, and the wrapper's and the library's refusals.  The launch itself:
tests/test_gpu_sheet.py."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import audiogan_amd.kernels as K
from audiogan_amd import _lib, sheet
from tests import sheet_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
BG, PAPER, INK = (np.array(c, dtype=np.uint8) for c in (M.BG, M.PAPER, M.INK))


# ---- tables ----------------------------------------------------------------------------------------------------------------
def test_thresholds_are_monotone_and_end_at_one():
    t = sheet.thresholds(80.0)
    assert t.dtype == np.float32 and t.shape == (256,)
    assert bool((t[1:] > t[:-1]).all()) and t[255] == f32(1) and t[0] == f32(1e-8)
    assert np.array_equal(sheet.thresholds(), t)
    t40 = sheet.thresholds(40.0)
    assert t40[0] == f32(1e-4) and t40[255] == f32(1) and bool((t40[1:] > t40[:-1]).all())
    with pytest.raises(ValueError):
        sheet.thresholds(0.0)


def test_colormap_is_ordered():
    c = sheet.colormap('helix')
    assert c.dtype == np.uint8 and c.shape == (256, 3) and tuple(c[0]) == (0, 0, 0) and tuple(c[255]) == (255, 255, 255)
    luma = c.astype(np.float64) @ np.array([0.299, 0.587, 0.114])
    assert bool((np.diff(luma) > -0.75).all()) and bool((np.diff(luma[::8]) > 0).all())          # brightness rises with the level
    assert len({tuple(v) for v in c}) >= 250
    g = sheet.colormap('grey')
    assert np.array_equal(g[:, 0], np.arange(256)) and np.array_equal(g[:, 0], g[:, 2])
    with pytest.raises(ValueError, match='jet'):
        sheet.colormap('jet')


def test_geometry():
    g = sheet.sheet_geometry(9, 384, cols=4, Hw=9, gutter=2)
    assert g == dict(H=2 + 3 * (138 + 2), W=2 + 4 * (3 + 2), rows=3, cols=4, Wt=3, Ht=138, Hw=9, gutter=2)
    assert sheet.sheet_geometry(1, 8, 4, 3, 0) == dict(H=132, W=1, rows=1, cols=1, Wt=1, Ht=132, Hw=3, gutter=0)
    assert sheet.sheet_geometry(64, 8192)['W'] == 2 + 8 * 66 and sheet.sheet_geometry(3, 129, 8)['Wt'] == 2
    for bad in (dict(B=0), dict(L=0), dict(cols=0), dict(Hw=2), dict(gutter=-1), dict(gutter=17)):
        with pytest.raises(ValueError):
            sheet.sheet_geometry(**dict(dict(B=2, L=256, cols=2, Hw=8, gutter=1), **bad))


# ---- levels: powers on either side of a threshold ---------------------------------------------------------------------------
def _spectrogram_of(power, Hw=3):
    """one clip of 256 samples whose single frame has the given 129 powers -> the 129 pixels of its spectrogram column, top down"""
    img = sheet.render_host(np.ones((1, 256), dtype=np.float32), None, power.reshape(1, 1, 129), np.array([1], dtype=np.int32),
                            cols=1, Hw=Hw, gutter=0)
    assert img.shape == (Hw + 129, 2, 3)
    return img[Hw:, 0]


def test_powers_on_either_side_of_a_threshold_land_on_the_stated_level():
    thr, cmap = sheet.thresholds(), sheet.colormap()
    pmax = f32(3.7)
    P = np.zeros(129, dtype=np.float32)
    want = np.zeros(129, dtype=np.int64)
    P[128], want[128] = pmax, 255
    for i, l_ in enumerate([1, 2, 17, 100, 128, 200, 254, 255]):
        edge = thr[l_] * pmax          # the fp32 product the rule names
        P[2 * i], want[2 * i] = edge, l_                                       # ON the threshold: the level itself (>=)
        P[2 * i + 1], want[2 * i + 1] = np.nextafter(edge, f32(0)), l_ - 1          # one ulp below: the level under it
    P[20], want[20] = thr[0] * pmax, 0
    P[21], want[21] = np.nextafter(thr[0] * pmax, f32(0)), 0          # below the whole range: level 0
    P[22], want[22] = 0.0, 0
    P[23], want[23] = f32('nan'), 0
    col = _spectrogram_of(P)
    assert np.array_equal(col[::-1], cmap[want])          # bin 0 is the BOTTOM pixel
    assert tuple(col[0]) == tuple(cmap[255])
    # an all-zero frame: level 0 everywhere, not a division by zero
    assert np.array_equal(_spectrogram_of(np.zeros(129, dtype=np.float32)), np.repeat(cmap[:1], 129, 0))


# ---- hand-written clips -----------------------------------------------------------------------------------------------------
def _tile(img, b, geo):
    y0 = geo['gutter'] + (b // geo['cols']) * (geo['Ht'] + geo['gutter'])
    x0 = geo['gutter'] + (b % geo['cols']) * (geo['Wt'] + geo['gutter'])
    return img[y0:y0 + geo['Ht'], x0:x0 + geo['Wt']]


def _is(pixels, colour):
    return bool((pixels.reshape(-1, 3) == colour).all())


def test_render_host_on_clips_of_every_edge_length():
    lens = [0, 1, 127, 128, 129, 255, 256]
    Hw, cols, gutter = 8, 4, 2
    wave = np.zeros((7, 256), dtype=np.float32)
    t = np.arange(256)
    for b, n in enumerate(lens):
        wave[b] = np.where(t % 2 == 0, 0.5, -0.5)          # every column holds +peak and -peak
        wave[b, n:] = np.nan                               # never read
    img = sheet.render_host(wave, np.array(lens), cols=cols, Hw=Hw, gutter=gutter)
    geo = sheet.sheet_geometry(7, 256, cols, Hw, gutter)
    assert img.shape == (geo['H'], geo['W'], 3) and geo['rows'] == 2 and geo['Wt'] == 2
    cmap = sheet.colormap()
    for b, n in enumerate(lens):
        tile = _tile(img, b, geo)
        strip, spec = tile[:Hw], tile[Hw:]
        ncol = (n + 127) // 128
        assert ncol == [0, 1, 1, 1, 2, 2, 2][b]
        assert _is(strip[:, ncol:], BG), (n, 'columns past the clip')
        if n >= 2:
            assert _is(strip[:, :ncol if n % 128 != 1 else ncol - 1], INK), n          # +-peak: ink from the first row to the last
        if n == 1:          # one sample at +peak: the top row alone
            assert _is(strip[0, 0], INK) and _is(strip[1:, 0], PAPER)
        if n == 129:        # the second column holds sample 128 alone, +0.5
            assert _is(strip[0, 1], INK) and _is(strip[1:, 1], PAPER)
        assert _is(spec[:, 1:], BG)                            # one frame whatever the length: column 0 only
        assert not _is(spec[:, 0], BG) or n == 0
    # n = 0: one zero-padded frame of power 0 -> level 0 down the column; no strip at all
    t0 = _tile(img, 0, geo)
    assert _is(t0[:Hw], BG) and np.array_equal(t0[Hw:, 0], np.repeat(cmap[:1], 129, 0))
    # gutters and the unused eighth cell
    mask = np.ones(img.shape[:2], dtype=bool)
    for b in range(7):
        y0, x0 = gutter + (b // 4) * (geo['Ht'] + gutter), gutter + (b % 4) * (geo['Wt'] + gutter)
        mask[y0:y0 + geo['Ht'], x0:x0 + geo['Wt']] = False
    assert mask.sum() > geo['Ht'] * geo['Wt'] and _is(img[mask], BG)
    assert _is(img[:gutter], BG) and _is(img[:, :gutter], BG) and _is(img[-gutter:], BG) and _is(img[:, -gutter:], BG)


def test_render_host_silence_a_single_sample_and_a_full_clip():
    Hw, L = 9, 384
    wave = np.zeros((3, L), dtype=np.float32)
    wave[1, 130] = -0.25                                                  # a single non-zero sample, in column 1
    tone = np.sin(2 * np.pi * 1000.0 * np.arange(L) / 8000.0)              # 1 kHz at 8 kHz: bin 32
    wave[2] = (0.8 * tone).astype(np.float32)
    img = sheet.render_host(wave, None, cols=4, Hw=Hw, gutter=1)
    geo = sheet.sheet_geometry(3, L, 4, Hw, 1)
    assert geo['cols'] == 3 and geo['rows'] == 1 and img.shape == (1 + Hw + 129 + 1, 1 + 3 * 4, 3)
    cmap = sheet.colormap()
    silent, single, full = (_tile(img, b, geo) for b in range(3))
    # silence: the centre line, and level 0 under it for both frames
    assert _is(silent[4, :], INK) and _is(silent[:4], PAPER) and _is(silent[5:Hw], PAPER)
    assert np.array_equal(silent[Hw:, :2].reshape(-1, 3), np.repeat(cmap[:1], 258, 0)) and _is(silent[Hw:, 2], BG)
    # the single sample: columns 0 and 2 draw zero (row rint(4.0) = 4), column 1 from zero down to -peak (the last row)
    assert _is(single[4, 0], INK) and _is(single[:4, 0], PAPER) and _is(single[5:Hw, 0], PAPER)
    assert _is(single[4:Hw, 1], INK) and _is(single[:4, 1], PAPER)
    assert np.array_equal(single[:Hw, 2], single[:Hw, 0])
    # an impulse is white: every bin of a frame that holds it is within a few dB of the frame's maximum
    assert not _is(single[Hw:, 0], cmap[0])
    # the full clip: three envelope columns, two frames, the brightest pixel at bin 32 = row Hw + 128 - 32
    assert not _is(full[:Hw, 2], BG) and _is(full[Hw:, 2], BG)
    column = full[Hw:, 0].astype(np.int64).sum(1)
    assert int(column.argmax()) == 128 - 32 and tuple(full[Hw + 96, 0]) == tuple(cmap[255])
    # bin 0 is at the bottom: a constant offset lights the last row
    dc = sheet.render_host(np.full((1, 256), 0.3, dtype=np.float32), None, cols=1, Hw=3, gutter=0)
    assert tuple(dc[3 + 128, 0]) == tuple(cmap[255]) and tuple(dc[3, 0]) == tuple(cmap[0])


def test_power_host_counts_frames_like_the_launch():
    wave = np.random.RandomState(0).standard_normal((4, 640)).astype(np.float32)
    power, nf = sheet.power_host(wave, [640, 639, 255, 0])
    assert power.shape == (4, 4, 129) and nf.tolist() == [4, 3, 1, 1] == [K.lt_frames(n) for n in (640, 639, 255, 0)]
    assert sheet.lt_frames(640) == K.lt_frames(640) and not power[2, 1:].any() and not power[3].any()


# ---- render_host against the model ----------------------------------------------------------------------------------------
def host_launch(wave, lens, power, nframes, thr, cmap, cols, Hw, gutter, bg, paper, ink):
    assert np.array_equal(thr, sheet.thresholds(80.0))
    return sheet.render_host(wave, lens, power, nframes, cols, Hw, gutter, 80.0, cmap, bg, paper, ink)


@pytest.mark.parametrize('pad', M.PADS)
def test_render_host_against_the_model_over_the_table(pad):
    for case in M.cases():
        M.run(M.as_launch(host_launch), case, pad)


def test_the_table_covers_what_it_says():
    cases = {c.name: c for c in M.cases()}
    assert len(cases) == len(M.cases()) == 8
    assert {c.B for c in cases.values()} >= {1, 3, 9} and {c.L for c in cases.values()} >= {8, 256, 384, 1000}
    assert set(cases['nine_384'].lens) >= {0, 1, 255, 256, 384, 500} and cases['nine_384'].B % cases['nine_384'].cols
    assert sheet.lt_frames(cases['two_tiles'].L) > K.SHEET_TILE_COLUMNS == 32
    assert cases['no_lens'].lens is None and cases['no_lens'].gutter == sheet.MAX_GUTTER
    assert {c.shift for c in cases.values()} == {0, 1, 2, 3}
    z = M.inputs(cases['nine_384'], 'nan')
    assert np.isnan(z['wave'][2, 255:]).all() and np.isnan(z['power'][0, 1:]).all() and not np.isnan(z['power'][4, :2]).any()
    z = M.inputs(cases['nine_384'], 'big')
    assert bool((z['wave'][2, 255:] == f32(3.0e6)).all())
    # every clip of two samples or more reaches both edges of its strip
    img, case = M.expected(cases['three_1000']), cases['three_1000']
    geo = sheet.sheet_geometry(3, 1000, 4, 16, 3)
    for b in range(3):
        strip = _tile(img, b, geo)[:16]
        assert (strip[0] == INK).all(1).any() and (strip[15] == INK).all(1).any()


@pytest.mark.parametrize('mutant', M.MUTANTS)
def test_the_checker_rejects_mutants_of_the_model(mutant):
    caught = []
    for pad in M.PADS:
        for case in M.cases():
            try:
                M.run(M.as_launch(M.render, mutate=mutant), case, pad)
            except AssertionError as e:
                caught.append((case.name, pad))
    assert caught, mutant
    want = dict(bin_flipped='one_tiny', gt_for_ge='one_tiny', peak_over_padded_row='nine_384',
                column_off_by_one='seven_edges')[mutant]          # (a clip of one sample: the shifted column is empty)
    assert want in {c for c, _ in caught}, (mutant, caught)
    if mutant == 'peak_over_padded_row':          # NaN padding is dropped by the maximum: only real values give it away
        assert {p for _, p in caught} == {'big'}


# ---- PNG ------------------------------------------------------------------------------------------------------------------
def read_png(path):
    """signature, chunk lengths and CRCs, IHDR of 8-bit RGB, inflate, filter 0 on every scanline -> uint8 [H, W, 3]"""
    raw = open(path, 'rb').read()
    assert raw[:8] == b'\x89PNG\r\n\x1a\n'
    at, chunks = 8, []
    while at < len(raw):
        n, kind = struct.unpack('>I4s', raw[at:at + 8])
        data = raw[at + 8:at + 8 + n]
        (crc,) = struct.unpack('>I', raw[at + 8 + n:at + 12 + n])
        assert crc == zlib.crc32(kind + data) & 0xffffffff, kind
        chunks.append((kind, data))
        at += 12 + n
    assert at == len(raw) and chunks[0][0] == b'IHDR' and chunks[-1] == (b'IEND', b'')
    W, H, depth, colour, comp, filt, lace = struct.unpack('>IIBBBBB', chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    lines = np.frombuffer(zlib.decompress(b''.join(d for k, d in chunks if k == b'IDAT')), dtype=np.uint8).reshape(H, 1 + 3 * W)
    assert not lines[:, 0].any()
    return lines[:, 1:].reshape(H, W, 3)


def test_png_round_trip(tmp_path):
    rng = np.random.RandomState(3)
    for shape in ((1, 1, 3), (5, 7, 3), (140, 33, 3)):
        img = rng.randint(0, 256, size=shape).astype(np.uint8)
        p = sheet.write_png(os.path.join(tmp_path, 'a.png'), img)
        assert np.array_equal(read_png(p), img)
        sheet.write_png(p, torch.from_numpy(img))
        assert np.array_equal(read_png(p), img)
    for bad in (np.zeros((4, 4), dtype=np.uint8), np.zeros((4, 4, 3), dtype=np.float32), np.zeros((0, 4, 3), dtype=np.uint8)):
        with pytest.raises(ValueError, match='write_png'):
            sheet.write_png(os.path.join(tmp_path, 'b.png'), bad)


def test_sheet_writer_takes_the_loops_on_sample_call(tmp_path):
    w = sheet.SheetWriter(os.path.join(tmp_path, 'sheets'), every=2, cols=2, Hw=8, gutter=1)
    wave = torch.from_numpy(np.random.RandomState(1).standard_normal((3, 384)).astype(np.float32))
    length = torch.tensor([384, 200, 0])
    assert w(1, wave, length, None) is None and not os.path.exists(w.dir)
    p = w(2, wave, length, None)
    assert os.path.basename(p) == 'sheet-2.png' and w.written == [p]
    geo = sheet.sheet_geometry(3, 384, 2, 8, 1)
    got = read_png(p)
    assert got.shape == (geo['H'], geo['W'], 3)
    assert np.array_equal(got, sheet.render_host(wave, length, cols=2, Hw=8, gutter=1))
    assert os.path.basename(w.write('real-sheet.png', wave, length)) == 'real-sheet.png'
    # a fixed capacity: a narrower batch (generate() returns rows as wide as its longest sample) is drawn at the same geometry
    w.samples = 384
    narrow = read_png(w(4, wave[:, :200], torch.tensor([200, 200, 0]), None))
    assert narrow.shape == got.shape
    assert np.array_equal(narrow, sheet.render_host(torch.nn.functional.pad(wave[:, :200], (0, 184)), [200, 200, 0], cols=2, Hw=8, gutter=1))
    w.samples = 100
    assert read_png(w(6, wave[:, :200], torch.tensor([200, 200, 0]), None)).shape[1] == 1 + 2 * 3          # a wider one keeps its width


# ---- refusals ---------------------------------------------------------------------------------------------------------------
class OnDevice(object):
    """a host tensor that says it lives on the device: what the wrapper's checks read before any launch"""

    def __init__(self, t):
        self.t, self.is_cuda = t, True

    def __getattr__(self, name):
        return getattr(self.t, name)


def _wrapper_args(**swap):
    z = dict(wave=torch.zeros(3, 384), lens=torch.zeros(3, dtype=torch.int64), power=torch.zeros(3, 2, 129),
             nframes=torch.zeros(3, dtype=torch.int32), thresholds=torch.zeros(256), cmap=torch.zeros(256, 3, dtype=torch.uint8),
             img=torch.zeros(142, 17, 3, dtype=torch.uint8))
    z.update(swap)
    return [None if z[k] is None else OnDevice(z[k]) for k in ('wave', 'lens', 'power', 'nframes', 'thresholds', 'cmap', 'img')]


@pytest.mark.parametrize('name,bad,exc', [
    ('wave', torch.zeros(3, 384, dtype=torch.float64), TypeError),
    ('lens', torch.zeros(3, dtype=torch.int32), TypeError),
    ('power', torch.zeros(3, 2, 129, dtype=torch.bfloat16), TypeError),
    ('nframes', torch.zeros(3, dtype=torch.int64), TypeError),
    ('thresholds', torch.zeros(256, dtype=torch.float64), TypeError),
    ('cmap', torch.zeros(256, 3), TypeError),
    ('img', torch.zeros(142, 17, 3), TypeError),
    ('wave', torch.zeros(384, 3).t(), AssertionError),                              # not unit stride along the samples
    ('lens', torch.zeros(4, dtype=torch.int64), AssertionError),                    # not one per clip
    ('power', torch.zeros(3, 2, 128), AssertionError),
    ('power', torch.zeros(2, 2, 129), AssertionError),
    ('nframes', torch.zeros(2, dtype=torch.int32), AssertionError),
    ('thresholds', torch.zeros(255), AssertionError),
    ('cmap', torch.zeros(3, 256, dtype=torch.uint8).t(), AssertionError),
    ('img', torch.zeros(142, 17, 4, dtype=torch.uint8), AssertionError),
    ('img', torch.zeros(142, 34, 3, dtype=torch.uint8)[:, ::2], AssertionError),
    ('img', torch.zeros(142, 51, dtype=torch.uint8), ValueError),
    ('wave', torch.zeros(384), ValueError),
])
def test_wrapper_refuses_before_the_launch(name, bad, exc):
    with pytest.raises(exc) as e:
        K.sheet_render(*_wrapper_args(**{name: bad}), 3, 9, 1)
    assert name in str(e.value), str(e.value)


def test_wrapper_refuses_host_tensors_and_bad_colours():
    a = _wrapper_args()
    with pytest.raises(RuntimeError, match='wave must be a CUDA'):
        K.sheet_render(torch.zeros(3, 384), *a[1:], 3, 9, 1)
    with pytest.raises(RuntimeError, match='img must be a CUDA'):
        K.sheet_render(*a[:6], torch.zeros(142, 17, 3, dtype=torch.uint8), 3, 9, 1)
    with pytest.raises(ValueError, match='ink'):
        K.sheet_render(*a, 3, 9, 1, ink=(0, 0, 256))
    assert not hasattr(K.sheet_render, 'timed_name') and K.SHEET_TILE_COLUMNS == 32 and K.SHEET_HOP == 128


def test_launcher_refuses_before_any_hip_call():
    """AG_ERR_ARG from host code, with no device in sight (the pointers are host memory: a launch would not survive them)"""
    buf = (C.c_char * 256)()
    p = C.addressof(buf) // 16 * 16 + 16

    def call(**kw):
        a = dict(wave=p, ld=384, lens=p, L=384, power=p, nframes=p, F=2, B=3, thr=p, cmap=p, bg=0, paper=0xffffff, ink=0, cols=3,
                 Hw=9, gutter=1, img=p, H=1 + 138 + 1, W=1 + 3 * 4)
        a.update(kw)
        return K.lib.ag_sheet_render(a['wave'], a['ld'], a['lens'], a['L'], a['power'], a['nframes'], a['F'], a['B'], a['thr'],
                                     a['cmap'], a['bg'], a['paper'], a['ink'], a['cols'], a['Hw'], a['gutter'], a['img'], a['H'],
                                     a['W'], None)
    for bad in (dict(wave=None), dict(power=None), dict(nframes=None), dict(thr=None), dict(cmap=None), dict(img=None),
                dict(B=0), dict(B=-1), dict(F=0), dict(L=0), dict(L=-5), dict(L=(1 << 30) + 1, ld=1 << 31), dict(ld=383),
                dict(Hw=2), dict(Hw=4097), dict(gutter=-1), dict(gutter=17), dict(cols=0), dict(H=0), dict(W=0),
                dict(H=139), dict(H=141), dict(W=12), dict(W=14), dict(cols=2), dict(cols=4), dict(B=4),
                dict(Hw=10), dict(gutter=2), dict(L=385),
                dict(cols=1, W=5, H=1 + 65536 * 139, B=3)):
        assert call(**bad) == _lib.AG_ERR_ARG, bad
        assert K.lib.ag_last_error().startswith(b'ag_sheet_render'), bad
    assert call(H=139) == _lib.AG_ERR_ARG and b'sheet_geometry' in K.lib.ag_last_error()
    header = open(os.path.join(ROOT, 'include', 'audiogan_hip.h')).read()
    for sym in ('ag_sheet_tile_columns', 'ag_sheet_render'):
        assert sym in _lib.SIGNATURES and 'int %s(' % sym in header
    assert '"sheet_render_kernel"' in header
    assert 'sheet.hip' in open(os.path.join(ROOT, 'audiogan_amd', 'csrc', 'Makefile')).read()
