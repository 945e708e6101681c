"""Sample sheets: a minibatch of ragged clips as ONE picture, each clip a waveform envelope over a spectrogram.

  sheet_geometry(B, L, cols, Hw, gutter)   the image geometry of a sheet of B clips of up to L samples
  thresholds(range_db)                     the 256 power ratios that stand in for a logarithm
  colormap(name)                           an analytic 256 x 3 table ('helix')
  render(wave, lens, ...)                  on the device: ``kernels.melcep_frames(power=)`` then ``kernels.sheet_render``
  render_host(wave, lens, ...)             the same rule in numpy, from a given or a host-computed power
  write_png(path, img)                     8-bit RGB, filter 0, with zlib and struct alone
  SheetWriter(dir, every, cols)            a ``TrainLoop`` ``on_sample`` callable: writes sheet-<gen_iter>.png

The reference plots every sample's waveform into TensorBoard on the host (audiogan.py:639-653, :674, :930).  Here the samples'
ragged lengths stay on the device after ``Generator.generate``: ag_sheet_render forms every clip's peak and spectral maximum in
its own prologue, so a sheet costs two launches and ONE device-to-host copy of the finished image - no read of lengths or peaks
between two graph replays.  The rule of both halves is exact (include/audiogan_hip.h: ag_sheet_render): ``render_host`` fed the
device's power gives the device's bytes."""
import os
import struct
import zlib

import numpy as np
import torch

BINS = 129          # bins 0 .. 128 of the 256-point DFT
HOP = 128           # samples per pixel column
FRAME = 256
MAX_GUTTER = 16
BG, PAPER, INK = (32, 32, 32), (255, 255, 255), (0, 0, 0)


def lt_frames(L):
    """the frame capacity of a clip of L samples (kernels.lt_frames)"""
    return (L - FRAME) // HOP + 1 if L >= FRAME else 1


def sheet_geometry(B, L, cols=8, Hw=64, gutter=2):
    """-> dict(H, W, rows, cols, Wt, Ht, Hw, gutter): tiles of Wt = ceil(L / 128) x Ht = Hw + 129 pixels, ``cols`` across (at most
    B), a gutter around every one: tile b has its top left pixel at (gutter + (b div cols) (Ht + gutter), gutter + (b mod cols)
    (Wt + gutter))."""
    B, L, cols, Hw, gutter = int(B), int(L), int(cols), int(Hw), int(gutter)
    if B <= 0 or L <= 0 or cols <= 0:
        raise ValueError('audiogan_amd: a sheet of %d clips of %d samples, %d across: all must be positive' % (B, L, cols))
    if Hw < 3 or not 0 <= gutter <= MAX_GUTTER:
        raise ValueError('audiogan_amd: a wave strip of %d rows (at least 3) and a gutter of %d (0 .. %d)' % (Hw, gutter, MAX_GUTTER))
    cols = min(cols, B)
    rows = (B + cols - 1) // cols
    Wt, Ht = (L + HOP - 1) // HOP, Hw + BINS
    return dict(H=gutter + rows * (Ht + gutter), W=gutter + cols * (Wt + gutter), rows=rows, cols=cols, Wt=Wt, Ht=Ht, Hw=Hw,
                gutter=gutter)


def thresholds(range_db=80.0):
    """float32 [256]: thresholds[l] = 10^((l / 255 - 1) range_db / 10), evaluated in float64 and rounded once.  A cell of power P
    in a clip of spectral maximum Pmax has the level max{l : P >= thresholds[l] * Pmax}: 255 levels over ``range_db`` decibels
    below the maximum, and no logarithm on the device."""
    range_db = float(range_db)
    if not 0 < range_db <= 300:
        raise ValueError('audiogan_amd: a range of %r dB: 0 < range_db <= 300' % range_db)
    l_ = np.arange(256, dtype=np.float64)
    return np.power(10.0, (l_ / 255.0 - 1.0) * range_db / 10.0).astype(np.float32)


def colormap(name='helix'):
    """uint8 [256, 3].  'helix': a spiral through colour space whose perceived brightness rises steadily from black to white
    (the cubehelix construction, D. A. Green 2011, start 0.5, -1.5 rotations, hue 1.2): ordered on a screen and in a
    grey-scale print.  'grey': a ramp."""
    t = np.arange(256, dtype=np.float64) / 255.0
    if name == 'grey':
        rgb = np.stack([t, t, t], 1)
    elif name == 'helix':
        phi = 2.0 * np.pi * (0.5 / 3.0 + 1.0 - 1.5 * t)
        a = 1.2 * t * (1.0 - t) / 2.0
        c, s = np.cos(phi), np.sin(phi)
        rgb = np.stack([t + a * (-0.14861 * c + 1.78277 * s), t + a * (-0.29227 * c - 0.90649 * s), t + a * (1.97294 * c)], 1)
    else:
        raise ValueError("audiogan_amd: no colour map %r ('helix', 'grey')" % (name,))
    return np.rint(np.clip(rgb, 0.0, 1.0) * 255.0).astype(np.uint8)


def _cmap(cmap):
    cmap = colormap(cmap) if isinstance(cmap, str) else np.ascontiguousarray(cmap, dtype=np.uint8)
    if cmap.shape != (256, 3):
        raise ValueError('audiogan_amd: a colour map is uint8 [256, 3], got %r' % (cmap.shape,))
    return cmap


# ---- the host ---------------------------------------------------------------------------------------------------------------
def power_host(wave, lens=None):
    """-> (power float32 [B, F, 129], nframes int32 [B]): |X|^2 of the 256-sample periodic-Hann frames at hop 128 that
    ``kernels.melcep_frames`` takes (one zero-padded frame for a clip shorter than 256 samples), by numpy's FFT in float64.
    Rows at or past a clip's frame count are zero."""
    wave = np.asarray(wave, dtype=np.float32)
    B, L = wave.shape
    n = np.full(B, L, dtype=np.int64) if lens is None else np.clip(np.asarray(lens, dtype=np.int64), 0, L)
    F = lt_frames(L)
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(FRAME) / FRAME)
    power, nframes = np.zeros((B, F, BINS), dtype=np.float32), np.zeros(B, dtype=np.int32)
    for b in range(B):
        x = np.zeros(max(int(n[b]), FRAME), dtype=np.float64)
        x[:n[b]] = wave[b, :n[b]]
        nf = lt_frames(int(n[b]))
        fr = np.stack([x[j * HOP:j * HOP + FRAME] for j in range(nf)]) * win
        power[b, :nf] = (np.abs(np.fft.rfft(fr, axis=1)) ** 2).astype(np.float32)
        nframes[b] = nf
    return power, nframes


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def render_host(wave, lens=None, power=None, nframes=None, cols=8, Hw=64, gutter=2, range_db=80.0, cmap='helix', bg=BG,
                paper=PAPER, ink=INK):
    """ag_sheet_render on the host, whole arrays at a time -> uint8 [H, W, 3] (numpy).  ``power`` / ``nframes``: as
    ``kernels.melcep_frames`` leaves them (given the device's, the bytes are the device's); default: ``power_host``."""
    wave = np.ascontiguousarray(_np(wave), dtype=np.float32)
    B, L = wave.shape
    geo = sheet_geometry(B, L, cols, Hw, gutter)
    n = np.full(B, L, dtype=np.int64) if lens is None else np.clip(_np(lens).astype(np.int64), 0, L)
    if power is None:
        power, nframes = power_host(wave, n)
    power = np.asarray(_np(power), dtype=np.float32)
    Wt, Ht, F = geo['Wt'], geo['Ht'], power.shape[1]
    nf = np.clip(_np(nframes).astype(np.int64), 0, min(F, Wt))
    thr, table = thresholds(range_db), _cmap(cmap)
    f32 = np.float32
    half, top = f32(0.5) * f32(Hw - 1), f32(Hw - 1)
    img = np.empty((geo['H'], geo['W'], 3), dtype=np.uint8)
    img[...] = np.asarray(bg, dtype=np.uint8)
    rows_i = np.arange(Hw)[:, None]
    with np.errstate(all='ignore'):
        for b in range(B):
            y0 = gutter + (b // geo['cols']) * (Ht + gutter)
            x0 = gutter + (b % geo['cols']) * (Wt + gutter)
            nb = int(n[b])
            ncol = (nb + HOP - 1) // HOP
            if ncol:
                x = np.full(ncol * HOP, np.nan, dtype=np.float32)
                x[:nb] = wave[b, :nb]
                peak = np.fmax.reduce(np.abs(x), initial=f32(0))
                seg = x.reshape(ncol, HOP)
                vmax, vmin = np.fmax.reduce(seg, 1), np.fmin.reduce(seg, 1)
                dead = np.isnan(vmax)
                vmax, vmin = np.where(dead, f32(0), vmax), np.where(dead, f32(0), vmin)
                if peak > 0:
                    def row(v):
                        y = (f32(1) - v / peak) * half
                        return np.rint(np.fmin(np.fmax(y, f32(0)), top)).astype(np.int64)
                    ra, rb = row(vmax), row(vmin)
                else:
                    ra = rb = np.full(ncol, (Hw - 1) // 2, dtype=np.int64)
                r0, r1 = np.minimum(ra, rb), np.maximum(ra, rb)
                inked = (rows_i >= r0[None, :]) & (rows_i <= r1[None, :])
                img[y0:y0 + Hw, x0:x0 + ncol] = np.where(inked[:, :, None], np.asarray(ink, dtype=np.uint8),
                                                         np.asarray(paper, dtype=np.uint8))
            m = int(nf[b])
            if m:
                P = power[b, :m]                                   # [m, 129]
                pmax = np.fmax.reduce(P.reshape(-1), initial=f32(0))
                level = np.zeros(P.shape, dtype=np.int64)
                if pmax > 0:
                    need = thr * pmax                              # fp32 products
                    count = (P[:, :, None] >= need[None, None, :]).sum(2)
                    level = np.maximum(count - 1, 0)
                img[y0 + Hw:y0 + Ht, x0:x0 + m] = table[level.T[::-1]]          # bin 0 at the bottom
    return img


# ---- the device -------------------------------------------------------------------------------------------------------------
_TABLES = {}


def _device_tables(range_db, cmap, device):
    device = torch.device(device)
    if device.type == 'cuda' and device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    table = _cmap(cmap)
    key = (float(range_db), table.tobytes(), str(device))
    if key not in _TABLES:
        _TABLES[key] = (torch.from_numpy(thresholds(range_db)).to(device), torch.from_numpy(table).to(device))
    return _TABLES[key]


def render(wave, lens=None, cols=8, Hw=64, gutter=2, range_db=80.0, cmap='helix', bg=BG, paper=PAPER, ink=INK, out=None,
           power=None, nframes=None):
    """``wave`` fp32 [B, L] on the device (unit stride along the samples), ``lens`` int64 [B] on the device or None -> uint8
    [H, W, 3] on the device (``sheet_geometry``): two launches - ``kernels.melcep_frames`` with ``power=``, then
    ``kernels.sheet_render`` - and no host read.  ``out``: the image to write; ``power`` / ``nframes``: buffers that receive
    what the first launch leaves ([B, F, 129] fp32, [B] int32), for callers that want them."""
    from . import kernels as K
    B, L = wave.shape
    geo = sheet_geometry(B, L, cols, Hw, gutter)
    dev = wave.device
    if lens is not None and lens.dtype != torch.int64:
        lens = lens.to(torch.int64)
    if power is None:
        power = torch.empty(B, K.lt_frames(L), K.LTAS_BINS, dtype=torch.float32, device=dev)
    if nframes is None:
        nframes = torch.empty(B, dtype=torch.int32, device=dev)
    thr, table = _device_tables(range_db, cmap, dev)
    if out is None:
        out = torch.empty(geo['H'], geo['W'], 3, dtype=torch.uint8, device=dev)
    K.melcep_frames(wave, lens, nframes=nframes, power=power)
    return K.sheet_render(wave, lens, power, nframes, thr, table, out, geo['cols'], Hw, gutter, bg=bg, paper=paper, ink=ink)


# ---- files ------------------------------------------------------------------------------------------------------------------
def _chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xffffffff)


def write_png(path, img, level=1):
    """``img`` uint8 [H, W, 3] (numpy or a tensor on any device) -> an 8-bit RGB PNG, every scanline with filter 0.  ``level``:
    zlib's; the default is its fastest - a sheet is written between two training iterations, and level 6 takes four times as
    long for a file 15 % smaller"""
    img = np.ascontiguousarray(_np(img))
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or 0 in img.shape:
        raise ValueError('audiogan_amd: write_png takes uint8 [H, W, 3], got %s %r' % (img.dtype, img.shape))
    H, W = img.shape[:2]
    raw = np.zeros((H, 1 + 3 * W), dtype=np.uint8)
    raw[:, 1:] = img.reshape(H, 3 * W)
    data = (b'\x89PNG\r\n\x1a\n' + _chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 8, 2, 0, 0, 0)) +
            _chunk(b'IDAT', zlib.compress(raw.tobytes(), level)) + _chunk(b'IEND', b''))
    with open(path, 'wb') as f:
        f.write(data)
    return path


class SheetWriter(object):
    """``TrainLoop(on_sample=SheetWriter(dir, every))``: the samples of every generator iteration that is a multiple of ``every``
    become ``<dir>/sheet-<gen_iter>.png``.  On the device: ``render``; on the host (a CPU loop): ``render_host``.  ``samples``:
    the capacity of a tile in samples - ``Generator.generate`` returns rows only as wide as its longest sample, and sheets of one
    run should share a geometry; a narrower batch is padded to it (one copy; the padding is never read), a wider one keeps its
    width.  Default: the width of whatever it is given."""

    def __init__(self, directory, every=1, cols=8, samples=None, **options):
        self.dir, self.every, self.cols, self.options = directory, max(1, int(every)), int(cols), options
        self.samples = samples
        self.written = []

    def sheet(self, wave, length):
        on_device = torch.is_tensor(wave) and wave.is_cuda
        if not on_device:
            wave = torch.from_numpy(np.ascontiguousarray(_np(wave), dtype=np.float32))
        wave = wave.detach().float()
        if self.samples and wave.size(1) < self.samples:
            wave = torch.nn.functional.pad(wave, (0, int(self.samples) - wave.size(1)))
        if on_device:
            return render(wave, length, cols=self.cols, **self.options)
        return render_host(wave, length, cols=self.cols, **self.options)

    def write(self, name, wave, length):
        os.makedirs(self.dir, exist_ok=True)
        path = write_png(os.path.join(self.dir, name), self.sheet(wave, length))
        self.written.append(path)
        return path

    def __call__(self, gen_iter, wave, length, stop_list=None):
        if gen_iter % self.every:
            return None
        return self.write('sheet-%d.png' % gen_iter, wave, length)
