"""Pixel-by-pixel model of ``audiogan_amd.kernels.sheet_render`` (ag_sheet_render; contract in include/audiogan_hip.h), the shared
case table, the checker and the mutants the checker must reject  --  TEST INFRASTRUCTURE.

The model walks tiles, columns and pixels one at a time in Python scalars of numpy.float32; ``sheet.render_host`` (whole arrays at
a time) and the launch must both give its bytes.  Inputs of a case are built so that every edge carries weight: one sample at
+peak and one at -peak per clip, powers that sit exactly ON a threshold and one ulp below it, and padding - wave samples at or
past a clip's length, power rows at or past its frame count - that holds either NaNs or large finite values."""
import collections

import numpy as np
import torch

from audiogan_amd import sheet

f32 = np.float32
BG, PAPER, INK = (32, 32, 32), (255, 255, 255), (0, 0, 0)
MUTANTS = ('bin_flipped', 'gt_for_ge', 'peak_over_padded_row', 'column_off_by_one')
PADS = ('nan', 'big')


def _row(v, peak, Hw):
    half, top = f32(0.5) * f32(Hw - 1), f32(Hw - 1)
    with np.errstate(all='ignore'):
        y = (f32(1) - f32(v) / f32(peak)) * half
    y = np.fmin(np.fmax(y, f32(0)), top)
    return int(np.rint(y))


def _max_dropping_nans(values):
    m = f32(0)
    for v in values:
        if v > m:          # (False for a NaN)
            m = v
    return m


def render(wave, lens, power, nframes, thr, cmap, cols, Hw, gutter, bg=BG, paper=PAPER, ink=INK, mutate=None):
    """numpy arrays in -> uint8 [H, W, 3]; ``mutate``: one of MUTANTS"""
    B, L = wave.shape
    F = power.shape[1]
    geo = sheet.sheet_geometry(B, L, cols, Hw, gutter)
    Wt, Ht, cols = geo['Wt'], geo['Ht'], geo['cols']
    img = np.empty((geo['H'], geo['W'], 3), dtype=np.uint8)
    img[:, :] = bg
    for b in range(B):
        n = L if lens is None else min(max(int(lens[b]), 0), L)
        nf = min(max(int(nframes[b]), 0), min(F, Wt))
        y0, x0 = gutter + (b // cols) * (Ht + gutter), gutter + (b % cols) * (Wt + gutter)
        row = wave[b]
        peak = _max_dropping_nans(np.abs(row if mutate == 'peak_over_padded_row' else row[:n]))
        pmax = _max_dropping_nans(power[b, :nf].reshape(-1))
        need = thr * pmax          # fp32 products
        for j in range(Wt):
            if 128 * j < n:
                t0 = 128 * j + (1 if mutate == 'column_off_by_one' else 0)
                vals = [v for v in row[t0:min(t0 + 128, n)] if v == v]
                if peak > 0:
                    ra, rb = _row(max(vals) if vals else 0, peak, Hw), _row(min(vals) if vals else 0, peak, Hw)
                else:
                    ra = rb = (Hw - 1) // 2
                for ty in range(Hw):
                    img[y0 + ty, x0 + j] = ink if min(ra, rb) <= ty <= max(ra, rb) else paper
            if j < nf:
                for k in range(129):
                    P = power[b, j, k]
                    level = 0
                    if pmax > 0:
                        hit = np.nonzero(P > need if mutate == 'gt_for_ge' else P >= need)[0]
                        level = int(hit[-1]) if len(hit) else 0
                    s = k if mutate == 'bin_flipped' else 128 - k
                    img[y0 + Hw + s, x0 + j] = cmap[level]
    return img


# ---- the case table ------------------------------------------------------------------------------------------------------
Case = collections.namedtuple('Case', 'name B L cols Hw gutter lens nframes extra shift')
#   lens: a list, or None (no lens tensor: every clip is L long); nframes: None = the frame count of each length, or a list;
#   extra: floats of row pitch beyond L; shift: bytes by which the image is moved off a 4-byte boundary


def cases():
    return [
        Case('one_tiny', 1, 8, 4, 3, 0, [8], None, 0, 0),
        Case('three_256', 3, 256, 4, 9, 1, [0, 1, 256], None, 3, 1),
        Case('seven_edges', 7, 256, 4, 8, 2, [0, 1, 127, 128, 129, 255, 256], None, 0, 2),
        Case('nine_384', 9, 384, 4, 9, 2, [0, 1, 255, 256, 384, 500, 127, 128, 129], None, 5, 3),
        Case('three_1000', 3, 1000, 4, 16, 3, [1000, 1200, 257], None, 24, 0),
        Case('no_lens', 3, 384, 2, 5, 16, None, None, 0, 1),
        Case('frame_counts', 4, 640, 4, 7, 1, [640, 640, 300, 640], [0, 9, -3, 2], 1, 2),
        Case('two_tiles', 2, 4400, 4, 6, 2, [4400, 4100], None, 8, 3),
    ]


def inputs(case, pad='nan', seed=0):
    """-> dict of numpy arrays: wave [B, L + extra] (the first L columns are the clip rows), lens, power [B, F, 129], nframes, thr, cmap"""
    rng = np.random.RandomState(seed + 17 * len(case.name))
    B, L = case.B, case.L
    F = sheet.lt_frames(L)
    fill = f32('nan') if pad == 'nan' else f32(3.0e6)
    thr, cmap = sheet.thresholds(80.0), sheet.colormap('helix')
    wave = np.full((B, L + case.extra), fill, dtype=np.float32)
    power = np.full((B, F, 129), fill, dtype=np.float32)
    lens = None if case.lens is None else np.asarray(case.lens, dtype=np.int64)
    nframes = np.zeros(B, dtype=np.int32)
    for b in range(B):
        n = L if lens is None else min(max(int(lens[b]), 0), L)
        x = (rng.standard_normal(n) * 0.2).astype(np.float32)
        if n >= 2:          # the two extremes, exactly +-peak
            top = f32(1.5) * np.abs(x).max() + f32(0.25)
            x[rng.randint(n)] = top
            i = rng.randint(n)
            x[i if x[i] != top else (i + 1) % n] = -top
        wave[b, :n] = x
        nf = sheet.lt_frames(n) if case.nframes is None else case.nframes[b]
        nframes[b] = nf
        m = min(max(nf, 0), F)
        P = np.exp(rng.uniform(-22.0, 0.0, size=(m, 129))).astype(np.float32) * f32(7.5)
        if m:
            pmax = P.max()
            flat = P.reshape(-1)
            at = rng.choice(flat.size, size=min(64, flat.size), replace=False)
            at = at[flat[at] != pmax]
            for q, i in enumerate(at):          # ON a threshold, and one ulp below it
                edge = thr[rng.randint(256)] * pmax
                flat[i] = edge if q % 2 == 0 else np.nextafter(edge, f32(0))
            if flat.size > 3:
                flat[rng.randint(flat.size)] = 0
        power[b, :m] = P
    return dict(wave=wave, lens=lens, power=power, nframes=nframes, thr=thr, cmap=cmap)


_EXPECTED = {}


def expected(case, seed=0):
    """the model's image of a case: computed once, shared, read-only (the padding's kind cannot matter: it is never read)"""
    key = (case.name, seed)
    if key not in _EXPECTED:
        z = inputs(case, 'nan', seed)
        img = render(z['wave'][:, :case.L], z['lens'], z['power'], z['nframes'], z['thr'], z['cmap'], case.cols, case.Hw,
                     case.gutter)
        img.setflags(write=False)
        _EXPECTED[key] = img
    return _EXPECTED[key]


GUARD = 64


def run(fn, case, pad='nan', on=None, seed=0):
    """``fn`` with the signature of ``kernels.sheet_render`` on the case's tensors (moved by ``on``), its image between guard bytes
    and ``shift`` bytes off alignment.  Asserts the model's bytes and intact guards; -> the image (a host tensor)."""
    on = on or (lambda t: t)
    z = inputs(case, pad, seed)
    want = expected(case, seed)
    H, W = want.shape[:2]
    t = lambda a: None if a is None else on(torch.from_numpy(a))      # noqa: E731
    wave = t(z['wave'])[:, :case.L]
    buf = on(torch.full((GUARD + 4 + H * W * 3 + GUARD,), 0xA5, dtype=torch.uint8))
    lo = GUARD + case.shift
    img = buf[lo:lo + H * W * 3].view(H, W, 3)
    out = fn(wave, t(z['lens']), t(z['power']), t(z['nframes']), t(z['thr']), t(z['cmap']), img, min(case.cols, case.B), case.Hw,
             case.gutter, bg=BG, paper=PAPER, ink=INK)
    assert out is img
    host = buf.cpu()
    got = host[lo:lo + H * W * 3].view(H, W, 3).numpy()
    assert bool((host[:lo] == 0xA5).all()) and bool((host[lo + H * W * 3:] == 0xA5).all()), (case.name, 'guard bytes')
    bad = np.argwhere((got != want).any(2))
    assert len(bad) == 0, (case.name, pad, '%d pixels differ, the first at %r: got %r, want %r'
                           % (len(bad), tuple(bad[0]), tuple(got[tuple(bad[0])]), tuple(want[tuple(bad[0])])))
    return torch.from_numpy(got.copy())


def as_launch(render_fn, **fixed):
    """a function with ``kernels.sheet_render``'s signature around a numpy renderer (the model, a mutant of it, or an adapter)"""
    def fn(wave, lens, power, nframes, thr, cmap, img, cols, Hw, gutter, bg=BG, paper=PAPER, ink=INK):
        out = render_fn(wave.numpy(), None if lens is None else lens.numpy(), power.numpy(), nframes.numpy(), thr.numpy(),
                        cmap.numpy(), cols, Hw, gutter, bg=bg, paper=paper, ink=ink, **fixed)
        img.copy_(torch.from_numpy(np.ascontiguousarray(out)))
        return img
    return fn
