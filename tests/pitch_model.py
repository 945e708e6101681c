"""Torch-CPU fp32 models of ``audiogan_amd.kernels.pitch_frames`` and ``pitch_path_accum`` (ag_pitch_frames, ag_pitch_path_accum;
contracts in include/audiogan_hip.h), the integer statement, the case tables with the reason for each case, the input
generators, the guarded runners, the checkers against ``audio.pitch64`` / ``evaluate.pitch_path_sums64`` and the mutants the
checkers must reject  --  TEST INFRASTRUCTURE shared by tests/test_pitch.py (CPU) and tests/test_gpu_pitch.py.

Bounds.
  integer pass   samples are integers in [-3, 3] and center = 0: every r and e is an integer of at most 2304 and e0 * e(tau) at
                 most 5 308 416 < 2^24, so with a correctly rounded sqrtf and division phi is a DETERMINED fp32 value.
                 ``integer_statement`` forms it from exact integer sums, numpy float32 operation by operation; nccf, peak, lag
                 and nframes must EQUAL it bit for bit.  Path sums: whole cents in 0..40 or -1, every sum below 2^24: equal to
                 float64.
  real pass      floor = the fp32 model's own error against float64 on the same case, not below 2^-24; bound = MARGIN x floor,
                 never above CAP = 1e-4 (phi has scale 1).  The lag is checked on EVERY frame by consistency with the float64
                 phi at slack eps = the case's bound (``check_lag_consistent``).  The path's counts are exact; sum d^2 is held
                 under the same rule relative to its own size."""
import numpy as np
import torch

from audiogan_amd import align, audio, evaluate
from tests.align_model import GUARD, GUARD_VALUE, guarded

W, HOP, SEG, TMIN, TMAX, LAG0, NLAG, NCC, TILE = 256, 128, 384, 20, 127, 19, 110, 112, 8
MARGIN, CAP, FLOOR_MIN = 16.0, 1e-4, 2.0 ** -24
SENTINEL = -7          # what lag and nframes hold before a launch
SR = 8000
f32 = np.float32

FRAME_MUTANTS = ('short_segment', 'lag_shift', 'e_tau_as_e0', 'mean_over_padding', 'global_max', 'octf_ignored', 'one_sided',
                 'reads_past_n')
PATH_MUTANTS = ('hi_exclusive', 'unvoiced_as_both', 'signed_gross', 'past_m')


class Rejected(AssertionError):
    """an assertion of a checker; ``tag`` names the assertion (the mutant tests ask which one fired)"""

    def __init__(self, tag, *what):
        AssertionError.__init__(self, '%s: %r' % (tag, what))
        self.tag = tag


def need(cond, tag, *what):
    if not cond:
        raise Rejected(tag, *what)


def frames_of(n):
    n = int(n)
    return (n - W) // HOP + 1 if n >= W else 1


# ----------------------------------------------------------------------------------------------------------------------
# the fp32 model of pitch_frames
# ----------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fmaf on float32 arrays: the product of two fp32 values is exact in float64"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def _wave_mean(seg, nv):
    """the kernel's mean of one segment: lane l adds seg[l + 64 k] in ascending k, then the xor butterfly 32, 16, .. 1"""
    a = np.zeros(64, dtype=f32)
    for k in range(SEG // 64):
        a = a + seg[64 * k:64 * k + 64]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        a = a + a[lanes ^ o]
    return a[0] / f32(nv)


def select32(phi, octf, mutate=None):
    """phi [nf, 110] fp32 -> column of tau* (0: none), all comparisons in fp32"""
    mid, left, right = phi[:, 1:-1], phi[:, :-2], phi[:, 2:]
    M = mid.max(1)
    if mutate == 'global_max':
        return np.where(M > 0, mid.argmax(1) + 1, 0)
    thr = (f32(octf) * M).astype(f32)
    ok = (mid >= left) & (M[:, None] > 0)
    if mutate != 'one_sided':
        ok &= mid >= right
    if mutate != 'octf_ignored':
        ok &= mid >= thr[:, None]
    return np.where(ok.any(1), ok.argmax(1) + 1, 0)


def phi32(seg, mutate=None):
    """seg [nf, 384] fp32 -> (phi [nf, 110], e0 [nf]): one fmaf chain per (frame, lag) in ascending t"""
    nf = seg.shape[0]
    first = LAG0 + (1 if mutate == 'lag_shift' else 0)
    pad = np.concatenate([seg, np.zeros((nf, 1), dtype=f32)], 1)          # (the shifted table's last lag reaches one further)
    idx = np.arange(NLAG)[:, None] + first
    r, e = np.zeros((nf, NLAG), dtype=f32), np.zeros((nf, NLAG), dtype=f32)
    e0 = np.zeros(nf, dtype=f32)
    for t in range(W - (1 if mutate == 'short_segment' else 0)):
        a, v = seg[:, t], pad[:, (idx + t)[:, 0]]
        e0 = _fma(a, a, e0)
        r = _fma(a[:, None], v, r)
        e = _fma(v, v, e)
    if mutate == 'e_tau_as_e0':
        e = np.repeat(e0[:, None], NLAG, 1)
    den = (e0[:, None] * e).astype(f32)
    with np.errstate(divide='ignore', invalid='ignore'):
        phi = np.where(den > 0, r / np.sqrt(den), f32(0)).astype(f32)
    return phi, e0


def pitch_frames(x, lens, octf=0.9, center=True, lag=None, peak=None, nccf=None, nframes=None, mutate=None):
    """the launch's contract on CPU tensors: writes rows j < nframes[b] of lag, peak (and nccf) and nothing else; reads nothing
    at or past the lengths"""
    assert x.dtype == torch.float32 and x.dim() == 2 and (x.size(1) == 1 or x.stride(1) == 1)
    if not 0.0 < float(f32(octf)) <= 1.0:
        raise ValueError('ag_pitch_frames: octf %g is outside (0, 1]' % octf)
    B, L = x.shape
    F = frames_of(L)
    lag = torch.empty(B, F, dtype=torch.int32) if lag is None else lag
    peak = torch.empty(B, F, 4) if peak is None else peak
    assert lag.dtype == torch.int32 and tuple(lag.shape) == (B, F) and tuple(peak.shape) == (B, F, 4)
    assert nccf is None or tuple(nccf.shape) == (B, F, NCC)
    xs = x.detach().numpy()
    for b in range(B):
        n = L if lens is None else max(0, min(int(lens[b]), L))
        nf = frames_of(n)
        if nframes is not None:
            nframes[b] = nf
        buf = np.zeros((nf - 1) * HOP + SEG, dtype=f32)
        m = min(len(buf), L if mutate == 'reads_past_n' else n)
        buf[:m] = xs[b, :m]
        seg = buf[np.arange(nf)[:, None] * HOP + np.arange(SEG)[None, :]]
        if center:
            for j in range(nf):
                nv = max(0, min(n - j * HOP, SEG))
                if nv > 0:
                    mean = _wave_mean(seg[j], SEG if mutate == 'mean_over_padding' else nv)
                    seg[j, :nv] = seg[j, :nv] - mean
        phi, e0 = phi32(seg, mutate)
        col = select32(phi, octf, mutate)
        rows, found = np.arange(nf), col > 0
        lag[b, :nf] = torch.from_numpy(np.where(found, col + LAG0, 0).astype(np.int32))
        pk = np.zeros((nf, 4), dtype=f32)
        for d in range(3):
            pk[:, d] = np.where(found, phi[rows, np.clip(col - 1 + d, 0, NLAG - 1)], f32(0))
        pk[:, 3] = e0 * f32(1.0 / W)
        peak[b, :nf] = torch.from_numpy(pk)
        if nccf is not None:
            nccf[b, :nf, :NLAG] = torch.from_numpy(phi)
            nccf[b, :nf, NLAG:] = 0.0
    return lag, peak


def integer_statement(x, lens, octf=0.9):
    """center = 0 on integer samples: (lag [B, F] int32, peak [B, F, 4] fp32, nccf [B, F, 112] fp32, nframes) from EXACT integer
    sums; den = e0 * e(tau) < 2^24 is exact, sqrt and the division are numpy float32's (correctly rounded).  Rows at or past
    the frame counts hold SENTINEL / NaN: never compared"""
    x = np.asarray(x)
    B, L = x.shape
    F = frames_of(L)
    lag = np.full((B, F), SENTINEL, dtype=np.int32)
    peak, nccf = np.full((B, F, 4), np.nan, dtype=f32), np.full((B, F, NCC), np.nan, dtype=f32)
    nframes = np.zeros(B, dtype=np.int32)
    for b in range(B):
        n = L if lens is None else max(0, min(int(lens[b]), L))
        nf = nframes[b] = frames_of(n)
        buf = np.zeros((nf - 1) * HOP + SEG, dtype=np.int64)
        m = min(n, len(buf))
        vals = x[b, :m]
        assert (vals == np.round(vals)).all() and (np.abs(vals) <= 3).all()
        buf[:m] = vals.astype(np.int64)
        seg = buf[np.arange(nf)[:, None] * HOP + np.arange(SEG)[None, :]]
        head = seg[:, :W]
        e0 = (head * head).sum(1)
        r = np.stack([(head * seg[:, LAG0 + k:LAG0 + k + W]).sum(1) for k in range(NLAG)], 1)
        e = np.stack([(seg[:, LAG0 + k:LAG0 + k + W] ** 2).sum(1) for k in range(NLAG)], 1)
        den = e0[:, None] * e
        assert den.max() < 2 ** 24 and np.abs(r).max() <= 2304
        with np.errstate(divide='ignore', invalid='ignore'):
            phi = np.where(den > 0, r.astype(f32) / np.sqrt(den.astype(f32)), f32(0)).astype(f32)
        col = select32(phi, octf)
        rows, found = np.arange(nf), col > 0
        lag[b, :nf] = np.where(found, col + LAG0, 0)
        for d in range(3):
            peak[b, :nf, d] = np.where(found, phi[rows, np.clip(col - 1 + d, 0, NLAG - 1)], f32(0))
        peak[b, :nf, 3] = e0.astype(f32) * f32(1.0 / W)
        nccf[b, :nf, :NLAG] = phi
        nccf[b, :nf, NLAG:] = 0
    return lag, peak, nccf, nframes


# ----------------------------------------------------------------------------------------------------------------------
# the fp32 model of pitch_path_accum: the kernel's own order (thread t: columns t, t + 256, ..; butterfly; waves ascending)
# ----------------------------------------------------------------------------------------------------------------------
def pitch_path_accum(pc_a, pc_b, lo, hi, nf_b=None, gross=None, out=None, mutate=None):
    assert pc_a.dtype == pc_b.dtype == torch.float32 and pc_a.dim() == pc_b.dim() == 2
    B, Fa, Fb = pc_a.size(0), pc_a.size(1), pc_b.size(1)
    assert 1 <= Fa <= 1024 and 1 <= Fb <= 1024 and lo.dtype == hi.dtype == torch.int32
    assert tuple(lo.shape) == tuple(hi.shape) == (B, Fb) and pc_b.size(0) == B
    out = torch.empty(B, 5) if out is None else out
    g = f32(1200.0 * np.log2(1.2) if gross is None else gross)
    A, Bc, lo_, hi_ = pc_a.numpy(), pc_b.numpy(), lo.numpy(), hi.numpy()
    lanes = np.arange(64)
    for b in range(B):
        m = Fb if nf_b is None else max(1, min(int(nf_b[b]), Fb))
        if mutate == 'past_m':
            m = Fb
        ss = np.zeros(256, dtype=f32)
        counts = np.zeros(4, dtype=np.int64)
        for j in range(m):
            r0, r1 = (max(0, min(int(v), Fa - 1)) for v in (lo_[b, j], hi_[b, j]))
            if mutate == 'hi_exclusive':
                r1 -= 1
            vb = Bc[b, j]
            cs = f32(0)
            for i in range(r0, r1 + 1):
                va = A[b, i]
                oa, ob = bool(va >= 0), bool(vb >= 0)
                counts[0] += 1
                counts[2] += oa != ob
                if (oa and ob) or mutate == 'unvoiced_as_both':
                    d = f32(va - vb)
                    counts[1] += 1
                    counts[3] += bool((d if mutate == 'signed_gross' else abs(d)) > g)
                    cs = f32(np.float64(d) * np.float64(d) + np.float64(cs))
            ss[j % 256] = ss[j % 256] + cs
        tot = f32(0)
        for w in range(4):
            a = ss[64 * w:64 * w + 64].copy()
            for o in (32, 16, 8, 4, 2, 1):
                a = a + a[lanes ^ o]
            tot = tot + a[0]
        out[b] = torch.tensor([float(c) for c in counts] + [float(tot)])
    return out


def install(monkeypatch):
    """after ``dtwalign_model.install``: the models in place of kernels.pitch_frames and kernels.pitch_path_accum"""
    import audiogan_amd.kernels as K
    for name, fn in (('pitch_frames', pitch_frames), ('pitch_path_accum', pitch_path_accum)):
        assert hasattr(K, name), 'pitch model has %s but audiogan_amd.kernels does not' % name
        monkeypatch.setattr(K, name, fn)


# ----------------------------------------------------------------------------------------------------------------------
# pitch_frames: inputs
# ----------------------------------------------------------------------------------------------------------------------
TONES_HZ = (70.0, 100.0, 133.0, 150.0, 220.0, 310.0, 390.0)
TONE_LAGS = (114, 80, 60, 53, 36, 26, 21)          # what audio.pitch64 gives (tests/test_pitch.py asserts it first)
TONE_SNR_DB = (40.0, 10.0)
TONE_DC, TONE_RMS, TONE_TOP_HZ = 0.3, 0.2, 3800.0


def harmonic(f0, n, snr_db=40.0, seed=0, dc=TONE_DC, switch_to=None):
    """float32 [n]: harmonics k f0 up to 3.8 kHz with amplitudes 1 / k (the envelope depends on the harmonic's NUMBER, so a
    tone at another pitch has the same one) and phases 0.7 k, at rms 0.2, on a DC offset, white noise ``snr_db`` below the
    tone.  ``switch_to``: the pitch of the second half"""
    t = np.arange(n) / float(SR)

    def wave(f):
        ks = np.arange(1, int(TONE_TOP_HZ // f) + 1)
        y = sum(np.sin(2 * np.pi * k * f * t + 0.7 * k) / k for k in ks)
        return y / np.sqrt(np.mean(y * y)) * TONE_RMS
    y = wave(f0)
    if switch_to is not None:
        y = np.where(np.arange(n) < n // 2, y, wave(switch_to))
    noise = TONE_RMS * 10.0 ** (-snr_db / 20.0) * np.random.RandomState(seed).randn(n)
    return (y + dc + noise).astype(f32)


def integer_row(kind, n, rs):
    """integers in [-3, 3]: 'random'; 'inside' - a random pattern repeated with period 37 (inside 20..127); 'below' - period
    10 (its multiples 20, 30, .. tie at phi = 1: the smallest wins); 'above' - a square wave of period 200 (phi falls from lag
    0 to lag 100: the strongest lag of 20..127 is 20, at the range's edge and no local maximum: lag 0)"""
    if kind == 'random':
        return rs.randint(-3, 4, size=n).astype(f32)
    if kind == 'above':
        return np.where((np.arange(n) // 100) % 2 == 0, 3, -3).astype(f32)
    period = dict(inside=37, below=10)[kind]
    return np.tile(rs.randint(-3, 4, size=period), n // period + 1)[:n].astype(f32)


INTEGER_KINDS = ('random', 'inside', 'below', 'above')
REAL_KINDS = ('tone', 'randn', 'switch')

# name -> B, L, lens (None: whole rows), pad (row pitch - L), off (floats the base is displaced by), nccf, octf, staging.  Why:
#   n_*          n_b in 0, 1, 255 | 256, 257, 383 | 384, 385, 511 | 512, 640: the frame count changes at 256 and 384 and the
#                384-sample segment is cut by the clip's end in every way; L = 704 is above every n_b (a ragged minibatch)
#   whole_rows   lens = None, B 1
#   tile_*       8 frames (one tile exactly), 9 (one more), 63 at L 8192 (several tiles, B 2; the second row ends mid-tile)
#   pitch_*      a row pitch above L: a multiple of 4 floats keeps the 16-byte loads, L + 3 takes the scalar staging
#   off_*        a base displaced by 1..3 floats: scalar staging
#   no_nccf      nccf absent
#   octf_one     octf = 1.0: only a lag that attains the maximum qualifies
FRAME_CASES = dict(
    n_0_1_255=dict(B=3, L=704, lens=(0, 1, 255)),
    n_256_257_383=dict(B=3, L=704, lens=(256, 257, 383)),
    n_384_385_511=dict(B=3, L=704, lens=(384, 385, 511)),
    n_512_640=dict(B=3, L=704, lens=(512, 640, 300)),
    whole_rows=dict(B=1, L=640, lens=None),
    tile_exact=dict(B=1, L=1152, lens=None),
    tile_plus_one=dict(B=3, L=1280, lens=(1280, 1152, 1279)),
    tiles_many=dict(B=2, L=8192, lens=(8192, 5000)),
    pitch_vector=dict(B=3, L=704, lens=(640, 385, 704), pad=4),
    pitch_scalar=dict(B=3, L=704, lens=(640, 385, 704), pad=3, staging='scalar'),
    off_1=dict(B=1, L=704, lens=(641,), off=1, staging='scalar'),
    off_2=dict(B=3, L=704, lens=(511, 704, 130), off=2, staging='scalar'),
    off_3=dict(B=3, L=704, lens=(384, 700, 257), off=3, pad=1, staging='scalar'),
    no_nccf=dict(B=3, L=704, lens=(511, 640, 257), nccf=False),
    octf_one=dict(B=3, L=704, lens=(704, 640, 400), octf=1.0),
)
# the special clips, one row each at L = 704 (4 frames): all zero (phi = 0, lag 0); the constant 0.5 with center = 1 (every
# centred sample is EXACTLY 0: partial sums of 0.5 and their quotient by the count are exact in fp32 and float64 - a constant
# like 0.3 would leave rounding residue with phi near 1); a 40 Hz sine with center = 1 (period 200 > 127: phi falls over
# 20..100, so the strongest lag is 20, at the range's edge and no local maximum -> lag 0)
SPECIAL = ('zeros', 'constant', 'edge')


def case_rows(name, kind_pass, seed=0):
    """-> (rows float32 [B, L], n per row): the data of a case in the 'integer' or the 'real' pass, NaN at and past n_b"""
    c = FRAME_CASES[name]
    B, L = c['B'], c['L']
    lens = [L] * B if c.get('lens') is None else list(c['lens'])
    rs = np.random.RandomState(1000 + seed + sum(ord(ch) for ch in name))
    rows = np.full((B, L), np.nan, dtype=f32)
    for b, n in enumerate(lens):
        if n == 0:
            continue
        if kind_pass == 'integer':
            rows[b, :n] = integer_row(INTEGER_KINDS[(b + len(name)) % 4], n, rs)
        else:
            kind = REAL_KINDS[(b + len(name)) % 3]
            f0 = TONES_HZ[(b + len(name)) % 7]
            if kind == 'randn':
                rows[b, :n] = rs.randn(n).astype(f32)
            else:
                rows[b, :n] = harmonic(f0, n, snr_db=TONE_SNR_DB[b % 2], seed=seed + b,
                                       switch_to=1.3 * f0 if kind == 'switch' else None)
    return rows, lens


def special_rows(which):
    n = 704
    if which == 'zeros':
        return np.zeros((1, n), dtype=f32)
    if which == 'constant':
        return np.full((1, n), 0.5, dtype=f32)
    return (0.25 * np.sin(2 * np.pi * 40.0 * np.arange(n) / SR))[None, :].astype(f32)


def tone_rows(n=4096):
    """the seven tones at both noise levels: [14, n], row 2 i + s is tone i at TONE_SNR_DB[s]"""
    return np.stack([harmonic(f, n, snr_db=s, seed=10 * i + k) for i, f in enumerate(TONES_HZ) for k, s in enumerate(TONE_SNR_DB)])


# ----------------------------------------------------------------------------------------------------------------------
# pitch_frames: the guarded runner
# ----------------------------------------------------------------------------------------------------------------------
def planned_staging(x):
    """the launcher's rule, restated: 16-byte loads need a 16-byte aligned base and a row pitch that is a multiple of 4"""
    ld = x.stride(0) if x.size(0) > 1 else max(x.stride(0), x.size(1))
    return 'vector' if x.data_ptr() % 16 == 0 and ld % 4 == 0 else 'scalar'


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def run_frames(fn, rows, lens, on=lambda t: t, pad=0, off=0, nccf=True, octf=0.9, center=True, staging='vector', kernel_name=None,
               **kw):
    """one case, twice.  ``rows`` [B, L] goes into a NaN buffer at row pitch L + pad, displaced by ``off`` floats; every output
    is NaN / SENTINEL filled between guards.  Afterwards: the two runs have the same bits everywhere, the guards are intact,
    rows at and past the frame counts are untouched, the staging path is the planned one (``kernel_name()``: the name the
    library reported, where there is one).  -> dict(lag, peak, nccf, nframes) numpy, and ``n`` per row"""
    B, L = rows.shape
    F, ld = frames_of(L), L + pad
    flat = torch.full((off + B * ld + 4,), float('nan'))
    flat[off:off + B * ld].view(B, ld)[:, :L] = torch.from_numpy(rows)
    flat = on(flat)
    x = flat[off:off + B * ld].view(B, ld)[:, :L]
    need(planned_staging(x) == staging, 'staging', planned_staging(x), staging)
    n = [L] * B if lens is None else [max(0, min(int(v), L)) for v in lens]
    lens_t = None if lens is None else on(torch.tensor(list(lens), dtype=torch.int64))
    runs = []
    for _ in range(2):
        bufs = dict(lag=guarded((B, F), dtype=torch.int32, fill=SENTINEL, on=on), peak=guarded((B, F, 4), on=on),
                    nframes=guarded((B,), dtype=torch.int32, fill=SENTINEL, on=on))
        if nccf:
            bufs['nccf'] = guarded((B, F, NCC), on=on)
        got = fn(x, lens_t, octf=octf, center=center, lag=bufs['lag'][1], peak=bufs['peak'][1],
                 nccf=bufs['nccf'][1] if nccf else None, nframes=bufs['nframes'][1], **kw)
        need(got[0] is bufs['lag'][1] and got[1] is bufs['peak'][1], 'returns')
        if kernel_name is not None:
            need(kernel_name() == 'pitch_frames_kernel<%d>' % (staging == 'vector'), 'kernel_name', kernel_name(), staging)
        runs.append({k: v[0].detach().cpu() for k, v in bufs.items()})
    for k in runs[0]:
        need(torch.equal(_bits(runs[0][k]), _bits(runs[1][k])), 'two_runs', k)
        g = runs[0][k]
        need(bool((g[:GUARD] == GUARD_VALUE).all() and (g[-GUARD:] == GUARD_VALUE).all()), 'guard', k)
    out = {k: v[GUARD:-GUARD].numpy() for k, v in runs[0].items()}
    out['lag'], out['peak'] = out['lag'].reshape(B, F), out['peak'].reshape(B, F, 4)
    out['nccf'] = out['nccf'].reshape(B, F, NCC) if nccf else None
    for b in range(B):
        nf = frames_of(n[b])
        need(out['nframes'][b] == nf, 'nframes', b, out['nframes'][b], nf)
        need(bool((out['lag'][b, nf:] == SENTINEL).all() and np.isnan(out['peak'][b, nf:]).all()), 'unwritten', b)
        need(out['nccf'] is None or bool(np.isnan(out['nccf'][b, nf:]).all()), 'unwritten', b)
    return out, n


# ----------------------------------------------------------------------------------------------------------------------
# pitch_frames: the checkers
# ----------------------------------------------------------------------------------------------------------------------
def check_integer(out, n, rows, octf=0.9):
    """bit for bit against the integer statement, on every frame that exists"""
    lens = np.asarray(n)
    want_lag, want_peak, want_nccf, want_nf = integer_statement(np.nan_to_num(rows), lens, octf)
    for b in range(len(n)):
        nf = int(want_nf[b])
        if out['nccf'] is not None:
            need(np.array_equal(out['nccf'][b, :nf].view(np.int32), want_nccf[b, :nf].view(np.int32)), 'nccf', b)
        need(np.array_equal(out['peak'][b, :nf, 3].view(np.int32), want_peak[b, :nf, 3].view(np.int32)), 'power', b)
        need(np.array_equal(out['lag'][b, :nf], want_lag[b, :nf]), 'lag', b, out['lag'][b, :nf], want_lag[b, :nf])
        need(np.array_equal(out['peak'][b, :nf, :3].view(np.int32), want_peak[b, :nf, :3].view(np.int32)), 'peak', b)


def check_lag_consistent(lag, phi64, octf, eps):
    """one frame: the returned tau* against the float64 phi [110] (lags 19..128) at slack eps.  The rule (ag_pitch_frames in
    include/audiogan_hip.h): tau* is the smallest tau in 20..127 with phi(tau) >= phi(tau - 1), phi(tau) >= phi(tau + 1) and
    phi(tau) >= octf * M, M the largest phi of 20..127; 0 when M <= 0 or none qualifies.  Accepted: a tau* != 0 that meets the
    three conditions with eps of slack each, while no smaller tau meets all three with more than eps to spare; tau* = 0 only
    if no tau meets them with more than eps to spare"""
    octf = float(f32(octf))
    mid, left, right = phi64[1:-1], phi64[:-2], phi64[2:]
    M = mid.max()
    sure = (mid >= left + eps) & (mid >= right + eps) & (mid >= octf * M + eps) & (M > eps)
    first_sure = int(np.argmax(sure)) + TMIN if sure.any() else None
    if lag == 0:
        need(first_sure is None, 'lag', 0, first_sure)
        return
    need(TMIN <= lag <= TMAX, 'lag', lag)
    c = lag - LAG0
    need(phi64[c] >= phi64[c - 1] - eps and phi64[c] >= phi64[c + 1] - eps and phi64[c] >= octf * M - eps and M > -eps,
         'lag', lag, phi64[c - 1:c + 2], M)
    need(first_sure is None or first_sure >= lag, 'lag', lag, first_sure)


def real_errors(out, n, rows, octf=0.9, center=True):
    """the errors of one run against audio.pitch64 -> (err of nccf, err of power relative to its scale); also returns the
    float64 outputs"""
    lens = np.asarray(n)
    ref = audio.pitch64(np.nan_to_num(rows.astype(np.float64)), lens, octf=octf, center=center)
    e_phi = e_pow = 0.0
    for b in range(len(n)):
        nf = int(ref[3][b])
        if out['nccf'] is not None:
            d = np.abs(out['nccf'][b, :nf].astype(np.float64) - ref[2][b, :nf])
            e_phi = max(e_phi, float(d.max()) if np.isfinite(d).all() else float('inf'))
        scale = max(float(ref[1][b, :nf, 3].max()), 1e-30)
        d = np.abs(out['peak'][b, :nf, 3].astype(np.float64) - ref[1][b, :nf, 3]) / scale
        e_pow = max(e_pow, float(d.max()) if np.isfinite(d).all() else float('inf'))
    return e_phi, e_pow, ref


def check_real(out, n, rows, floor_out, octf=0.9, center=True, expect_lag=None):
    """``out`` against float64 under the bound rule, ``floor_out`` being the fp32 model's outputs on the same case (both with
    nccf).  -> dict(phi=err / floor, power=err / floor): the measured ratios"""
    f_phi, f_pow, ref = real_errors(floor_out, n, rows, octf, center)
    e_phi, e_pow, _ = real_errors(out, n, rows, octf, center)
    f_phi, f_pow = max(f_phi, FLOOR_MIN), max(f_pow, FLOOR_MIN)
    b_phi, b_pow = min(MARGIN * f_phi, CAP), min(MARGIN * f_pow, CAP)
    need(e_phi <= b_phi, 'nccf', e_phi, b_phi)
    need(e_pow <= b_pow, 'power', e_pow, b_pow)
    for b in range(len(n)):
        nf = int(ref[3][b])
        for j in range(nf):
            lag = int(out['lag'][b, j])
            phi64 = ref[2][b, j, :NLAG]
            if expect_lag is not None:
                need(abs(lag - expect_lag[b]) <= expect_lag.get('slack', {}).get(b, 0), 'lag_expected', b, j, lag, expect_lag[b])
            check_lag_consistent(lag, phi64, octf, b_phi)
            want = phi64[lag - LAG0 - 1:lag - LAG0 + 2] if lag else np.zeros(3)
            d = np.abs(out['peak'][b, j, :3].astype(np.float64) - want)
            need(np.isfinite(d).all() and d.max() <= b_phi, 'peak', b, j, d.max(), b_phi)
    return dict(phi=e_phi / f_phi, power=e_pow / f_pow)


TONE_SLACK_ROWS = (1, 13)          # 70 Hz and 390 Hz at 10 dB


def tone_expectation():
    """row -> expected lag of ``tone_rows``; 'slack': rows where a frame may be one lag off.  Every row has its lag outright in
    every frame, at 40 dB and at 10 dB, but two: 70 Hz and 390 Hz at 10 dB, where ``audio.pitch64`` ITSELF gives either
    neighbour frame by frame (114 in 28 frames and 115 in 3; 21 in 18 frames and 20 in 13 - tests/test_pitch.py asserts that
    it varies there and nowhere else).  The periods, 8000 / 70 = 114.29 and 8000 / 390 = 20.51, fall between two lags, and
    at 10 dB the noise moves phi by about 0.04 a lag (sqrt(2 (2 s^2 n^2 + n^4)) / (16 (s^2 + n^2)) with n^2 = 0.1 s^2), more
    than phi differs between the two neighbours.  There the assertion is 'within one lag' - still no octave error, which is
    what the rule is for"""
    e = {2 * i + k: TONE_LAGS[i] for i in range(len(TONES_HZ)) for k in range(2)}
    e['slack'] = {r: 1 for r in TONE_SLACK_ROWS}
    return e


# ----------------------------------------------------------------------------------------------------------------------
# pitch_path_accum: cases, runner, checkers
# ----------------------------------------------------------------------------------------------------------------------
def random_path(n, m, rs):
    """a path from (0, 0) to (n-1, m-1) in steps (1, 0), (0, 1), (1, 1) -> (lo [m], hi [m])"""
    i = j = 0
    lo, hi = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
    while (i, j) != (n - 1, m - 1):
        moves = [mv for mv in ((1, 1), (1, 0), (0, 1)) if i + mv[0] < n and j + mv[1] < m]
        di, dj = moves[rs.randint(len(moves))]
        if dj:
            hi[j] = i
            lo[j + 1] = i + di
        i, j = i + di, j + dj
    hi[m - 1] = n - 1
    return lo, hi


# name -> B, Fa, Fb, pairs (n, m) per row, path kind, voicing per row.  Why:
#   Fb 1, 2, 65, 257, 1024   one column; two; past one wave; past one round of the 256 threads; the capacity (four rounds)
#   vertical     m = 1, lo = 0, hi = n - 1: every cell in one column's chain;  horizontal: n = 1, one cell a column
#   diagonal     lo = hi = j;  path64: the path of align.path64 on random cepstra;  random: a random monotone path
#   m below Fb   everywhere but 'whole': lo / hi past m hold out-of-range integers and pc_b NaN, never to be read
#   voicing      'unvoiced' / 'voiced' / 'alternating' / 'random' on both sides
#   whole        nf_b = None
PATH_CASES = dict(
    one_column=dict(B=1, Fa=5, Fb=1, pairs=((5, 1),), path='vertical', voicing=('random',)),
    vertical=dict(B=3, Fa=40, Fb=2, pairs=((40, 1), (7, 1), (1, 1)), path='vertical', voicing=('voiced', 'alternating', 'unvoiced')),
    horizontal=dict(B=3, Fa=3, Fb=65, pairs=((1, 64), (1, 30), (1, 1)), path='horizontal', voicing=('alternating', 'voiced', 'random')),
    diagonal=dict(B=3, Fa=257, Fb=257, pairs=((256, 256), (100, 100), (65, 65)), path='diagonal',
                  voicing=('random', 'unvoiced', 'voiced')),
    path64=dict(B=3, Fa=40, Fb=65, pairs=((33, 64), (40, 17), (5, 9)), path='path64', voicing=('random', 'voiced', 'alternating')),
    capacity=dict(B=1, Fa=1024, Fb=1024, pairs=((1024, 1000),), path='random', voicing=('random',)),
    whole=dict(B=3, Fa=20, Fb=2, pairs=((20, 2), (9, 2), (2, 2)), path='random', voicing=('random', 'voiced', 'random'), whole=True),
)


def path_case(name, kind_pass, seed=0):
    """-> dict(pc_a, pc_b, lo, hi, nf_b, gross, pairs): CPU tensors.  'integer': whole cents in 0..40 or -1, gross = 10 (a
    difference of exactly 10 is NOT gross); 'real': cents uniform in 400..4000 or -1, gross = the default"""
    c = PATH_CASES[name]
    B, Fa, Fb = c['B'], c['Fa'], c['Fb']
    rs = np.random.RandomState(77 + seed + sum(ord(ch) for ch in name))
    pc_a, pc_b = np.full((B, Fa), np.nan, dtype=f32), np.full((B, Fb), np.nan, dtype=f32)
    lo, hi = np.full((B, Fb), -(1 << 20), dtype=np.int32), np.full((B, Fb), 1 << 20, dtype=np.int32)          # (past m)

    def cents(k, voicing):
        v = rs.randint(0, 41, size=k).astype(f32) if kind_pass == 'integer' else rs.uniform(400.0, 4000.0, size=k).astype(f32)
        on = dict(unvoiced=np.zeros(k, bool), voiced=np.ones(k, bool), alternating=np.arange(k) % 2 == 0,
                  random=rs.rand(k) < 0.7)[voicing]
        return np.where(on, v, f32(-1))
    for b, (n, m) in enumerate(c['pairs']):
        pc_a[b, :n], pc_b[b, :m] = cents(n, c['voicing'][b]), cents(m, c['voicing'][b])
        if c['path'] == 'vertical':
            l, h = np.zeros(1, dtype=np.int64), np.full(1, n - 1)
        elif c['path'] == 'horizontal':
            l, h = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
        elif c['path'] == 'diagonal':
            l = h = np.arange(m)
        elif c['path'] == 'path64':
            _, l, h = align.path64(np.pad(rs.randn(n, 12), ((0, 0), (1, 3))), n, np.pad(rs.randn(m, 12), ((0, 0), (1, 3))), m)
        else:
            l, h = random_path(n, m, rs)
        lo[b, :m], hi[b, :m] = l, h
    nf_b = None if c.get('whole') else torch.tensor([m for _, m in c['pairs']], dtype=torch.int32)
    return dict(pc_a=torch.from_numpy(pc_a), pc_b=torch.from_numpy(pc_b), lo=torch.from_numpy(lo), hi=torch.from_numpy(hi),
                nf_b=nf_b, gross=10.0 if kind_pass == 'integer' else None, pairs=c['pairs'])


def gross_edge_case():
    """a difference exactly at gross and one fp32 step either side of it (b = 0 is voiced: not negative), on a diagonal path:
    only the step above counts"""
    g = f32(1200.0 * np.log2(1.2))
    a = np.array([[g, np.nextafter(g, f32(np.inf)), np.nextafter(g, f32(0))]], dtype=f32)
    z = torch.zeros(1, 3)
    idx = torch.arange(3, dtype=torch.int32)[None, :].clone()
    return dict(pc_a=torch.from_numpy(a), pc_b=z, lo=idx, hi=idx.clone(), nf_b=torch.tensor([3], dtype=torch.int32), gross=None,
                pairs=((3, 3),))


def run_path(fn, case, on=lambda t: t, **kw):
    """twice, into a NaN-filled guarded output -> float64 numpy [B, 5]"""
    B = case['pc_a'].size(0)
    args = [on(case[k]) for k in ('pc_a', 'pc_b', 'lo', 'hi')]
    nf_b = None if case['nf_b'] is None else on(case['nf_b'])
    runs = []
    for _ in range(2):
        flat, out = guarded((B, 5), on=on)
        need(fn(*args, nf_b=nf_b, gross=case['gross'], out=out, **kw) is out, 'returns')
        runs.append(flat.detach().cpu())
    need(torch.equal(_bits(runs[0]), _bits(runs[1])), 'two_runs')
    g = runs[0]
    need(bool((g[:GUARD] == GUARD_VALUE).all() and (g[-GUARD:] == GUARD_VALUE).all()), 'guard')
    return g[GUARD:-GUARD].view(B, 5).double().numpy()


def check_path(got, case, floor_got=None):
    """counts exact; sum d^2 equal to float64 (``floor_got`` None: the integer pass) or within MARGIN x floor of it relative to
    its size.  -> the measured err / floor"""
    want = evaluate.pitch_path_sums64(case['pc_a'], case['pc_b'], case['lo'], case['hi'], case['nf_b'], case['gross'])
    for k, tag in enumerate(('cells', 'both', 'differ', 'gross')):
        need(np.array_equal(got[:, k], want[:, k]), tag, got[:, k], want[:, k])
    if floor_got is None:
        assert want[:, 4].max() < 2 ** 24
        need(np.array_equal(got[:, 4], want[:, 4]), 'ssq', got[:, 4], want[:, 4])
        return 0.0
    scale = np.maximum(want[:, 4], 1e-30)
    floor = max(float((np.abs(floor_got[:, 4] - want[:, 4]) / scale).max()), FLOOR_MIN)
    err = float((np.abs(got[:, 4] - want[:, 4]) / scale).max())
    need(err <= MARGIN * floor, 'ssq', err, floor)
    return err / floor


# ----------------------------------------------------------------------------------------------------------------------
# the property pair: a tone and the same tone at 1.25 x the pitch, same envelope
# ----------------------------------------------------------------------------------------------------------------------
PROPERTY_HZ, PROPERTY_RATIO, PROPERTY_N = 120.0, 1.25, 4096
PROPERTY_CENTS = 1200.0 * np.log2(PROPERTY_RATIO)          # 386.3


def property_pair():
    """float32 [2, n], [2, n]: rows (tone, tone) against (tone at 1.25 x, the same tone): the second pair is the control"""
    a = harmonic(PROPERTY_HZ, PROPERTY_N, seed=1)
    b = harmonic(PROPERTY_HZ * PROPERTY_RATIO, PROPERTY_N, seed=2)
    return np.stack([a, a]), np.stack([b, harmonic(PROPERTY_HZ, PROPERTY_N, seed=3)])


def pitch_distance64(wave_a, wave_b):
    """the float64 path of evaluate.pitch_distance: align_model.melcep64, align.path64, audio.pitch64, pitch_cents and
    pitch_path_sums64 -> (dict of [B] float64 tensors, aligned distance in dB [B])"""
    from tests import align_model
    B = wave_a.shape[0]
    sums, mcd = np.zeros((B, 5)), np.zeros(B)
    pad = lambda c: np.concatenate([c, np.zeros((len(c), 16 - c.shape[1]))], 1)          # noqa: E731
    for b in range(B):
        cents = []
        ceps = []
        for w in (wave_a[b:b + 1], wave_b[b:b + 1]):
            lag, peak, _, _ = audio.pitch64(w)
            cents.append(evaluate.pitch_cents(torch.from_numpy(lag), torch.from_numpy(peak)))
            ceps.append(pad(align_model.melcep64(w, [w.shape[1]])[0][1]))
        total, lo, hi = align.path64(ceps[0], len(ceps[0]), ceps[1], len(ceps[1]))
        sums[b] = evaluate.pitch_path_sums64(cents[0], cents[1], lo[None, :].astype(np.int32), hi[None, :].astype(np.int32))[0]
        mcd[b] = evaluate.MCD_DB * total / (len(ceps[0]) + len(ceps[1]))
    return evaluate.pitch_scores(sums), mcd
