"""Torch-CPU models of the aligned-distance kernels of ``audiogan_amd.kernels`` (ag_melcep_frames, ag_dtw_cost; contracts in
include/audiogan_hip.h), their float64 restatements, the shared test inputs and the checkers  --  TEST INFRASTRUCTURE,
installed after ``kernel_model.install`` and ``eval_model.install``.

Bounds.
  power      per frame |P - P64| <= eval_model.LTAS_BOUND (2e-5) of that frame's largest bin, P64 from np.fft.rfft.
  cepstra    the rule of tests/recurrent_cases.py: FLOOR = the error of the fp32 torch model of the step against float64, per
             clip as a fraction of the clip's largest |c|, the largest over the case's clips, not below 2^-24 (no fp32 value
             is closer to a float64 one than the rounding of its own store); bound = CEP_MARGIN * floor.
  dtw        integer inputs: bit for bit (every partial sum is an integer below 2^24).  Real inputs:
             |D32 - D64| <= (n + m + 16) 2^-23 D64 - min is 1-Lipschitz and every term is positive, so a path's total carries
             one rounding (2^-24 relative) per addition, at most n + m - 1 of them, and each local cost its own few: 12
             squares and sums under a square root halve, the 16 is room for them; the factor 2 (2^-23) covers the float64
             minimum path differing from the fp32 one."""
import numpy as np
import torch

from tests import eval_model
from tests.eval_model import BINS, LTAS_BOUND, frame_count

BANDS, NCEP, CEPW = 24, 13, 16
LOG_FLOOR = 1e-10
FLOOR_MIN = 2.0 ** -24
# margin over the fp32 model's own error.  16, the rule's default: the kernel differs from the model in the order of its
# sums only (fma chains in ascending index against torch's blocked sums), which the recurrent cases show costs a few floors
CEP_MARGIN = 16.0
DTW_MAX = 1024


def tables():
    """(mel [24, 129], dct [13, 24]) fp32 on the CPU - the product's own values"""
    import audiogan_amd.kernels as K
    return K.mel_table(device='cpu'), K.dct_table(device='cpu')


def _clamp_len(lens, b, L):
    return L if lens is None else max(0, min(int(lens[b]), L))


# ----------------------------------------------------------------------------------------------------------------------
# melcep_frames: fp32 model and float64 restatements
# ----------------------------------------------------------------------------------------------------------------------
def cep_from_power(P, mel, dct):
    """[.., 129] -> [.., 13] in P's dtype (the tables are converted to it)"""
    E = P @ mel.to(P.dtype).t()
    return torch.log(E + torch.tensor(LOG_FLOOR, dtype=torch.float32).to(P.dtype)) @ dct.to(P.dtype).t()


def melcep_frames(x, lens, mel=None, dct=None, cep=None, nframes=None, power=None):
    assert x.dtype == torch.float32 and x.dim() == 2 and (x.size(1) == 1 or x.stride(1) == 1)
    B, L = x.shape
    F = frame_count(L)
    tm, td = tables()
    mel, dct = tm if mel is None else mel, td if dct is None else dct
    if cep is None:
        cep = torch.empty(B, F, CEPW)
    assert tuple(cep.shape) == (B, F, CEPW) and cep.dtype == torch.float32
    assert power is None or (tuple(power.shape) == (B, F, BINS) and power.dtype == torch.float32)
    for b in range(B):
        n = _clamp_len(lens, b, L)
        f = eval_model._frames(x[b].detach(), n, torch.float32) * eval_model._WIN32
        re, im = f @ eval_model._COS32, f @ eval_model._SIN32
        P = re * re + im * im
        nf = f.size(0)
        cep[b, :nf, :NCEP] = cep_from_power(P, mel, dct)
        cep[b, :nf, NCEP:] = 0.0
        if power is not None:
            power[b, :nf] = P
        if nframes is not None:
            assert nframes.dtype == torch.int32
            nframes[b] = nf
    return cep


def melcep64(x, lens):
    """float64: per clip (P64 [nf, 129] from np.fft.rfft, cep64 [nf, 13]); reads nothing at or past the lengths"""
    x = np.asarray(x)
    B, L = x.shape
    mel, dct = tables()
    out = []
    for b in range(B):
        n = _clamp_len(lens, b, L)
        f = eval_model._frames(torch.from_numpy(np.ascontiguousarray(x[b])).double(), n, torch.float64).numpy()
        P = torch.from_numpy(np.abs(np.fft.rfft(f * eval_model._WIN64, axis=1)) ** 2)
        out.append((P.numpy(), cep_from_power(P, mel, dct).numpy()))
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------
LONG = dict(L=4480, ld=4483, lens=(4480, 4352, 4224, 2304, 2303, 100, 0))
LONG_FRAMES = (34, 33, 32, 17, 16, 1, 1)          # around frame tiles of 16 and of 32; a zero-padded frame; an empty clip
MELCEP_CASES = [(k, 'short') for k in eval_model.LTAS_KINDS] + [('randn', 'long')]
E2E_KINDS = ('randn', 'walk')          # not 'sine': bands far from the tone hold less than the rounding of its leakage
GUARD, GUARD_VALUE = 64, 777.0


def melcep_case(kind, size):
    """-> (buf, lens, L, frames): eval_model.ltas_case at the issue's shapes"""
    if size == 'short':
        buf, lens = eval_model.ltas_case(kind)
        return buf, lens, eval_model.LTAS_L, eval_model.LTAS_FRAMES
    buf, lens = eval_model.ltas_case(kind, **LONG)
    return buf, lens, LONG['L'], LONG_FRAMES


def guarded(shape, dtype=torch.float32, fill=float('nan'), on=lambda t: t):
    """-> (flat buffer, view): ``shape`` filled with ``fill`` between two rows of GUARD guard values"""
    numel = int(np.prod(shape))
    flat = on(torch.full((numel + 2 * GUARD,), fill, dtype=dtype))
    flat[:GUARD] = GUARD_VALUE
    flat[GUARD + numel:] = GUARD_VALUE
    return flat, flat[GUARD:GUARD + numel].view(*shape)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def run_melcep(fn, ltas_fn, kind, size, on=lambda t: t):
    """every check of the issue on one case.  ``fn`` / ``ltas_fn``: melcep_frames / ltas_power of the kernels or of the
    models; ``on``: moves a CPU tensor to where they run.  Returns the measured error / floor ratios."""
    buf, lens, L, frames = melcep_case(kind, size)
    B, F = len(lens), frame_count(L)
    x, ln = on(buf)[:, :L], on(lens)
    mel, dct = tables()
    fcep, cep = guarded((B, F, CEPW), on=on)
    fpow, power = guarded((B, F, BINS), on=on)
    before = (_bits(fcep).clone(), _bits(fpow).clone())
    nf = on(torch.full((B,), -1, dtype=torch.int32))
    assert fn(x, ln, cep=cep, nframes=nf, power=power) is cep
    # (e) frame counts, untouched memory, zero columns, repeatability, the optional output
    assert nf.cpu().tolist() == list(frames)
    for flat, was, width in ((fcep, before[0], CEPW), (fpow, before[1], BINS)):
        now = _bits(flat)
        assert torch.equal(now[:GUARD], was[:GUARD]) and torch.equal(now[-GUARD:], was[-GUARD:])
        now, was = now[GUARD:-GUARD].view(B, F, width), was[GUARD:-GUARD].view(B, F, width)
        for b, n in enumerate(frames):
            assert torch.equal(now[b, n:], was[b, n:]), (b, n)
    got_c, got_p = cep.detach().cpu(), power.detach().cpu()
    for b, n in enumerate(frames):
        assert torch.isfinite(got_c[b, :n]).all() and torch.isfinite(got_p[b, :n]).all()
        assert (_bits(got_c[b, :n, NCEP:]) == 0).all()
    fcep2, cep2 = guarded((B, F, CEPW), on=on)
    fpow2, power2 = guarded((B, F, BINS), on=on)
    fn(x, ln, cep=cep2, nframes=nf, power=power2)
    assert torch.equal(_bits(fcep2), _bits(fcep)) and torch.equal(_bits(fpow2), _bits(fpow))
    fcep3, cep3 = guarded((B, F, CEPW), on=on)
    fn(x, ln, cep=cep3)
    assert torch.equal(_bits(fcep3), _bits(fcep))
    # (a) power per frame, (b) its mean against ltas_power
    ref = melcep64(buf[:, :L].numpy(), lens.numpy())
    ltas = ltas_fn(x, ln).detach().cpu().double().numpy()
    worst_p = worst_l = 0.0
    for b, n in enumerate(frames):
        P64 = ref[b][0]
        assert P64.shape == (n, BINS)
        P = got_p[b, :n].double().numpy()
        err = np.abs(P - P64).max(1) / np.maximum(P64.max(1), 1e-300)
        worst_p = max(worst_p, float(err.max()))
        assert (err <= LTAS_BOUND).all(), (b, err)
        errl = np.abs(P.mean(0) - ltas[b]).max() / max(ltas[b].max(), 1e-300)
        worst_l = max(worst_l, float(errl))
        assert errl <= 2 * LTAS_BOUND, (b, errl)
    # (c) teacher-forced: float64 from the power that was returned; (d) end to end
    ratios = {}
    for tag, want, model in (
            ('forced', [cep_from_power(got_p[b, :n].double(), mel, dct).numpy() for b, n in enumerate(frames)],
             [cep_from_power(got_p[b, :n], mel, dct).double().numpy() for b, n in enumerate(frames)]),
            ('e2e', [r[1] for r in ref],
             [melcep_frames(buf[b:b + 1, :L], lens[b:b + 1])[0, :n, :NCEP].double().numpy() for b, n in enumerate(frames)])):
        if tag == 'e2e' and kind not in E2E_KINDS:
            continue
        scale = [np.abs(w).max() for w in want]
        floor = max(FLOOR_MIN, max(float(np.abs(m - w).max() / s) for m, w, s in zip(model, want, scale)))
        err = [float(np.abs(got_c[b, :n, :NCEP].double().numpy() - want[b]).max() / scale[b]) for b, n in enumerate(frames)]
        ratios[tag] = max(err) / floor
        print('melcep_frames %s/%s %s: worst error %.2e of the clip\'s largest |c|, floor %.2e, ratio %.2f (bound %g)'
              % (kind, size, tag, max(err), floor, ratios[tag], CEP_MARGIN))
        assert max(err) <= CEP_MARGIN * floor, (tag, err, floor)
    print('melcep_frames %s/%s power: worst %.2e of the frame\'s largest bin, mean against ltas_power %.2e (bounds %g, %g)'
          % (kind, size, worst_p, worst_l, LTAS_BOUND, 2 * LTAS_BOUND))
    ratios.update(power=worst_p, ltas=worst_l)
    return ratios


# ----------------------------------------------------------------------------------------------------------------------
# dtw_cost: fp32 model, float64 reference, mutants
# ----------------------------------------------------------------------------------------------------------------------
def dtw_total(d, diag_weight=2.0, start_weight=2.0):
    """the recursion over a local-cost matrix d [n, m] in d's dtype, one anti-diagonal at a time -> D(n-1, m-1)"""
    n, m = d.shape
    dt = d.dtype
    inf = np.array(np.inf, dtype=dt)
    dw, sw = dt.type(diag_weight), dt.type(start_weight)
    prev2 = prev = None          # D on diagonals s - 2 and s - 1, indexed by row i (inf where the cell does not exist)
    for s in range(n + m - 1):
        i = np.arange(n)
        j = s - i
        ok = (j >= 0) & (j < m)
        dd = np.where(ok, d[i, np.clip(j, 0, m - 1)], inf).astype(dt)
        if s == 0:
            cur = np.full(n, inf, dtype=dt)
            cur[0] = sw * d[0, 0]
        else:
            up = np.concatenate(([inf], prev[:-1])).astype(dt)           # D(i-1, j): row i-1 on diagonal s-1
            left = prev                                                     # D(i, j-1): row i on diagonal s-1
            dg = (np.concatenate(([inf], prev2[:-1])).astype(dt) if prev2 is not None else np.full(n, inf, dtype=dt))
            cur = np.minimum(np.minimum(up + dd, left + dd), dg + dw * dd).astype(dt)
            cur = np.where(ok, cur, inf).astype(dt)
        prev2, prev = prev, cur
    return prev[n - 1]


def local_cost(a, b, dtype, cols=slice(1, 13)):
    a, b = np.asarray(a, dtype=dtype)[:, cols], np.asarray(b, dtype=dtype)[:, cols]
    df = a[:, None, :] - b[None, :, :]
    return np.sqrt((df * df).sum(-1, dtype=dtype)).astype(dtype)


MUTANTS = ('diag1', 'col0', 'drop12', 'start1', 'pastcount')


def dtw_cost(cep_a, nf_a, cep_b, nf_b, out=None, mutate=None):
    assert cep_a.dtype == cep_b.dtype == torch.float32 and cep_a.dim() == cep_b.dim() == 3
    B, Fa, Fb = cep_a.size(0), cep_a.size(1), cep_b.size(1)
    assert cep_b.size(0) == B and cep_a.size(2) == cep_b.size(2) == CEPW and Fa <= DTW_MAX and Fb <= DTW_MAX
    if out is None:
        out = torch.empty(B)
    cols = {'col0': slice(0, 13), 'drop12': slice(1, 12)}.get(mutate, slice(1, 13))
    for b in range(B):
        n = Fa if nf_a is None else max(1, min(int(nf_a[b]), Fa))
        m = Fb if nf_b is None else max(1, min(int(nf_b[b]), Fb))
        if mutate == 'pastcount':
            n = min(n + 1, Fa)
        d = local_cost(cep_a[b, :n].detach().numpy(), cep_b[b, :m].detach().numpy(), np.float32, cols)
        out[b] = float(dtw_total(d, 1.0 if mutate == 'diag1' else 2.0, 1.0 if mutate == 'start1' else 2.0))
    return out


def dtw64(cep_a, nf_a, cep_b, nf_b):
    """float64 numpy [B]; reads nothing past the counts or outside columns 1..12"""
    cep_a, cep_b = np.asarray(cep_a), np.asarray(cep_b)
    return np.array([dtw_total(local_cost(cep_a[b, :max(1, int(n))], cep_b[b, :max(1, int(m))], np.float64))
                     for b, (n, m) in enumerate(zip(nf_a, nf_b))])


DTW_F = 132
DTW_PAIRS = ((1, 1), (1, 7), (7, 1), (2, 2), (63, 64), (64, 65), (65, 63), (128, 129), (129, 2), (33, 130))
DTW_LONG = ((1024, 1024), (1024, 1))          # capacity 1024, a batch of one each, in the integer pass only


def dtw_case(pairs, Fa, Fb, integer, seed=0):
    """-> (cep_a [B, Fa, 16], nf_a, cep_b [B, Fb, 16], nf_b): NaN in rows past the counts and in columns 0 and 13..15.
    ``integer``: columns 1, 4, 7, 12 hold one integer in [-3, 3] per frame and the rest of 1..12 are 0, so d = 2 |delta|"""
    rs = np.random.RandomState(seed)
    B = len(pairs)
    seqs = []
    for F, side in ((Fa, 0), (Fb, 1)):
        c = np.full((B, F, CEPW), np.nan, dtype=np.float32)
        for b, p in enumerate(pairs):
            k = p[side]
            if integer:
                v = np.zeros((k, 12), dtype=np.float32)
                v[:, [0, 3, 6, 11]] = rs.randint(-3, 4, size=(k, 1))
            else:
                v = rs.randn(k, 12).astype(np.float32)
            c[b, :k, 1:13] = v
        seqs.append(torch.from_numpy(c))
    nf_a = torch.tensor([p[0] for p in pairs], dtype=torch.int32)
    nf_b = torch.tensor([p[1] for p in pairs], dtype=torch.int32)
    return seqs[0], nf_a, seqs[1], nf_b


def dtw_real_bound(n, m, D64):
    return (n + m + 16) * 2.0 ** -23 * D64


def _run_guarded(fn, ca, na, cb, nb, on):
    flat, out = guarded((ca.size(0),), on=on)
    assert fn(on(ca), on(na), on(cb), on(nb), out=out) is out
    f = flat.detach().cpu()
    assert (f[:GUARD] == GUARD_VALUE).all() and (f[-GUARD:] == GUARD_VALUE).all()
    return out.detach().cpu()


def check_dtw_integer(fn, on=lambda t: t, long=True):
    cases = [(DTW_PAIRS, DTW_F, DTW_F)] + ([((p,), DTW_MAX, DTW_MAX) for p in DTW_LONG] if long else [])
    for pairs, Fa, Fb in cases:
        ca, na, cb, nb = dtw_case(pairs, Fa, Fb, True)
        want = dtw64(ca.numpy(), na.numpy(), cb.numpy(), nb.numpy())
        assert (want == np.round(want)).all() and want.max() < 2 ** 24
        got = _run_guarded(fn, ca, na, cb, nb, on).double().numpy()
        print('dtw_cost integer pass %s: got %s want %s' % (pairs, got, want))
        assert np.array_equal(got, want), (pairs, got, want)


def check_dtw_real(fn, on=lambda t: t):
    ca, na, cb, nb = dtw_case(DTW_PAIRS, DTW_F, DTW_F, False)
    want = dtw64(ca.numpy(), na.numpy(), cb.numpy(), nb.numpy())
    got = _run_guarded(fn, ca, na, cb, nb, on).double().numpy()
    bound = np.array([dtw_real_bound(n, m, w) for (n, m), w in zip(DTW_PAIRS, want)])
    ratio = np.abs(got - want) / want
    print('dtw_cost real pass: |D32 - D64| / D64 %s, bound / D64 %s' % (np.array2string(ratio, precision=2),
                                                                       np.array2string(bound / want, precision=2)))
    assert np.isfinite(got).all() and (np.abs(got - want) <= bound).all(), (got, want)
    return float((np.abs(got - want) / bound).max())


def check_dtw_properties(fn, on=lambda t: t):
    ca, na, cb, nb = dtw_case(((66, 66), (1, 1), (64, 64), (65, 65)), DTW_F, DTW_F, False, seed=3)
    self_ = _run_guarded(fn, ca, na, ca, na, on)
    assert (_bits(self_) == 0).all(), self_          # exactly +0
    twice = torch.full_like(cb, float('nan'))
    for b, n in enumerate(na.tolist()):
        twice[b, :2 * n, 1:13] = ca[b, :n, 1:13].repeat_interleave(2, dim=0)
    rep = _run_guarded(fn, ca, na, twice, na * 2, on)
    assert (_bits(rep) == 0).all(), rep
    ca, na, cb, nb = dtw_case(DTW_PAIRS, DTW_F, DTW_F, False, seed=5)
    ab, ba = _run_guarded(fn, ca, na, cb, nb, on), _run_guarded(fn, cb, nb, ca, na, on)
    assert torch.equal(_bits(ab), _bits(ba)), (ab, ba)
    assert torch.equal(_bits(ab), _bits(_run_guarded(fn, ca, na, cb, nb, on)))
    assert (ab > 0).all()


# ----------------------------------------------------------------------------------------------------------------------
# the two-tone clips of the issue: a 0.5-amplitude 400 Hz tone that switches to 1800 Hz, 8192 samples at 8 kHz, 1e-3 noise
# ----------------------------------------------------------------------------------------------------------------------
TWO_TONE_SEED = 11


def two_tone(switch=0.5, n=8192, sr=8000.0, seed=TWO_TONE_SEED):
    """float32 [n]"""
    t = np.arange(n, dtype=np.float64) / sr
    k = int(round(switch * n))
    x = 0.5 * np.where(np.arange(n) < k, np.sin(2 * np.pi * 400.0 * t), np.sin(2 * np.pi * 1800.0 * t))
    return torch.from_numpy((x + 1e-3 * np.random.RandomState(seed).randn(n)).astype(np.float32))


def check_two_tone(aligned_distance, ltas_fn, on=lambda t: t):
    """rows: A against itself, A reversed, and the same word said again with its switch point 19 % earlier and 19 % later
    (at 0.405 and 0.595 of the clip), each with noise of its own - the noise-only bands alone put two takes of one word
    about 12 dB apart"""
    A = two_tone()
    a = on(torch.stack([A, A, A, A]))
    b = on(torch.stack([A, A.flip(0), two_tone(0.5 * 0.81, seed=TWO_TONE_SEED + 1),
                        two_tone(0.5 * 1.19, seed=TWO_TONE_SEED + 2)]))
    ln = on(torch.full((4,), A.numel(), dtype=torch.int64))
    mcd = aligned_distance(a, ln, b, ln).cpu()
    assert mcd.dtype == torch.float64 and tuple(mcd.shape) == (4,)
    db = lambda p: 10.0 * np.log10(p.detach().cpu().double().numpy() + 1e-10)          # noqa: E731
    ltas = np.sqrt(((db(ltas_fn(a, ln)) - db(ltas_fn(b, ln))) ** 2).mean(1))
    print('two-tone clips: mcd_db %s, ltas_db %s' % (mcd.tolist(), ltas.tolist()))
    assert float(mcd[0]) == 0.0
    assert float(mcd[1]) > 5.0 * float(mcd[2]) and float(mcd[1]) > 5.0 * float(mcd[3])
    assert ltas[1] < ltas[2] and ltas[1] < ltas[3]
    return mcd, ltas


ALL = ('melcep_frames', 'dtw_cost')


def install(monkeypatch):
    """after ``kernel_model.install`` and ``eval_model.install``: the aligned-distance kernels' CPU models"""
    import audiogan_amd.kernels as K
    for n in ALL:
        assert hasattr(K, n), 'align model has %s but audiogan_amd.kernels does not' % n
        monkeypatch.setattr(K, n, globals()[n])
