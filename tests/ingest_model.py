"""Torch-CPU model of ``audiogan_amd.kernels.resample_poly`` (ag_resample_poly; contract in include/audiogan_hip.h), its float64
reference, the shared case table and the checkers  --  TEST INFRASTRUCTURE, installed after ``kernel_model.install``.

Bounds (derived, not measured).
  bound pass    for any order of an fp32 sum of ``taps`` products of fp32 coefficients with mono samples formed from C channels
                  |y - y64| <= (taps + C + 3) 2^-24 sum_t |bank[p, t] x_t| + 1e-30
                y64: the same rule in float64 (``audio.resample_rule64``, Python / int64 indices) on the same fp32 bank and the
                same source values (the mean of a frame's channels in float64, int16 times 2^-15).
  integer pass  a bank of integers in [-8, 8], sources of integers in [-64, 64], 1, 2 or 4 channels: every partial sum is an
                integer multiple of a power of two below 2^24 of it, every scale is a power of two, so fp32 is exact and
                the launch must equal float64 bit for bit.
Every case also checks: the output counts, guards and the row pitch beyond n_out untouched, all n_out entries written,
rows of length 0 all zero, nothing at or past a row's length read (NaN / a large value lies there)."""
import numpy as np
import torch

from audiogan_amd import audio

GUARD, GUARD_VALUE = 64, 777.0
RATES = (48000, 44100, 11025, 16000, 6000, 4000)          # L/M: 1/6, 80/441, 320/441 (the largest bank), 1/2, 4/3, 2/1
EXTRA_RATES = (192000,)          # 1/24, 811 taps: a window that does not fit a tile of 1024 outputs - the launcher halves it
KINDS = (0, 1)
OUTS = (1023, 1024, 1025, 2049)          # either side of a tile boundary of 1024 outputs, and past two tiles
FAR_START = 1 << 33          # out_start of the far cases: N M passes 2^41 at 44.1 kHz
MUTANTS = ('phase_mod_m', 'base_plus_1', 'uncentred', 'nm32', 'past_len', 'scale_32767', 'no_average')


def shape_of(sr):
    """(L, M, half, taps) of the product's bank"""
    L, M, half, bank = audio.resample_bank(sr)
    return L, M, half, bank.size(1)


def frames_for(k, L, M):
    """the most frames that give k outputs: ceil(n L / M) = k"""
    return (k * M) // L


def length_pool(sr):
    L, M, half, _ = shape_of(sr)
    return [0, 1, half - 1] + [frames_for(k, L, M) for k in OUTS]


def cases(sr, channels, integer=False):
    """the sub-cases of one rate: both kinds x the channel counts, three ragged rows each - every length of the pool is used
    at every rate - noise and a full-scale square wave in turn; plus one far case (out_start = 2^33)"""
    pool = length_pool(sr)
    out, i = [], 0
    for kind in KINDS:
        for C in channels:
            lens = (pool[i % 7], pool[(i + 3) % 7], pool[(i + 5) % 7])
            out.append(dict(sr=sr, kind=kind, C=C, lens=lens, wave=('noise', 'square')[i & 1], integer=integer, seed=i,
                            in_start=0, out_start=0, n_out=None))
            i += 1
    L, M, half, _ = shape_of(sr)
    n_out = 300
    lo = (FAR_START * M) // L - half - 5
    n_in = ((FAR_START + n_out - 1) * M) // L + half + 6 - lo
    out.append(dict(sr=sr, kind=i & 1, C=channels[1], lens=(n_in, n_in - 2 * half, 0), wave='noise', integer=integer, seed=i,
                    in_start=lo, out_start=FAR_START, n_out=n_out))
    return out


def build(case):
    """-> dict of CPU tensors and facts: a pitched source with NaN (fp32) / 23456 (int16) at and past each row's length"""
    rs = np.random.RandomState(1000 + case['seed'])
    sr, kind, C, lens = case['sr'], case['kind'], case['C'], case['lens']
    L, M, half, taps = shape_of(sr)
    if case['integer']:
        bank = torch.from_numpy(rs.randint(-8, 9, size=(L, taps)).astype(np.float32))
    else:
        bank = audio.resample_bank(sr)[3]
    B = len(lens)
    n_in = max(lens) + 3
    pitch = n_in * C + 5
    dt = np.int16 if kind else np.float32
    buf = np.full((B, pitch), 23456 if kind else np.nan, dtype=dt)
    for b, n in enumerate(lens):
        if case['integer']:
            v = rs.randint(-64, 65, size=(n, C))
        elif case['wave'] == 'noise':
            v = rs.randint(-32768, 32768, size=(n, C)) if kind else rs.uniform(-1, 1, size=(n, C))
        else:
            t = np.arange(n)[:, None] + case['in_start']
            sq = np.where(((t // (17 + 3 * np.arange(C)[None, :])) & 1) == 0, 1.0, -1.0)
            v = np.where(sq > 0, 32767, -32768) if kind else sq
        buf[b, :n * C] = v.astype(dt).reshape(-1)
    n_out = case['n_out'] if case['n_out'] is not None else audio.out_count(n_in, L, M)
    src = torch.from_numpy(buf)
    return dict(src=src, bank=bank, L=L, M=M, half=half, taps=taps, B=B, n_in=n_in, C=C, n_out=n_out, pitch=pitch,
                lens=torch.tensor(lens, dtype=torch.int64))


def reference(case, d):
    """float64 per row: (y64 [n_out], s = sum_t |bank x_t| [n_out])"""
    out = []
    scale = 2.0 ** -15 if case['kind'] else 1.0
    bank = d['bank'].double().numpy()
    for b, n in enumerate(case['lens']):
        x = d['src'][b, :n * d['C']].double().numpy().reshape(n, d['C']).sum(1) / d['C'] * scale
        kw = dict(out_start=case['out_start'], n_out=d['n_out'], in_start=case['in_start'])
        out.append((audio.resample_rule64(x, bank, d['L'], d['M'], **kw),
                    audio.resample_rule64(np.abs(x), np.abs(bank), d['L'], d['M'], **kw)))
    return out


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def run_case(fn, case, on=lambda t: t):
    """one launch under every check that does not need the reference -> (d, y [B, n_out] float64 numpy)"""
    d = build(case)
    B, n_out, C = d['B'], d['n_out'], d['C']
    ldd = n_out + 7
    flat = on(torch.full((B * ldd + 2 * GUARD,), float('nan')))
    flat[:GUARD] = GUARD_VALUE
    flat[GUARD + B * ldd:] = GUARD_VALUE
    before = _bits(flat).clone()
    dst = flat[GUARD:GUARD + B * ldd].view(B, ldd)[:, :n_out]
    src = on(d['src'])[:, :d['n_in'] * C]
    src = src.unflatten(1, (d['n_in'], C)) if C > 1 else src
    got, counts = fn(src, on(d['lens']), on(d['bank']), d['L'], d['M'], dst=dst, in_start=case['in_start'],
                     out_start=case['out_start'])
    assert got is dst
    assert counts.cpu().tolist() == [audio.out_count(n, d['L'], d['M']) for n in case['lens']]
    now = _bits(flat)
    assert torch.equal(now[:GUARD], before[:GUARD]) and torch.equal(now[-GUARD:], before[-GUARD:]), 'guards'
    body, was = now[GUARD:-GUARD].view(B, ldd), before[GUARD:-GUARD].view(B, ldd)
    assert torch.equal(body[:, n_out:], was[:, n_out:]), 'the row pitch beyond n_out'
    y = dst.detach().cpu()
    assert torch.isfinite(y).all(), 'every entry of n_out is written, and nothing at or past a length is read'
    for b, n in enumerate(case['lens']):
        if n == 0:
            assert (y[b] == 0).all(), 'a row of length 0'
    return d, y.double().numpy()


def check_bound(fn, sr, on=lambda t: t, channels=(1, 2, 3)):
    """-> the largest |y - y64| / bound over the rate's cases"""
    return check_bound_cases(fn, cases(sr, channels), on)


def far_case(sr, channels=(1, 2, 3)):
    """the rate's launch at out_start = 2^33 with the matching in_start"""
    return cases(sr, channels)[-1]


def check_bound_cases(fn, table, on=lambda t: t):
    worst = 0.0
    for case in table:
        sr = case['sr']
        d, y = run_case(fn, case, on)
        k = (d['taps'] + d['C'] + 3) * 2.0 ** -24
        ratios = [float((np.abs(y[b] - y64) / (k * s + 1e-30)).max()) for b, (y64, s) in enumerate(reference(case, d))]
        print('resample_poly bound pass %d Hz kind %d C %d lens %s %s out_start %d: largest |y - y64| / bound %.4f'
              % (sr, case['kind'], case['C'], case['lens'], case['wave'], case['out_start'], max(ratios)))
        assert max(ratios) <= 1.0, (case, ratios)
        worst = max(worst, max(ratios))
    return worst


def check_integer(fn, sr, on=lambda t: t, channels=(1, 2, 4)):
    for case in cases(sr, channels, integer=True):
        d, y = run_case(fn, case, on)
        for b, (y64, s) in enumerate(reference(case, d)):
            assert s.max() * (2.0 ** 15 if case['kind'] else 1.0) < 2 ** 24
            assert np.array_equal(y[b], y64), (case, b, np.abs(y[b] - y64).max())
    print('resample_poly integer pass %d Hz: equal' % sr)


# ----------------------------------------------------------------------------------------------------------------------
# the model of the launch
# ----------------------------------------------------------------------------------------------------------------------
def resample_poly(src, src_len, bank, L, M, dst=None, n_out=None, in_start=0, out_start=0, mutate=None):
    assert src.dtype in (torch.float32, torch.int16) and bank.dtype == torch.float32 and src.dim() in (2, 3)
    s = src.detach().cpu().numpy()
    s = s[:, :, None] if s.ndim == 2 else s
    B, n_in, C = s.shape
    bk = bank.detach().cpu().numpy()
    assert bk.shape[0] == L and bk.shape[1] % 2 == 1 and bk.shape[1] >= 3 and L * bk.shape[1] * 4 <= 65536 and 1 <= C <= 8
    taps = bk.shape[1]
    half = (taps - 1) // 2
    if n_out is None:
        n_out = dst.size(1) if dst is not None else audio.out_count(n_in, L, M)
    if dst is None:
        dst = torch.empty(B, n_out)
    assert tuple(dst.shape) == (B, n_out) and dst.dtype == torch.float32
    q = (np.arange(n_out, dtype=np.int64) + int(out_start)) * int(M)
    if mutate == 'nm32':
        q = q.astype(np.int32).astype(np.int64)
    base, p = q // L, (q % M if mutate == 'phase_mod_m' else q % L)
    if mutate == 'base_plus_1':
        base = base + 1
    idx = base[:, None] + np.arange(taps)[None, :] - (0 if mutate == 'uncentred' else half)
    r = idx - int(in_start)
    coef = bk[p]                                                        # [n_out, taps]
    lens = np.full(B, n_in) if src_len is None else np.clip(src_len.detach().cpu().numpy(), 0, n_in)
    scale = np.float32(1.0 / 32767.0 if mutate == 'scale_32767' else 2.0 ** -15)
    invc = np.float32(1.0) if mutate == 'no_average' else np.float32(1.0) / np.float32(C)
    for b in range(B):
        n = n_in if mutate == 'past_len' else int(lens[b])
        acc = np.zeros(n_out, dtype=np.float32)
        if n > 0 and n_out > 0:
            ok = (r >= 0) & (r < n)
            fr = s[b][np.clip(r, 0, n_in - 1)].astype(np.float32)      # [n_out, taps, C]
            mono = fr[:, :, 0].copy()
            for c in range(1, C):
                mono += fr[:, :, c]
            mono *= invc
            if src.dtype == torch.int16:
                mono *= scale
            x = np.where(ok, mono, np.float32(0.0)).astype(np.float32)
            for t in range(taps):
                acc += coef[:, t] * x[:, t]
        dst[b] = torch.from_numpy(acc).to(dst.device)
    ln = torch.from_numpy(np.asarray(lens, dtype=np.int64))
    return dst, (ln * L + (M - 1)) // M


def resample_ok(L, M, taps, channels, kind):
    return L >= 1 and M >= 1 and taps >= 3 and taps % 2 == 1 and L * taps * 4 <= 65536 and 1 <= channels <= 8 and kind in (0, 1)


ALL = ('resample_poly', 'resample_ok')


def install(monkeypatch):
    """after ``kernel_model.install``: the CPU model of the resampling launch and of its predicate"""
    import audiogan_amd.kernels as K
    for n in ALL:
        assert hasattr(K, n), 'ingest model has %s but audiogan_amd.kernels does not' % n
        monkeypatch.setattr(K, n, globals()[n])


# ----------------------------------------------------------------------------------------------------------------------
# WAV files built byte by byte, and the small tree of recordings both test files ingest
# ----------------------------------------------------------------------------------------------------------------------
def wav_bytes(payload, sr, channels, bits, tag=1, extensible=False, before=b'', data_size=None, riff=b'RIFF', wave=b'WAVE'):
    """a RIFF WAV image around ``payload`` (the bytes of the data chunk); ``before``: raw chunks between fmt and data"""
    import struct
    block = channels * bits // 8
    if extensible:
        fmt = struct.pack('<HHIIHHHHIH', 0xFFFE, channels, sr, sr * block, block, bits, 22, bits, 0, tag) + \
            b'\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71'
    else:
        fmt = struct.pack('<HHIIHH', tag, channels, sr, sr * block, block, bits)
    size = len(payload) if data_size is None else data_size
    body = wave + b'fmt ' + struct.pack('<I', len(fmt)) + fmt + before + b'data' + struct.pack('<I', size) + payload
    return riff + struct.pack('<I', len(body)) + body


def pcm16(x):
    return np.asarray(x).astype('<i2').tobytes()


TREE_MAXLEN = 8000


def make_tree(root):
    """root/<word>/*.wav: 16 kHz mono int16, 44.1 kHz stereo int16, 48 kHz float, one silent file, one longer than
    TREE_MAXLEN at 8 kHz, one that is no WAV file; and a manifest of two segments of the first file.  -> (entries, facts)"""
    import os
    from audiogan_amd import ingest
    rs = np.random.RandomState(7)

    def put(word, name, blob):
        os.makedirs(os.path.join(root, word), exist_ok=True)
        path = os.path.join(root, word, name)
        with open(path, 'wb') as f:
            f.write(blob)
        return path

    def tone(sr, f, secs, amp):
        return amp * np.sin(2 * np.pi * f * np.arange(int(sr * secs)) / sr)

    a1 = np.round(tone(16000, 440.0, 0.5, 12000.0) + rs.uniform(-200, 200, 8000)).astype(np.int16)
    a2 = np.stack([np.round(tone(44100, 300.0, 0.4, 9000.0)), np.round(tone(44100, 700.0, 0.4, 5000.0))], 1).astype(np.int16)
    b1 = (tone(48000, 1000.0, 0.3, 0.25) + rs.uniform(-0.01, 0.01, 14400)).astype(np.float32)
    long_ = np.round(tone(16000, 200.0, 1.2, 3000.0)).astype(np.int16)
    long_[-1] = 5
    paths = dict(
        a1=put('alpha', 'a1.wav', wav_bytes(pcm16(a1), 16000, 1, 16)),
        a2=put('alpha', 'a2.wav', wav_bytes(pcm16(a2), 44100, 2, 16)),
        b1=put('beta', 'b1.wav', wav_bytes(b1.astype('<f4').tobytes(), 48000, 1, 32, tag=3)),
        silent=put('beta', 'silent.wav', wav_bytes(pcm16(np.zeros(4000)), 16000, 1, 16)),
        broken=put('gamma', 'broken.wav', b'RIFX' + bytes(40)),
        long=put('gamma', 'long.wav', wav_bytes(pcm16(long_), 16000, 1, 16)))
    tsv = os.path.join(root, 'segments.tsv')
    with open(tsv, 'w') as f:
        f.write('# two words of one recording\nalpha/a1.wav\tdelta\t0.05\t0.2\n\n'
                'alpha/a1.wav\tdelta\t0.25\t0.45   # the second\n')
    entries = list(ingest.scan_tree(root)) + ingest.read_manifest(tsv)
    y1 = audio.resample64(a1, 16000).astype(np.float32)
    want = dict(alpha=[y1, audio.resample64(a2, 44100).astype(np.float32)],
                beta=[audio.resample64(b1, 48000).astype(np.float32)],
                delta=[y1[400:1600], y1[2000:3600]])
    return entries, dict(paths=paths, tsv=tsv, want=want, sources=dict(a1=(a1, 16000), a2=(a2, 44100), b1=(b1, 48000)))
