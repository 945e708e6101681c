"""Models of ``audiogan_amd.kernels.frame_power`` / ``activity_segments`` (ag_frame_power, ag_activity_segments; contract in
include/audiogan_hip.h), the float64 statement of the power, the case tables and the checkers both test files share  --
TEST INFRASTRUCTURE.

Bounds (derived, not measured).
  bound pass    a frame's power is a sum of ``win`` non-negative terms formed in fp32 in some tree order, times fp32(1 / win):
                  |p - p64| <= (win + 3) 2^-24 p64 + 2^-100
                (win - 1 additions and the squares, at most win roundings on any path of any tree, 2^-24 each, first order
                with the +3 covering the rounding of 1 / win, of the product and the second-order terms; 2^-100 for sums that
                underflow).  p64: the same mean in float64 on the same fp32 samples (``power64``, Python integers).
  integer pass  samples of integers in [-64, 64] and win <= 4096: every partial sum is an integer below 2^24, so fp32 is
                exact in any order and the launch must equal fp32(sum) * fp32(1 / win) bit for bit.
  segments      integers: ``seg``, ``count`` and the bits of ``pmax`` equal ``audio.activity_rule`` exactly.
Every case also checks: NaN-filled (power) / -1-filled (segments) destinations between guard words that must survive, the row
pitch beyond the width untouched, all n_frames entries written, nothing at or past a row's length read (NaN lies there),
segment entries at and past min(count, K) still -1."""
import numpy as np
import torch

from audiogan_amd import audio

GUARD, GUARD_VALUE = 64, 777.0
SHAPES = ((200, 80), (256, 64), (1, 1), (4096, 4096), (4096, 1))
FAR = 1 << 33
MUTANTS = ('drop_before_close', 'ge', 'pad_unclipped', 'count_capped')


# ----------------------------------------------------------------------------------------------------------------------
# the power: float64 statement, cases, checkers
# ----------------------------------------------------------------------------------------------------------------------
def power64(x, n, win, hop, n_frames, in_start=0, f_start=0):
    """float64 [n_frames]: frame f = f_start + j is the mean of x^2 over absolute samples f hop .. f hop + win - 1, where the
    row ``x[:n]`` holds samples in_start .. in_start + n - 1 and every other sample is zero.  Python integers."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)[:int(n)]
    first = int(f_start) * int(hop)
    z = np.zeros(max(0, (n_frames - 1) * hop + win), dtype=np.float64)          # absolute samples first ..
    lo, hi = max(first, int(in_start)), min(first + len(z), int(in_start) + len(x))
    if hi > lo:
        z[lo - first:hi - first] = x[lo - int(in_start):hi - int(in_start)] ** 2
    if n_frames == 0:
        return np.zeros(0)
    rows = np.lib.stride_tricks.as_strided(z, shape=(n_frames, win), strides=(hop * z.strides[0], z.strides[0]), writeable=False)
    return rows.sum(1) / float(win)


def length_pool(win, hop, tile):
    """0, 1, win - 1, win, win + 1 samples, and the most samples of tile - 1, tile and tile + 1 frames (ceil(n / hop) frames)"""
    return [0, 1, win - 1, win, win + 1, (tile - 1) * hop, tile * hop, (tile + 1) * hop]


def power_cases(win, hop, tile, integer=False):
    """three launches of three ragged rows: every length of the pool is used; noise of amplitude 1e-3 and a full-scale square
    wave in turn"""
    pool = length_pool(win, hop, tile)
    out = []
    for i in range(3):
        lens = (pool[(3 * i) % 8], pool[(3 * i + 1) % 8], pool[(3 * i + 2) % 8])
        out.append(dict(win=win, hop=hop, lens=lens, wave=('noise', 'square')[i & 1], integer=integer, seed=i, in_start=0, f_start=0,
                        n_frames=None))
    return out


def far_cases(win, hop):
    """f_start hop and in_start past 2^33 on rows of a few hundred samples: the row starts 5 samples before the first frame,
    and 7 samples after it (those 7 read as zero)"""
    f_start = FAR // hop + 11
    n_frames = 5
    span = (n_frames - 1) * hop + win
    return [dict(win=win, hop=hop, lens=(span + 9, max(1, span // 2), 0), wave='noise', integer=False, seed=40 + k, in_start=f_start * hop + d,
                 f_start=f_start, n_frames=n_frames) for k, d in enumerate((-5, 7))]


def build_power(case):
    rs = np.random.RandomState(2000 + case['seed'] + 7 * case['win'] + case['hop'])
    lens = case['lens']
    n_in = max(lens) + 3
    pitch = n_in + 5
    buf = np.full((len(lens), pitch), np.nan, dtype=np.float32)
    for b, n in enumerate(lens):
        if case['integer']:
            v = rs.randint(-64, 65, size=n)
        elif case['wave'] == 'noise':
            v = rs.uniform(-1e-3, 1e-3, size=n)
        else:
            v = np.where((((np.arange(n) + case['in_start']) // 17) & 1) == 0, 1.0, -1.0)
        buf[b, :n] = v
    n_frames = case['n_frames'] if case['n_frames'] is not None else (n_in + case['hop'] - 1) // case['hop']
    return dict(src=torch.from_numpy(buf), lens=torch.tensor(lens, dtype=torch.int64), n_in=n_in, n_frames=n_frames, B=len(lens))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def run_power(fn, case, on=lambda t: t):
    """one launch under every check that needs no reference -> (d, p [B, n_frames] fp32 numpy)"""
    d = build_power(case)
    B, nfr = d['B'], d['n_frames']
    ldd = nfr + 7
    flat = on(torch.full((B * ldd + 2 * GUARD,), float('nan')))
    flat[:GUARD] = GUARD_VALUE
    flat[GUARD + B * ldd:] = GUARD_VALUE
    before = _bits(flat).clone()
    dst = flat[GUARD:GUARD + B * ldd].view(B, ldd)[:, :nfr]
    src = on(d['src'])[:, :d['n_in']]                                       # a row pitch above the width
    got = fn(src, on(d['lens']), case['win'], case['hop'], dst=dst, in_start=case['in_start'], f_start=case['f_start'])
    assert got is dst
    now = _bits(flat)
    assert torch.equal(now[:GUARD], before[:GUARD]) and torch.equal(now[-GUARD:], before[-GUARD:]), 'guards'
    body, was = now[GUARD:-GUARD].view(B, ldd), before[GUARD:-GUARD].view(B, ldd)
    assert torch.equal(body[:, nfr:], was[:, nfr:]), 'the row pitch beyond n_frames'
    p = dst.detach().cpu()
    assert torch.isfinite(p).all(), 'every entry of n_frames is written, and nothing at or past a length is read'
    for b, n in enumerate(case['lens']):
        if n == 0:
            assert (p[b] == 0).all(), 'a row of length 0'
    return d, p.numpy()


def reference_power(case, d, b):
    return power64(d['src'][b].numpy(), case['lens'][b], case['win'], case['hop'], d['n_frames'], case['in_start'], case['f_start'])


def check_power_bound(fn, table, on=lambda t: t):
    """-> the largest |p - p64| / bound over the table's launches"""
    worst = 0.0
    for case in table:
        d, p = run_power(fn, case, on)
        k = (case['win'] + 3) * 2.0 ** -24
        ratios = []
        for b in range(d['B']):
            p64 = reference_power(case, d, b)
            ratios.append(float((np.abs(p[b].astype(np.float64) - p64) / (k * p64 + 2.0 ** -100)).max()) if len(p64) else 0.0)
        print('frame_power bound pass win %d hop %d lens %s %s f_start %d in_start %d: largest |p - p64| / bound %.4f'
              % (case['win'], case['hop'], case['lens'], case['wave'], case['f_start'], case['in_start'], max(ratios)))
        assert max(ratios) <= 1.0, (case, ratios)
        worst = max(worst, max(ratios))
    return worst


def check_power_integer(fn, table, on=lambda t: t):
    for case in table:
        assert case['integer'] and case['win'] <= 4096
        d, p = run_power(fn, case, on)
        for b in range(d['B']):
            total = np.rint(reference_power(case, d, b) * case['win'])
            assert total.max(initial=0.0) < 2 ** 24
            want = total.astype(np.float32) * (np.float32(1.0) / np.float32(case['win']))
            assert np.array_equal(p[b].view(np.int32), want.view(np.int32)), (case, b)
    print('frame_power integer pass win %d hop %d: equal' % (table[0]['win'], table[0]['hop']))


def frame_power(src, src_len, win, hop, dst=None, n_frames=None, in_start=0, f_start=0):
    """numpy model of the launch, in its order: block sums over g = gcd(win, hop) samples as a chain s = x x + s (the fused
    step formed in float64 and rounded to fp32: exact up to a rare double rounding), then a chain of fp32 additions over a
    frame's win / g block sums, times fp32(1 / win)"""
    assert src.dtype == torch.float32 and src.dim() == 2 and 1 <= hop <= win <= 4096
    s = src.detach().cpu().numpy()
    B, n_in = s.shape
    if n_frames is None:
        n_frames = dst.size(1) if dst is not None else (n_in + hop - 1) // hop
    if dst is None:
        dst = torch.empty(B, n_frames)
    assert tuple(dst.shape) == (B, n_frames) and dst.dtype == torch.float32
    lens = np.full(B, n_in) if src_len is None else np.clip(src_len.detach().cpu().numpy(), 0, n_in)
    g = int(np.gcd(win, hop))
    wq, hq = win // g, hop // g
    first = int(f_start) * hop
    for b in range(B):
        if n_frames == 0:
            continue
        z = np.zeros((n_frames - 1) * hop + win, dtype=np.float32)
        lo, hi = max(first, int(in_start)), min(first + len(z), int(in_start) + int(lens[b]))
        if hi > lo:
            z[lo - first:hi - first] = s[b, lo - int(in_start):hi - int(in_start)]
        blocks = z.reshape(-1, g).astype(np.float64)
        sums = np.zeros(blocks.shape[0], dtype=np.float32)
        for i in range(g):
            sums = (blocks[:, i] * blocks[:, i] + sums.astype(np.float64)).astype(np.float32)
        acc = np.zeros(n_frames, dtype=np.float32)
        at = np.arange(n_frames) * hq
        for i in range(wq):
            acc = acc + sums[at + i]
        dst[b] = torch.from_numpy(acc * (np.float32(1.0) / np.float32(win))).to(dst.device)
    return dst


# ----------------------------------------------------------------------------------------------------------------------
# the segments: hand-written facts, generated patterns, the checker, the model and its mutants
# ----------------------------------------------------------------------------------------------------------------------
def _flags(text):
    return [float(c == '1') for c in text]


def _fact(name, text, want, min_gap=3, min_run=3, pad=0, win=25, hop=10, length=None, K=8, count=None):
    return dict(name=name, rows=[_flags(text)], nf=[len(text)], lens=[len(text) * hop + 1000 if length is None else length],
                min_gap=min_gap, min_run=min_run, pad=pad, win=win, hop=hop, K=K, ratio=0.5, floor=0.0,
                want=[want], count=[len(want) if count is None else count])


# 0/1 power with ratio 0.5: a frame is active where the text holds a 1.  want: the (start, end) samples, worked out by hand
FACTS = [
    _fact('a gap of min_gap - 1 closes', '1110011', [(0, 6 * 10 + 25)]),
    _fact('a gap of min_gap does not', '11100011100', [(0, 2 * 10 + 25), (60, 8 * 10 + 25)]),
    _fact('a run of min_run - 1 drops', '110000111', [(60, 8 * 10 + 25)]),
    _fact('a run of min_run stays', '1110000111', [(0, 45), (70, 9 * 10 + 25)]),
    _fact('close happens before drop', '100111', [(0, 5 * 10 + 25)]),
    _fact('padded runs that touch merge', '1100011', [(0, 90)], min_gap=0, min_run=1, pad=1, win=20),
    _fact('one sample apart they do not', '1100011', [(0, 39), (40, 89)], min_gap=0, min_run=1, pad=1, win=19),
    _fact('the end is clipped to len, the start to 0', '1011', [(0, 35)], min_gap=1, min_run=1, pad=1, length=35),
    _fact('the end alone', '0011', [(10, 38)], min_gap=1, min_run=1, pad=1, length=38),
    _fact('the first and the last frame active', '1000001', [(0, 25), (60, 85)], min_gap=2, min_run=1),
    _fact('F = 1', '1', [(0, 25)], min_gap=1, min_run=1),
    _fact('F = 1, inactive run rules off', '1', [(0, 25)], min_gap=0, min_run=0),
    _fact('more runs than K', '1010101', [(0, 10), (20, 30)], min_gap=1, min_run=1, win=10, K=2, count=4),
    _fact('an all-zero row', '00000', []),
    _fact('a NaN row', '11111', [], count=-1),
]
FACTS[-1]['rows'][0][2] = float('nan')
FACTS[-1]['want'] = [None]


def chunk_patterns(chunk):
    """patterns that cross the launch's internal chunk of ``chunk`` frames: a gap and a run that straddle the boundary, runs
    that end and start exactly on it, and the alternating pattern over two chunks and a bit (the most runs a row can hold)
    with K below, equal to and above the count"""
    def row(F, *ones):
        r = np.zeros(F, dtype=np.float32)
        for a, e in ones:
            r[a:e] = 1.0
        return r.tolist()
    F = chunk + 40
    base = dict(win=25, hop=10, ratio=0.5, floor=0.0, K=8)
    out = [
        dict(base, name='a gap of 3 over the boundary closes at min_gap 4', min_gap=4, min_run=1, pad=0, nf=[F, F, F - 7],
             rows=[row(F, (chunk - 4, chunk - 1), (chunk + 2, chunk + 6)), row(F, (chunk - 5, chunk - 2), (chunk + 2, chunk + 6)),
                   row(F, (0, 1), (chunk - 1, chunk), (chunk + 3, F))]),
        dict(base, name='a run of 5 over the boundary: min_run 5 keeps it, a run of 4 drops', min_gap=0, min_run=5, pad=2,
             nf=[F, F, F], rows=[row(F, (chunk - 2, chunk + 3)), row(F, (chunk - 2, chunk + 2), (chunk + 10, chunk + 15)),
                                 row(F, (chunk - 5, chunk), (chunk + 64, chunk + 69))]),
        dict(base, name='runs that end and start on the boundary; the last frame of the row', min_gap=1, min_run=1, pad=0,
             nf=[F, F, 2 * chunk], rows=[row(2 * chunk, (0, chunk)), row(2 * chunk, (chunk, F)), row(2 * chunk, (63, 65), (2 * chunk - 1, 2 * chunk))]),
    ]
    for c in out:
        c['lens'] = [n * 10 + 15 for n in c['nf']]
    F = 2 * chunk + 37
    alt = (np.arange(F) % 2 == 0).astype(np.float32).tolist()
    n_runs = (F + 1) // 2
    for K in (n_runs - 3, n_runs, n_runs + 5):
        out.append(dict(name='alternating, K %d of %d runs' % (K, n_runs), rows=[alt, alt[1:] + [0.0]], nf=[F, F - 1], lens=[F * 10, F * 10],
                        min_gap=1, min_run=1, pad=0, win=10, hop=10, ratio=0.5, floor=0.0, K=K))
    return out


def run_segments(fn, case, on=lambda t: t):
    """one launch into a -1-filled ``seg`` between guards -> (seg [B, K, 2], count [B], pmax bits [B]) numpy"""
    B, K = len(case['rows']), case['K']
    F = max(len(r) for r in case['rows'])
    power = torch.full((B, F + 3), float('nan'))                            # a row pitch above F, NaN past each row's frames
    for b, r in enumerate(case['rows']):
        power[b, :len(r)] = torch.tensor(r)
    flat = on(torch.full((B * K * 2 + 2 * GUARD,), -1, dtype=torch.int64))
    flat[:GUARD] = 777
    flat[GUARD + B * K * 2:] = 777
    seg = flat[GUARD:GUARD + B * K * 2].view(B, K, 2)
    nf = torch.tensor(case['nf'], dtype=torch.int32)
    lens = torch.tensor(case['lens'], dtype=torch.int64)
    got, count, pmax = fn(on(power)[:, :F], on(nf), on(lens), case['ratio'], case['floor'], case['min_gap'], case['min_run'],
                          case['pad'], case['win'], case['hop'], K=K, seg=seg)
    assert got is seg
    assert (flat[:GUARD] == 777).all() and (flat[GUARD + B * K * 2:] == 777).all(), 'guards'
    return seg.cpu().numpy(), count.cpu().numpy(), pmax.cpu().numpy().view(np.int32), power[:, :F].numpy()


def check_segments(fn, table, on=lambda t: t):
    """``seg``, ``count`` and ``pmax`` against ``audio.activity_rule``; what lies at and past min(count, K) still holds -1"""
    for case in table:
        seg, count, pmax, power = run_segments(fn, case, on)
        want, wcount, wpmax = audio.activity_rule(power, case['nf'], case['lens'], case['ratio'], case['floor'], case['min_gap'],
                                                  case['min_run'], case['pad'], case['win'], case['hop'])
        assert count.dtype == np.int32 and count.tolist() == wcount.tolist(), (case['name'], count.tolist(), wcount.tolist())
        assert np.array_equal(pmax, wpmax.view(np.int32)), (case['name'], pmax, wpmax)
        for b, w in enumerate(want):
            k = 0 if w is None else min(len(w), case['K'])
            if k:
                assert np.array_equal(seg[b, :k], w[:k]), (case['name'], b, seg[b, :k].tolist(), w[:k].tolist())
            assert (seg[b, k:] == -1).all(), (case['name'], b, 'entries past min(count, K) written')
            if 'want' in case:          # the hand-written expectation
                assert (w is None and case['want'][b] is None) or [tuple(r) for r in w.tolist()] == case['want'][b] or \
                    case['K'] < len(w), (case['name'], w, case['want'][b])
                assert int(count[b]) == case['count'][b], (case['name'], count[b])


def activity_segments(power, nf, lens, ratio, floor, min_gap, min_run, pad, win, hop, K=256, seg=None, mutate=None):
    """torch / numpy model of the launch: steps 1 to 6 of the header taken literally, frame by frame on arrays of flags"""
    p_all = power.detach().cpu().numpy()
    B, F = p_all.shape
    if seg is None:
        seg = torch.full((B, K, 2), -1, dtype=torch.int64)
    count, pmax = torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.float32)
    for b in range(B):
        n = int(min(max(int(nf[b]), 0), F))
        ln = max(int(lens[b]), 0)
        p = p_all[b, :n]
        if not np.isfinite(p).all():
            count[b], pmax[b] = -1, float('nan')
            continue
        if n == 0:
            continue
        top = p.max()
        if top == 0 and not (p.view(np.int32) == 0).any():          # only -0 in the row
            top = np.float32(-0.0)
        pmax[b] = float(top)
        thr = np.maximum(np.float32(top * np.float32(ratio)), np.float32(floor))
        act = (p >= thr) if mutate == 'ge' else (p > thr)

        def close(a):
            on_ = np.flatnonzero(a)
            a = a.copy()
            for i, j in zip(on_[:-1], on_[1:]):
                if 0 < j - i - 1 < min_gap:
                    a[i + 1:j] = True
            return a

        def runs(a):
            e = np.flatnonzero(np.diff(np.concatenate([[0], a.astype(np.int8), [0]])))
            return list(zip(e[0::2].tolist(), e[1::2].tolist()))

        def drop(a):
            a = a.copy()
            for s, e in runs(a):
                if e - s < min_run:
                    a[s:e] = False
            return a
        act = close(drop(act)) if mutate == 'drop_before_close' else drop(close(act))
        out = []
        for s, e in runs(act):
            s0, s1 = (s - pad) * hop, (e - 1 + pad) * hop + win
            if mutate != 'pad_unclipped':
                s0, s1 = max(0, s0), min(ln, s1)
            if out and s0 <= out[-1][1]:
                out[-1][1] = max(out[-1][1], s1)
            else:
                out.append([s0, s1])
        count[b] = min(len(out), K) if mutate == 'count_capped' else len(out)
        for k, r in enumerate(out[:K]):
            seg[b, k] = torch.tensor(r, dtype=torch.int64)
    return seg, count, pmax


# ----------------------------------------------------------------------------------------------------------------------
# signals and the tree of recordings both test files ingest
# ----------------------------------------------------------------------------------------------------------------------
BURST_RATES = (8000, 16000, 22050, 44100, 48000)


def burst_signal(sr):
    """one second at ``sr`` Hz: +-1e-4 uniform noise from RandomState(3), a 0.5-amplitude 500 Hz square burst from 0.3 s to
    0.7 s; resampled to 8 kHz with ``audio.resample64`` -> float32 [8000]"""
    t = np.arange(sr) / float(sr)
    x = np.random.RandomState(3).uniform(-1e-4, 1e-4, sr)
    sq = np.where(np.floor(t * 1000.0) % 2 == 0, 0.5, -0.5)
    x = x + np.where((t >= 0.3) & (t < 0.7), sq, 0.0)
    return audio.resample64(x.astype(np.float32), sr).astype(np.float32)


def margin(y, **options):
    """from the float64 power: the smallest factor between a frame's power and the threshold, over the frames of ``y``"""
    q = audio.activity_params(8000, **options)
    p = audio.frame_power64(y, len(y), q['win'], q['hop'])
    thr = max(p.max() * float(q['ratio']), float(q['floor']))
    with np.errstate(divide='ignore'):
        return float(np.exp(np.abs(np.log(np.maximum(p, 1e-300) / thr)).min()))


def make_gate_tree(root):
    """root/<word>/*.wav at 8 kHz (float samples: nothing is resampled, so expectations are exact sample indices):
    alpha/two.wav    2 s of +-1e-4 noise with 0.5-amplitude square bursts over samples [2400, 4800) and [8800, 11200), 0.5 s apart
    beta/click.wav   1.5 s of noise, a burst over [2400, 4800) and a one-sample click at 9660, which lies in 2 frames
    beta/noise.wav   1 s of noise only
    and a manifest entry that cuts 0.2 s .. 0.8 s of two.wav under the word gamma.  -> (entries, facts)
    At the defaults (25 / 10 ms: win 200, hop 80; pad 3 frames) the burst [2400, 4800) is active in frames 28 .. 59: samples
    [(28 - 3) 80, (59 + 3) 80 + 200) = [2000, 5160); [8800, 11200) in frames 108 .. 139: [8400, 11560)."""
    import os
    from audiogan_amd import ingest
    from tests.ingest_model import wav_bytes
    rs = np.random.RandomState(11)

    def put(word, name, x):
        os.makedirs(os.path.join(root, word), exist_ok=True)
        path = os.path.join(root, word, name)
        with open(path, 'wb') as f:
            f.write(wav_bytes(x.astype('<f4').tobytes(), 8000, 1, 32, tag=3))
        return path

    def noise(n):
        return rs.uniform(-1e-4, 1e-4, n).astype(np.float32)

    def burst(x, a, e):
        x[a:e] += np.where((np.arange(a, e) // 8) % 2 == 0, 0.5, -0.5).astype(np.float32)

    two, click, quiet = noise(16000), noise(12000), noise(8000)
    burst(two, 2400, 4800)
    burst(two, 8800, 11200)
    burst(click, 2400, 4800)
    click[9660] = 0.5
    paths = dict(two=put('alpha', 'two.wav', two), click=put('beta', 'click.wav', click), noise=put('beta', 'noise.wav', quiet))
    tsv = os.path.join(root, 'cut.tsv')
    with open(tsv, 'w') as f:
        f.write('alpha/two.wav\tgamma\t0.2\t0.8\n')
    entries = list(ingest.scan_tree(root)) + ingest.read_manifest(tsv)
    segments = {paths['two']: [[(2000, 5160), (8400, 11560)], [(2000, 5160)]], paths['click']: [[(2000, 5160)]], paths['noise']: [[]]}
    trim = dict(alpha=[two[2000:11560]], beta=[click[2000:5160]], gamma=[two[2000:5160]])
    split = dict(alpha=[two[2000:5160], two[8400:11560]], beta=[click[2000:5160]], gamma=[two[2000:5160]])
    clips = [two, click, quiet, two[1600:6400]]
    return entries, dict(paths=paths, segments=segments, trim=trim, split=split, clips=clips,
                         seconds_trimmed=dict(trim=(16000 - 9560 + 12000 - 3160 + 4800 - 3160) / 8000.0,
                                              split=(16000 - 2 * 3160 + 12000 - 3160 + 4800 - 3160) / 8000.0))


def check_gate_store(store, report, facts, mode):
    """the store and the report of ``build_store(trim=True)`` (mode 'trim') or ``(split=True)`` on the tree, bit for bit"""
    want = facts[mode]
    assert list(store) == ['alpha', 'beta', 'gamma'] and report['kept'] == {w: len(c) for w, c in want.items()}
    assert report['dropped'] == dict(silent=[facts['paths']['noise']], too_long=[], unreadable=[])
    assert {p: [[tuple(r) for r in e] for e in s] for p, s in report['segments'].items()} == facts['segments']
    assert abs(report['seconds_trimmed'] - facts['seconds_trimmed'][mode]) < 1e-9
    for w, clips in want.items():
        assert store[w].dtype == np.float32 and store[w].shape == (len(clips), max(len(c) for c in clips))
        for i, c in enumerate(clips):
            assert np.array_equal(store[w][i, :len(c)].view(np.int32), c.view(np.int32)) and not store[w][i, len(c):].any(), (w, i)
    assert abs(report['seconds_out'] - sum(len(c) for cs in want.values() for c in cs) / 8000.0) < 1e-9
